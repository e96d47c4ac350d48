// sl_gp4_queue.h - bookkeeping of the open 16-cell blocks of k_gp_sweep4<.., EARLY = true>
// (sl_gp4.hip), shared by the kernel and the stand-alone program the host tests drive it with.
//
// A workgroup decides every 16-cell block on its own.  A block the bounds leave open after the
// panels 0 .. s - 1 waits in the queue of STAGE s until four of them make a composite 64-cell tile
// for panel s.  What runs next:
//   * the DEEPEST stage that holds four blocks (its blocks are the nearest to their answer, and the
//     stage behind it then holds at most three: no queue ever holds more than seven records);
//   * otherwise the next source tile (mean phase: up to four blocks enter stage 0);
//   * once the source tiles are used up, the SHALLOWEST stage that holds anything, partly filled
//     (its open blocks fill the stages behind it before those run).
// A queue is a ring of GP4Q_CAP record positions; a record is moved by the kernel (first cell,
// means, |a|^2 planes), this header only hands out the positions.
//
// Plain C++ on integers: g++ compiles it for the tests.
#pragma once

#ifndef SL_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SL_HD __host__ __device__ __forceinline__
#else
#define SL_HD inline
#endif
#endif

constexpr int GP4Q_CAP = 8;          // ring positions per stage (seven can be occupied)
constexpr int GP4Q_MAX_FILL = 7;
constexpr int GP4Q_STAGES = 32;      // panels of 256 rows: up to 8192 training points
constexpr int GP4Q_SLOTS = 4;        // blocks of a composite tile
constexpr int GP4Q_SOURCE = -1;      // gp4q_schedule: a source tile was drawn
constexpr int GP4Q_DONE = -2;        //                nothing is left

struct Gp4Queues {
    unsigned char head[GP4Q_STAGES];
    unsigned char count[GP4Q_STAGES];
};

SL_HD void gp4q_init(Gp4Queues& q) {
    for (int s = 0; s < GP4Q_STAGES; ++s) q.head[s] = q.count[s] = 0;
}

// The stage whose panel runs next, or -1: draw a source tile (source_left) / nothing is left.
SL_HD int gp4q_next(const Gp4Queues& q, int nstages, bool source_left) {
    for (int s = nstages - 1; s >= 0; --s)
        if (q.count[s] >= GP4Q_SLOTS) return s;
    if (source_left) return -1;
    for (int s = 0; s < nstages; ++s)
        if (q.count[s]) return s;
    return -1;
}

// Takes up to four records off stage s: pos[w] = ring position of slot w, -1 for an empty slot.
SL_HD int gp4q_pop(Gp4Queues& q, int s, int (&pos)[GP4Q_SLOTS]) {
    const int n = q.count[s] < GP4Q_SLOTS ? q.count[s] : GP4Q_SLOTS;
    for (int w = 0; w < GP4Q_SLOTS; ++w) pos[w] = w < n ? (q.head[s] + w) % GP4Q_CAP : -1;
    q.head[s] = (unsigned char)((q.head[s] + n) % GP4Q_CAP);
    q.count[s] = (unsigned char)(q.count[s] - n);
    return n;
}

// Ring position of the rank-th record (0 .. 3) of a push of several onto stage s; the queue itself
// changes with gp4q_push, once every writer has asked.
SL_HD int gp4q_push_pos(const Gp4Queues& q, int s, int rank) {
    return (q.head[s] + q.count[s] + rank) % GP4Q_CAP;
}

// n records were written at gp4q_push_pos(q, s, 0 .. n - 1).  False: the ring would overflow
// (cannot happen under the order of gp4q_next; the tests check it).
SL_HD bool gp4q_push(Gp4Queues& q, int s, int n) {
    if (q.count[s] + n > GP4Q_MAX_FILL) return false;
    q.count[s] = (unsigned char)(q.count[s] + n);
    return true;
}

SL_HD bool gp4q_empty(const Gp4Queues& q, int nstages) {
    for (int s = 0; s < nstages; ++s)
        if (q.count[s]) return false;
    return true;
}

// ---- the list of stage-0 records and the segments of a launch ---------------------------------
// Large launches decide the blocks in a kernel of their own (k_gp_mean_blocks, sl_gp4_mean.hip):
// the shard is cut into segments of S source tiles, the mean kernel appends one record per block it
// leaves open to a list (order free, position from a device counter), and the panel kernel's
// "source" action draws the next four records of that list: a full stage-0 composite, only the
// last draw may be partly filled.
struct Gp4ListArgs {
    const long long* cell;       // first cell of every record (nullptr: source tiles in the kernel itself)
    const double* mean;          // [record][16][d] posterior means
    const unsigned* count;       // records the mean kernel appended
    int fold;                    // a later segment: fold the key already in the workgroup's partial
    int halves;                  // decide and queue 8-cell halves (sl_gp4_halves.h); 0: whole blocks
};

SL_HD long long gp4l_draws(long long n) { return (n + GP4Q_SLOTS - 1) / GP4Q_SLOTS; }

// Record of slot w of draw t for a list of n records, -1: the slot stays empty.
SL_HD long long gp4l_slot(long long t, int w, long long n) {
    const long long r = t * GP4Q_SLOTS + w;
    return r < n ? r : -1;
}

// Source tiles per segment: the largest power of two whose worst case - every block of every tile
// open, 4 S records of 16 d means and a first cell - fits `budget` bytes (at least one tile).
SL_HD long long gp4l_segment_tiles(long long budget, int d) {
    const long long per_tile = GP4Q_SLOTS * (16LL * d * 8 + 8);
    long long s = 1;
    while (2 * s * per_tile <= budget) s *= 2;
    return s;
}
SL_HD long long gp4l_segments(long long ntiles, long long seg) { return (ntiles + seg - 1) / seg; }
// Tiles [first, first + n) of segment k.
SL_HD long long gp4l_segment_first(long long seg, long long k) { return k * seg; }
SL_HD long long gp4l_segment_count(long long ntiles, long long seg, long long k) {
    const long long left = ntiles - k * seg;
    return left < 0 ? 0 : (left < seg ? left : seg);
}

// What a workgroup does next: the stage (>= 0) whose panel runs on the composite tile of the
// records at pos[0 .. 3], GP4Q_SOURCE (draw() handed out a source tile) or GP4Q_DONE.  draw()
// returns false once the source tiles are used up (remembered in src_done: it is not asked again).
template <class Draw>
SL_HD int gp4q_schedule(Gp4Queues& q, int nstages, int& src_done, int (&pos)[GP4Q_SLOTS], Draw&& draw) {
    int st = gp4q_next(q, nstages, !src_done);
    if (st < 0 && !src_done) {
        if (draw()) return GP4Q_SOURCE;
        src_done = 1;
        st = gp4q_next(q, nstages, false);
    }
    if (st < 0) return GP4Q_DONE;
    gp4q_pop(q, st, pos);
    return st;
}
