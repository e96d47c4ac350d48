// sl_gp4_halves.h - bookkeeping of the open 8-cell HALVES of k_gp_sweep4<.., EARLY = true>
// (sl_gp4.hip), beside sl_gp4_queue.h (whose functions stay what they were: the list of stage-0
// records, the segments of a launch and the block rings of the older host programs).
//
// decide_block gives two verdicts per 16-cell block, one per half of eight cells.  A record
// therefore carries a live-half code - GP4H_BOTH, GP4H_LOW (cells 0 .. 7) or GP4H_HIGH (cells
// 8 .. 15) - and still names its block's FIRST cell: a cell's k_x bits depend on its position in the
// run that starts there, so the wavefront replays the whole block's generation and stores only the
// live columns.  A slot of a composite tile then holds one full block, or the low half of one block
// in columns 0 .. 7 beside the high half of another in columns 8 .. 15.
//
// Per stage there are three rings: full records, low halves, high halves.  A composite tile is four
// full slots or four paired slots, never a mix (the second generation of a paired slot is then
// uniform over the workgroup).  A stage is RUNNABLE when it can fill such a tile - four full
// records, or four low AND four high halves - or when one of its half rings holds GP4H_HALF_RUN
// records: the imbalance has filled it, and a paired composite runs with lone halves (the partner
// columns empty).  What runs next:
//   * the DEEPEST runnable stage: every stage behind it is then not runnable, that is, holds at
//     most 3 full records and at most GP4H_HALF_RUN - 1 of either half; a pass adds at most four
//     records to each ring of the stage behind it, so a full ring never holds more than 7 and a half
//     ring never more than GP4H_HALF_RUN + 3 records;
//   * otherwise the next source tile (its blocks enter the rings of stage 0, which is not runnable);
//   * once the source tiles are used up, the SHALLOWEST stage that holds anything, partly filled:
//     its full records first, then its halves.
// The kernel moves the records; this header only hands out ring positions.  Position `pos` of ring
// `kind` of stage s is record s * GP4H_RECS + gp4h_base(kind) + pos of the workgroup's scratch.
//
// Plain C++ on integers: g++ compiles it for the host tests, which drive it from a stand-alone program.
#pragma once
#include "sl_gp4_queue.h"

constexpr int GP4H_LOW = 1, GP4H_HIGH = 2, GP4H_BOTH = 3;      // live-half code: bit h = half h is open
constexpr int GP4H_RING_FULL = 0, GP4H_RING_LOW = 1, GP4H_RING_HIGH = 2, GP4H_RINGS = 3;
constexpr int GP4H_HALF_RUN = 8;                               // a half ring this full runs without waiting for partners
constexpr int GP4H_CAP_FULL = GP4Q_CAP;                        // 8 positions, 7 can be occupied
constexpr int GP4H_CAP_HALF = GP4H_HALF_RUN + 4;               // 12 positions, 11 can be occupied
constexpr int GP4H_RECS = GP4H_CAP_FULL + 2 * GP4H_CAP_HALF;   // record positions per stage

SL_HD int gp4h_ring_of(int live) { return live == GP4H_BOTH ? GP4H_RING_FULL : live == GP4H_LOW ? GP4H_RING_LOW : GP4H_RING_HIGH; }
SL_HD int gp4h_cap(int ring) { return ring == GP4H_RING_FULL ? GP4H_CAP_FULL : GP4H_CAP_HALF; }
SL_HD int gp4h_max_fill(int ring) { return gp4h_cap(ring) - 1; }
SL_HD int gp4h_base(int ring) {
    return ring == GP4H_RING_FULL ? 0 : ring == GP4H_RING_LOW ? GP4H_CAP_FULL : GP4H_CAP_FULL + GP4H_CAP_HALF;
}

struct Gp4HalfQueues {
    unsigned char head[GP4Q_STAGES][GP4H_RINGS];
    unsigned char count[GP4Q_STAGES][GP4H_RINGS];
};

SL_HD void gp4h_init(Gp4HalfQueues& q) {
    for (int s = 0; s < GP4Q_STAGES; ++s)
        for (int r = 0; r < GP4H_RINGS; ++r) q.head[s][r] = q.count[s][r] = 0;
}

SL_HD bool gp4h_full_ready(const Gp4HalfQueues& q, int s) { return q.count[s][GP4H_RING_FULL] >= GP4Q_SLOTS; }
SL_HD bool gp4h_pair_ready(const Gp4HalfQueues& q, int s) {
    const int l = q.count[s][GP4H_RING_LOW], h = q.count[s][GP4H_RING_HIGH];
    return (l >= GP4Q_SLOTS && h >= GP4Q_SLOTS) || l >= GP4H_HALF_RUN || h >= GP4H_HALF_RUN;
}
SL_HD bool gp4h_runnable(const Gp4HalfQueues& q, int s) { return gp4h_full_ready(q, s) || gp4h_pair_ready(q, s); }
SL_HD int gp4h_held(const Gp4HalfQueues& q, int s) {
    return q.count[s][GP4H_RING_FULL] + q.count[s][GP4H_RING_LOW] + q.count[s][GP4H_RING_HIGH];
}

// The stage whose panel runs next, or -1: draw a source tile (source_left) / nothing is left.
SL_HD int gp4h_next(const Gp4HalfQueues& q, int nstages, bool source_left) {
    for (int s = nstages - 1; s >= 0; --s)
        if (gp4h_runnable(q, s)) return s;
    if (source_left) return -1;
    for (int s = 0; s < nstages; ++s)
        if (gp4h_held(q, s)) return s;
    return -1;
}

// Takes up to n records off ring r of stage s: pos[w] = ring position of slot w, -1: empty.
SL_HD int gp4h_take(Gp4HalfQueues& q, int s, int r, int (&pos)[GP4Q_SLOTS]) {
    const int cap = gp4h_cap(r);
    const int n = q.count[s][r] < GP4Q_SLOTS ? q.count[s][r] : GP4Q_SLOTS;
    for (int w = 0; w < GP4Q_SLOTS; ++w) pos[w] = w < n ? (q.head[s][r] + w) % cap : -1;
    q.head[s][r] = (unsigned char)((q.head[s][r] + n) % cap);
    q.count[s][r] = (unsigned char)(q.count[s][r] - n);
    return n;
}

// The composite tile of stage s.  Returns 0: up to four full records at pos_a (of the full ring);
// 1: paired slots, slot w = the low half at pos_a[w] (low ring) beside the high half at pos_b[w]
// (high ring), either may be -1.  Full records go first when they fill a tile, or when the halves
// do not have to run (the flush).
SL_HD int gp4h_pop(Gp4HalfQueues& q, int s, int (&pos_a)[GP4Q_SLOTS], int (&pos_b)[GP4Q_SLOTS]) {
    for (int w = 0; w < GP4Q_SLOTS; ++w) pos_b[w] = -1;
    if (gp4h_full_ready(q, s) || (!gp4h_pair_ready(q, s) && q.count[s][GP4H_RING_FULL])) {
        gp4h_take(q, s, GP4H_RING_FULL, pos_a);
        return 0;
    }
    gp4h_take(q, s, GP4H_RING_LOW, pos_a);
    gp4h_take(q, s, GP4H_RING_HIGH, pos_b);
    return 1;
}

// Ring position of the rank-th record (0 .. 3) of a push of several onto ring r of stage s; the
// ring itself changes with gp4h_push, once every writer has asked.
SL_HD int gp4h_push_pos(const Gp4HalfQueues& q, int s, int r, int rank) {
    return (q.head[s][r] + q.count[s][r] + rank) % gp4h_cap(r);
}

// n records were written at gp4h_push_pos(q, s, r, 0 .. n - 1).  False: the ring would overflow
// (cannot happen under the order of gp4h_next; the host program checks it).
SL_HD bool gp4h_push(Gp4HalfQueues& q, int s, int r, int n) {
    if (q.count[s][r] + n > gp4h_max_fill(r)) return false;
    q.count[s][r] = (unsigned char)(q.count[s][r] + n);
    return true;
}

SL_HD bool gp4h_empty(const Gp4HalfQueues& q, int nstages) {
    for (int s = 0; s < nstages; ++s)
        if (gp4h_held(q, s)) return false;
    return true;
}

// What a workgroup does next: the stage (>= 0) whose panel runs on the composite tile gp4h_pop
// describes (paired = its return value), GP4Q_SOURCE (draw() handed out a source tile) or
// GP4Q_DONE.  draw() returns false once the source tiles are used up (remembered in src_done).
template <class Draw>
SL_HD int gp4h_schedule(Gp4HalfQueues& q, int nstages, int& src_done, int (&pos_a)[GP4Q_SLOTS],
                        int (&pos_b)[GP4Q_SLOTS], int& paired, Draw&& draw) {
    paired = 0;
    int st = gp4h_next(q, nstages, !src_done);
    if (st < 0 && !src_done) {
        if (draw()) return GP4Q_SOURCE;
        src_done = 1;
        st = gp4h_next(q, nstages, false);
    }
    if (st < 0) return GP4Q_DONE;
    paired = gp4h_pop(q, st, pos_a, pos_b);
    return st;
}
