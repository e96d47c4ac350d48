// gp4_list_sim.cpp - stand-alone host program that drives the list and segment arithmetic of
// sl_gp4_queue.h together with its queue functions, the way a block-mode launch of k_gp_sweep4 does
// behind k_gp_mean_blocks: the shard is cut into segments of source tiles; per segment the mean
// kernel appends the blocks it leaves open to a list (any order, positions from a counter), then
// some workgroups draw four records at a time with a shared ticket - a stage-0 composite tile -
// run the deeper panels from their own queues, and flush.
//
//   gp4_list_sim random <seed> <tiles> <stages> <segment> <workgroups>
//   gp4_list_sim file <path> <segment> <workgroups>      "<stages> <blocks>" then one leave-stage per
//                                                        block (-1: the block does not exist, 0: the
//                                                        mean decides it, >= stages: never decided
//                                                        before the last panel), four per tile
//   gp4_list_sim lengths <stages>                        lists of 0, 1, 4 k and 4 k + 1 records
//
// Checks: every open block enters panel 0 exactly once, every block runs the panels 0 .. leave - 1
// once each and in order, no list position and no ring position is handed out twice, the segments
// cover every tile once, and nothing is left over after a segment's flush.  Prints one line of
// counts; exit status 1 with a message otherwise.
// (tests/test_gp4_list_host.py builds it with -fsanitize=address,undefined.)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sl_gp4_queue.h"

static int fail(const char* what, long a = 0, long b = 0) {
    std::fprintf(stderr, "gp4_list_sim: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

struct Workgroup {
    Gp4Queues q;
    int src_done = 0, pos[GP4Q_SLOTS], open[GP4Q_SLOTS] = {0, 0, 0, 0}, push_stage = 0;
    std::vector<long> ring;          // the block at every ring position, -1: free
    bool done = false;
};

struct Counts {
    long segments = 0, records = 0, draws = 0, partial_draws = 0, flush_partial = 0;
    std::vector<long> composites;
};

// One segment: `list` holds the open blocks in the order the mean kernel appended them.
static int run_segment(int stages, const std::vector<int>& leave, const std::vector<long>& list, int nwg,
                       std::vector<int>& panels_done, std::mt19937& rng, Counts& counts) {
    const long long n = (long long)list.size();
    std::vector<char> drawn(list.size(), 0);
    std::vector<Workgroup> wgs((size_t)nwg);
    for (Workgroup& g : wgs) {
        gp4q_init(g.q);
        g.ring.assign((size_t)stages * GP4Q_CAP, -1);
    }
    long long ticket = 0;
    long active = nwg, passes = 0;
    while (active) {
        if (++passes > 64 * (long)leave.size() + 64L * nwg + 64) return fail("the loop does not end", passes);
        Workgroup& g = wgs[(size_t)(rng() % (unsigned)nwg)];      // the workgroups run at their own pace
        if (g.done) continue;
        int m = 0;
        for (int w = 0; w < GP4Q_SLOTS; ++w) { m += g.open[w]; g.open[w] = 0; }
        if (m && !gp4q_push(g.q, g.push_stage, m)) return fail("queue over capacity", g.push_stage, g.q.count[g.push_stage] + m);
        long long t = -1;
        int act = gp4q_schedule(g.q, stages, g.src_done, g.pos, [&]() {
            t = ticket++;
            return t < gp4l_draws(n);
        });
        if (act == GP4Q_DONE) {
            if (!gp4q_empty(g.q, stages)) return fail("queues not empty after the flush");
            for (long at : g.ring) if (at >= 0) return fail("a record was left in a ring", at);
            g.done = true;
            --active;
            continue;
        }
        for (int s = 0; s < stages; ++s)
            if (g.q.count[s] > GP4Q_MAX_FILL) return fail("queue over capacity", s, g.q.count[s]);
        long block_of_slot[GP4Q_SLOTS];
        int filled = 0;
        if (act == GP4Q_SOURCE) {                  // a draw of the list: panel 0 on its records
            act = 0;
            counts.draws += 1;
            for (int w = 0; w < GP4Q_SLOTS; ++w) {
                const long long r = gp4l_slot(t, w, n);
                block_of_slot[w] = -1;
                if (r < 0) continue;
                if (r >= n) return fail("list position out of range", (long)r, (long)n);
                if (drawn[(size_t)r]) return fail("list position handed out twice", (long)r);
                drawn[(size_t)r] = 1;
                block_of_slot[w] = list[(size_t)r];
                ++filled;
            }
            if (filled < GP4Q_SLOTS) {
                counts.partial_draws += 1;
                if (t != gp4l_draws(n) - 1) return fail("a partly filled draw that is not the last", (long)t);
            }
        } else {
            for (int w = 0; w < GP4Q_SLOTS; ++w) {
                block_of_slot[w] = -1;
                if (g.pos[w] < 0) continue;
                long& at = g.ring[(size_t)act * GP4Q_CAP + g.pos[w]];
                if (at < 0) return fail("popped an empty ring position", act, g.pos[w]);
                block_of_slot[w] = at;
                at = -1;
                ++filled;
            }
            counts.flush_partial += filled < GP4Q_SLOTS;
        }
        if (!filled) return fail("composite tile without a block", act);
        counts.composites[(size_t)act] += 1;
        for (int w = 0; w < GP4Q_SLOTS; ++w) {
            const long b = block_of_slot[w];
            if (b < 0) continue;
            if (panels_done[(size_t)b] != act) return fail("panel out of order", b, act);
            panels_done[(size_t)b] += 1;
        }
        const int done = act + 1;
        int rank = 0;
        for (int w = 0; w < GP4Q_SLOTS; ++w) {
            const long b = block_of_slot[w];
            if (b < 0) continue;
            if (!(done < stages && leave[(size_t)b] > done)) continue;
            const int at = gp4q_push_pos(g.q, done, rank++);
            if (at < 0 || at >= GP4Q_CAP) return fail("ring position out of range", at);
            if (g.ring[(size_t)done * GP4Q_CAP + at] >= 0) return fail("ring position handed out twice", done, at);
            g.ring[(size_t)done * GP4Q_CAP + at] = b;
            g.open[w] = 1;
        }
        g.push_stage = done;
    }
    for (size_t r = 0; r < drawn.size(); ++r)
        if (!drawn[r]) return fail("a record never entered panel 0", (long)r);
    return 0;
}

static int simulate(int stages, const std::vector<int>& leave, long long seg, int nwg, unsigned seed) {
    if (stages < 1 || stages > GP4Q_STAGES) return fail("stages out of range", stages);
    if (seg < 1 || nwg < 1) return fail("bad segment size or workgroup count", (long)seg, nwg);
    const long long ntiles = (long long)leave.size() / 4;
    std::mt19937 rng(seed);
    std::vector<int> panels_done(leave.size(), 0);
    std::vector<char> tile_seen((size_t)ntiles, 0);
    Counts counts;
    counts.composites.assign((size_t)stages, 0);
    const long long nseg = gp4l_segments(ntiles, seg);
    for (long long k = 0; k < nseg; ++k) {
        const long long t0 = gp4l_segment_first(seg, k), nt = gp4l_segment_count(ntiles, seg, k);
        if (nt < 1 || nt > seg || t0 + nt > ntiles) return fail("bad segment", (long)t0, (long)nt);
        std::vector<long> list;
        for (long long t = t0; t < t0 + nt; ++t) {
            if (tile_seen[(size_t)t]) return fail("a tile in two segments", (long)t);
            tile_seen[(size_t)t] = 1;
            for (int w = 0; w < 4; ++w)
                if (leave[(size_t)(4 * t + w)] > 0) list.push_back((long)(4 * t + w));
        }
        if ((long long)list.size() > GP4Q_SLOTS * seg) return fail("list over its capacity", (long)list.size());
        std::shuffle(list.begin(), list.end(), rng);                // the order of the list is free
        counts.segments += 1;
        counts.records += (long)list.size();
        if (run_segment(stages, leave, list, nwg, panels_done, rng, counts)) return 1;
    }
    if (gp4l_segment_count(ntiles, seg, nseg) != 0) return fail("tiles behind the last segment");
    for (long long t = 0; t < ntiles; ++t)
        if (!tile_seen[(size_t)t]) return fail("a tile in no segment", (long)t);
    long work = 0;
    for (size_t b = 0; b < leave.size(); ++b) {
        const int want = leave[b] < 0 ? 0 : (leave[b] < stages ? leave[b] : stages);
        if (panels_done[b] != want) return fail("block ran the wrong number of panels", (long)b, panels_done[b]);
        work += want;
    }
    std::printf("ok tiles=%lld stages=%d segments=%ld records=%ld draws=%ld partial_draws=%ld block_panels=%ld "
                "flush_partial=%ld composites=", ntiles, stages, counts.segments, counts.records, counts.draws,
                counts.partial_draws, work, counts.flush_partial);
    for (int s = 0; s < stages; ++s) std::printf("%s%ld", s ? "," : "", counts.composites[(size_t)s]);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && !std::strcmp(argv[1], "random")) {
        const unsigned seed = (unsigned)std::atol(argv[2]);
        std::mt19937 rng(seed);
        const long tiles = std::atol(argv[3]);
        const int stages = std::atoi(argv[4]);
        std::vector<int> leave((size_t)tiles * 4);
        // phases of different character: mostly decided by the mean, mostly open, ragged tiles
        for (size_t b = 0; b < leave.size(); ++b) {
            const int phase = (int)((b / 4) * 5 / (size_t)(tiles ? tiles : 1));
            const unsigned r = rng();
            int v = (int)(r % (unsigned)(stages + 1));
            if (phase == 1) v = (r >> 8) % 4 ? 0 : v;
            if (phase == 2) v = (r >> 8) % 4 ? stages : v;
            if (phase == 3 && (r >> 16) % 5 == 0) v = -1;
            leave[b] = v;
        }
        return simulate(stages, leave, std::atoll(argv[5]), std::atoi(argv[6]), seed + 1);
    }
    if (argc == 5 && !std::strcmp(argv[1], "file")) {
        std::FILE* f = std::fopen(argv[2], "r");
        if (!f) return fail("cannot open the sequence file");
        int stages = 0;
        long blocks = 0;
        if (std::fscanf(f, "%d %ld", &stages, &blocks) != 2 || blocks < 0 || blocks % 4) {
            std::fclose(f);
            return fail("bad header");
        }
        std::vector<int> leave((size_t)blocks);
        for (long b = 0; b < blocks; ++b)
            if (std::fscanf(f, "%d", &leave[(size_t)b]) != 1) {
                std::fclose(f);
                return fail("short sequence file", b);
            }
        std::fclose(f);
        return simulate(stages, leave, std::atoll(argv[3]), std::atoi(argv[4]), 7u);
    }
    if (argc == 3 && !std::strcmp(argv[1], "lengths")) {
        // one segment whose list has exactly n records: 0, 1, 4 k and 4 k + 1 among them
        const int stages = std::atoi(argv[2]);
        // the segment size of a scratch budget: 512 MiB of means and 8 MiB of first cells at d = 4
        if (gp4l_segment_tiles(520LL << 20, 4) != 1LL << 18) return fail("segment size at d = 4");
        for (int d = 1; d <= 6; ++d) {
            const long long s = gp4l_segment_tiles(520LL << 20, d), per_tile = 4 * (16LL * d * 8 + 8);
            if (s * per_tile > (520LL << 20) || 2 * s * per_tile <= (520LL << 20)) return fail("segment size", d, (long)s);
        }
        if (gp4l_segment_tiles(1, 4) != 1) return fail("segment size of a tiny budget");
        for (long n : {0L, 1L, 2L, 3L, 4L, 5L, 8L, 9L, 64L, 65L}) {
            std::vector<int> leave(4 * 20, 0);
            for (long b = 0; b < n; ++b) leave[(size_t)b] = 1 + (int)(b % stages);
            if (gp4l_draws(n) != (n + 3) / 4) return fail("draws of a list", n);
            for (int nwg : {1, 3})
                if (simulate(stages, leave, 20, nwg, (unsigned)n)) return 1;
        }
        return 0;
    }
    std::fprintf(stderr, "usage: gp4_list_sim random <seed> <tiles> <stages> <segment> <workgroups> | "
                         "file <path> <segment> <workgroups> | lengths <stages>\n");
    return 2;
}
