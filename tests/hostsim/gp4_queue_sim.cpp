// gp4_queue_sim.cpp - stand-alone host program that drives sl_gp4_queue.h the way one workgroup of
// k_gp_sweep4<.., EARLY = true> does: source tiles of four 16-cell blocks, each block open until a
// given stage, composite tiles of four queued blocks, the flush at the end.
//
//   gp4_queue_sim random <seed> <tiles> <stages>     random open / decide sequences
//   gp4_queue_sim file <path>                        "<stages> <blocks>" then one leave-stage per block
//                                                    (-1: the block does not exist, >= stages: never
//                                                    decided before the last panel), four per tile
//
// Checks: every block runs the panels 0 .. leave - 1 exactly once each and in order, no queue ever
// holds more than GP4Q_MAX_FILL records, no ring position is handed out twice, and the flush
// leaves every queue empty.  Prints one line of counts; exit status 1 with a message otherwise.
// (tests/test_gp4_queue_host.py builds it with -fsanitize=address,undefined.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sl_gp4_queue.h"

static int fail(const char* what, long a = 0, long b = 0) {
    std::fprintf(stderr, "gp4_queue_sim: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

static int simulate(int stages, const std::vector<int>& leave) {
    if (stages < 1 || stages > GP4Q_STAGES) return fail("stages out of range", stages);
    const long ntiles = (long)leave.size() / 4;
    std::vector<int> panels_done(leave.size(), 0);
    // what the kernel keeps in the workgroup's scratch: the block at every ring position
    std::vector<long> ring((size_t)stages * GP4Q_CAP, -1);
    Gp4Queues q;
    gp4q_init(q);
    int src_done = 0, pos[GP4Q_SLOTS];
    long next_tile = 0, tile = 0;
    std::vector<long> composites(stages, 0), partial(stages, 0);
    int open[GP4Q_SLOTS] = {0, 0, 0, 0}, push_stage = 0;
    long block_of_slot[GP4Q_SLOTS];
    for (long pass = 0;; ++pass) {
        if (pass > 64 * (long)leave.size() + 64) return fail("the loop does not end", pass);
        int n = 0;
        for (int w = 0; w < GP4Q_SLOTS; ++w) { n += open[w]; open[w] = 0; }
        if (n && !gp4q_push(q, push_stage, n)) return fail("queue over capacity", push_stage, q.count[push_stage] + n);
        const int act = gp4q_schedule(q, stages, src_done, pos, [&]() {
            if (next_tile >= ntiles) return false;
            tile = next_tile++;
            return true;
        });
        if (act == GP4Q_DONE) break;
        for (int s = 0; s < stages; ++s)
            if (q.count[s] > GP4Q_MAX_FILL) return fail("queue over capacity", s, q.count[s]);
        int done;
        if (act == GP4Q_SOURCE) {
            for (int w = 0; w < GP4Q_SLOTS; ++w) block_of_slot[w] = leave[4 * tile + w] >= 0 ? 4 * tile + w : -1;
            done = 0;
        } else {
            int filled = 0;
            for (int w = 0; w < GP4Q_SLOTS; ++w) {
                block_of_slot[w] = -1;
                if (pos[w] < 0) continue;
                long& at = ring[(size_t)act * GP4Q_CAP + pos[w]];
                if (at < 0) return fail("popped an empty ring position", act, pos[w]);
                block_of_slot[w] = at;
                at = -1;
                ++filled;
                if (panels_done[block_of_slot[w]] != act) return fail("panel out of order", block_of_slot[w], act);
                panels_done[block_of_slot[w]] += 1;
            }
            if (!filled) return fail("composite tile without a block", act);
            composites[act] += 1;
            partial[act] += filled < GP4Q_SLOTS;
            done = act + 1;
        }
        // every slot decides; the open ones are written to the ring positions of their ranks
        int rank = 0;
        for (int w = 0; w < GP4Q_SLOTS; ++w) {
            const long b = block_of_slot[w];
            if (b < 0) continue;
            const bool still_open = done < stages && leave[b] > done;
            if (!still_open) continue;
            const int at = gp4q_push_pos(q, done, rank++);
            if (at < 0 || at >= GP4Q_CAP) return fail("ring position out of range", at);
            if (ring[(size_t)done * GP4Q_CAP + at] >= 0) return fail("ring position handed out twice", done, at);
            ring[(size_t)done * GP4Q_CAP + at] = b;
            open[w] = 1;
        }
        push_stage = done;
    }
    if (!gp4q_empty(q, stages)) return fail("queues not empty after the flush");
    if (next_tile != ntiles) return fail("source tiles left", next_tile, ntiles);
    for (long at : ring) if (at >= 0) return fail("a record was left in a ring", at);
    long work = 0;
    for (size_t b = 0; b < leave.size(); ++b) {
        const int want = leave[b] < 0 ? 0 : (leave[b] < stages ? leave[b] : stages);
        if (panels_done[b] != want) return fail("block ran the wrong number of panels", (long)b, panels_done[b]);
        work += want;
    }
    std::printf("ok tiles=%ld stages=%d block_panels=%ld composites=", ntiles, stages, work);
    for (int s = 0; s < stages; ++s) std::printf("%s%ld", s ? "," : "", composites[s]);
    std::printf(" partial=");
    for (int s = 0; s < stages; ++s) std::printf("%s%ld", s ? "," : "", partial[s]);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "random")) {
        std::mt19937 rng((unsigned)std::atol(argv[2]));
        const long tiles = std::atol(argv[3]);
        const int stages = std::atoi(argv[4]);
        std::vector<int> leave((size_t)tiles * 4);
        // phases of different character: mostly decided early, mostly open, ragged tiles
        for (size_t b = 0; b < leave.size(); ++b) {
            const int phase = (int)((b / 4) * 5 / (tiles ? tiles : 1));
            const unsigned r = rng();
            int v = (int)(r % (unsigned)(stages + 1));
            if (phase == 1) v = (r >> 8) % 4 ? 0 : v;
            if (phase == 2) v = (r >> 8) % 4 ? stages : v;
            if (phase == 3 && (r >> 16) % 5 == 0) v = -1;
            leave[b] = v;
        }
        return simulate(stages, leave);
    }
    if (argc == 3 && !std::strcmp(argv[1], "file")) {
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
        return simulate(stages, leave);
    }
    std::fprintf(stderr, "usage: gp4_queue_sim random <seed> <tiles> <stages> | file <path>\n");
    return 2;
}
