// gp4_halves_sim.cpp - stand-alone host program that drives sl_gp4_halves.h the way one workgroup of
// k_gp_sweep4<.., EARLY = true> does: 16-cell blocks whose two 8-cell halves stay open until a given
// stage each, rings of full records, low halves and high halves per stage, composite tiles of four
// full slots or four paired slots, the flush at the end.
//
//   gp4_halves_sim random <seed> <tiles> <stages> <mode>
//   gp4_halves_sim file <path> <mode>      "<stages> <blocks>" then TWO leave-stages per block (low
//                                          half, high half; -1 -1: the block does not exist; >= stages:
//                                          never decided before the last panel), four blocks per tile
// mode:  kernel   source tiles in the panel kernel itself (small launches): every half is decided
//                 before panel 0 and enters the rings of stage 0 by its code
//        list     the source pass ran in k_gp_mean_blocks: a block it left open (either half) is a
//                 record of the list, four records a draw, and runs panel 0 as a full slot
//        blocks   as kernel, but one verdict per block (SL_GP4_HALVES=0): only full rings are used
//
// Checks: every half runs the panels it reaches exactly once each and in order; a paired slot holds
// a low-half record beside a high-half record and a full slot a full record, never a mix in one
// composite; no ring position is handed out twice; no ring exceeds its fill; the flush leaves every
// ring empty.  Prints one line of counts; exit status 1 with a message otherwise.
// (tests/test_gp4_halves_host.py builds it with -fsanitize=address,undefined.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sl_gp4_halves.h"

static int fail(const char* what, long a = 0, long b = 0) {
    std::fprintf(stderr, "gp4_halves_sim: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

enum Mode { KERNEL, LIST, BLOCKS };
struct Rec { long block; int live; };

static int simulate(int stages, const std::vector<int>& leave, Mode mode) {
    if (stages < 1 || stages > GP4Q_STAGES) return fail("stages out of range", stages);
    const long nblocks = (long)leave.size() / 2, ntiles = nblocks / 4;
    auto clamp = [&](int v) { return v < 0 ? 0 : (v < stages ? v : stages); };
    std::vector<int> done_panels(leave.size(), 0);
    std::vector<Rec> ring((size_t)stages * GP4H_RECS, Rec{-1, 0});
    std::vector<long> list;                                 // LIST: the blocks the mean kernel left open
    if (mode == LIST)
        for (long b = 0; b < nblocks; ++b)
            if (leave[2 * b] > 0 || leave[2 * b + 1] > 0) list.push_back(b);
    const long nsource = mode == LIST ? (long)gp4l_draws((long long)list.size()) : ntiles;
    Gp4HalfQueues q;
    gp4h_init(q);
    int src_done = 0, pos[GP4Q_SLOTS], posb[GP4Q_SLOTS], paired = 0;
    long next_tile = 0, tile = 0;
    std::vector<long> full(stages, 0), pairs(stages, 0), lone(stages, 0), partial(stages, 0), slots(stages, 0);
    int open[GP4H_RINGS][GP4Q_SLOTS] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, push_stage = 0;
    for (long pass = 0;; ++pass) {
        if (pass > 128 * (long)leave.size() + 64) return fail("the loop does not end", pass);
        for (int r = 0; r < GP4H_RINGS; ++r) {
            int n = 0;
            for (int w = 0; w < GP4Q_SLOTS; ++w) { n += open[r][w]; open[r][w] = 0; }
            if (n && !gp4h_push(q, push_stage, r, n)) return fail("ring over capacity", push_stage, r);
        }
        int act = gp4h_schedule(q, stages, src_done, pos, posb, paired, [&]() {
            if (next_tile >= nsource) return false;
            tile = next_tile++;
            return true;
        });
        if (act == GP4Q_DONE) break;
        for (int s = 0; s < stages; ++s)
            for (int r = 0; r < GP4H_RINGS; ++r)
                if (q.count[s][r] > gp4h_max_fill(r)) return fail("ring over capacity", s, r);
        // what the four slots hold: record a (full, or the low half) and record b (the high half)
        Rec a[GP4Q_SLOTS], b[GP4Q_SLOTS];
        for (int w = 0; w < GP4Q_SLOTS; ++w) a[w] = b[w] = Rec{-1, 0};
        int done;
        if (act == GP4Q_SOURCE && mode != LIST) {
            for (int w = 0; w < GP4Q_SLOTS; ++w)
                if (leave[2 * (4 * tile + w)] >= 0) a[w] = Rec{4 * tile + w, GP4H_BOTH};
            done = 0;
        } else {
            int filled = 0;
            const bool listed = act == GP4Q_SOURCE;
            if (listed) {
                act = 0;
                for (int w = 0; w < GP4Q_SLOTS; ++w) {
                    const long long r = gp4l_slot(tile, w, (long long)list.size());
                    if (r >= 0) a[w] = Rec{list[(size_t)r], GP4H_BOTH};
                }
            } else {
                for (int w = 0; w < GP4Q_SLOTS; ++w) {
                    if (pos[w] >= 0) {
                        const int r = paired ? GP4H_RING_LOW : GP4H_RING_FULL;
                        if (pos[w] >= gp4h_cap(r)) return fail("ring position out of range", r, pos[w]);
                        Rec& at = ring[(size_t)act * GP4H_RECS + gp4h_base(r) + pos[w]];
                        if (at.block < 0) return fail("popped an empty ring position", act, pos[w]);
                        if (at.live != (paired ? GP4H_LOW : GP4H_BOTH)) return fail("wrong kind of record in a slot", act, at.live);
                        a[w] = at;
                        at = Rec{-1, 0};
                    }
                    if (posb[w] >= 0) {
                        if (!paired) return fail("a full slot with a second record", act, w);
                        if (posb[w] >= gp4h_cap(GP4H_RING_HIGH)) return fail("ring position out of range", 2, posb[w]);
                        Rec& at = ring[(size_t)act * GP4H_RECS + gp4h_base(GP4H_RING_HIGH) + posb[w]];
                        if (at.block < 0) return fail("popped an empty ring position", act, posb[w]);
                        if (at.live != GP4H_HIGH) return fail("wrong kind of record in a slot", act, at.live);
                        b[w] = at;
                        at = Rec{-1, 0};
                    }
                }
            }
            for (int w = 0; w < GP4Q_SLOTS; ++w) {
                for (const Rec* r : {&a[w], &b[w]}) {
                    if (r->block < 0) continue;
                    for (int h = 0; h < 2; ++h) {
                        if (!((r->live >> h) & 1)) continue;
                        int& n = done_panels[2 * r->block + h];
                        if (n != act) return fail("panel out of order", r->block, act);
                        n += 1;
                    }
                }
                const bool any = a[w].block >= 0 || b[w].block >= 0;
                filled += any;
                slots[act] += any;
                if (paired && any && (a[w].block < 0 || b[w].block < 0)) lone[act] += 1;
                if (a[w].block >= 0 && a[w].block == b[w].block) return fail("both halves of a block paired in one slot: it should be a full record", a[w].block);
            }
            if (!filled) return fail("composite tile without a record", act);
            (paired ? pairs : full)[act] += 1;
            partial[act] += filled < GP4Q_SLOTS;
            done = act + 1;
        }
        // every slot decides per half; what stays open is written to the ring of its code
        int rank[GP4H_RINGS] = {0, 0, 0};
        auto put = [&](int w, long block, int live) -> int {
            const int r = gp4h_ring_of(live);
            const int at = gp4h_push_pos(q, done, r, rank[r]++);
            if (at < 0 || at >= gp4h_cap(r)) return fail("ring position out of range", r, at);
            Rec& to = ring[(size_t)done * GP4H_RECS + gp4h_base(r) + at];
            if (to.block >= 0) return fail("ring position handed out twice", done, at);
            to = Rec{block, live};
            if (open[r][w]) return fail("a slot pushes twice onto one ring", w, r);
            open[r][w] = 1;
            return 0;
        };
        for (int w = 0; w < GP4Q_SLOTS; ++w) {
            int still_a = 0, still_b = 0;
            auto still_of = [&](const Rec& r) {
                int still = 0;
                if (r.block < 0 || done >= stages) return 0;
                for (int h = 0; h < 2; ++h)
                    if (((r.live >> h) & 1) && leave[2 * r.block + h] > done) still |= 1 << h;
                if (mode == BLOCKS && still) still = r.live;
                return still;
            };
            still_a = still_of(a[w]);
            still_b = still_of(b[w]);
            if (!paired && still_a == GP4H_BOTH) {
                if (put(w, a[w].block, GP4H_BOTH)) return 1;
            } else {
                if ((still_a & GP4H_LOW) && put(w, a[w].block, GP4H_LOW)) return 1;
                if ((still_a & GP4H_HIGH) && put(w, a[w].block, GP4H_HIGH)) return 1;
                if ((still_b & GP4H_HIGH) && put(w, b[w].block, GP4H_HIGH)) return 1;
                if (still_b & GP4H_LOW) return fail("a high-half record with an open low half", b[w].block);
            }
        }
        push_stage = done;
    }
    if (!gp4h_empty(q, stages)) return fail("rings not empty after the flush");
    if (next_tile != nsource) return fail("source tiles left", next_tile, nsource);
    for (const Rec& at : ring) if (at.block >= 0) return fail("a record was left in a ring", at.block);
    long work = 0;
    for (long blk = 0; blk < nblocks; ++blk) {
        const int lo = clamp(leave[2 * blk]), hi = clamp(leave[2 * blk + 1]);
        for (int h = 0; h < 2; ++h) {
            int want = h ? hi : lo;
            if (mode == BLOCKS) want = lo > hi ? lo : hi;
            if (mode == LIST && (lo > 0 || hi > 0) && want < 1) want = 1;    // panel 0 ran on the whole block
            if (done_panels[2 * blk + h] != want) return fail("a half ran the wrong number of panels", blk, done_panels[2 * blk + h]);
            work += want;
        }
    }
    auto row = [&](const char* name, const std::vector<long>& v) {
        std::printf(" %s=", name);
        for (int s = 0; s < stages; ++s) std::printf("%s%ld", s ? "," : "", v[s]);
    };
    std::printf("ok tiles=%ld stages=%d half_panels=%ld", ntiles, stages, work);
    row("full", full);
    row("paired", pairs);
    row("lone", lone);
    row("partial", partial);
    row("slots", slots);
    std::printf("\n");
    return 0;
}

static bool mode_of(const char* text, Mode& mode) {
    if (!std::strcmp(text, "kernel")) mode = KERNEL;
    else if (!std::strcmp(text, "list")) mode = LIST;
    else if (!std::strcmp(text, "blocks")) mode = BLOCKS;
    else return false;
    return true;
}

int main(int argc, char** argv) {
    Mode mode = KERNEL;
    if (argc == 6 && !std::strcmp(argv[1], "random") && mode_of(argv[5], mode)) {
        std::mt19937 rng((unsigned)std::atol(argv[2]));
        const long tiles = std::atol(argv[3]);
        const int stages = std::atoi(argv[4]);
        std::vector<int> leave((size_t)tiles * 8);
        // phases of different character: mostly decided early, mostly open, ragged tiles, halves
        // that mostly leave together, and a stretch in which only LOW halves stay (the imbalance
        // that fills one half ring)
        for (size_t b = 0; b < leave.size() / 2; ++b) {
            const int phase = (int)((b / 4) * 6 / (tiles ? tiles : 1));
            int v[2];
            for (int h = 0; h < 2; ++h) {
                const unsigned r = rng();
                v[h] = (int)(r % (unsigned)(stages + 1));
                if (phase == 1) v[h] = (r >> 8) % 4 ? 0 : v[h];
                if (phase == 2) v[h] = (r >> 8) % 4 ? stages : v[h];
            }
            const unsigned r = rng();
            if (phase == 4 && r % 8) v[1] = v[0];
            if (phase == 5) v[1] = r % 16 ? 0 : v[1];
            if (phase == 3 && (r >> 16) % 5 == 0) v[0] = v[1] = -1;
            leave[2 * b] = v[0];
            leave[2 * b + 1] = v[1];
        }
        return simulate(stages, leave, mode);
    }
    if (argc == 4 && !std::strcmp(argv[1], "file") && mode_of(argv[3], mode)) {
        std::FILE* f = std::fopen(argv[2], "r");
        if (!f) return fail("cannot open the sequence file");
        int stages = 0;
        long blocks = 0;
        if (std::fscanf(f, "%d %ld", &stages, &blocks) != 2 || blocks < 0 || blocks % 4) {
            std::fclose(f);
            return fail("bad header");
        }
        std::vector<int> leave((size_t)blocks * 2);
        for (size_t i = 0; i < leave.size(); ++i)
            if (std::fscanf(f, "%d", &leave[i]) != 1) {
                std::fclose(f);
                return fail("short sequence file", (long)i);
            }
        std::fclose(f);
        for (long b = 0; b < blocks; ++b)
            if ((leave[2 * b] < 0) != (leave[2 * b + 1] < 0)) return fail("half a block does not exist", b);
        return simulate(stages, leave, mode);
    }
    std::fprintf(stderr, "usage: gp4_halves_sim random <seed> <tiles> <stages> <mode> | file <path> <mode>"
                         "   (mode: kernel | list | blocks)\n");
    return 2;
}
