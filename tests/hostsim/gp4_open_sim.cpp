// gp4_open_sim.cpp - the open-block list of a segmented block-mode GP sweep on the host: the rule of
// sl_gp4_open.h driven chunk by chunk the way k_gp_open_count and k_gp_open_scatter
// (sl_gp4_predecide.hip) drive it - one "workgroup" per chunk of tiles, 256 "lanes" that take one
// 32-bit word of four tile bytes a round, the count of every chunk first, then every chunk's entries
// behind the sum of the counts of the chunks before it.
//
//     gp4_open_sim BYTES NTILES LIST
//
// BYTES: a file of NTILES tile bytes (bit jb = block jb decided).  LIST: written, the list as 32-bit
// block numbers.  Prints "ok ntiles=N chunks=C length=L"; exit status 1 when the two passes
// disagree, an entry does not stand at its rank or the list leaves its allocation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sl_gp4_open.h"

namespace {

constexpr int LANES = 256;
constexpr int ROUNDS = gp4o::CHUNK_TILES / (4 * LANES);

int fail(const char* what, long long a, long long b) {
    std::printf("FAILED: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

// the word the lane of round r of a chunk loads, and its open mask (lane_mask of the kernels)
uint32_t lane_mask(const std::vector<unsigned char>& padded, long long ntiles, long long chunk, int r, int lane,
                   long long& t) {
    t = chunk * gp4o::CHUNK_TILES + 4 * (long long)(r * LANES + lane);
    if (t >= ntiles) return 0u;
    uint32_t word;
    std::memcpy(&word, padded.data() + t, 4);                 // (little endian, like the device)
    const long long left = ntiles - t;
    return gp4o::open_mask16(word, left < 4 ? (int)left : 4);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) return fail("usage: gp4_open_sim BYTES NTILES LIST", argc, 0);
    const long long ntiles = std::atoll(argv[2]);
    if (ntiles < 1) return fail("ntiles", ntiles, 0);
    // the device allocation: exactly the bytes of the tiles and the four behind them that a word may read
    std::vector<unsigned char> padded((size_t)ntiles + 4, 0xa5);
    {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) return fail("cannot open the bytes", 0, 0);
        const size_t got = std::fread(padded.data(), 1, (size_t)ntiles, f);
        std::fclose(f);
        if (got != (size_t)ntiles) return fail("short file", (long long)got, ntiles);
    }
    if (gp4o::tile_bytes(ntiles) < (size_t)ntiles + 4) return fail("tile_bytes", (long long)gp4o::tile_bytes(ntiles), ntiles);
    const long long nchunks = gp4o::chunks(ntiles);
    if (gp4o::count_bytes(ntiles) < (size_t)nchunks * 4) return fail("count_bytes", nchunks, 0);
    // pass 1: the count of every chunk, by words - and by the bytes of the chunk, which must agree
    std::vector<uint32_t> counts((size_t)nchunks);
    for (long long c = 0; c < nchunks; ++c) {
        uint32_t n = 0;
        for (int r = 0; r < ROUNDS; ++r)
            for (int lane = 0; lane < LANES; ++lane) {
                long long t;
                n += (uint32_t)gp4o::popcount32(lane_mask(padded, ntiles, c, r, lane, t));
            }
        const long long first = c * gp4o::CHUNK_TILES;
        const long long len = ntiles - first < gp4o::CHUNK_TILES ? ntiles - first : gp4o::CHUNK_TILES;
        if (n != gp4o::open_count(padded.data() + first, len)) return fail("count of a chunk", c, n);
        counts[(size_t)c] = n;
    }
    // pass 2: every chunk on its own - the counts before it, then a scan over the lanes of each round
    const size_t cap = 4 * (size_t)ntiles;                   // entries the allocation holds (16 bytes per tile)
    std::vector<uint32_t> list(cap, 0xffffffffu);
    std::vector<unsigned char> written(cap, 0);
    unsigned long long length = 0;
    for (long long c = 0; c < nchunks; ++c) {
        uint32_t base = 0;
        for (long long b = 0; b < c; ++b) base += counts[(size_t)b];
        for (int r = 0; r < ROUNDS; ++r) {
            uint32_t before = 0;                             // exclusive scan over the round's lanes
            for (int lane = 0; lane < LANES; ++lane) {
                long long t;
                uint32_t m = lane_mask(padded, ntiles, c, r, lane, t);
                uint32_t at = base + before;
                before += (uint32_t)gp4o::popcount32(m);
                while (m) {
                    const int i = __builtin_ctz(m);
                    m &= m - 1u;
                    if (at >= cap) return fail("entry outside the list", at, (long long)cap);
                    if (written[at]) return fail("position written twice", at, 0);
                    list[at] = (uint32_t)(4 * t) + (uint32_t)i;
                    written[at] = 1;
                    ++at;
                }
            }
            base += before;
        }
        if (c == nchunks - 1) length = base;
    }
    // every entry at its rank (counts before its chunk + open_rank inside it), nothing else written
    {
        std::vector<uint32_t> start((size_t)nchunks, 0);
        for (long long c = 1; c < nchunks; ++c) start[(size_t)c] = start[(size_t)c - 1] + counts[(size_t)c - 1];
        for (unsigned long long at = 0; at < cap; ++at) {
            if ((at < length) != (written[at] != 0)) return fail("written positions are not [0, length)", (long long)at, (long long)length);
            if (at >= length) continue;
            const long long tile = list[at] / 4, c = tile / gp4o::CHUNK_TILES;
            if (tile >= ntiles) return fail("entry beyond the shard", (long long)at, tile);
            const uint32_t want = start[(size_t)c] + gp4o::open_rank(padded.data() + c * gp4o::CHUNK_TILES,
                                                                      tile - c * gp4o::CHUNK_TILES, (int)(list[at] & 3u));
            if (want != at) return fail("entry not at its rank", (long long)at, want);
            if (!((gp4o::open_nibble(padded[(size_t)tile]) >> (list[at] & 3u)) & 1u)) return fail("entry of a decided block", (long long)at, tile);
        }
    }
    {
        std::FILE* f = std::fopen(argv[3], "wb");
        if (!f) return fail("cannot write the list", 0, 0);
        const size_t put = std::fwrite(list.data(), 4, (size_t)length, f);
        std::fclose(f);
        if (put != (size_t)length) return fail("short write", (long long)put, (long long)length);
    }
    std::printf("ok ntiles=%lld chunks=%lld length=%llu\n", ntiles, nchunks, length);
    return 0;
}
