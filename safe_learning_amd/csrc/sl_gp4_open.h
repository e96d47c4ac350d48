// sl_gp4_open.h - the rule of the open-block list of a segmented block-mode GP sweep: which 16-cell
// blocks k_gp_predecide (sl_gp4_predecide.hip) has left open, how many a run of tile bytes holds and
// where a block stands in the list.  k_gp_open_count / k_gp_open_scatter (sl_gp4_predecide.hip)
// build the list with these functions, k_gp_mean_open (sl_gp4_mean.hip) works through it.
//
// The pass writes one byte per 64-cell tile of the shard, bit jb = block jb is decided; it also marks
// the blocks that lie wholly at or beyond `hi`, so a CLEAR bit is the whole rule.  The list holds the
// 32-bit block numbers 4 tile + jb of the open blocks in ascending order (the block's first cell is
// lo + 16 (4 tile + jb)).  It is an ordered compaction in two passes over chunks of CHUNK_TILES
// tiles with no waiting between workgroups: the count of every chunk, then every chunk's entries
// at the sum of the counts before it.  Inside a chunk the bytes are taken four at a time, as the
// 32-bit words the kernels load: bit 4 k + jb of a word's open mask is block jb of its tile k, which
// is block number 4 (first tile of the word) + (4 k + jb).
//
// Plain C++ on integers: g++ compiles it for the host tests, which drive it from a stand-alone program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef SL_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SL_HD __host__ __device__ __forceinline__
#else
#define SL_HD inline
#endif
#endif

namespace gp4o {

constexpr int CHUNK_TILES = 4096;        // tiles per workgroup of the two list kernels (four words a lane)
constexpr int HEAD_BYTES = 64;           // the list's head, in front of the tile bytes
// 64-bit words of the head: the list's length, the tiles of the shard it was built for, 1 = built
constexpr int HEAD_LENGTH = 0, HEAD_NTILES = 1, HEAD_BUILT = 2;

SL_HD int popcount32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// the open blocks of a tile: bit jb of the result = block jb is open
SL_HD uint32_t open_nibble(uint32_t byte) { return ~byte & 15u; }

// the open mask of a word of four tile bytes (little endian: byte k = tile k of the word) of which
// the first `valid` (<= 4) are tiles of the shard; the others read as decided
SL_HD uint32_t open_mask16(uint32_t word, int valid) {
    uint32_t m = 0u;
    for (int k = 0; k < 4; ++k)
        if (k < valid) m |= open_nibble((word >> (8 * k)) & 255u) << (4 * k);
    return m;
}

// open blocks of a run of n tile bytes
SL_HD uint32_t open_count(const unsigned char* bytes, long long n) {
    uint32_t c = 0u;
    for (long long t = 0; t < n; ++t) c += (uint32_t)popcount32(open_nibble(bytes[t]));
    return c;
}

// rank of block jb of tile t of a chunk (bytes: the chunk's first byte) among the chunk's open blocks:
// the open blocks in front of it
SL_HD uint32_t open_rank(const unsigned char* bytes, long long t, int jb) {
    return open_count(bytes, t) + (uint32_t)popcount32(open_nibble(bytes[t]) & ((1u << jb) - 1u));
}

SL_HD long long chunks(long long ntiles) { return (ntiles + CHUNK_TILES - 1) / CHUNK_TILES; }
// bytes of d_gp4_pre behind the lattice table: head, tile bytes (read as words), chunk counts, list
// (the worst case: every block open); each part on a 16-byte boundary
SL_HD size_t tile_bytes(long long ntiles) { return ((size_t)ntiles + 4 + 15) & ~(size_t)15; }
SL_HD size_t count_bytes(long long ntiles) { return ((size_t)chunks(ntiles) * 4 + 15) & ~(size_t)15; }
SL_HD size_t total_bytes(long long ntiles) {
    return HEAD_BYTES + tile_bytes(ntiles) + count_bytes(ntiles) + 16 * (size_t)ntiles;
}

}  // namespace gp4o
