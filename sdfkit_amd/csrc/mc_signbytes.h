// mc_signbytes.h -- the bit logic of the ordered compaction's count pass as pure functions of sign words and sign bytes: which
// cells of a 64-cell segment are active (segment_mask), and how a lane of k_count_bytes (mc_kernels.hip) turns the sampler's byte
// form bits8[y][x/8][z] into the X-packed words of eight consecutive sign planes without the transposer pass.  Included by
// mc_kernels.hip; like mc_decide.h the qualifiers (__device__, __forceinline__) come from whoever includes this file:
// <hip/hip_runtime.h> in the product, tests/cpp/signbytes_host.cpp defines them away to run the very same text on the host
// (tests/test_signbytes_host.py).  Nothing here is HIP-specific.
#pragma once
#include <stdint.h>

namespace sdfk {

__device__ __forceinline__ uint64_t shr1_in(uint64_t w, uint64_t next) { return (w >> 1) | (next << 63); }

// activity of the 64 cells x = 64*xw .. 64*xw+63 of one cell row: a/b/c/d = sign words of the
// voxel rows (y,z) (y+1,z) (y,z+1) (y+1,z+1), *n = the following word of the same row.
// `rem` = number of cells of this word that exist (x < ncx); the word after the last one of a
// row may hold anything: it only reaches bit 63, a cell that never exists.
// Corners: v0=a v1=as v2=bs v3=b v4=c v5=cs v6=ds v7=d.  A cell is active when some corner
// differs from v0; its sign word is 0xA5 or 0x5A (case 13) when v1,v3,v4,v6 differ from v0 and
// v2,v5,v7 equal it.
__device__ __forceinline__ uint64_t segment_mask(uint64_t a, uint64_t an, uint64_t b, uint64_t bn, uint64_t c, uint64_t cn,
                                                 uint64_t d, uint64_t dn, int rem, uint64_t& m13)
{
    const uint64_t as = shr1_in(a, an), bs = shr1_in(b, bn), cs = shr1_in(c, cn), ds = shr1_in(d, dn);
    const uint64_t valid = rem >= 64 ? ~0ull : (rem <= 0 ? 0ull : ((1ull << rem) - 1ull));
    const uint64_t x1 = a ^ as, x3 = a ^ b, x4 = a ^ c, x6 = a ^ ds;
    const uint64_t eq = (a ^ bs) | (a ^ cs) | (a ^ d);
    m13 = (x1 & x3 & x4 & x6) & ~eq & valid;
    return (x1 | x3 | x4 | x6 | eq) & valid;
}

// An 8 x 8 byte matrix in eight 64-bit registers, transposed in place: byte j of r[i] <-> byte i of r[j] (three rounds of
// masked exchanges: 32-bit halves, 16-bit pairs, bytes).
// In: r[i] = the eight bytes z .. z+7 of byte row x/8 = 8*xw + i of bits8 (one 8-byte load).  Out: r[j] = the X word xw of
// plane z + j, exactly what k_bits_transpose stores at bits[z + j][y][xw].
__device__ __forceinline__ void signbytes_transpose8(uint64_t r[8])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t t = ((r[i] >> 32) ^ r[i + 4]) & 0x00000000ffffffffull;
        r[i + 4] ^= t;
        r[i] ^= t << 32;
    }
#pragma unroll
    for (int h = 0; h < 8; h += 4)
#pragma unroll
        for (int i = h; i < h + 2; i++) {
            const uint64_t t = ((r[i] >> 16) ^ r[i + 2]) & 0x0000ffff0000ffffull;
            r[i + 2] ^= t;
            r[i] ^= t << 16;
        }
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const uint64_t t = ((r[i] >> 8) ^ r[i + 1]) & 0x00ff00ff00ff00ffull;
        r[i + 1] ^= t;
        r[i] ^= t << 8;
    }
}

// The "next word" input of segment_mask for plane z + j, from the eight bytes z .. z+7 of the FOLLOWING byte row
// (x/8 = 8*(xw+1)): segment_mask only lets bit 0 of that word in (cell 63's x+1 corner), and bit 0 of word xw + 1 is bit 0 of
// that byte.
__device__ __forceinline__ uint64_t signbytes_next(uint64_t following_row, int j) { return (following_row >> (8 * j)) & 1ull; }

// What one lane of k_count_bytes computes.  Voxel rows y (v = 0) and y + 1 (v = 1) of segment column (y, xw), planes z .. z+8:
//   rows[v][0..7]  the 8-byte loads of byte rows 8*xw .. 8*xw+7 (bytes = planes z .. z+7); transposed in place to the words
//   rows[v][8]     the 8-byte load of byte row 8*(xw+1)
//   w8[v], n8[v]   word and next bit of plane z + 8 (the neighbouring lane's plane 0, or the chunk's edge bytes)
// Layers z + j, j < nlayers, get their activity mask m[j] and case-13 mask m13[j]; the others 0.
__device__ __forceinline__ void signbytes_lane_masks(uint64_t rows[2][9], const uint64_t w8[2], const uint64_t n8[2], int rem, int nlayers,
                                                     uint64_t m[8], uint64_t m13[8])
{
    signbytes_transpose8(rows[0]);
    signbytes_transpose8(rows[1]);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t c = j < 7 ? rows[0][j < 7 ? j + 1 : 0] : w8[0], cn = j < 7 ? signbytes_next(rows[0][8], j + 1) : n8[0];
        const uint64_t d = j < 7 ? rows[1][j < 7 ? j + 1 : 0] : w8[1], dn = j < 7 ? signbytes_next(rows[1][8], j + 1) : n8[1];
        uint64_t q13;
        const uint64_t q = segment_mask(rows[0][j], signbytes_next(rows[0][8], j), rows[1][j], signbytes_next(rows[1][8], j), c, cn, d, dn, rem, q13);
        m[j] = j < nlayers ? q : 0ull;
        m13[j] = j < nlayers ? q13 : 0ull;
    }
}

}  // namespace sdfk
