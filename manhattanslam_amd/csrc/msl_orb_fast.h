// msl_orb_fast.h -- the integer pieces of k_fast (msl_orb.hip) on plain values: the quick test of four horizontally adjacent pixels on packed
// 16-bit pairs, and the FAST-9/16 corner score.  No memory access, no HIP call: the kernel hands in what it read from its LDS tile, and a host
// program can call the same functions (tests/fast_host.cpp).  In device code a pair is a 32-bit register and the operations are the packed 16-bit
// instructions (v_pk_min_i16, v_pk_max_i16, v_pk_add_i16, v_pk_sub_i16); host code runs the same expressions on a struct of two shorts.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MSL_FAST_HD __host__ __device__ __forceinline__
#define MSL_FAST_UNROLL _Pragma("unroll")
#else
#define MSL_FAST_HD inline
#define MSL_FAST_UNROLL
#endif

namespace msl {
namespace orb {

#if defined(__HIP_DEVICE_COMPILE__)
typedef short s16x2 __attribute__((ext_vector_type(2)));
MSL_FAST_HD s16x2 pk_make(int lo, int hi) { return (s16x2){(short)lo, (short)hi}; }
MSL_FAST_HD s16x2 pk_min(s16x2 a, s16x2 b) { return __builtin_elementwise_min(a, b); }
MSL_FAST_HD s16x2 pk_max(s16x2 a, s16x2 b) { return __builtin_elementwise_max(a, b); }
MSL_FAST_HD s16x2 pk_add(s16x2 a, s16x2 b) { return a + b; }
MSL_FAST_HD s16x2 pk_sub(s16x2 a, s16x2 b) { return a - b; }
MSL_FAST_HD s16x2 pk_from_bits(uint32_t w) { return __builtin_bit_cast(s16x2, w); }
MSL_FAST_HD uint32_t pk_bits(s16x2 a) { return __builtin_bit_cast(uint32_t, a); }
#else
struct s16x2 { short x, y; };
MSL_FAST_HD s16x2 pk_make(int lo, int hi) { s16x2 r; r.x = (short)lo; r.y = (short)hi; return r; }
MSL_FAST_HD s16x2 pk_min(s16x2 a, s16x2 b) { return pk_make(a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y); }
MSL_FAST_HD s16x2 pk_max(s16x2 a, s16x2 b) { return pk_make(a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y); }
MSL_FAST_HD s16x2 pk_add(s16x2 a, s16x2 b) { return pk_make(a.x + b.x, a.y + b.y); }
MSL_FAST_HD s16x2 pk_sub(s16x2 a, s16x2 b) { return pk_make(a.x - b.x, a.y - b.y); }
MSL_FAST_HD s16x2 pk_from_bits(uint32_t w) { return pk_make((int)(int16_t)(w & 0xFFFFu), (int)(int16_t)(w >> 16)); }
MSL_FAST_HD uint32_t pk_bits(s16x2 a) { return (uint32_t)(uint16_t)a.x | ((uint32_t)(uint16_t)a.y << 16); }
#endif

// Bytes 0, 1 (half = 0) or 2, 3 (half = 1) of a word of four pixels, zero-extended to a 16-bit pair.
MSL_FAST_HD s16x2 fast_pair(uint32_t w, int half) {
    const uint32_t h = half ? w >> 16 : w;
    return pk_from_bits((h & 0xFFu) | ((h & 0xFF00u) << 8));
}

// The four bytes that start n bytes (1..3) into the little-endian byte string lo, hi (one v_alignbyte_b32 / v_perm_b32).
MSL_FAST_HD uint32_t fast_bytes(uint32_t lo, uint32_t hi, int n) { return (lo >> (8 * n)) | (hi << (32 - 8 * n)); }

// Quick rejection (the classic FAST high-speed test on the 4 even opposite pairs) for four horizontally adjacent pixels at once.  c holds
// the four centre pixels, one per byte, and r0, r8, r4, r12, r2, r10, r6, r14 the ring positions of the same name for each of them (ring
// position k as in fast_score16: 0 = three rows down, 4 = three columns right, 8 = three rows up, 12 = three columns left, 2 / 6 / 10 / 14 the
// diagonal (2, 2) offsets between them).  Bit e of the result says that pixel e passes at threshold th (0 <= th <= 16000):
//     bright: every opposite pair has a member with v - ring > th   <=>  v - max over the pairs of min(ring_a, ring_b) > th
//     dark:   every opposite pair has a member with v - ring < -th  <=>  min over the pairs of max(ring_a, ring_b) - v > th
// A 9-arc of 16 contains at least one pixel of every opposite pair, so a pixel whose score reaches th passes; a pixel that fails cannot score
// >= th.  Its score is left 0, which changes neither the threshold tests nor the non-maximum suppression of any kept pixel (a kept pixel
// scores >= th, above every such neighbour either way).
// (one half of it: the pairs of two of the four pixels -> the word whose two sign bits say "passes")
MSL_FAST_HD uint32_t fast_quick_pair(s16x2 v, s16x2 a0, s16x2 a8, s16x2 a4, s16x2 a12, s16x2 a2, s16x2 a10, s16x2 a6, s16x2 a14, s16x2 t) {
    const s16x2 lo = pk_max(pk_max(pk_min(a0, a8), pk_min(a4, a12)), pk_max(pk_min(a2, a10), pk_min(a6, a14)));
    const s16x2 hi = pk_min(pk_min(pk_max(a0, a8), pk_max(a4, a12)), pk_min(pk_max(a2, a10), pk_max(a6, a14)));
    // bright <=> lo + th - v < 0, dark <=> v + th - hi < 0: the sign bits of the two halves
    return pk_bits(pk_sub(pk_add(lo, t), v)) | pk_bits(pk_sub(pk_add(v, t), hi));
}
MSL_FAST_HD unsigned fast_quick_bits(uint32_t sign0, uint32_t sign1) {
    return ((sign0 >> 15) & 1u) | ((sign0 >> 30) & 2u) | ((sign1 >> 13) & 4u) | ((sign1 >> 28) & 8u);
}
MSL_FAST_HD unsigned fast_quick4(uint32_t c, uint32_t r0, uint32_t r8, uint32_t r4, uint32_t r12, uint32_t r2, uint32_t r10, uint32_t r6,
                                 uint32_t r14, int th) {
    const s16x2 t = pk_make(th, th);
    uint32_t sign[2];
    MSL_FAST_UNROLL
    for (int half = 0; half < 2; half++)
        sign[half] = fast_quick_pair(fast_pair(c, half), fast_pair(r0, half), fast_pair(r8, half), fast_pair(r4, half), fast_pair(r12, half),
                                     fast_pair(r2, half), fast_pair(r10, half), fast_pair(r6, half), fast_pair(r14, half), t);
    return fast_quick_bits(sign[0], sign[1]);
}

// The same test on the words as the kernel reads them: four pixels that start n bytes (0..3) into the little-endian byte string lo, hi.  The byte
// offset and the widening to a 16-bit pair are ONE byte permute per pair (v_perm_b32: selector bytes 0..7 pick a byte of the string, 0x0c a zero)
// where fast_pair(fast_bytes(lo, hi, n), half) is a v_alignbyte_b32 and three more instructions.
struct FastSrc { uint32_t lo, hi; int n; };
MSL_FAST_HD uint32_t fast_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    uint32_t r = 0;
    for (int b = 0; b < 4; b++) {
        const uint32_t s = (sel >> (8 * b)) & 0xFFu;   // (only the selector values this header uses)
        const uint32_t byte = s < 4 ? (lo >> (8 * s)) & 0xFFu : s < 8 ? (hi >> (8 * (s - 4))) & 0xFFu : 0u;
        r |= byte << (8 * b);
    }
    return r;
#endif
}
MSL_FAST_HD s16x2 fast_pair_at(FastSrc s, int half) {
    const uint32_t b = (uint32_t)(s.n + 2 * half);   // bytes b, b + 1 of the string, each zero-extended to 16 bits
    return pk_from_bits(fast_perm(s.hi, s.lo, b | 0x0c00u | ((b + 1u) << 16) | 0x0c000000u));
}
MSL_FAST_HD unsigned fast_quick4_at(FastSrc c, FastSrc r0, FastSrc r8, FastSrc r4, FastSrc r12, FastSrc r2, FastSrc r10, FastSrc r6, FastSrc r14, int th) {
    const s16x2 t = pk_make(th, th);
    uint32_t sign[2];
    MSL_FAST_UNROLL
    for (int half = 0; half < 2; half++)
        sign[half] = fast_quick_pair(fast_pair_at(c, half), fast_pair_at(r0, half), fast_pair_at(r8, half), fast_pair_at(r4, half), fast_pair_at(r12, half),
                                     fast_pair_at(r2, half), fast_pair_at(r10, half), fast_pair_at(r6, half), fast_pair_at(r14, half), t);
    return fast_quick_bits(sign[0], sign[1]);
}

// FAST-9/16 corner score of a pixel of value v with the 16 ring values ring[0..15] (in ring order):
// score = max(a, -b) - 1 with a = max over the 16 nine-arcs of min(d), b = min over arcs of max(d), d = v - ring; since
// -b = max over arcs of min(-d), both halves are the same min/max network: run it once on packed pairs.  v is the same in all sixteen d, so the
// network runs on (r, -r) and v is added once at the end: over an arc min(v - r) = v + min(-r) and min(r - v) = min(r) - v, and the maximum over
// the arcs commutes with the constant likewise.  0 <= v, ring[k] <= 255: every value stays within +-255, the initial -256 below all of them.
// One multiplication builds a pair: r * -65535 = r - (r << 16), low half r, high half -r mod 2^16 (three instructions per ring value before).
MSL_FAST_HD int fast_score16(int v, const int *ring) {
    s16x2 x[16], lo2[16], lo4[16];
    MSL_FAST_UNROLL
    for (int k = 0; k < 16; k++) x[k] = pk_from_bits((uint32_t)(ring[k] * -65535));
    MSL_FAST_UNROLL
    for (int k = 0; k < 16; k++) lo2[k] = pk_min(x[k], x[(k + 1) & 15]);
    MSL_FAST_UNROLL
    for (int k = 0; k < 16; k++) lo4[k] = pk_min(lo2[k], lo2[(k + 2) & 15]);
    s16x2 a = pk_make(-256, -256);
    MSL_FAST_UNROLL
    for (int k = 0; k < 16; k++) a = pk_max(a, pk_min(pk_min(lo4[k], lo4[(k + 4) & 15]), x[(k + 8) & 15]));
    const int p = v + a.y, n = a.x - v;   // a.y = -min over arcs of max(r), a.x = max over arcs of min(r)
    return (p > n ? p : n) - 1;
}

}  // namespace orb
}  // namespace msl
