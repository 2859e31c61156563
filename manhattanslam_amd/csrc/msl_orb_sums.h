// msl_orb_sums.h -- integer pieces of the ORB kernels (msl_orb.hip) on plain values.  No memory access, no HIP call: the kernels hand in the
// words they loaded, and a host program can call the same functions (tests/orb_sums_host.cpp).
//   k_describe  IC_Angle: the intensity-centroid moments m10 = sum u I and m01 = sum v I over the circular 31 x 31 patch (src/ORBextractor.cc:75-99),
//               taken four pixels at a time from the dwords a wave loads.  Integer sums of at most 961 products below 2^13: exact in any order.
//   k_pyramid   one pixel of the 11-bit fixed-point bilinear resize (k_resize's expression) from aligned words of its two source rows.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MSL_SUMS_HD __host__ __device__ __forceinline__
#else
#define MSL_SUMS_HD inline
#endif

namespace msl {
namespace orb {

constexpr int IC_ROWS = 31, IC_ROW_WORDS = 8, IC_WORDS = IC_ROWS * IC_ROW_WORDS;   // rows v = -15 .. 15; a row is staged as columns u = -16 .. 15

// sum over the four bytes of a * b, plus c (v_dot4_u32_u8)
MSL_SUMS_HD uint32_t sums_udot4(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int e = 0; e < 4; e++) c += ((a >> (8 * e)) & 0xFFu) * ((b >> (8 * e)) & 0xFFu);
    return c;
#endif
}

// sum over the two 16-bit fields of a * b (v_dot2_u32_u16)
MSL_SUMS_HD uint32_t sums_udot2(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b), 0u, false);
#else
    return (a & 0xFFFFu) * (b & 0xFFFFu) + (a >> 16) * (b >> 16);
#endif
}

// The two adjacent source bytes of a pixel, b[o] and b[o + 1] of the little-endian byte string lo, hi (o = 0 .. 3), as two 16-bit fields
// (one v_perm_b32: selector bytes 0 - 3 take from lo, 4 - 7 from hi, 12 gives 0).
MSL_SUMS_HD uint32_t resize_pair(uint32_t lo, uint32_t hi, int o) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, 0x0c010c00u + (uint32_t)o * 0x00010001u);
#else
    const uint64_t s = ((uint64_t)hi << 32 | lo) >> (8 * o);
    return (uint32_t)(s & 0xFFu) | ((uint32_t)((s >> 8) & 0xFFu) << 16);
#endif
}

// One output pixel of the resize: k_resize's expression  h = r[s0] c0 + r[s1] c1 per source row, v = ((cy0 (h0 >> 4) >> 16) + (cy1 (h1 >> 4) >> 16) + 2) >> 2,
// clamped to a byte.  pair0 / pair1 hold (r[s0], r[s0 + 1]) of the two rows and cx the column tap's (c0, c1) as 16-bit fields.  This needs what
// every column tap of cv::resize's tables has (the host plan checks it): 0 <= c0, c1 <= 2048, and s1 == s0 + 1 or c1 == 0.
MSL_SUMS_HD uint32_t resize_px(uint32_t pair0, uint32_t pair1, uint32_t cx, int cy0, int cy1) {
    const int h0 = (int)sums_udot2(pair0, cx), h1 = (int)sums_udot2(pair1, cx);
    int v = (((cy0 * (h0 >> 4)) >> 16) + ((cy1 * (h1 >> 4)) >> 16) + 2) >> 2;
    v = v < 0 ? 0 : v > 255 ? 255 : v;
    return (uint32_t)v;
}

// umax[0..15] (each <= 15) as sixteen nibbles, umax[v] in bits 4 v .. 4 v + 3: a lane looks its row's up with one shift
MSL_SUMS_HD uint64_t ic_pack_umax(const int *umax) {
    uint64_t p = 0;
    for (int v = 0; v < 16; v++) p |= (uint64_t)((unsigned)umax[v] & 15u) << (4 * v);
    return p;
}

// Weight words of patch word i (row i / 8, columns 4 (i % 8) .. + 3): byte e of `one` is 1 where the pixel lies inside the circle (|u| <= umax[|v|]),
// byte e of `col` is its staged column u + 16 (1 .. 31) there; both 0 outside.
MSL_SUMS_HD void ic_weights(int i, uint64_t umaxNib, uint32_t &one, uint32_t &col) {
    const int r = i >> 3, q = i & 7, v = r - 15, av = v < 0 ? -v : v;
    const int um = (int)((umaxNib >> (4 * av)) & 15u);
    // columns 16 - um .. 16 + um are inside: the word's first nlo and last nhi bytes are not
    int nlo = 16 - um - 4 * q, nhi = 4 * q + 3 - (16 + um);
    nlo = nlo < 0 ? 0 : nlo > 4 ? 4 : nlo;
    nhi = nhi < 0 ? 0 : nhi > 4 ? 4 : nhi;
    const uint32_t lo = nlo >= 4 ? 0u : 0x01010101u << (8 * nlo), hi = nhi >= 4 ? 0u : 0x01010101u >> (8 * nhi);
    one = lo & hi;
    col = (0x03020100u + 0x04040404u * (uint32_t)q) & (one * 255u);
}

// Adds patch word i (pixels w, one per byte) to the three running sums: sI = sum I, sCI = sum (u + 16) I, sVI = sum v I over the pixels inside the circle.
MSL_SUMS_HD void ic_add_word(uint32_t w, int i, uint64_t umaxNib, uint32_t &sI, uint32_t &sCI, int &sVI) {
    uint32_t one, col;
    ic_weights(i, umaxNib, one, col);
    const uint32_t s = sums_udot4(w, one, 0u);
    sI += s;
    sCI = sums_udot4(w, col, sCI);
    sVI += ((i >> 3) - 15) * (int)s;
}

// m10 from the totals: sum u I = sum (u + 16) I - 16 sum I
MSL_SUMS_HD int ic_m10(uint32_t sI, uint32_t sCI) { return (int)sCI - 16 * (int)sI; }

}  // namespace orb
}  // namespace msl
