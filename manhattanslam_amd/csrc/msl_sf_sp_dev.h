// msl_sf_sp_dev.h -- what the translation units of the frame-batched superpixel stage for gfx950 (MI355X) share (internal; the units: msl_sf.h, the
// stage's overview: msl_sf_superpixel.hip).  Three parts: the exact-arithmetic pins, the 16-lane row operations (a DPP row = the lanes of one seed),
// and the host side of the units.
#pragma once

#include "msl_sf.h"
#include "msl_sf_sp_arith.h"

using namespace msl;
using namespace msl::sf;

// Everything on the device side stays in an unnamed namespace, where it was while the stage was one file: with the same symbols every kernel's
// instruction stream stays what it was (profiles/README.md).
namespace {

// ---- exact arithmetic ------------------------------------------------------------------------------------------------------
// The float / double mixtures on plain values -- the division by 100.0, the cost terms, the Newton quotient and the comparisons with 0.01 / 0.2 --
// are in msl_sf_sp_arith.h, which a host program includes too.
//
// Comparisons of a FLOAT x with one of the reference's DOUBLE constants c (HUBER_RANGE 0.4, MAX_ANGLE_COS 0.1, the 0.05 / 0.1 depth limits), which
// C++ evaluates as (double)x OP c: none of these constants is a float, and for each of them the float nearest to it, cf = (float)c, is the float
// next ABOVE it (asserted below), so there is no float in [c, cf) and the sets of floats on either side of c and of cf are the same:
//   (double)x <  c  <=>  x <  cf        (double)x >  -c  <=>  x >  -cf
//   (double)x >= c  <=>  x >= cf        (double)x <= -c  <=>  x <= -cf        (double)x > c  <=>  x >= cf
// (NaN: false on both sides.)  One v_cmp_f32 instead of v_cvt_f64_f32 + v_cmp_f64 per test.
constexpr float HUBER_RANGE_F = (float)HUBER_RANGE, MAX_ANGLE_COS_F = (float)MAX_ANGLE_COS, DEPTH_005_F = 0.05f, DEPTH_01_F = 0.1f;
static_assert((double)HUBER_RANGE_F > HUBER_RANGE && (double)sp_float_below(HUBER_RANGE_F) < HUBER_RANGE, "0.4f is the float next above 0.4");
static_assert((double)MAX_ANGLE_COS_F > MAX_ANGLE_COS && (double)sp_float_below(MAX_ANGLE_COS_F) < MAX_ANGLE_COS, "0.1f is the float next above 0.1");
static_assert((double)DEPTH_005_F > 0.05 && (double)sp_float_below(DEPTH_005_F) < 0.05, "0.05f is the float next above 0.05");
static_assert((double)DEPTH_01_F > 0.1 && (double)sp_float_below(DEPTH_01_F) < 0.1, "0.1f is the float next above 0.1");
__device__ __forceinline__ bool in_huber_band(float r) { return r < HUBER_RANGE_F && r > -HUBER_RANGE_F; }   // residual < HUBER_RANGE && residual > -HUBER_RANGE

// Strictly sequential (left-to-right) float sums over 16-byte aligned LDS arrays; wide LDS reads are issued
// ahead of the dependent add chain so the chain runs at VALU latency instead of LDS latency.  (kb_seed_plane; kb_update_seeds uses the chains below.)
__device__ __forceinline__ float seq_sum_f32(const float *a, int n, float s) {
    int p = 0;
    for (; p + 8 <= n; p += 8) {
        const float4 u = *reinterpret_cast<const float4 *>(a + p), v = *reinterpret_cast<const float4 *>(a + p + 4);
        s += u.x; s += u.y; s += u.z; s += u.w; s += v.x; s += v.y; s += v.z; s += v.w;
    }
    for (; p < n; p++) s += a[p];
    return s;
}
// Huber/Newton numerator (:494-503) in list order: finite terms are 2*residual (a float add; identical to the double
// add rounded to float), +-inf marks a tail element whose contribution is the DOUBLE constant +-HUBER_RANGE.
__device__ __forceinline__ float huber_term_add(float s, float t) {
    return __builtin_isinf(t) ? (float)((double)s + (t > 0 ? HUBER_RANGE : -1 * HUBER_RANGE)) : s + t;
}

// ---- row operations: the 16 lanes of a DPP row = one seed group -----------------------------------------------------------
// Four consecutive elements loaded as one access of whatever alignment the element type guarantees (global memory
// tolerates dword-/byte-aligned wide loads).
template <typename T> struct Quad { T v[4]; };
template <typename T> __device__ __forceinline__ Quad<T> load_quad(const T *p) { Quad<T> q; __builtin_memcpy(&q, p, sizeof(q)); return q; }
template <typename T> __device__ __forceinline__ Quad<T> load_quad(gptr<T> p) {
    Quad<T> q;
#pragma unroll
    for (int e = 0; e < 4; e++) q.v[e] = p[e];
    return q;
}

// The same strictly sequential sums without the LDS round trips: a ROTATING chain over the 16 lanes of a DPP row.  Lane i of the row holds the
// elements i, 16 + i, 32 + i, ... of the list (one per block of 16); step k of the chain lets every lane compute (value of its left neighbour) +
// (its element of block k / 16), row_ror:1 making lane 0 the neighbour of lane 15.  Lane k mod 16 then holds exactly s_k = s_(k-1) + e_k -- its
// neighbour held s_(k-1) after the step before -- while the lanes behind the front hold garbage nobody reads.  Elements beyond the end of a list
// are +0.0f: s + (+0.0f) == s for every s the chain can hold (it starts at +0.0f, and a float sum is -0.0f only if both operands are), so after
// any number of whole blocks lane 15 holds the sum of the list in list order, bit for bit what a left-to-right walk with `s += e` (seq_sum_f32) or huber_term_add returns.  One
// v_add_f32 with a DPP operand per element, for the four seeds of a wave at once.
__device__ __forceinline__ float row_ror1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xF, 0xF, false));   // row_ror:1
}
__device__ __forceinline__ float chain_block_f32(float s, float t) {
#pragma unroll
    for (int q = 0; q < 16; q++) s = row_ror1(s) + t;
    return s;
}
__device__ __forceinline__ float chain_block_huber(float s, float t) {
#pragma unroll
    for (int q = 0; q < 16; q++) s = huber_term_add(row_ror1(s), t);
    return s;
}

// Inclusive prefix sum over the 16 lanes of a DPP row (= one seed group); lanes without a source read 0.
__device__ __forceinline__ int row_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);   // row_shr:8
    return v;
}

// 16-lane (DPP row = seed group) exchanges in the VALU instead of __shfl / __shfl_xor, which compile to ds_bpermute: a trip through the LDS crossbar per
// value (plus the address arithmetic in front of it and a dependent wait behind it) where a DPP move or operand costs one VALU slot and a few cycles.
// Only controls that give EVERY lane a source lane (row rotations, quad permutes, row_newbcast), so `old` is never read (bound_ctrl).
template <int CTRL> __device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) { return __int_as_float(dpp_i32<CTRL>(__float_as_int(v))); }
template <int N> __device__ __forceinline__ int row_lane_i32(int v) { return dpp_i32<0x150 + N>(v); }      // lane N of the row, to all its lanes (row_newbcast)
template <int N> __device__ __forceinline__ float row_lane_f32(float v) { return dpp_f32<0x150 + N>(v); }
// sum / maximum over the 16 lanes of a row, every lane receives it: row_ror:8, row_ror:4, quad_perm [2,3,0,1], quad_perm [1,0,3,2].  For integers, and for
// floats whose partial sums are all exact (integer-valued sums below 2^24), any order gives the same result as the xor butterfly this replaces.
__device__ __forceinline__ int row_sum_i32(int v) { v += dpp_i32<0x128>(v); v += dpp_i32<0x124>(v); v += dpp_i32<0x4E>(v); v += dpp_i32<0xB1>(v); return v; }
__device__ __forceinline__ float row_sum_exact_f32(float v) { v += dpp_f32<0x128>(v); v += dpp_f32<0x124>(v); v += dpp_f32<0x4E>(v); v += dpp_f32<0xB1>(v); return v; }
__device__ __forceinline__ float row_max_f32(float v) {
    v = fmaxf(v, dpp_f32<0x128>(v)); v = fmaxf(v, dpp_f32<0x124>(v)); v = fmaxf(v, dpp_f32<0x4E>(v)); v = fmaxf(v, dpp_f32<0xB1>(v));
    return v;
}
// maximum over the four rows of a wave of a value that is uniform inside each row: a scalar
__device__ __forceinline__ int rows_max_i32(int v) {
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// FP64 sums over the 16 lanes of a DPP row (= one seed group): row rotations by 8 and 4 and quad permutes run in the VALU (a few cycles) instead of
// ds_bpermute round trips through the LDS crossbar.  The schedules -- the one-value butterfly sp_group_sum and the transposed sp_group_sum4 /
// sp_group_sum10 kb_seed_plane uses -- are in msl_sf_sp_arith.h, written on the lane operations below.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v) {
    const unsigned long long u = __double_as_longlong(v);
    // (bound_ctrl: the row rotations and quad permutes used here give every lane a source lane, so the `old` operand is never read -- without it the
    // compiler materialises a zero for it in front of every move: 2 of 5 instructions per value and step of the group sums)
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
// The lane operations on a double per lane.  sel: a DPP move with a bank mask and `old` = the value the lane keeps does the select and the move in one
// instruction per register half.
struct RowOpsD {
    template <int CTRL, int BANKS> static __device__ __forceinline__ double sel(double old, double src) {
        const unsigned long long uo = __double_as_longlong(old), us = __double_as_longlong(src);
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)uo, (int)(unsigned)us, CTRL, 0xF, BANKS, false);
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(uo >> 32), (int)(unsigned)(us >> 32), CTRL, 0xF, BANKS, false);
        return __longlong_as_double(((unsigned long long)hi << 32) | lo);
    }
    template <int CTRL> static __device__ __forceinline__ double mov(double v) { return dpp_mov_d<CTRL>(v); }
    static __device__ __forceinline__ double add(double a, double b) { return a + b; }
};

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
namespace msl {
namespace sf {

// W mod 8 in {1, 2, 3}: a window quad can stick out over the right edge (the STRADDLE instantiations of kb_update_seeds and kb_seed_plane)
inline bool sp_quad_straddles(int W) { return (W % SP) >= 1 && (W % SP) <= 3; }
inline dim3 sp_seed_grid(const SfDev &P, int nFrames) { return dim3((P.nseeds + 255) / 256, (unsigned)nFrames); }   // one thread per seed, blockIdx.y = slot

// The steps of sp_launch_stage (msl_sf_superpixel.hip), each in the unit that holds its kernels; P's per-slot pointers address the first of the
// nFrames keyframes.
void sp_launch_seed_init(KernelProfiler &prof, hipStream_t st, const SfDev &P, int nFrames);                         // msl_sf_sp_assign.hip
void sp_launch_pixel_pass(KernelProfiler &prof, hipStream_t st, const SfDev &P, int nFrames, int it, bool propLds);  // msl_sf_sp_assign.hip
void sp_launch_seed_pass(KernelProfiler &prof, hipStream_t st, const SfDev &P, int nFrames, int it);                 // msl_sf_sp_seeds.hip
void sp_launch_plane(KernelProfiler &prof, hipStream_t st, const SfDev &P, int nFrames);                             // msl_sf_sp_plane.hip

}  // namespace sf
}  // namespace msl
