// msl_match_math.h -- device arithmetic the searches on the matcher handle share, each piece pinned or written once
// (internal): cv::gemm's 3x3 float kernels, cv::invert, Mat::dot and cv::norm of float 3-vectors, the camera centre, the counter-based
// sampler, the search mode, the popcount distance and descriptor load, the two-smallest-keys pair and its wave reduction, the LDS key sort
// that groups features by vocabulary node, the rotation-consistency cull, the scale prediction.
#pragma once

#include "msl_common.h"

#include <climits>

namespace msl {

constexpr int TH_LOW = 50;                         // src/ORBmatcher.cc:33

// d[r] = (float)(alpha * sum_k A(r, k) b[k] + c[r]) with double accumulation: cv::gemm's CV_32F kernel.  S: the row stride of A (4: the
// rotation inside rows 0-2 of a 4x4 pose)
template <int S = 4>
__device__ __forceinline__ void gemm3(const float *A, bool transA, double alpha, const float b[3], const float *c, float d[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)(transA ? A[k * S + r] : A[r * S + k]) * (double)b[k];
        d[r] = (float)(s * alpha + (c ? (double)c[r] : 0.0));
    }
}

// D = alpha * op(A) op(B) for 3x3 float matrices of row stride SA / SB (D: stride 3): cv::gemm's float kernel, as gemm3
template <int SA, int SB>
__device__ __forceinline__ void gemm33(const float *A, bool tA, const float *B, bool tB, double alpha, float *Dm) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)(tA ? A[k * SA + r] : A[r * SA + k]) * (double)(tB ? B[c * SB + k] : B[k * SB + c]);
            Dm[r * 3 + c] = (float)(s * alpha + 0.0);
        }
}

// cv::invert of a 3x3 float matrix (the closed form): determinant and cofactors in double, times 1 / det, each element rounded
__device__ __forceinline__ void inv33(const float *m, float *o) {
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    double d = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
    d = 1.0 / d;
    o[0] = (float)((m11 * m22 - m12 * m21) * d); o[1] = (float)((m02 * m21 - m01 * m22) * d); o[2] = (float)((m01 * m12 - m02 * m11) * d);
    o[3] = (float)((m12 * m20 - m10 * m22) * d); o[4] = (float)((m00 * m22 - m02 * m20) * d); o[5] = (float)((m02 * m10 - m00 * m12) * d);
    o[6] = (float)((m10 * m21 - m11 * m20) * d); o[7] = (float)((m01 * m20 - m00 * m21) * d); o[8] = (float)((m00 * m11 - m01 * m10) * d);
}

// Mat::dot and cv::norm of float 3-vectors: double products summed in double from 0 in index order, sqrt in double; the caller rounds where
// the reference assigns to float
__device__ __forceinline__ double dot3_dacc(const float a[3], const float b[3]) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) s += (double)a[k] * (double)b[k];
    return s;
}
__device__ __forceinline__ double norm3_dacc(const float v[3]) { return sqrt(dot3_dacc(v, v)); }

// Ow = -Rwc * tcw of the pose T (rows 0-2 of Tcw): KeyFrame::SetPose
__device__ __forceinline__ void camera_centre(const float *T, float Ow[3]) {
    const float tcw[3] = {T[3], T[7], T[11]};
    gemm3(T, true, -1.0, tcw, nullptr, Ow);
}

// Frame::ComputePlaneWorldCoeff (src/Frame.cc:656-660): pM = mTcw^T * coef (cv::Mat CV_32F product): double accumulation in k order, one rounding; row 3 of mTcw is 0 0 0 1.
__device__ __forceinline__ void world_coef(const float *T, const float *c, float *pM) {
    for (int r = 0; r < 4; r++) {
        double s = 0.0;
        for (int k = 0; k < 4; k++) {
            const float a = k < 3 ? T[4 * k + r] : (r == 3 ? 1.0f : 0.0f);
            s += (double)a * (double)c[k];
        }
        pM[r] = (float)s;
    }
}

// The counter-based sampler of the RANSAC loops: draw j of iteration k, a value in [0, left) =
// mulhi32(fmix32(fmix32(seed ^ k * 0x9E3779B1) ^ (j + 1) * 0x85EBCA77), left).  sampler_iteration is the inner hash, the same for every j.
__device__ __forceinline__ unsigned fmix32(unsigned h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ unsigned sampler_iteration(unsigned seed, int k) { return fmix32(seed ^ (unsigned)k * 0x9E3779B1u); }
__device__ __forceinline__ int sampler_draw(unsigned h0, int j, unsigned left) {
    return (int)__umulhi(fmix32(h0 ^ (unsigned)(j + 1) * 0x85EBCA77u), left);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bForward / bBackward of the two last-frame searches (src/ORBmatcher.cc:560-571, src/LSDmatcher.cpp:24-35): 0 = neither, 1 = forward,
// 2 = backward.  Tc / Tl: rows 0-2 of the current / last mTcw.
__device__ __forceinline__ int search_mode(const float *Tc, const float *Tl, float mb) {
    const float tcw[3] = {Tc[3], Tc[7], Tc[11]}, tlw[3] = {Tl[3], Tl[7], Tl[11]};
    float twc[3], tlc[3];
    gemm3(Tc, true, -1.0, tcw, nullptr, twc);      // twc = -Rcw.t() * tcw
    gemm3(Tl, false, 1.0, twc, tlw, tlc);          // tlc = Rlw * twc + tlw
    return tlc[2] > mb ? 1 : (-tlc[2] > mb ? 2 : 0);
}

// DescriptorDistance of two 256-bit descriptors (src/ORBmatcher.cc:835-849 and src/LSDmatcher.cpp:236-249 are the same popcount)
__device__ __forceinline__ int hamming256(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// The 32 bytes of a descriptor as two 16-byte loads
__device__ __forceinline__ void load_desc(const uint8_t *p, uint4 &a, uint4 &b) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    a = q[0]; b = q[1];
}

// The two smallest keys offered so far, b1 <= b2 (both start at the type's maximum = none).  Branch-free, so b1 / b2 stay in registers
// (no private array).  With (distance << bits | index) keys this is the reference's strict-< best / second-best update in walk order.
template <typename T>
__device__ __forceinline__ void two_smallest(T key, T &b1, T &b2) {
    const T hi = key < b1 ? b1 : key;
    b2 = hi < b2 ? hi : b2;
    b1 = key < b1 ? key : b1;
}

// The two smallest of the keys held by the lanes of a width-W group (every lane gets both): merging (a1 <= a2) with (b1 <= b2).
template <typename T>
__device__ __forceinline__ void two_min(T &m1, T &m2, int width) {
    for (int o = 1; o < width; o <<= 1) {
        const T b1 = __shfl_xor(m1, o, width), b2 = __shfl_xor(m2, o, width);
        const T lo = m1 < b1 ? m1 : b1, hi = m1 < b1 ? b1 : m1;
        const T s = m2 < b2 ? m2 : b2;
        m1 = lo; m2 = hi < s ? hi : s;
    }
}

// Ascending bitonic sort of n (a power of two) 64-bit keys in LDS by the whole block.  With (node << bits | feature) keys this is the
// grouping of a FeatureVector: the features of a node are contiguous and ascending, the nodes ascending.
__device__ __forceinline__ void bitonic_sort(unsigned long long *a, int n) {
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const unsigned long long x = a[i], y = a[j];
                if ((x > y) == up) { a[i] = y; a[j] = x; }
            }
        }
    __syncthreads();
}

__host__ __device__ __forceinline__ int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// The rotation-consistency histogram of the point searches (src/ORBmatcher.cc:33-35, e.g. :643-649 and :199-206): HISTO_LENGTH bins, the bin of
// a rotation is round(rot * (1 / HISTO_LENGTH)) after rot += 360 for rot < 0, bin HISTO_LENGTH folds to 0 (so only bins 0..12 occur, as in
// ORB-SLAM2).  Returns -1 for a value outside [0, HISTO_LENGTH).
constexpr int ROT_HISTO_LENGTH = 30;
__device__ __forceinline__ int rot_bin(float rot) {
    if (rot < 0.0) rot += 360.0f;
    int b = (int)roundf(rot * (1.0f / ROT_HISTO_LENGTH));
    if (b == ROT_HISTO_LENGTH) b = 0;
    return b >= 0 && b < ROT_HISTO_LENGTH ? b : -1;
}

// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:799-830) on bin counts: keep[0..2] = ind1, ind2, ind3 (-1 = none)
__device__ __forceinline__ void three_maxima(const int *hist, int keep[3]) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < ROT_HISTO_LENGTH; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    keep[0] = ind1; keep[1] = ind2; keep[2] = ind3;
}

// The rotation-consistency cull of a workgroup of NT threads (src/ORBmatcher.cc:643-674, :199-243): bin(i) is the rot_bin of match i, or -1
// when i holds no match (or its rotation has no bin); every match outside the three kept bins goes to drop(i).  s_hist[ROT_HISTO_LENGTH] is
// zero and visible on entry; returns behind a barrier.
template <int NT, class Bin, class Drop>
__device__ __forceinline__ void rotation_cull(int n, int *s_hist, int *s_keep, Bin bin, Drop drop) {
    for (int i = threadIdx.x; i < n; i += NT) {
        const int b = bin(i);
        if (b >= 0) atomicAdd(&s_hist[b], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) three_maxima(s_hist, s_keep);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += NT) {
        const int b = bin(i);
        if (b >= 0 && b != s_keep[0] && b != s_keep[1] && b != s_keep[2]) drop(i);
    }
    __syncthreads();
}

// ceil(log(maxDistance / dist) / logScale) as an int, not clamped (MapLine::PredictScale, src/MapLine.cpp:320-328).  log is glibc's logf in
// the reference; here the double log of the float, rounded once.  A quotient that is not a finite int (NaN, +-inf)
// converts to INT_MIN as on x86-64.
__device__ __forceinline__ int predict_level(float maxDistance, float dist, float logScale) {
    const float ratio = maxDistance / dist;
    const float q = ceilf((float)log((double)ratio) / logScale);
    return (q >= -2147483648.0f && q < 2147483648.0f) ? (int)q : INT_MIN;
}

// MapPoint::PredictScale (src/MapPoint.cc:350-364): the same level clamped to [0, nlevels - 1]
__device__ __forceinline__ int predict_scale(float maxDistance, float dist, float logScale, int nlevels) {
    return clampi(predict_level(maxDistance, dist, logScale), 0, nlevels - 1);
}

}  // namespace msl
