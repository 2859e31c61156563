// msl_line_project.h -- the endpoint projection of a map line and the window record it fills, shared by the line searches
// (msl_line_match.hip) and the line fusion (msl_line_fuse.hip) (internal).
#pragma once

#include "msl_match_math.h"

namespace msl {

// The GetLinesInArea call of one line: endpoints, radius and octave range.  ok == 0: the line has no window (skipped before the call).
struct LineQ {
    float x1, y1, x2, y2, r;
    int minLevel, maxLevel, ok;
};

__device__ __forceinline__ int wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }   // x86-64's int wrap, without UB

// The endpoint projection both searches share (src/LSDmatcher.cpp:43-79 = src/Frame.cc:264-297; LSDmatcher::Fuse :283-317 is the same
// text): the Vector6d converted to float as Mat_<float> << does, Rcw * P + tcw through cv::gemm's float kernel, both depths tested before
// projecting (Z == 0 passes), u / v left to right without contraction, bounds tests that a NaN passes.
__device__ __forceinline__ bool project_line(const msl_match_params &b, const float *Tc, const double *P, float SP[3], float EP[3], LineQ &q) {
    const float tcw[3] = {Tc[3], Tc[7], Tc[11]};
    for (int k = 0; k < 3; k++) { SP[k] = (float)P[k]; EP[k] = (float)P[3 + k]; }
    float SPc[3], EPc[3];
    gemm3(Tc, false, 1.0, SP, tcw, SPc);
    gemm3(Tc, false, 1.0, EP, tcw, EPc);
    if (SPc[2] < 0.0f || EPc[2] < 0.0f) return false;
    const float invz1 = 1.0f / SPc[2];
    const float u1 = b.fx * SPc[0] * invz1 + b.cx;
    const float v1 = b.fy * SPc[1] * invz1 + b.cy;
    if (u1 < b.minX || u1 > b.maxX) return false;
    if (v1 < b.minY || v1 > b.maxY) return false;
    const float invz2 = 1.0f / EPc[2];
    const float u2 = b.fx * EPc[0] * invz2 + b.cx;
    const float v2 = b.fy * EPc[1] * invz2 + b.cy;
    if (u2 < b.minX || u2 > b.maxX) return false;
    if (v2 < b.minY || v2 > b.maxY) return false;
    q.x1 = u1; q.y1 = v1; q.x2 = u2; q.y2 = v2;
    return true;
}

}  // namespace msl
