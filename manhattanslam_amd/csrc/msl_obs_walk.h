// msl_obs_walk.h -- the parts of a wave's walk over one map element's observations (CSR over the element table, msl.h), 64 at a time and in
// list order (internal).  k_line_refresh (msl_line_fuse.hip, double sums) builds its loop from all of them; k_refresh (msl_mappoint.hip,
// float sums, with its descriptor compaction in between) takes the range and the list-order add and keeps obs_chunk, obs_ref_index and
// write_item_and_row written out, as k_covis keeps the range: the compiler orders operands differently around the shared forms there, and
// these kernels' instruction text is pinned.  Every function is called by the whole wave.
#pragma once

#include "msl_match_math.h"

namespace msl {

// Dev below: a kernel's argument struct with the observation table under the names off, okf, oidx, nObs and the keyframe count nTab.

// The observation range [b, e) of element id, clamped into the table of nObs observations
template <class Dev>
__device__ __forceinline__ void obs_range(const Dev &D, int id, int &b, int &e) {
    b = clampi(D.off[id], 0, D.nObs);
    e = clampi(D.off[id + 1], b, D.nObs);
}

// Observation o of a range that ends at e: its keyframe and feature index (-1 past the end) and whether the keyframe is inside the table.
// Returns the ballot of the valid lanes, in list order from bit 0.
template <class Dev>
__device__ __forceinline__ unsigned long long obs_chunk(const Dev &D, int o, int e, int &k, int &idx, bool &valid) {
    k = -1; idx = -1;
    if (o < e) { k = D.okf[o]; idx = D.oidx[o]; }
    valid = k >= 0 && k < D.nTab;
    return __ballot(valid);
}

// mObservations[pRefKF]: the feature index of the first observation by the reference keyframe (isRef: this lane's is one).  refIdx stays
// as it is, 0 from the caller = map::operator[] of an absent key, while none is met.
__device__ __forceinline__ void obs_ref_index(bool isRef, int idx, bool &refSeen, int &refIdx) {
    const unsigned long long mr = __ballot(isRef);
    if (!refSeen && mr) { refIdx = __shfl(idx, __ffsll(mr) - 1); refSeen = true; }
}

// acc = acc + t of every lane in m, in list order: the same sum in every lane
template <class T>
__device__ __forceinline__ void obs_add_in_order(unsigned long long m, const T (&t)[3], T (&acc)[3]) {
    while (m) {
        const int j = __ffsll(m) - 1;
        m &= m - 1;
#pragma unroll
        for (int a = 0; a < 3; a++) acc[a] = acc[a] + __shfl(t[a], j);
    }
}

// One lane's epilogue for an N-vector: item f's output and, when there is a table and the value was written, row id of the table
template <int N, class T>
__device__ __forceinline__ void write_item_and_row(T *out, T *table, bool wrote, int f, int id, const T (&v)[N]) {
#pragma unroll
    for (int a = 0; a < N; a++) {
        out[N * (size_t)f + a] = v[a];
        if (table && wrote) table[N * (size_t)id + a] = v[a];
    }
}

}  // namespace msl
