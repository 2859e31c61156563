// msl_plane_tables.h -- what the plane chain shares: msl_plane_associate / msl_manhattan_detect (msl_plane.hip), msl_plane_clouds /
// msl_map_plane_merge (msl_plane_cloud.hip), msl_keyframe_decision (msl_keyframe.hip) and msl_keyframe_planes / msl_manhattan_observe
// (msl_keyframe_planes.hip).  The capacity limits of the chain, the layout of a Manhattan table entry, the
// search over such a table, the three-int sort of its keys and the held-row predicate (internal; the refusal of an argument outside its
// range, in_range, is in msl_match_handle.h).  msl_pose_kernel.h takes the plane count of a frame from it; msl_index_check.h stays a
// plain C++ header without it: its callers pass the layout.
#pragma once

#include "msl_common.h"

namespace msl {

// ---- limits -----------------------------------------------------------------------------------------------------------------------------------
// The planes of a frame or keyframe (pcap, max_planes: one lane each; the plane residuals of the pose optimisers), the map planes of a
// frame (mcap), the points of its plane clouds (ptcap, fptcap), the entries of its full / partial Manhattan table (fcap / qcap), its
// keyframe rows (kcap) and the frames of a call (a grid dimension).  The map *points* of msl_match.hip / msl_local_map.hip and the
// keyframes of msl_reloc.hip / msl_pnp.hip are other quantities with limits of their own: hence the PLANE in three of the names.
constexpr int MAX_PCAP = 64, MAX_PLANE_MCAP = 4096, MAX_PLANE_PTCAP = 1 << 22, MAX_FCAP = 65536, MAX_QCAP = 65536, MAX_PLANE_KCAP = 4096;
constexpr int MAX_PLANE_FRAMES = 65535;

// ---- the entry of a Manhattan table -----------------------------------------------------------------------------------------------------------
// w key ints (map-plane rows, ascending), the keyframe slot, then the keyframe-plane index of every key: {a, b, c, kf, ia, ib, ic} in the
// full table, {a, b, kf, ia, ib} in the partial one (msl.h, msl_manhattan_detect).
namespace mf {
constexpr int FULL = 3, PART = 2;                                       // the key widths
constexpr int stride(int w) { return 2 * w + 1; }
constexpr int kf_at(int w) { return w; }                                // the keyframe slot
constexpr int index_at(int w, int q) { return w + 1 + q; }              // the keyframe-plane index of key q
// msl_manhattan_observe's scratch per table entry: the merged entry and the lower bound of a new key
constexpr int scratch_ints(int w) { return stride(w) + 1; }
}  // namespace mf

// ---- device helpers ---------------------------------------------------------------------------------------------------------------------------
// The number of entries of a table sorted by its W key ints whose key is below `key`; *found: the entry there has it.  (k_manhattan keeps
// its own closed-interval find_entry in msl_plane.hip, for its instruction text: see there.)
template <int W>
__device__ __forceinline__ int lower_bound_key(const int32_t *tab, int n, const int *key, bool *found) {
    constexpr int ST = mf::stride(W);
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int32_t *e = tab + (size_t)mid * ST;
        int c = 0;
        for (int q = 0; q < W && c == 0; q++) c = e[q] < key[q] ? -1 : (e[q] > key[q] ? 1 : 0);
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    bool same = lo < n;
    for (int q = 0; q < W && same; q++) same = tab[(size_t)lo * ST + q] == key[q];
    *found = same;
    return lo;
}

// The keyframe-plane index of map plane m in a table entry (the position of m among its keys), or -1.
__device__ __forceinline__ int kf_index(const int32_t *e, int w, int m) {
    for (int q = 0; q < w; q++)
        if (e[q] == m) return e[mf::index_at(w, q)];
    return -1;
}

__device__ __forceinline__ void sort3(int &a, int &b, int &c) {
    if (a > b) { int t = a; a = b; b = t; }
    if (b > c) { int t = b; b = c; c = t; }
    if (a > b) { int t = a; a = b; b = t; }
}

// The map plane m a frame plane holds (mvpMapPlanes[i]) when it is not NULL and not bad, else -1; flags: the frame's mp_flags row.
// k_manhattan_observe, which also requires its frame enabled, keeps this test and sort3 written out (see there).
__device__ __forceinline__ int held_row(int m, const uint8_t *flags, int nMap) {
    if (m < 0 || m >= nMap || !(flags[m] & 1)) return -1;
    return m;
}
// Not shared on purpose: the verticality gate.  msl_manhattan_detect tests !(a > th || a < -th) (reference src/Tracking.cc:679, 699:
// closed bounds, a NaN passes), msl_manhattan_observe a < th && a > -th (src/LocalMapping.cc:192, 209: open bounds, a NaN fails).  They
// differ at |a| == th and at NaN, and each is pinned to its reference line.

}  // namespace msl
