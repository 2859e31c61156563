// msl_mappoint_check.h -- what a host-memory call of msl_refresh_map_points / msl_covisibility checks of its index arrays before any launch
// (msl_mappoint.hip): the observation table (CSR over the point table), the reference keyframes and the item list.  Pure host functions on
// plain arrays: no HIP call, no allocation through the library, no global state, so a plain C++ program can call them
// (tests/mappoint_csr_host.cpp).  Each returns true, or false with a message that names the field in err.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <vector>

namespace msl {
namespace mappoint {

// obs_off[n_pts + 1] ascending from >= 0 to n_obs_total, obs_kf inside the table of n_tab keyframes, obs_idx (may be null: not read by the
// call) below n_kps[obs_kf] and the table's cap.
inline bool csr_ok(int n_tab, int cap, int n_pts, int n_obs_total, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx,
                   const int32_t *n_kps, char *err, size_t err_len) {
    if (obs_off[0] < 0) { snprintf(err, err_len, "obs_off[0] is %d, below 0", (int)obs_off[0]); return false; }
    for (int p = 0; p < n_pts; p++)
        if (obs_off[p + 1] < obs_off[p]) {
            snprintf(err, err_len, "obs_off descends at point %d (%d after %d)", p, (int)obs_off[p + 1], (int)obs_off[p]);
            return false;
        }
    if (obs_off[n_pts] != n_obs_total) {
        snprintf(err, err_len, "obs_off[n_pts] is %d, n_obs_total %d", (int)obs_off[n_pts], n_obs_total);
        return false;
    }
    for (int o = obs_off[0]; o < n_obs_total; o++) {
        const int k = obs_kf[o];
        if (k < 0 || k >= n_tab) { snprintf(err, err_len, "obs_kf[%d] is keyframe %d of %d", o, k, n_tab); return false; }
        if (!obs_idx) continue;
        const int i = obs_idx[o], n = n_kps[k] < cap ? n_kps[k] : cap;
        if (i < 0 || i >= n) { snprintf(err, err_len, "obs_idx[%d] is keypoint %d of %d in keyframe %d", o, i, n, k); return false; }
    }
    return true;
}

// The items of a call: n_items indices into a table of n rows, distinct when `distinct` (what: the argument's name).
inline bool items_ok(const char *what, int n, int n_items, const int32_t *items, bool distinct, char *err, size_t err_len) {
    std::vector<uint8_t> seen(distinct ? (size_t)n : 0, 0);
    for (int f = 0; f < n_items; f++) {
        const int id = items[f];
        if (id < 0 || id >= n) { snprintf(err, err_len, "%s[%d] is %d of %d", what, f, id, n); return false; }
        if (!distinct) continue;
        if (seen[(size_t)id]) { snprintf(err, err_len, "%s holds %d twice", what, id); return false; }
        seen[(size_t)id] = 1;
    }
    return true;
}

// pt_ref[id] inside the keyframe table for every item (ids already checked by items_ok)
inline bool refs_ok(int n_tab, int n_items, const int32_t *ids, const int32_t *pt_ref, char *err, size_t err_len) {
    for (int f = 0; f < n_items; f++) {
        const int r = pt_ref[ids[f]];
        if (r < 0 || r >= n_tab) { snprintf(err, err_len, "pt_ref[%d] is keyframe %d of %d", (int)ids[f], r, n_tab); return false; }
    }
    return true;
}

}  // namespace mappoint
}  // namespace msl
