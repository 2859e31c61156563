// msl_cull_check.h -- what a host-memory call of the culling entry points (msl_cull_keyframes, msl_cull_recent: msl_cull.hip) checks of its
// arrays before any launch: the candidate rows and the origin of msl_cull_keyframes, the counters and ids of msl_cull_recent.  The
// observation table is msl_mappoint_check.h's csr_ok.  Pure host functions on plain arrays: no HIP call, no allocation through the library,
// no global state, so a plain C++ program can call them (tests/cull_check_host.cpp).  Each returns true, or false with a message that names
// the field in err; the caller puts its own name in front ("%s: %s").
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <vector>

namespace msl {
namespace cull {

// The candidate rows of n_items items, ccap slots each: n_cand[f] inside 0 .. ccap and, only then, every entry below it inside the table of
// n_tab keyframes and distinct within its row.
inline bool cand_ok(int n_items, int n_tab, int ccap, const int32_t *cand, const int32_t *n_cand, char *err, size_t err_len) {
    std::vector<int32_t> seen((size_t)n_tab, -1);
    for (int f = 0; f < n_items; f++) {
        if (n_cand[f] < 0 || n_cand[f] > ccap) { snprintf(err, err_len, "n_cand[%d] is %d outside 0 .. ccap = %d", f, (int)n_cand[f], ccap); return false; }
        for (int r = 0; r < n_cand[f]; r++) {
            const int k = cand[(size_t)f * ccap + r];
            if (k < 0 || k >= n_tab) { snprintf(err, err_len, "cand[%d][%d] is keyframe %d of %d", f, r, k, n_tab); return false; }
            if (seen[(size_t)k] == f) { snprintf(err, err_len, "cand[%d] holds keyframe %d twice", f, k); return false; }
            seen[(size_t)k] = f;
        }
    }
    return true;
}

// The keyframe with mnId == 0: -1 (not in the table) or a table index.
inline bool origin_ok(int n_tab, int origin, char *err, size_t err_len) {
    if (origin < -1 || origin >= n_tab) { snprintf(err, err_len, "origin is keyframe %d of %d", origin, n_tab); return false; }
    return true;
}

// The n recent elements of msl_cull_recent: counters and ids not negative; in the integer ratio form (int_form) no element that is not bad
// (flags bit 0) with visible == 0, which the reference divides by.
inline bool recent_ok(int n, bool int_form, const int32_t *found, const int32_t *visible, const int32_t *first_kf_id, const uint8_t *flags,
                      char *err, size_t err_len) {
    for (int i = 0; i < n; i++) {
        if (found[i] < 0) { snprintf(err, err_len, "found[%d] is %d, below 0", i, (int)found[i]); return false; }
        if (visible[i] < 0) { snprintf(err, err_len, "visible[%d] is %d, below 0", i, (int)visible[i]); return false; }
        if (first_kf_id[i] < 0) { snprintf(err, err_len, "first_kf_id[%d] is %d, below 0", i, (int)first_kf_id[i]); return false; }
        if (int_form && (flags[i] & 1) && visible[i] == 0) {
            snprintf(err, err_len, "visible[%d] is 0 in the integer ratio form (a division by zero in the reference)", i);
            return false;
        }
    }
    return true;
}

}  // namespace cull
}  // namespace msl
