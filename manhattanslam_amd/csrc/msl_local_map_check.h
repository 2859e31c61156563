// msl_local_map_check.h -- what a host-memory call of the local-map entry points (msl_local_keyframes, msl_local_points, msl_local_lines:
// msl_local_map.hip) checks of its index arrays before any launch: the ids a frame holds, the covisibility rows and the parent links of the
// keyframe table, and a list of local keyframes.  The observation table is msl_mappoint_check.h's csr_ok.  Pure host functions on plain
// arrays: no HIP call, no allocation through the library, no global state, so a plain C++ program can call them
// (tests/localmap_check_host.cpp).  Each returns true, or false with a message that names the field in err; the caller puts its own name
// in front ("%s: %s").
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <vector>

namespace msl {
namespace localmap {

// The ids n_frames frames hold, cap slots each: n[f] inside 0 .. cap and, only then, every slot below n[f] -1 or an id of the table of n_ids
// rows (what / count: the arguments' names).
inline bool held_ok(const char *what, const char *count, int n_frames, int cap, int n_ids, const int32_t *held, const int32_t *n, char *err,
                    size_t err_len) {
    for (int f = 0; f < n_frames; f++) {
        if (n[f] < 0 || n[f] > cap) { snprintf(err, err_len, "%s[%d] is %d outside 0 .. %d", count, f, (int)n[f], cap); return false; }
        for (int i = 0; i < n[f]; i++) {
            const int id = held[(size_t)f * cap + i];
            if (id < -1 || id >= n_ids) { snprintf(err, err_len, "%s[%d][%d] is %d of %d", what, f, i, id, n_ids); return false; }
        }
    }
    return true;
}

// The covisibility rows and the parent links of a table of n_tab keyframes: n_conn[k] inside 0 .. ccap and, only then, its entries inside
// the table; parent[k] -1 or another keyframe of the table.
inline bool graph_ok(int n_tab, int ccap, const int32_t *conn, const int32_t *n_conn, const int32_t *parent, char *err, size_t err_len) {
    for (int k = 0; k < n_tab; k++) {
        if (n_conn[k] < 0 || n_conn[k] > ccap) { snprintf(err, err_len, "n_conn[%d] is %d outside 0 .. ccap = %d", k, (int)n_conn[k], ccap); return false; }
        for (int r = 0; r < n_conn[k]; r++) {
            const int c = conn[(size_t)k * ccap + r];
            if (c < 0 || c >= n_tab) { snprintf(err, err_len, "conn[%d][%d] is keyframe %d of %d", k, r, c, n_tab); return false; }
        }
        const int p = parent[k];
        if (p < -1 || p >= n_tab) { snprintf(err, err_len, "parent[%d] is keyframe %d of %d", k, p, n_tab); return false; }
        if (p == k) { snprintf(err, err_len, "parent[%d] is the keyframe itself", k); return false; }
    }
    return true;
}

// A list of keyframes per frame, n_tab slots each: n[f] inside 0 .. n_tab and, only then, every entry below n[f] inside the table and
// distinct (what / count: the arguments' names).
inline bool list_ok(const char *what, const char *count, int n_frames, int n_tab, const int32_t *list, const int32_t *n, char *err, size_t err_len) {
    std::vector<int32_t> seen((size_t)n_tab, -1);
    for (int f = 0; f < n_frames; f++) {
        if (n[f] < 0 || n[f] > n_tab) { snprintf(err, err_len, "%s[%d] is %d outside 0 .. n_tab = %d", count, f, (int)n[f], n_tab); return false; }
        for (int r = 0; r < n[f]; r++) {
            const int k = list[(size_t)f * n_tab + r];
            if (k < 0 || k >= n_tab) { snprintf(err, err_len, "%s[%d][%d] is keyframe %d of %d", what, f, r, k, n_tab); return false; }
            if (seen[(size_t)k] == f) { snprintf(err, err_len, "%s[%d] holds keyframe %d twice", what, f, k); return false; }
            seen[(size_t)k] = f;
        }
    }
    return true;
}

}  // namespace localmap
}  // namespace msl
