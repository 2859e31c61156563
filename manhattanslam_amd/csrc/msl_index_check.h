// msl_index_check.h -- what a host-memory call of a LocalMapping entry point checks of its index arrays before any launch.  Shared by the
// observation table (CSR over the point or line table: csr_ok), items and reference keyframes (items_ok, refs_ok: msl_mappoint.hip,
// msl_line_fuse.hip), the items and candidate lists of the two fusions (lists_ok: msl_fuse.hip, msl_line_fuse.hip), the targets of
// msl_fuse_candidates (targets_ok), the neighbours of msl_triangulate_new_points (neighbours_ok: msl_triangulate.hip), the held ids, the graph
// and the keyframe rows of the local map (held_ok, graph_ok, kf_rows_ok: msl_local_map.hip), and the candidate rows, the origin and the recent
// elements of the cullings (kf_rows_ok, origin_ok, recent_ok: msl_cull.hip), and the offsets, vertex indices and target rows of the plane clouds
// (offsets_ok, vertex_indices_ok, merge_into_ok: msl_plane_cloud.hip), and the counts, held planes, keyframe rows and Manhattan tables of a
// keyframe with planes (counts_ok, plane_match_ok, kf_slots_ok: msl_keyframe_planes.hip; tables_sorted_ok: msl_keyframe_planes.hip and
// msl_manhattan_detect in msl_plane.hip, which pass the entry layout of msl_plane_tables.h), and the order of the observation ranges and the log
// of msl_observations_apply (obs_ascending_ok, obs_ops_ok: msl_observations.hip), and the weights, ordered rows, parents and log of
// msl_connections_apply and msl_fuse_targets (weights_ok, conn_rows_ok, parents_ok, conn_ops_ok: msl_connections.hip).  Pure host functions on plain arrays: no HIP call, no
// allocation through the library, no global state, so a plain C++ program can call them (tests/mappoint_csr_host.cpp,
// tests/mapping_lists_host.cpp, tests/localmap_check_host.cpp, tests/cull_check_host.cpp, tests/plane_cloud_check_host.cpp,
// tests/kfplanes_check_host.cpp, tests/observations_check_host.cpp, tests/connections_check_host.cpp).  Each returns true, or false with a message that names the field in err; the caller puts its own name in
// front ("%s: %s").
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <vector>

namespace msl {
namespace check {

// ==== the observation table, items and reference keyframes ===================================================================================
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

// ==== the items of the fusions, of msl_fuse_candidates and of msl_triangulate_new_points ====================================================
// The items and lists of a fusion call: every item's target keyframe inside the table of n_tab and its list inside the n_lists lists; every
// list's length inside 0 .. lcap and, only then, its entries: -1 (as often as it likes) or an id of the table of n rows, no id twice in one
// list.  noun: what the ids name, "point" or "line".
inline bool lists_ok(const char *noun, int n_tab, int n, int n_items, int n_lists, int lcap, const int32_t *tgt, const int32_t *list,
                     const int32_t *cand, const int32_t *n_cand, char *err, size_t err_len) {
    for (int f = 0; f < n_items; f++)
        if (tgt[f] < 0 || tgt[f] >= n_tab || list[f] < 0 || list[f] >= n_lists) {
            snprintf(err, err_len, "item %d names keyframe %d of %d or list %d of %d", f, (int)tgt[f], n_tab, (int)list[f], n_lists);
            return false;
        }
    std::vector<int32_t> seen((size_t)n, -1);
    for (int l = 0; l < n_lists; l++) {
        if (n_cand[l] < 0 || n_cand[l] > lcap) { snprintf(err, err_len, "list %d has n_cand %d outside 0 .. %d", l, (int)n_cand[l], lcap); return false; }
        for (int j = 0; j < n_cand[l]; j++) {
            const int id = cand[(size_t)l * lcap + j];
            if (id == -1) continue;
            if (id < 0 || id >= n) { snprintf(err, err_len, "list %d entry %d is %s %d of %d", l, j, noun, id, n); return false; }
            if (seen[(size_t)id] == l) { snprintf(err, err_len, "list %d holds %s %d twice (pass -1 for a later duplicate)", l, noun, id); return false; }
            seen[(size_t)id] = l;
        }
    }
    return true;
}

// The items of msl_triangulate_new_points: the current keyframe inside the table, n_neigh inside 0 .. ncap, the neighbours inside the
// table, distinct and none the current keyframe.
inline bool neighbours_ok(int n_tab, int n_items, int ncap, const int32_t *cur, const int32_t *neigh, const int32_t *n_neigh, char *err,
                          size_t err_len) {
    for (int f = 0; f < n_items; f++) {
        bool ok = cur[f] >= 0 && cur[f] < n_tab && n_neigh[f] >= 0 && n_neigh[f] <= ncap;
        for (int r = 0; ok && r < n_neigh[f]; r++) {
            const int k = neigh[(size_t)f * ncap + r];
            ok = k >= 0 && k < n_tab && k != cur[f];
            for (int q = 0; ok && q < r; q++) ok = neigh[(size_t)f * ncap + q] != k;
        }
        if (!ok) {
            snprintf(err, err_len, "item %d names a keyframe outside the table of %d, repeats a neighbour, lists its current keyframe as a "
                     "neighbour, or has n_neigh outside 0 .. %d", f, n_tab, ncap);
            return false;
        }
    }
    return true;
}

// The items of msl_fuse_candidates: n_targets inside 0 .. tcap and, only then, the targets inside the table
inline bool targets_ok(int n_tab, int n_items, int tcap, const int32_t *targets, const int32_t *n_targets, char *err, size_t err_len) {
    for (int f = 0; f < n_items; f++) {
        bool ok = n_targets[f] >= 0 && n_targets[f] <= tcap;
        for (int t = 0; ok && t < n_targets[f]; t++) ok = targets[(size_t)f * tcap + t] >= 0 && targets[(size_t)f * tcap + t] < n_tab;
        if (!ok) {
            snprintf(err, err_len, "item %d names a keyframe outside the table of %d, or has n_targets outside 0 .. %d", f, n_tab, tcap);
            return false;
        }
    }
    return true;
}

// ==== the local map and the cullings =========================================================================================================
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

// n_rows rows of keyframes, `stride` slots each (a list of local keyframes per frame with stride n_tab, the candidates of a culling item
// with stride ccap): n[f] inside 0 .. stride and, only then, every entry below n[f] inside the table of n_tab keyframes and distinct within
// its row (what / count / limit: the names of the rows, of their counts and of the stride).
inline bool kf_rows_ok(const char *what, const char *count, const char *limit, int n_rows, int n_tab, int stride, const int32_t *rows,
                       const int32_t *n, char *err, size_t err_len) {
    std::vector<int32_t> seen((size_t)n_tab, -1);
    for (int f = 0; f < n_rows; f++) {
        if (n[f] < 0 || n[f] > stride) { snprintf(err, err_len, "%s[%d] is %d outside 0 .. %s = %d", count, f, (int)n[f], limit, stride); return false; }
        for (int r = 0; r < n[f]; r++) {
            const int k = rows[(size_t)f * stride + r];
            if (k < 0 || k >= n_tab) { snprintf(err, err_len, "%s[%d][%d] is keyframe %d of %d", what, f, r, k, n_tab); return false; }
            if (seen[(size_t)k] == f) { snprintf(err, err_len, "%s[%d] holds keyframe %d twice", what, f, k); return false; }
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

// ==== the observation edits ==================================================================================================================
// Every range of the observation table (already checked by csr_ok) strictly ascending in obs_kf: std::map's order, a keyframe at most once.
inline bool obs_ascending_ok(int n_pts, const int32_t *obs_off, const int32_t *obs_kf, char *err, size_t err_len) {
    for (int p = 0; p < n_pts; p++)
        for (int o = obs_off[p] + 1; o < obs_off[p + 1]; o++)
            if (obs_kf[o] <= obs_kf[o - 1]) {
                snprintf(err, err_len, "obs_kf[%d] is keyframe %d after %d in the range of point %d: not strictly ascending", o, (int)obs_kf[o],
                         (int)obs_kf[o - 1], p);
                return false;
            }
    return true;
}

// The op codes of msl_observations_apply (msl.h's MSL_OBS_*; msl_observations.hip asserts that they are the same) and the log's limits
constexpr int OBS_ADD = 1, OBS_ERASE = 2, OBS_SET_BAD = 3, OBS_REPLACE = 4, OBS_KF_ERASE = 5, OBS_MAX_KF_ERASE = 256;

// The log of msl_observations_apply, ops[o] = { op, a, b, c }: a known code; the id, keyframe and keypoint an op reads inside n_pts, n_tab and
// n_kps[b] (clamped to cap); every OBS_KF_ERASE in front of every other op and at most OBS_MAX_KF_ERASE of them; ocap at least n_obs_total +
// the OBS_ADD ops.
inline bool obs_ops_ok(int n_tab, int cap, int n_pts, int n_obs_total, int n_ops, int ocap, const int32_t *n_kps, const int32_t *ops, char *err,
                       size_t err_len) {
    int n_add = 0, n_kf_erase = 0;
    bool other = false;
    for (int o = 0; o < n_ops; o++) {
        const int op = ops[4 * (size_t)o], a = ops[4 * (size_t)o + 1], b = ops[4 * (size_t)o + 2], c = ops[4 * (size_t)o + 3];
        if (op < OBS_ADD || op > OBS_KF_ERASE) { snprintf(err, err_len, "ops[%d].op is %d, not an MSL_OBS_* code", o, op); return false; }
        if (op != OBS_KF_ERASE && (a < 0 || a >= n_pts)) { snprintf(err, err_len, "ops[%d].a is id %d of %d", o, a, n_pts); return false; }
        if (op == OBS_REPLACE) {
            if (b < 0 || b >= n_pts) { snprintf(err, err_len, "ops[%d].b is id %d of %d", o, b, n_pts); return false; }
        } else if (op != OBS_SET_BAD && (b < 0 || b >= n_tab)) {
            snprintf(err, err_len, "ops[%d].b is keyframe %d of %d", o, b, n_tab);
            return false;
        }
        if (op == OBS_ADD) {
            const int n = n_kps[b] < cap ? n_kps[b] : cap;
            if (c < 0 || c >= n) { snprintf(err, err_len, "ops[%d].c is keypoint %d of %d in keyframe %d", o, c, n, b); return false; }
            n_add++;
        }
        if (op == OBS_KF_ERASE) {
            if (other) { snprintf(err, err_len, "ops[%d] is an MSL_OBS_KF_ERASE behind another op", o); return false; }
            if (++n_kf_erase > OBS_MAX_KF_ERASE) {
                snprintf(err, err_len, "ops[%d] is MSL_OBS_KF_ERASE number %d of at most %d", o, n_kf_erase, OBS_MAX_KF_ERASE);
                return false;
            }
        } else {
            other = true;
        }
    }
    if ((long long)ocap < (long long)n_obs_total + n_add) {
        snprintf(err, err_len, "ocap is %d, below n_obs_total + the %d MSL_OBS_ADD ops = %lld", ocap, n_add, (long long)n_obs_total + n_add);
        return false;
    }
    return true;
}

// ==== the graph edits ========================================================================================================================
// The op codes of msl_connections_apply (msl.h's MSL_CONN_*; msl_connections.hip asserts that they are the same)
constexpr int CONN_UPDATE = 1, CONN_KF_BAD = 2;

// n_rows rows of n_tab weights, none negative (what: the argument's name)
inline bool weights_ok(const char *what, int n_rows, int n_tab, const int32_t *w, char *err, size_t err_len) {
    for (int f = 0; f < n_rows; f++)
        for (int j = 0; j < n_tab; j++)
            if (w[(size_t)f * n_tab + j] < 0) { snprintf(err, err_len, "%s[%d][%d] is %d, below 0", what, f, j, (int)w[(size_t)f * n_tab + j]); return false; }
    return true;
}

// The ordered rows of a table of n_tab keyframes whose n_conn is the full count: n_conn[k] inside 0 .. n_tab and the entries below it
// that the row of ccap holds inside the table.
inline bool conn_rows_ok(int n_tab, int ccap, const int32_t *conn, const int32_t *n_conn, char *err, size_t err_len) {
    for (int k = 0; k < n_tab; k++) {
        if (n_conn[k] < 0 || n_conn[k] > n_tab) { snprintf(err, err_len, "n_conn[%d] is %d outside 0 .. n_tab = %d", k, (int)n_conn[k], n_tab); return false; }
        for (int r = 0; r < n_conn[k] && r < ccap; r++) {
            const int c = conn[(size_t)k * ccap + r];
            if (c < 0 || c >= n_tab) { snprintf(err, err_len, "conn[%d][%d] is keyframe %d of %d", k, r, c, n_tab); return false; }
        }
    }
    return true;
}

// parent[k] -1 or a keyframe of the table
inline bool parents_ok(int n_tab, const int32_t *parent, char *err, size_t err_len) {
    for (int k = 0; k < n_tab; k++)
        if (parent[k] < -1 || parent[k] >= n_tab) { snprintf(err, err_len, "parent[%d] is keyframe %d of %d", k, (int)parent[k], n_tab); return false; }
    return true;
}

// The log of msl_connections_apply, ops[o] = { op, a, b, c }: a known code, the keyframe inside the table, the weight row of a CONN_UPDATE
// inside the n_rows rows.
inline bool conn_ops_ok(int n_tab, int n_rows, int n_ops, const int32_t *ops, char *err, size_t err_len) {
    for (int o = 0; o < n_ops; o++) {
        const int op = ops[4 * (size_t)o], a = ops[4 * (size_t)o + 1], b = ops[4 * (size_t)o + 2];
        if (op != CONN_UPDATE && op != CONN_KF_BAD) { snprintf(err, err_len, "ops[%d].op is %d, not an MSL_CONN_* code", o, op); return false; }
        if (a < 0 || a >= n_tab) { snprintf(err, err_len, "ops[%d].a is keyframe %d of %d", o, a, n_tab); return false; }
        if (op == CONN_UPDATE && (b < 0 || b >= n_rows)) { snprintf(err, err_len, "ops[%d].b is weight row %d of %d", o, b, n_rows); return false; }
    }
    return true;
}

// ==== the plane clouds =======================================================================================================================
// The offsets of n_frames CSR tables, rows + 1 entries each, of which the first n[f] rows (clamped to 0 .. rows) are read: ascending from
// >= 0 to at most limit (what / count: the arguments' names).
inline bool offsets_ok(const char *what, const char *count, int n_frames, int rows, int limit, const int32_t *off, const int32_t *n, char *err,
                       size_t err_len) {
    for (int f = 0; f < n_frames; f++) {
        const int m = n[f] < 0 ? 0 : (n[f] > rows ? rows : n[f]);
        const int32_t *o = off + (size_t)f * (rows + 1);
        if (o[0] < 0) { snprintf(err, err_len, "%s[%d][0] is %d, below 0", what, f, (int)o[0]); return false; }
        for (int r = 0; r < m; r++)
            if (o[r + 1] < o[r]) { snprintf(err, err_len, "%s[%d] descends at row %d of %s (%d after %d)", what, f, r, count, (int)o[r + 1], (int)o[r]); return false; }
        if (o[m] > limit) { snprintf(err, err_len, "%s[%d][%d] is %d, beyond %d", what, f, m, (int)o[m], limit); return false; }
    }
    return true;
}

// The vertex indices of the detector planes (offsets already checked by offsets_ok): inside the cloud of n_vertices.
inline bool vertex_indices_ok(int n_frames, int max_planes, int n_vertices, const int32_t *vertex_offsets, const int32_t *vertex_indices,
                              const int32_t *n_planes, char *err, size_t err_len) {
    for (int f = 0; f < n_frames; f++) {
        const int m = n_planes[f] < 0 ? 0 : (n_planes[f] > max_planes ? max_planes : n_planes[f]);
        const int32_t *o = vertex_offsets + (size_t)f * (max_planes + 1);
        for (int q = o[0]; q < o[m]; q++) {
            const int v = vertex_indices[(size_t)f * n_vertices + q];
            if (v < 0 || v >= n_vertices) { snprintf(err, err_len, "vertex_indices[%d][%d] is vertex %d of %d", f, q, v, n_vertices); return false; }
        }
    }
    return true;
}

// merge_into of the first n_planes[f] frame planes: -1 or a row of the frame's n_map[f] map planes (both counts clamped).
inline bool merge_into_ok(int n_frames, int pcap, int mcap, const int32_t *merge_into, const int32_t *n_planes, const int32_t *n_map, char *err,
                          size_t err_len) {
    for (int f = 0; f < n_frames; f++) {
        const int np = n_planes[f] < 0 ? 0 : (n_planes[f] > pcap ? pcap : n_planes[f]);
        const int nm = n_map[f] < 0 ? 0 : (n_map[f] > mcap ? mcap : n_map[f]);
        for (int k = 0; k < np; k++) {
            const int j = merge_into[(size_t)f * pcap + k];
            if (j < -1 || j >= nm) { snprintf(err, err_len, "merge_into[%d][%d] is row %d of %d", f, k, j, nm); return false; }
        }
    }
    return true;
}

// ==== the keyframe planes and the Manhattan tables ===========================================================================================
// Per-frame counts inside 0 .. cap (what / limit: the names of the counts and of the capacity).
inline bool counts_ok(const char *what, const char *limit, int n_frames, int cap, const int32_t *n, char *err, size_t err_len) {
    for (int f = 0; f < n_frames; f++)
        if (n[f] < 0 || n[f] > cap) { snprintf(err, err_len, "%s[%d] is %d outside 0 .. %s = %d", what, f, (int)n[f], limit, cap); return false; }
    return true;
}

// The first `slots` of the three map planes every frame plane below n_planes[f] names: -1 or a row of the frame's n_map[f] map planes
// (counts already checked by counts_ok; what: the argument's name).
inline bool plane_match_ok(const char *what, int n_frames, int pcap, int slots, const int32_t *match, const int32_t *n_planes,
                           const int32_t *n_map, char *err, size_t err_len) {
    for (int f = 0; f < n_frames; f++)
        for (int k = 0; k < n_planes[f]; k++)
            for (int s = 0; s < slots; s++) {
                const int j = match[3 * ((size_t)f * pcap + k) + s];
                if (j < -1 || j >= n_map[f]) { snprintf(err, err_len, "%s[%d][%d][%d] is row %d of %d", what, f, k, s, j, (int)n_map[f]); return false; }
            }
    return true;
}

// The keyframe of every frame: its row inside the keyframe tables of kcap rows and its id not negative (slot / id: the n_frames values).
inline bool kf_slots_ok(int n_frames, int kcap, const int32_t *slot, const int32_t *id, int stride, char *err, size_t err_len) {
    for (int f = 0; f < n_frames; f++) {
        const int s = slot[(size_t)f * stride], i = id[(size_t)f * stride];
        if (s < 0 || s >= kcap) { snprintf(err, err_len, "frames[%d].kf_slot is keyframe %d of %d", f, s, kcap); return false; }
        if (i < 0) { snprintf(err, err_len, "frames[%d].kf_id is %d, below 0", f, i); return false; }
    }
    return true;
}

// n_frames Manhattan tables of cap entries of `stride` ints (callers pass mf::stride(w) of msl_plane_tables.h), of which the first n[f],
// clamped to 0 .. cap as the kernels clamp it, are read: the first w ints of an entry ascending, the entries strictly ascending by them,
// lexicographically (what: the table's name).  msl_manhattan_observe refuses a count outside 0 .. cap first (counts_ok);
// msl_manhattan_detect accepts it.
inline bool tables_sorted_ok(const char *what, int n_frames, int cap, int stride, int w, const int32_t *tab, const int32_t *n, char *err,
                             size_t err_len) {
    for (int f = 0; f < n_frames; f++)
        for (int e = 0, m = n[f] < cap ? n[f] : cap; e < m; e++) {
            const int32_t *x = tab + ((size_t)f * cap + e) * stride;
            bool ok = true;
            for (int q = 1; q < w; q++) ok = ok && x[q - 1] <= x[q];
            if (ok && e > 0) {
                int c = 0;
                for (int q = 0; q < w && c == 0; q++) c = x[q - stride] < x[q] ? -1 : (x[q - stride] > x[q] ? 1 : 0);
                ok = c < 0;
            }
            if (!ok) { snprintf(err, err_len, "%s[%d] is not sorted by its keys at entry %d", what, f, e); return false; }
        }
    return true;
}

}  // namespace check
}  // namespace msl
