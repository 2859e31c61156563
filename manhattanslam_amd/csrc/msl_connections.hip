// msl_connections.hip -- the producer of the keyframe graph for gfx950: msl_connections_apply[_batch] executes a log of UpdateConnections /
// SetBadFlag edits (reference src/KeyFrame.cc:113-145, :266-316, :349-360, :382-442 and :455-467) on the weight maps, the ordered rows, the
// parents and the flags where they live; msl_fuse_targets[_batch] is vpTargetKFs of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:
// 527-543).  tests/connections_model.py is the sequential model.
//   k_conn_run      one workgroup walks the log in order, threads across the weight row.  An edit writes the cw entries at once and leaves
//                   the ordered row of a keyframe to later: per keyframe a mode in the handle's scratch says how the row is to be rebuilt,
//                   FULL from the whole map (UpdateBestCovisibles) or CUT at th from the keyframe's own row (the ordered vector
//                   UpdateConnections writes: a function of cw[k], which is that weight row until an edit makes the row FULL).  The tree
//                   loop of SetBadFlag reads ordered rows, so the walker rebuilds the pending rows of the children first: an LDS bitonic
//                   sort of the 64-bit keys (weight << 32 | index), descending.  The loop itself is a workgroup maximum of (weight, first
//                   child, first position) over the (child, position) pairs whose entry is a candidate, once per re-parented child
//   k_conn_rows     one workgroup per keyframe: rebuilds the rows still pending
//   k_conn_touched  one workgroup: the ascending list of the keyframes written, by a scan, and the counts
//   k_fuse_targets  one wave per item; the stamps are one bit per keyframe, 64 bits in each lane
// No float operations, no atomics: the log is walked in order, a sort of distinct keys has one result, every other byte is written once.
// Synchronisation of k_conn_run.  Every branch that leads to a barrier is taken on values that all waves read alike: a value is read in
// a barrier interval in which no thread writes it.  An op begins behind the barrier that ends the one before.  op_update reads flags[k]
// on entry and writes it behind its two block_max barriers; op_bad reads flags[a] and parent[a] on entry and writes flags[a] behind its
// first barrier.  Within an interval thread j writes column j of row a (or k), entry a (or k) of row j and the marks of keyframe j, and
// reads those alone; thread 0 adds the keyframe's own scalars, which differ from every j that is written (j != a, j != k).  The child
// and candidate maps are written by thread 0 between the barriers of block_max and the one that ends the round.
#include "msl_match_handle.h"
#include "msl_index_check.h"
#include "msl_match_math.h"

namespace {

using namespace msl;

typedef unsigned long long u64;

constexpr int RUN_NT = 1024, ROW_NT = 256, TGT_NT = 256, MAX_OPS = MSL_CONN_MAX_OPS;
constexpr int MODE_CLEAN = 0, MODE_FULL = 1, MODE_CUT = 2;
constexpr int FLAG_LIVE = 1, FLAG_NOT_ERASE = 2, FLAG_CONNECTED = 4;
static_assert(MAX_TAB == 4096, "the sort holds MAX_TAB keys in 32 KB of LDS; child and position take 12 bits each of a tree key");
static_assert(check::CONN_UPDATE == MSL_CONN_UPDATE && check::CONN_KF_BAD == MSL_CONN_KF_BAD, "msl_index_check.h names the codes of msl.h");
static_assert(sizeof(msl_conn_op) == 16, "ops are read as four ints");

struct ConnDev {
    int nTab, ccap, nRows, nOps, tcap, origin, th, pow2;
    const int32_t *weight; const msl_conn_op *ops;
    int32_t *cw, *conn, *connW, *nConn, *parent; uint8_t *flags;
    uint8_t *opStatus; int32_t *touched, *counts;
    uint8_t *mode, *wrote; int32_t *ctr;                                       // scratch: per keyframe; { turned bad, ChangeParent calls }
};

// The largest key of the workgroup, in every thread (s_red: 16 entries)
__device__ __forceinline__ u64 block_max(u64 v, u64 *s_red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const u64 o = __shfl_xor(v, off); v = o > v ? o : v; }
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if (lane_id() == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 all = 0;
    for (int i = 0; i < nw; i++) all = s_red[i] > all ? s_red[i] : all;
    return all;
}

// What UpdateConnections selects of a weight row: the largest weight with the lowest index among equal maxima (strict > in ascending
// order), as (w << 32 | ~index); 0 for a row without a positive weight
__device__ __forceinline__ u64 max_key(int w, int i) { return w > 0 ? (u64)w << 32 | (0xFFFFFFFFu - (unsigned)i) : 0; }

// Row j of conn, conn_w and n_conn[j] from row j of cw, by the whole workgroup.  MODE_FULL: every positive entry.  MODE_CUT: the entries
// at or above th or, if none reaches it, the single maximum.  Descending weight, equal weights by descending index.
__device__ void rebuild_row(const ConnDev &D, int j, int mode, u64 *s_key, u64 *s_red) {
    const int t = threadIdx.x, nt = blockDim.x, n = D.nTab, P = D.pow2;
    const int32_t *row = D.cw + (size_t)j * n;
    bool any_th = true;
    int jmax = -1;
    if (mode == MODE_CUT) {
        u64 best = 0;
        for (int i = t; i < n; i += nt) { const u64 k = max_key(row[i], i); best = k > best ? k : best; }
        best = block_max(best, s_red);
        any_th = (int)(best >> 32) >= D.th;
        jmax = best ? (int)(0xFFFFFFFFu - (unsigned)best) : -1;
    }
    __syncthreads();
    for (int i = t; i < P; i += nt) {
        const int w = i < n ? row[i] : 0;
        const bool keep = w > 0 && (mode == MODE_FULL || (any_th ? w >= D.th : i == jmax));
        s_key[i] = keep ? (u64)w << 32 | (unsigned)i : 0;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int s = k >> 1; s > 0; s >>= 1) {
            for (int i = t; i < P; i += nt) {
                const int l = i ^ s;
                if (l > i) {
                    const u64 a = s_key[i], b = s_key[l];
                    if ((i & k) == 0 ? a < b : a > b) { s_key[i] = b; s_key[l] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = t; i < P; i += nt)
        if (s_key[i] != 0 && (i + 1 == P || s_key[i + 1] == 0)) D.nConn[j] = i + 1;
    if (t == 0 && s_key[0] == 0) D.nConn[j] = 0;
    for (int r = t; r < D.ccap; r += nt) {
        const u64 k = s_key[r];                                                // ccap <= n_tab <= P
        D.conn[(size_t)j * D.ccap + r] = k ? (int)(unsigned)k : -1;
        D.connW[(size_t)j * D.ccap + r] = (int)(k >> 32);
    }
    __syncthreads();
}

// ==== k_conn_run: the log in order, one workgroup ============================================================================================
// The writes of UpdateConnections of keyframe k with KFcounter = weight row f
__device__ __forceinline__ int op_update(const ConnDev &D, int k, int f, u64 *s_red) {
    const int t = threadIdx.x, n = D.nTab;
    const int flags = D.flags[k];
    if (!(flags & FLAG_LIVE)) return MSL_CONN_ALREADY_BAD;
    const int32_t *W = D.weight + (size_t)f * n;
    u64 best = 0, top = 0;                                                     // top: the first of the ordered row when a weight reaches th
    for (int i = t; i < n; i += RUN_NT) {
        const int w = i == k ? 0 : W[i];
        const u64 a = max_key(w, i), b = w >= D.th ? (u64)w << 32 | (unsigned)i : 0;
        best = a > best ? a : best; top = b > top ? b : top;
    }
    best = block_max(best, s_red);
    if (!best) return MSL_CONN_EMPTY;
    top = block_max(top, s_red);
    const bool any_th = top != 0;
    const int jmax = (int)(0xFFFFFFFFu - (unsigned)best), first = any_th ? (int)(unsigned)top : jmax;
    for (int i = t; i < n; i += RUN_NT) {
        const int w = i == k ? 0 : max(W[i], 0);
        if (w > 0 && (any_th ? w >= D.th : i == jmax) && D.cw[(size_t)i * n + k] != w) {   // AddConnection; an equal weight is its return
            D.cw[(size_t)i * n + k] = w; D.mode[i] = MODE_FULL; D.wrote[i] = 1;
        }
        D.cw[(size_t)k * n + i] = w;
    }
    int st = MSL_CONN_DONE;
    const bool link = !(flags & FLAG_CONNECTED) && k != D.origin;
    if (link) st |= MSL_CONN_PARENT_SET;
    if (t == 0) {
        D.mode[k] = MODE_CUT; D.wrote[k] = 1;
        if (link) { D.parent[k] = first; D.flags[k] = (uint8_t)(flags | FLAG_CONNECTED); }
    }
    return st;
}

// The connection and tree half of SetBadFlag of keyframe a
__device__ __forceinline__ int op_bad(const ConnDev &D, int a, int &n_bad, int &n_change, u64 *s_key, u64 *s_red, uint8_t *s_child, uint8_t *s_cand) {
    const int t = threadIdx.x, n = D.nTab, ccap = D.ccap;
    const int flags = D.flags[a];
    if (a == D.origin || (flags & FLAG_NOT_ERASE)) return MSL_CONN_KEPT;
    if (!(flags & FLAG_LIVE)) return MSL_CONN_ALREADY_BAD;
    const int pa = D.parent[a];
    for (int j = t; j < n; j += RUN_NT) {
        if (j != a && D.cw[(size_t)a * n + j] > 0 && D.cw[(size_t)j * n + a] > 0) {   // EraseConnection
            D.cw[(size_t)j * n + a] = 0; D.mode[j] = MODE_FULL; D.wrote[j] = 1;
        }
        D.cw[(size_t)a * n + j] = 0;
        s_child[j] = j != a && D.parent[j] == a && (D.flags[j] & FLAG_LIVE);
        s_cand[j] = j == pa;
    }
    for (int r = t; r < ccap; r += RUN_NT) { D.conn[(size_t)a * ccap + r] = -1; D.connW[(size_t)a * ccap + r] = 0; }
    __syncthreads();
    // behind the barrier: every wave has read flags[a] for the two returns above.  Nothing below reads these four of keyframe a (a is no
    // child of itself), and the next op reads them behind the barrier that ends this one
    if (t == 0) { D.nConn[a] = 0; D.mode[a] = MODE_CLEAN; D.wrote[a] = 1; D.flags[a] = (uint8_t)(flags & ~FLAG_LIVE); }
    for (int c = 0; c < n; c++) {                                              // the rows the loop reads, after this op's erasures
        if (!s_child[c]) continue;
        const int mode = D.mode[c];
        if (mode == MODE_CLEAN) continue;
        rebuild_row(D, c, mode, s_key, s_red);
        if (t == 0) D.mode[c] = MODE_CLEAN;
        __syncthreads();
    }
    const int wave = t >> 6, lane = t & 63;
    for (;;) {
        u64 best = 0;
        for (int c = wave; c < n; c += RUN_NT / WAVE) {
            if (!s_child[c]) continue;
            const int len = clampi(D.nConn[c], 0, ccap);
            for (int pos = lane; pos < len; pos += WAVE) {
                const int e = D.conn[(size_t)c * ccap + pos];
                if (e < 0 || e >= n || !s_cand[e]) continue;
                const u64 key = ((u64)max(D.cw[(size_t)c * n + e], 0) + 1) << 24 | (u64)(4095 - c) << 12 | (u64)(4095 - pos);
                best = key > best ? key : best;
            }
        }
        best = block_max(best, s_red);
        if (!best) break;
        const int c = 4095 - (int)(best >> 12 & 4095), pos = 4095 - (int)(best & 4095);
        if (t == 0) { D.parent[c] = D.conn[(size_t)c * ccap + pos]; D.wrote[c] = 1; s_child[c] = 0; s_cand[c] = 1; }
        n_change++;
        __syncthreads();
    }
    for (int base = 0; base < n; base += RUN_NT) {                             // no link to any candidate: the original parent
        const int c = base + t;
        const bool left = c < n && s_child[c];
        if (left) { D.parent[c] = pa; D.wrote[c] = 1; }
        n_change += __syncthreads_count(left);
    }
    n_bad++;
    return MSL_CONN_DONE;
}

__global__ __launch_bounds__(RUN_NT) void k_conn_run(ConnDev D) {
    __shared__ u64 s_key[MAX_TAB], s_red[16];
    __shared__ uint8_t s_child[MAX_TAB], s_cand[MAX_TAB];
    const int t = threadIdx.x;
    for (int j = t; j < D.nTab; j += RUN_NT) { D.mode[j] = MODE_CLEAN; D.wrote[j] = 0; }
    int n_bad = 0, n_change = 0;
    __syncthreads();
    for (int o = 0; o < D.nOps; o++) {
        const msl_conn_op op = D.ops[o];
        const bool a_ok = op.a >= 0 && op.a < D.nTab;
        int st = 0;
        if (op.op == MSL_CONN_UPDATE) {
            if (a_ok && op.b >= 0 && op.b < D.nRows) st = op_update(D, op.a, op.b, s_red);
        } else if (op.op == MSL_CONN_KF_BAD) {
            if (a_ok) st = op_bad(D, op.a, n_bad, n_change, s_key, s_red, s_child, s_cand);
        }
        if (t == 0) D.opStatus[o] = (uint8_t)st;
        __syncthreads();                                                       // the next op reads what this one wrote
    }
    if (t == 0) { D.ctr[0] = n_bad; D.ctr[1] = n_change; }
}

// ==== k_conn_rows: the rows still pending, one workgroup each ================================================================================
__global__ __launch_bounds__(ROW_NT) void k_conn_rows(ConnDev D) {
    __shared__ u64 s_key[MAX_TAB], s_red[16];
    const int j = blockIdx.x, mode = D.mode[j];
    if (mode != MODE_CLEAN) rebuild_row(D, j, mode, s_key, s_red);
}

// ==== k_conn_touched: the keyframes written, ascending, and the counts =======================================================================
__global__ __launch_bounds__(RUN_NT) void k_conn_touched(ConnDev D) {
    __shared__ unsigned s_wave[32];
    const int t = threadIdx.x, per = (D.nTab + RUN_NT - 1) / RUN_NT, b = t * per, e = min(b + per, D.nTab);
    unsigned mine = 0, over = 0, total, total_over, rank, ex_over;
    for (int j = b; j < e; j++)
        if (D.wrote[j]) { mine++; over += D.nConn[j] > D.ccap; }
    block_excl_scan_pair(mine, over, s_wave, &total, &total_over, rank, ex_over);
    for (int j = b; j < e; j++)
        if (D.wrote[j]) { if (rank < (unsigned)D.tcap) D.touched[rank] = j; rank++; }
    for (int r = (int)total + t; r < D.tcap; r += RUN_NT) D.touched[r] = -1;
    if (t == 0) { D.counts[0] = (int)total; D.counts[1] = D.ctr[0]; D.counts[2] = D.ctr[1]; D.counts[3] = (int)total_over; }
}

// ==== k_fuse_targets: one wave per item ======================================================================================================
struct TargetsDev {
    int nTab, ccap, nItems, nn, nn2, tcap;
    const int32_t *conn, *nConn; const uint8_t *flags; const int32_t *cur;
    int32_t *targets, *nTargets;
};

__global__ __launch_bounds__(TGT_NT) void k_fuse_targets(TargetsDev D) {
    const int f = blockIdx.x * (TGT_NT / WAVE) + (threadIdx.x >> 6), lane = lane_id(), n = D.nTab;
    if (f >= D.nItems) return;
    int32_t *out = D.targets + (size_t)f * D.tcap;
    const int c = D.cur[f];
    u64 stamps = 0;                                                            // keyframe k: bit k & 63 of lane k >> 6
    int count = 0;
    const int n1 = c >= 0 && c < n ? min(clampi(D.nConn[c], 0, D.ccap), D.nn) : 0;
    for (int i = 0; i < n1; i++) {
        const int k1 = D.conn[(size_t)c * D.ccap + i];
        if (k1 < 0 || k1 >= n || !(D.flags[k1] & FLAG_LIVE)) continue;
        if (__shfl(stamps, k1 >> 6) >> (k1 & 63) & 1) continue;
        if (lane == 0 && count < D.tcap) out[count] = k1;
        count++;
        if (lane == k1 >> 6) stamps |= 1ull << (k1 & 63);
        const int n2 = min(clampi(D.nConn[k1], 0, D.ccap), D.nn2);
        for (int base = 0; base < n2; base += WAVE) {
            const int r = base + lane, k2 = r < n2 ? D.conn[(size_t)k1 * D.ccap + r] : -1;
            const bool in = k2 >= 0 && k2 < n;
            const bool stamped = __shfl(stamps, in ? k2 >> 6 : 0) >> (in ? k2 & 63 : 0) & 1;
            const bool ok = in && (D.flags[k2] & FLAG_LIVE) && !stamped && k2 != c;
            const u64 m = __ballot(ok);
            const int at = count + __popcll(m & ((1ull << lane) - 1ull));
            if (ok && at < D.tcap) out[at] = k2;
            count += __popcll(m);
        }
    }
    for (int r = count + lane; r < D.tcap; r += WAVE) out[r] = -1;
    if (lane == 0) D.nTargets[f] = count;
}

// ==== host side ==============================================================================================================================
const char *const WHO = "msl_connections_apply", *const WHO_TARGETS = "msl_fuse_targets";

bool graph_limits(const char *who, int n_tab, int ccap) {
    if (!in_range(who, "n_tab", n_tab, 1, MAX_TAB)) return false;
    if (ccap < 1 || ccap > n_tab) { set_error("%s: ccap %d outside 1 .. n_tab = %d", who, ccap, n_tab); return false; }
    return true;
}

int check_apply(int n_tab, int ccap, int n_rows, int n_ops, int tcap, int origin, int th, const int32_t *weight, const msl_conn_op *ops,
                int32_t *cw, int32_t *conn, int32_t *conn_w, int32_t *n_conn, int32_t *parent, uint8_t *kf_flags, msl_mem mem,
                uint8_t *op_status, int32_t *touched, int32_t *counts, msl_mem) {
    const char *who = WHO;
    if (!none_null(who, {MSL_NAMED(ops), MSL_NAMED(cw), MSL_NAMED(conn), MSL_NAMED(conn_w), MSL_NAMED(n_conn), MSL_NAMED(parent),
                         MSL_NAMED(kf_flags), MSL_NAMED(op_status), MSL_NAMED(touched), MSL_NAMED(counts)}))
        return MSL_ERR_INVALID;
    if (!graph_limits(who, n_tab, ccap)) return MSL_ERR_INVALID;
    if (n_rows < 0 || n_rows > n_tab) { set_error("%s: n_rows %d outside 0 .. n_tab = %d", who, n_rows, n_tab); return MSL_ERR_INVALID; }
    if (n_rows > 0 && !weight) { set_error("%s: weight is NULL", who); return MSL_ERR_INVALID; }
    if (n_rows == 0 && weight) { set_error("%s: weight is given while n_rows is 0", who); return MSL_ERR_INVALID; }
    if (!in_range(who, "n_ops", n_ops, 1, MAX_OPS)) return MSL_ERR_INVALID;
    if (tcap < 1 || tcap > n_tab) { set_error("%s: tcap %d outside 1 .. n_tab = %d", who, tcap, n_tab); return MSL_ERR_INVALID; }
    char why[256];
    if (!check::origin_ok(n_tab, origin, why, sizeof(why))) return refuse(who, why);
    if (th < 1) { set_error("%s: th %d below 1", who, th); return MSL_ERR_INVALID; }
    if (mem == MSL_MEM_HOST && (!check::conn_ops_ok(n_tab, n_rows, n_ops, &ops->op, why, sizeof(why)) ||
                                !check::conn_rows_ok(n_tab, ccap, conn, n_conn, why, sizeof(why)) ||
                                !check::parents_ok(n_tab, parent, why, sizeof(why)) ||
                                !check::weights_ok("weight", n_rows, n_tab, weight, why, sizeof(why)) ||
                                !check::weights_ok("cw", n_tab, n_tab, cw, why, sizeof(why))))
        return refuse(who, why);
    return MSL_OK;
}

int launch_apply(msl_match *h, int n_tab, int ccap, int n_rows, int n_ops, int tcap, int origin, int th, const int32_t *weight,
                 const msl_conn_op *ops, int32_t *cw, int32_t *conn, int32_t *conn_w, int32_t *n_conn, int32_t *parent, uint8_t *kf_flags,
                 msl_mem mem, uint8_t *op_status, int32_t *touched, int32_t *counts, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t T = (size_t)n_tab;
    ConnDev D{};
    D.nTab = n_tab; D.ccap = ccap; D.nRows = n_rows; D.nOps = n_ops; D.tcap = tcap; D.origin = origin; D.th = th;
    for (D.pow2 = 2; D.pow2 < n_tab; D.pow2 <<= 1) {}
    Stage S(h, mem, out_mem);
    D.weight = S.in(weight, (size_t)n_rows * T); D.ops = S.in(ops, (size_t)n_ops);
    D.cw = S.inout_in_mem(cw, T * T); D.conn = S.inout_in_mem(conn, T * ccap); D.connW = S.inout_in_mem(conn_w, T * ccap);
    D.nConn = S.inout_in_mem(n_conn, T); D.parent = S.inout_in_mem(parent, T); D.flags = S.inout_in_mem(kf_flags, T);
    D.opStatus = S.out(op_status, (size_t)n_ops); D.touched = S.out(touched, (size_t)tcap); D.counts = S.out(counts, 4);
    MSL_HIP_TRY(S.error());
    const size_t per = (T + 255) / 256 * 256;
    MSL_HIP_TRY(grow_all(h->stream, {{h->connWork, 2 * per + 256}}));
    D.mode = (uint8_t *)h->connWork.p; D.wrote = D.mode + per; D.ctr = (int32_t *)(D.mode + 2 * per);
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(k_conn_run, dim3(1), dim3(RUN_NT), 0, st, D);
    hipLaunchKernelGGL(k_conn_rows, dim3((unsigned)n_tab), dim3(ROW_NT), 0, st, D);
    hipLaunchKernelGGL(k_conn_touched, dim3(1), dim3(RUN_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_targets(int n_tab, int ccap, int n_items, int nn, int nn2, int tcap, const int32_t *conn, const int32_t *n_conn,
                  const uint8_t *kf_flags, const int32_t *cur, msl_mem mem, int32_t *targets, int32_t *n_targets, msl_mem) {
    const char *who = WHO_TARGETS;
    if (!none_null(who, {MSL_NAMED(conn), MSL_NAMED(n_conn), MSL_NAMED(kf_flags), MSL_NAMED(cur), MSL_NAMED(targets), MSL_NAMED(n_targets)}))
        return MSL_ERR_INVALID;
    if (!graph_limits(who, n_tab, ccap)) return MSL_ERR_INVALID;
    if (n_items < 1 || n_items > n_tab) { set_error("%s: n_items %d outside 1 .. n_tab = %d", who, n_items, n_tab); return MSL_ERR_INVALID; }
    if (nn < 1 || nn > n_tab) { set_error("%s: nn %d outside 1 .. n_tab = %d", who, nn, n_tab); return MSL_ERR_INVALID; }
    if (nn2 < 1 || nn2 > n_tab) { set_error("%s: nn2 %d outside 1 .. n_tab = %d", who, nn2, n_tab); return MSL_ERR_INVALID; }
    if (!in_range(who, "tcap", tcap, 1, MAX_TAB)) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST && (!check::conn_rows_ok(n_tab, ccap, conn, n_conn, why, sizeof(why)) ||
                                !check::items_ok("cur", n_tab, n_items, cur, false, why, sizeof(why))))
        return refuse(who, why);
    return MSL_OK;
}

int launch_targets(msl_match *h, int n_tab, int ccap, int n_items, int nn, int nn2, int tcap, const int32_t *conn, const int32_t *n_conn,
                   const uint8_t *kf_flags, const int32_t *cur, msl_mem mem, int32_t *targets, int32_t *n_targets, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t T = (size_t)n_tab;
    TargetsDev D{};
    D.nTab = n_tab; D.ccap = ccap; D.nItems = n_items; D.nn = nn; D.nn2 = nn2; D.tcap = tcap;
    Stage S(h, mem, out_mem);
    D.conn = S.in(conn, T * ccap); D.nConn = S.in(n_conn, T); D.flags = S.in(kf_flags, T); D.cur = S.in(cur, (size_t)n_items);
    D.targets = S.out(targets, (size_t)n_items * tcap); D.nTargets = S.out(n_targets, (size_t)n_items);
    MSL_HIP_TRY(S.error());
    const int per = TGT_NT / WAVE;
    hipLaunchKernelGGL(k_fuse_targets, dim3((unsigned)((n_items + per - 1) / per)), dim3(TGT_NT), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_connections_apply(msl_match *h, int n_tab, int ccap, int n_rows, int n_ops, int tcap, int origin, int th, const int32_t *weight,
                          const msl_conn_op *ops, int32_t *cw, int32_t *conn, int32_t *conn_w, int32_t *n_conn, int32_t *parent,
                          uint8_t *kf_flags, msl_mem mem, uint8_t *op_status, int32_t *touched, int32_t *counts, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO, check_apply, launch_apply, h, n_tab, ccap, n_rows, n_ops, tcap, origin, th, weight, ops, cw, conn, conn_w, n_conn,
                       parent, kf_flags, mem, op_status, touched, counts, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_connections_apply_batch(int device, int n_tab, int ccap, int n_rows, int n_ops, int tcap, int origin, int th, const int32_t *weight,
                                const msl_conn_op *ops, int32_t *cw, int32_t *conn, int32_t *conn_w, int32_t *n_conn, int32_t *parent,
                                uint8_t *kf_flags, msl_mem mem, uint8_t *op_status, int32_t *touched, int32_t *counts,
                                msl_mem out_mem) noexcept {
    try {
    return batch_form(check_apply, launch_apply, device, mem == MSL_MEM_DEVICE, n_tab, ccap, n_rows, n_ops, tcap, origin, th, weight, ops, cw,
                      conn, conn_w, n_conn, parent, kf_flags, mem, op_status, touched, counts, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_fuse_targets(msl_match *h, int n_tab, int ccap, int n_items, int nn, int nn2, int tcap, const int32_t *conn, const int32_t *n_conn,
                     const uint8_t *kf_flags, const int32_t *cur, msl_mem mem, int32_t *targets, int32_t *n_targets, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_TARGETS, check_targets, launch_targets, h, n_tab, ccap, n_items, nn, nn2, tcap, conn, n_conn, kf_flags, cur, mem,
                       targets, n_targets, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_fuse_targets_batch(int device, int n_tab, int ccap, int n_items, int nn, int nn2, int tcap, const int32_t *conn, const int32_t *n_conn,
                           const uint8_t *kf_flags, const int32_t *cur, msl_mem mem, int32_t *targets, int32_t *n_targets,
                           msl_mem out_mem) noexcept {
    try {
    return batch_form(check_targets, launch_targets, device, mem == MSL_MEM_DEVICE, n_tab, ccap, n_items, nn, nn2, tcap, conn, n_conn, kf_flags,
                      cur, mem, targets, n_targets, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
