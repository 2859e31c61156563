// msl_observations.hip -- the producer of the observation table for gfx950: msl_observations_apply[_batch] executes a log of
// AddObservation / EraseObservation / SetBadFlag / Replace / KeyFrame::SetBadFlag edits (reference src/MapPoint.cc:83-187,
// src/MapLine.cpp:75-172, src/KeyFrame.cc:185-197 and :362-368) on the CSR table, the slots and the per-point arrays where they live, and
// writes the new CSR table.  tests/observations_model.py is the sequential model.
//   k_obs_run     one wave walks the log in order.  A point an op names gets a work slot in the handle's scratch: its per-point values and
//                 its observations, at most MSL_OBS_MAX, packed (keyframe << 13 | keypoint) and unordered, in a pool: a list that only
//                 shrinks has the room of its length on entry, one that grows moves once to room for MSL_OBS_MAX.  No op depends on the order of a
//                 list (the reference keyframe after an erasure is the smallest one left, Replace asks of every taken keyframe whether the
//                 survivor observes it, and the taken keyframes are distinct).  An op loads the lists it needs into LDS, lanes across the
//                 entries, and stores them back.  Slot writes go to a log in execution order.  Nothing of the caller's is written but
//                 op_status
//   k_obs_finish  one workgroup per work slot: sorts the list (rank sort in LDS), compares list and values with the point's state on
//                 entry (that is `touched`), and writes the per-point values back
//   k_obs_len, k_obs_scan, k_obs_write   the rebuild, the part that streams the table: per point the new length and whether it is
//                 touched, a scan of both over the points (workgroup sums, their scan, the scan again with its base), then one thread per
//                 point copies its range from the old table or from its work slot and places its id in `touched`
//   k_obs_slots   one workgroup replays the slot writes in order, 256 at a time; of two writes of one slot in a chunk the later stays
// Every kernel behind k_obs_run reads the count of too-long points from device memory and leaves the caller's arrays alone if it is not 0.
// The work is proportional to the log except for the rebuild and one memset of n_pts ints; no atomics.
#include "msl_match_handle.h"
#include "msl_index_check.h"
#include "msl_obs_walk.h"

namespace {

using namespace msl;

constexpr int RUN_NT = WAVE, SLOT_NT = 256, SCAN_NT = 1024, LMAX = MSL_OBS_MAX, MAX_OPS = MSL_OBS_MAX_OPS, MAX_KF_ERASE = MSL_OBS_MAX_KF_ERASE;
constexpr int IDX_BITS = 13;
static_assert(MAX_CAP == 1 << IDX_BITS && MAX_TAB << IDX_BITS > 0, "an observation packs into (keyframe << 13 | keypoint)");
static_assert(LMAX == SLOT_NT && LMAX == 4 * RUN_NT, "one thread per entry in k_obs_finish, four entries per lane in k_obs_run");
static_assert(MAX_PTS <= SCAN_NT * SCAN_NT, "the workgroup sums of the rebuild are scanned by one workgroup");
static_assert(check::OBS_ADD == MSL_OBS_ADD && check::OBS_ERASE == MSL_OBS_ERASE && check::OBS_SET_BAD == MSL_OBS_SET_BAD &&
              check::OBS_REPLACE == MSL_OBS_REPLACE && check::OBS_KF_ERASE == MSL_OBS_KF_ERASE && check::OBS_MAX_KF_ERASE == MAX_KF_ERASE,
              "msl_index_check.h names the codes of msl.h");
static_assert(sizeof(msl_obs_op) == 16, "ops are read as four ints");

enum { CTR_SLOTS, CTR_WRITES, CTR_LONG, CTR_BAD, CTR_TOTAL, CTR_TOUCHED, CTR_N = 8 };

struct ObsDev {
    int nTab, cap, nPts, nObs, nOps, ocap, tcap, nBlocks;
    long long wcap;
    int poolCap;
    const int32_t *nKps; const float *uright; const int32_t *off, *okf, *oidx; const msl_obs_op *ops;
    int32_t *held; uint8_t *flags; int32_t *ptNobs, *ref, *found, *visible, *replaced;
    int32_t *offOut, *okfOut, *oidxOut; uint8_t *opStatus; int32_t *touched, *counts;
    // scratch: per point its work slot; the counters; per workgroup of the rebuild (length, touched) sums and their scan; per work slot the
    // point, its values and its list; the slot writes
    int32_t *slotOf, *ctr, *blk, *blkBase;
    int32_t *wId, *wLen, *wOff, *wRoom, *wNobs, *wRef, *wFound, *wVisible, *wReplaced, *wList; uint8_t *wFlags, *wLong, *wChanged;
    int2 *wlog;
};

__device__ __forceinline__ int obs_pack(int k, int i) { return (k & (MAX_TAB - 1)) << IDX_BITS | (i & (MAX_CAP - 1)); }
__device__ __forceinline__ int obs_weight(const ObsDev &D, int e) {
    const int k = e >> IDX_BITS, i = e & (MAX_CAP - 1);
    return D.uright && k < D.nTab && i < D.cap && D.uright[(size_t)k * D.cap + i] >= 0 ? 2 : 1;
}
__device__ __forceinline__ int obs_slot_addr(const ObsDev &D, int e) {
    const int k = e >> IDX_BITS, i = e & (MAX_CAP - 1);
    return k < D.nTab && i < D.cap ? k * D.cap + i : -1;
}

// ==== k_obs_run: the log in order, one wave ==================================================================================================
struct Point { int id, slot, n, off, room, flags, nobs, ref, found, visible, replaced; bool tooLong; };   // uniform over the wave
struct Run { int nSlots, nLong, nBad, poolTop; long long nWrites; };

__device__ __forceinline__ void pt_store(const ObsDev &D, const Point &P, const int *L) {
    const int lane = threadIdx.x;
    for (int j = lane; j < P.n; j += RUN_NT) D.wList[P.off + j] = L[j];
    if (lane == 0) {
        D.wLen[P.slot] = P.n; D.wOff[P.slot] = P.off; D.wRoom[P.slot] = P.room; D.wNobs[P.slot] = P.nobs; D.wRef[P.slot] = P.ref; D.wFound[P.slot] = P.found; D.wVisible[P.slot] = P.visible;
        D.wReplaced[P.slot] = P.replaced; D.wFlags[P.slot] = (uint8_t)P.flags; D.wLong[P.slot] = P.tooLong;
    }
    __syncthreads();
}

// The state of point p and its list in L: from its work slot, or from the tables on entry into a new slot
__device__ __forceinline__ void pt_open(const ObsDev &D, Run &R, int p, Point &P, int *L) {
    const int lane = threadIdx.x;
    __syncthreads();
    P.id = p; P.slot = D.slotOf[p];
    if (P.slot >= 0) {
        const int s = P.slot;
        P.n = D.wLen[s]; P.off = D.wOff[s]; P.room = D.wRoom[s]; P.nobs = D.wNobs[s]; P.ref = D.wRef[s]; P.found = D.wFound[s]; P.visible = D.wVisible[s]; P.replaced = D.wReplaced[s];
        P.flags = D.wFlags[s]; P.tooLong = D.wLong[s];
        for (int j = lane; j < P.n; j += RUN_NT) L[j] = D.wList[P.off + j];
        __syncthreads();
        return;
    }
    int b, e;
    obs_range(D, p, b, e);
    P.slot = R.nSlots++;
    P.n = e - b; P.tooLong = P.n > LMAX;
    // ranges that overlap (offsets that are not ascending: device memory only) can outgrow the pool, which is sized for disjoint ones
    P.tooLong = P.tooLong || P.n > D.poolCap - R.poolTop;
    if (P.tooLong) { P.n = 0; R.nLong++; }
    P.off = R.poolTop; P.room = P.n; R.poolTop += P.n;
    for (int j = lane; j < P.n; j += RUN_NT) L[j] = obs_pack(D.okf[b + j], D.oidx[b + j]);
    P.flags = D.flags[p]; P.nobs = D.ptNobs[p]; P.ref = D.ref[p];
    P.found = D.found ? D.found[p] : 0; P.visible = D.visible ? D.visible[p] : 0; P.replaced = D.replaced ? D.replaced[p] : -1;
    if (lane == 0) { D.slotOf[p] = P.slot; D.wId[P.slot] = p; }
    __syncthreads();
    pt_store(D, P, L);
}

// Room for MSL_OBS_MAX entries for a list about to grow beyond its own (the entries are in LDS: the next pt_store writes them there)
// False: the pool is full (overlapping ranges, see pt_open), and the point counts as too long.
__device__ __forceinline__ bool pt_grow(const ObsDev &D, Run &R, Point &P) {
    if (P.room == LMAX) return true;
    if (LMAX > D.poolCap - R.poolTop) return false;
    P.off = R.poolTop; P.room = LMAX; R.poolTop += LMAX;
    return true;
}

// The position of keyframe k in a list, or -1
__device__ __forceinline__ int list_find(const int *L, int n, int k) {
    for (int base = 0; base < n; base += RUN_NT) {
        const int j = base + (int)threadIdx.x;
        const unsigned long long m = __ballot(j < n && L[j] >> IDX_BITS == k);
        if (m) return base + __ffsll(m) - 1;
    }
    return -1;
}

// The writes held_id[k][i] = value of entries [0, n) of a list, appended to the log
__device__ __forceinline__ void log_list(const ObsDev &D, Run &R, const int *L, int n, int value) {
    for (int j = threadIdx.x; j < n; j += RUN_NT)
        if (R.nWrites + j < D.wcap) D.wlog[R.nWrites + j] = make_int2(obs_slot_addr(D, L[j]), value);
    R.nWrites += n;
}

// SetBadFlag of an open point
__device__ __forceinline__ int pt_set_bad(const ObsDev &D, Run &R, Point &P, const int *L) {
    const bool live = P.flags & 1;
    const int st = (live || P.n > 0 ? MSL_OBS_CHANGED : 0) | (live ? MSL_OBS_TURNED_BAD : 0);
    log_list(D, R, L, P.n, -1);
    P.flags &= ~1; P.n = 0; R.nBad += live;
    return st;
}

__device__ __forceinline__ int op_erase(const ObsDev &D, Run &R, int a, int k, int *L) {
    Point P;
    pt_open(D, R, a, P, L);
    if (P.tooLong) return 0;
    const int pos = list_find(L, P.n, k);
    if (pos < 0) return 0;
    P.nobs -= obs_weight(D, L[pos]);
    __syncthreads();
    if (threadIdx.x == 0) L[pos] = L[P.n - 1];
    P.n--;
    __syncthreads();
    if (P.ref == k) {                                                          // the first keyframe left; none: -1 (the reference reads end())
        unsigned lo = 0xFFFFFFFFu;
        for (int j = threadIdx.x; j < P.n; j += RUN_NT) lo = min(lo, (unsigned)(L[j] >> IDX_BITS));
        P.ref = P.n ? (int)wave_min(lo) : -1;
    }
    int st = MSL_OBS_CHANGED;
    if (P.nobs <= 2) st |= pt_set_bad(D, R, P, L);
    pt_store(D, P, L);
    return st;
}

__device__ __forceinline__ int op_add(const ObsDev &D, Run &R, int a, int k, int i, int *L) {
    Point P;
    pt_open(D, R, a, P, L);
    if (P.tooLong) return 0;
    int st = 0;
    if (list_find(L, P.n, k) < 0) {
        if (P.n == LMAX || !pt_grow(D, R, P)) { P.tooLong = true; R.nLong++; pt_store(D, P, L); return 0; }
        __syncthreads();
        if (threadIdx.x == 0) L[P.n] = obs_pack(k, i);
        P.n++; P.nobs += obs_weight(D, obs_pack(k, i));
        st = MSL_OBS_CHANGED;
        __syncthreads();
    }
    if (threadIdx.x == 0 && R.nWrites < D.wcap) D.wlog[R.nWrites] = make_int2(k * D.cap + i, a);
    R.nWrites++;
    pt_store(D, P, L);
    return st;
}

__device__ __forceinline__ int op_set_bad(const ObsDev &D, Run &R, int a, int *L) {
    Point P;
    pt_open(D, R, a, P, L);
    if (P.tooLong) return 0;
    const int st = pt_set_bad(D, R, P, L);
    pt_store(D, P, L);
    return st;
}

__device__ __forceinline__ int op_replace(const ObsDev &D, Run &R, int a, int b, int *LA, int *LB) {
    if (a == b) return 0;
    Point A, B;
    pt_open(D, R, a, A, LA);
    pt_open(D, R, b, B, LB);
    if (A.tooLong || B.tooLong) return 0;
    const int lane = threadIdx.x;
    bool mv[LMAX / RUN_NT];                                                    // entry lane + 64 c of a moves to b: b does not observe its keyframe
    int moved = 0;
#pragma unroll
    for (int c = 0; c < LMAX / RUN_NT; c++) {
        const int j = lane + RUN_NT * c;
        mv[c] = false;
        if (j < A.n) {
            const int k = LA[j] >> IDX_BITS;
            bool in_b = false;
            for (int q = 0; q < B.n; q++) in_b |= LB[q] >> IDX_BITS == k;
            mv[c] = !in_b;
        }
        moved += __popcll(__ballot(mv[c]));
    }
    if (B.n + moved > LMAX || (moved && !pt_grow(D, R, B))) { B.tooLong = true; R.nLong++; pt_store(D, B, LB); return 0; }
    __syncthreads();
    int base = B.n, w = 0;
#pragma unroll
    for (int c = 0; c < LMAX / RUN_NT; c++) {
        const int j = lane + RUN_NT * c;
        const unsigned long long m = __ballot(mv[c]);
        if (j < A.n) {
            const int e = LA[j];
            if (R.nWrites + j < D.wcap) D.wlog[R.nWrites + j] = make_int2(obs_slot_addr(D, e), mv[c] ? b : -1);
            if (mv[c]) { LB[base + __popcll(m & ((1ull << lane) - 1ull))] = e; w += obs_weight(D, e); }
        }
        base += __popcll(m);
    }
    R.nWrites += A.n;
    const bool live = A.flags & 1;
    const int st = (live || A.n > 0 || (D.replaced && A.replaced != b) || A.found != 0 || A.visible != 0 ? MSL_OBS_CHANGED : 0) |
                   (live ? MSL_OBS_TURNED_BAD : 0);
    B.n = base; B.nobs += wave_sum(w);
    B.found = (int)((unsigned)B.found + (unsigned)A.found); B.visible = (int)((unsigned)B.visible + (unsigned)A.visible);
    A.flags &= ~1; A.n = 0; A.replaced = b; R.nBad += live;
    __syncthreads();
    pt_store(D, A, LA);
    pt_store(D, B, LB);
    return st;
}

__global__ __launch_bounds__(RUN_NT) void k_obs_run(ObsDev D) {
    __shared__ int s_a[LMAX], s_b[LMAX];
    const int lane = threadIdx.x;
    Run R{0, 0, 0, 0, 0};
    int n_kf_erase = 0;
    for (int o = 0; o < D.nOps; o++) {
        const msl_obs_op op = D.ops[o];
        const bool a_ok = op.a >= 0 && op.a < D.nPts, kf_ok = op.b >= 0 && op.b < D.nTab;
        int st = 0;
        if (op.op == MSL_OBS_ADD) {
            if (a_ok && kf_ok && op.c >= 0 && op.c < clampi(D.nKps[op.b], 0, D.cap)) st = op_add(D, R, op.a, op.b, op.c, s_a);
        } else if (op.op == MSL_OBS_ERASE) {
            if (a_ok && kf_ok) st = op_erase(D, R, op.a, op.b, s_a);
        } else if (op.op == MSL_OBS_SET_BAD) {
            if (a_ok) st = op_set_bad(D, R, op.a, s_a);
        } else if (op.op == MSL_OBS_REPLACE) {
            if (a_ok && op.b >= 0 && op.b < D.nPts) st = op_replace(D, R, op.a, op.b, s_a, s_b);
        } else if (op.op == MSL_OBS_KF_ERASE) {
            if (kf_ok && n_kf_erase++ < MAX_KF_ERASE) {
                const int n = clampi(D.nKps[op.b], 0, D.cap);                  // the slots on entry: the slot log is replayed behind this kernel
                for (int base = 0; base < n; base += RUN_NT) {
                    const int mine = base + lane < n ? D.held[(size_t)op.b * D.cap + base + lane] : -1;
                    for (int i = 0; i < min(RUN_NT, n - base); i++) {
                        const int p = __shfl(mine, i);
                        if (p >= 0 && p < D.nPts) st |= op_erase(D, R, p, op.b, s_a);
                    }
                }
            }
        }
        if (lane == 0) D.opStatus[o] = (uint8_t)st;
    }
    if (lane == 0) {
        D.ctr[CTR_SLOTS] = R.nSlots; D.ctr[CTR_WRITES] = (int)(R.nWrites < D.wcap ? R.nWrites : D.wcap); D.ctr[CTR_LONG] = R.nLong;
        D.ctr[CTR_BAD] = R.nBad;
    }
}

// ==== k_obs_finish: one workgroup per work slot ==============================================================================================
__global__ __launch_bounds__(SLOT_NT) void k_obs_finish(ObsDev D) {
    __shared__ int s_in[LMAX], s_sorted[LMAX];
    const int t = threadIdx.x, n_slots = D.ctr[CTR_SLOTS];
    const bool too_long = D.ctr[CTR_LONG] != 0;
    for (int s = blockIdx.x; s < n_slots; s += gridDim.x) {
        const int p = D.wId[s], n = D.wLen[s], off = D.wOff[s];
        const int e = t < n ? D.wList[off + t] : 0;
        s_in[t] = e;
        __syncthreads();
        if (t < n) {                                                           // keyframes are distinct; equal entries (broken tables) keep their order
            int r = 0;
            for (int j = 0; j < n; j++) r += s_in[j] < e || (s_in[j] == e && j < t);
            s_sorted[r] = e;
        }
        __syncthreads();
        int b, en;
        obs_range(D, p, b, en);
        bool same = en - b == n;
        if (same && t < n) same = obs_pack(D.okf[b + t], D.oidx[b + t]) == s_sorted[t];
        if (t < n) D.wList[off + t] = s_sorted[t];
        const bool list_same = __syncthreads_and(same);
        if (t == 0) {
            const int flags = D.wFlags[s], nobs = D.wNobs[s], ref = D.wRef[s], found = D.wFound[s], visible = D.wVisible[s], replaced = D.wReplaced[s];
            bool changed = !list_same || flags != D.flags[p] || nobs != D.ptNobs[p] || ref != D.ref[p];
            if (D.found) changed = changed || found != D.found[p] || visible != D.visible[p];
            if (D.replaced) changed = changed || replaced != D.replaced[p];
            D.wChanged[s] = changed && !D.wLong[s];
            if (!too_long && changed) {
                D.flags[p] = (uint8_t)flags; D.ptNobs[p] = nobs; D.ref[p] = ref;
                if (D.found) { D.found[p] = found; D.visible[p] = visible; }
                if (D.replaced) D.replaced[p] = replaced;
            }
        }
        __syncthreads();
    }
}

// ==== the rebuild ============================================================================================================================
// The new length of point p's range and whether the point is touched
__device__ __forceinline__ void new_length(const ObsDev &D, int p, int &slot, unsigned &len, unsigned &touched) {
    slot = -1; len = 0; touched = 0;
    if (p >= D.nPts) return;
    slot = D.slotOf[p];
    if (slot >= 0) { len = (unsigned)D.wLen[slot]; touched = D.wChanged[slot]; return; }
    int b, e;
    obs_range(D, p, b, e);
    len = (unsigned)(e - b);
}

__global__ __launch_bounds__(SCAN_NT) void k_obs_len(ObsDev D) {
    __shared__ unsigned s_wave[32];
    int slot;
    unsigned len, touched, tot_len, tot_touched, ex_len, ex_touched;
    new_length(D, blockIdx.x * SCAN_NT + threadIdx.x, slot, len, touched);
    block_excl_scan_pair(len, touched, s_wave, &tot_len, &tot_touched, ex_len, ex_touched);
    if (threadIdx.x == 0) { D.blk[2 * blockIdx.x] = (int)tot_len; D.blk[2 * blockIdx.x + 1] = (int)tot_touched; }
}

__global__ __launch_bounds__(SCAN_NT) void k_obs_scan(ObsDev D) {
    __shared__ unsigned s_wave[32];
    const int t = threadIdx.x;
    const unsigned len = t < D.nBlocks ? (unsigned)D.blk[2 * t] : 0u, touched = t < D.nBlocks ? (unsigned)D.blk[2 * t + 1] : 0u;
    unsigned tot_len, tot_touched, ex_len, ex_touched;
    block_excl_scan_pair(len, touched, s_wave, &tot_len, &tot_touched, ex_len, ex_touched);
    if (t < D.nBlocks) { D.blkBase[2 * t] = (int)ex_len; D.blkBase[2 * t + 1] = (int)ex_touched; }
    if (t == 0) {
        const int n_long = D.ctr[CTR_LONG];
        D.ctr[CTR_TOTAL] = (int)tot_len; D.ctr[CTR_TOUCHED] = (int)tot_touched;
        D.counts[0] = n_long ? D.nObs : (int)tot_len; D.counts[1] = n_long ? 0 : (int)tot_touched; D.counts[2] = n_long;
        D.counts[3] = n_long ? 0 : D.ctr[CTR_BAD];
        if (!n_long) D.offOut[D.nPts] = (int)tot_len;
    }
}

__global__ __launch_bounds__(SCAN_NT) void k_obs_write(ObsDev D) {
    __shared__ unsigned s_wave[32];
    const int p = blockIdx.x * SCAN_NT + threadIdx.x;
    int slot;
    unsigned len, touched, tot_len, tot_touched, ex_len, ex_touched;
    new_length(D, p, slot, len, touched);
    block_excl_scan_pair(len, touched, s_wave, &tot_len, &tot_touched, ex_len, ex_touched);
    if (D.ctr[CTR_LONG] != 0) return;
    if (p < D.tcap && p >= D.ctr[CTR_TOUCHED]) D.touched[p] = -1;              // behind the count (tcap <= n_pts: the grid covers it)
    if (p >= D.nPts) return;
    const unsigned at = (unsigned)D.blkBase[2 * blockIdx.x] + ex_len, rank = (unsigned)D.blkBase[2 * blockIdx.x + 1] + ex_touched;
    D.offOut[p] = (int)at;
    if (touched && rank < (unsigned)D.tcap) D.touched[rank] = p;
    if (slot >= 0) {
        const int from = D.wOff[slot];
        for (unsigned j = 0; j < len && at + j < (unsigned)D.ocap; j++) {
            const int e = D.wList[from + j];
            D.okfOut[at + j] = e >> IDX_BITS; D.oidxOut[at + j] = e & (MAX_CAP - 1);
        }
    } else {
        const int b = clampi(D.off[p], 0, D.nObs);
        for (unsigned j = 0; j < len && at + j < (unsigned)D.ocap; j++) { D.okfOut[at + j] = D.okf[b + j]; D.oidxOut[at + j] = D.oidx[b + j]; }
    }
}

// ==== k_obs_slots: the slot writes in order ==================================================================================================
__global__ __launch_bounds__(SLOT_NT) void k_obs_slots(ObsDev D) {
    __shared__ int s_addr[SLOT_NT];
    if (D.ctr[CTR_LONG] != 0) return;
    const int t = threadIdx.x, n = D.ctr[CTR_WRITES];
    for (int base = 0; base < n; base += SLOT_NT) {
        const int2 w = base + t < n ? D.wlog[base + t] : make_int2(-1, 0);
        s_addr[t] = w.x;
        __syncthreads();
        bool last = w.x >= 0;
        for (int j = t + 1; last && j < SLOT_NT; j++) last = s_addr[j] != w.x;
        if (last) D.held[w.x] = w.y;
        __syncthreads();                                                       // the next chunk's writes come behind this one's
    }
}

// ==== host side ==============================================================================================================================
const char *const WHO = "msl_observations_apply";

int check_apply(int n_tab, int cap, int n_pts, int n_obs_total, int n_ops, int ocap, int tcap, const int32_t *n_kps, const float *uright,
                const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const msl_obs_op *ops, int32_t *held_id, uint8_t *pt_flags,
                int32_t *pt_nobs, int32_t *pt_ref, int32_t *pt_found, int32_t *pt_visible, int32_t *pt_replaced, msl_mem mem, int32_t *obs_off_out,
                int32_t *obs_kf_out, int32_t *obs_idx_out, uint8_t *op_status, int32_t *touched, int32_t *counts, msl_mem) {
    const char *who = WHO;
    if (!none_null(who, {MSL_NAMED(n_kps), MSL_NAMED(obs_off), MSL_NAMED(obs_kf), MSL_NAMED(obs_idx), MSL_NAMED(ops), MSL_NAMED(held_id),
                         MSL_NAMED(pt_flags), MSL_NAMED(pt_nobs), MSL_NAMED(pt_ref), MSL_NAMED(obs_off_out), MSL_NAMED(obs_kf_out),
                         MSL_NAMED(obs_idx_out), MSL_NAMED(op_status), MSL_NAMED(touched), MSL_NAMED(counts)}))
        return MSL_ERR_INVALID;
    if (!pt_found != !pt_visible) {
        set_error("%s: %s is NULL while %s is given", who, pt_found ? "pt_visible" : "pt_found", pt_found ? "pt_found" : "pt_visible");
        return MSL_ERR_INVALID;
    }
    if (!table_limits(who, n_tab, cap, n_pts)) return MSL_ERR_INVALID;
    if (n_obs_total < 0) { set_error("%s: n_obs_total %d below 0", who, n_obs_total); return MSL_ERR_INVALID; }
    if (!in_range(who, "n_ops", n_ops, 1, MAX_OPS)) return MSL_ERR_INVALID;
    if (ocap < n_obs_total) { set_error("%s: ocap %d below n_obs_total = %d", who, ocap, n_obs_total); return MSL_ERR_INVALID; }
    if (tcap < 1 || tcap > n_pts) { set_error("%s: tcap %d outside 1 .. n_pts = %d", who, tcap, n_pts); return MSL_ERR_INVALID; }
    char why[256];
    if (mem == MSL_MEM_HOST && (!check::csr_ok(n_tab, cap, n_pts, n_obs_total, obs_off, obs_kf, obs_idx, n_kps, why, sizeof(why)) ||
                                !check::obs_ascending_ok(n_pts, obs_off, obs_kf, why, sizeof(why)) ||
                                !check::obs_ops_ok(n_tab, cap, n_pts, n_obs_total, n_ops, ocap, n_kps, &ops->op, why, sizeof(why))))
        return refuse(who, why);
    (void)uright; (void)pt_replaced;
    return MSL_OK;
}

template <class T>
T *carve(char *&at, size_t count) {
    T *p = (T *)at;
    at += (sizeof(T) * count + 255) / 256 * 256;
    return p;
}

int launch_apply(msl_match *h, int n_tab, int cap, int n_pts, int n_obs_total, int n_ops, int ocap, int tcap, const int32_t *n_kps,
                 const float *uright, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const msl_obs_op *ops,
                 int32_t *held_id, uint8_t *pt_flags, int32_t *pt_nobs, int32_t *pt_ref, int32_t *pt_found, int32_t *pt_visible,
                 int32_t *pt_replaced, msl_mem mem, int32_t *obs_off_out, int32_t *obs_kf_out, int32_t *obs_idx_out, uint8_t *op_status,
                 int32_t *touched, int32_t *counts, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t T = (size_t)n_tab, np = (size_t)n_pts, no = (size_t)n_obs_total, oc = (size_t)ocap;
    ObsDev D{};
    D.nTab = n_tab; D.cap = cap; D.nPts = n_pts; D.nObs = n_obs_total; D.nOps = n_ops; D.ocap = ocap; D.tcap = tcap;
    D.nBlocks = (n_pts + SCAN_NT - 1) / SCAN_NT;
    Stage S(h, mem, out_mem);
    D.nKps = S.in(n_kps, T); D.uright = S.in(uright, T * cap); D.off = S.in(obs_off, np + 1);
    D.okf = S.in(no ? obs_kf : nullptr, no); D.oidx = S.in(no ? obs_idx : nullptr, no); D.ops = S.in(ops, (size_t)n_ops);
    D.held = S.inout_in_mem(held_id, T * cap); D.flags = S.inout_in_mem(pt_flags, np); D.ptNobs = S.inout_in_mem(pt_nobs, np);
    D.ref = S.inout_in_mem(pt_ref, np); D.found = S.inout_in_mem(pt_found, np); D.visible = S.inout_in_mem(pt_visible, np);
    D.replaced = S.inout_in_mem(pt_replaced, np);
    // the new table keeps its bytes when a point is too long: a host-memory array is staged with its contents
    D.offOut = S.inout(obs_off_out, np + 1); D.okfOut = S.inout(oc ? obs_kf_out : nullptr, oc); D.oidxOut = S.inout(oc ? obs_idx_out : nullptr, oc);
    D.opStatus = S.out(op_status, (size_t)n_ops); D.touched = S.out(touched, (size_t)tcap); D.counts = S.out(counts, 4);
    MSL_HIP_TRY(S.error());
    // Every op names at most two points, an MSL_OBS_KF_ERASE at most cap; a point has one slot.  A slot write is an MSL_OBS_ADD's own, the
    // death of an observation (SetBadFlag: each of the n_obs_total + n_ops observations dies once) or one of the at most MSL_OBS_MAX an
    // MSL_OBS_REPLACE takes.
    const size_t kfe = (size_t)(n_ops < MAX_KF_ERASE ? n_ops : MAX_KF_ERASE) * cap, named = 2 * (size_t)n_ops + kfe;
    const size_t slots = named < np ? named : np;
    const size_t deaths = no + n_ops < slots * LMAX ? no + n_ops : slots * LMAX;
    const size_t alive = no + n_ops < (size_t)LMAX ? no + n_ops : (size_t)LMAX;   // the most one MSL_OBS_REPLACE takes
    D.wcap = (long long)((size_t)n_ops + deaths + (size_t)n_ops * alive);
    const size_t index_bytes = 256 * 3 + sizeof(int32_t) * (np + CTR_N + 4 * SCAN_NT) + 256;
    // the pool: the lists on entry of the points named, and room for MSL_OBS_MAX for each of the at most n_ops lists that grow
    const size_t pool = (no < slots * LMAX ? no : slots * LMAX) + (size_t)n_ops * LMAX;
    D.poolCap = (int)pool;
    const size_t slot_bytes = 256 * 13 + slots * (sizeof(int32_t) * 9 + 3) + sizeof(int32_t) * pool;
    MSL_HIP_TRY(grow_all(h->stream, {{h->obsIndex, index_bytes}, {h->obsSlots, slot_bytes}, {h->obsWrites, sizeof(int2) * (size_t)D.wcap}}));
    char *at = (char *)h->obsIndex.p;
    D.slotOf = carve<int32_t>(at, np); D.ctr = carve<int32_t>(at, CTR_N); D.blk = carve<int32_t>(at, 2 * SCAN_NT); D.blkBase = carve<int32_t>(at, 2 * SCAN_NT);
    at = (char *)h->obsSlots.p;
    D.wId = carve<int32_t>(at, slots); D.wLen = carve<int32_t>(at, slots); D.wOff = carve<int32_t>(at, slots); D.wRoom = carve<int32_t>(at, slots); D.wNobs = carve<int32_t>(at, slots); D.wRef = carve<int32_t>(at, slots);
    D.wFound = carve<int32_t>(at, slots); D.wVisible = carve<int32_t>(at, slots); D.wReplaced = carve<int32_t>(at, slots);
    D.wList = carve<int32_t>(at, pool); D.wFlags = carve<uint8_t>(at, slots); D.wLong = carve<uint8_t>(at, slots);
    D.wChanged = carve<uint8_t>(at, slots);
    D.wlog = (int2 *)h->obsWrites.p;
    hipStream_t st = h->stream;
    MSL_HIP_TRY(hipMemsetAsync(D.slotOf, 0xFF, sizeof(int32_t) * np, st));
    const unsigned finish_blocks = (unsigned)(slots < 2048 ? slots : 2048);
    hipLaunchKernelGGL(k_obs_run, dim3(1), dim3(RUN_NT), 0, st, D);
    hipLaunchKernelGGL(k_obs_finish, dim3(finish_blocks), dim3(SLOT_NT), 0, st, D);
    hipLaunchKernelGGL(k_obs_len, dim3((unsigned)D.nBlocks), dim3(SCAN_NT), 0, st, D);
    hipLaunchKernelGGL(k_obs_scan, dim3(1), dim3(SCAN_NT), 0, st, D);
    hipLaunchKernelGGL(k_obs_write, dim3((unsigned)D.nBlocks), dim3(SCAN_NT), 0, st, D);
    hipLaunchKernelGGL(k_obs_slots, dim3(1), dim3(SLOT_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_observations_apply(msl_match *h, int n_tab, int cap, int n_pts, int n_obs_total, int n_ops, int ocap, int tcap, const int32_t *n_kps,
                           const float *uright, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const msl_obs_op *ops,
                           int32_t *held_id, uint8_t *pt_flags, int32_t *pt_nobs, int32_t *pt_ref, int32_t *pt_found, int32_t *pt_visible,
                           int32_t *pt_replaced, msl_mem mem, int32_t *obs_off_out, int32_t *obs_kf_out, int32_t *obs_idx_out,
                           uint8_t *op_status, int32_t *touched, int32_t *counts, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO, check_apply, launch_apply, h, n_tab, cap, n_pts, n_obs_total, n_ops, ocap, tcap, n_kps, uright, obs_off, obs_kf,
                       obs_idx, ops, held_id, pt_flags, pt_nobs, pt_ref, pt_found, pt_visible, pt_replaced, mem, obs_off_out, obs_kf_out,
                       obs_idx_out, op_status, touched, counts, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_observations_apply_batch(int device, int n_tab, int cap, int n_pts, int n_obs_total, int n_ops, int ocap, int tcap,
                                 const int32_t *n_kps, const float *uright, const int32_t *obs_off, const int32_t *obs_kf,
                                 const int32_t *obs_idx, const msl_obs_op *ops, int32_t *held_id, uint8_t *pt_flags, int32_t *pt_nobs,
                                 int32_t *pt_ref, int32_t *pt_found, int32_t *pt_visible, int32_t *pt_replaced, msl_mem mem,
                                 int32_t *obs_off_out, int32_t *obs_kf_out, int32_t *obs_idx_out, uint8_t *op_status, int32_t *touched,
                                 int32_t *counts, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_apply, launch_apply, device, mem == MSL_MEM_DEVICE, n_tab, cap, n_pts, n_obs_total, n_ops, ocap, tcap, n_kps, uright,
                      obs_off, obs_kf, obs_idx, ops, held_id, pt_flags, pt_nobs, pt_ref, pt_found, pt_visible, pt_replaced, mem, obs_off_out,
                      obs_kf_out, obs_idx_out, op_status, touched, counts, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
