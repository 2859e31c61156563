// msl_sf_replay.hip -- map stage of the surfel fusion, the end of a deferred window: k_defer_tail -> k_replay -> k_gather -> k_scatter leave
// the array as the window's classic compactions (reference src/SurfelMapping.cpp:366-391) would have.  The stage's overview: msl_sf_map_dev.h.

#include "msl_sf_map_dev.h"

namespace {
// =============================================================================================
// Deferred compaction: the end of a window
// =============================================================================================
// k_defer_tail: what is left to do per keyframe once the window's F fuse launches are through.
//   workgroups 0 .. F - 1          : the updated-surfel count of keyframe f (sum of its per-sub-block counts) -> running total, CTR_UPDATED for the last
//   workgroups F .. F + NFRONT - 1 : the new surfels of the LAST keyframe (there is no next fuse launch to materialise them)
__global__ __launch_bounds__(64) void k_defer_tail(SfDev P, FuseArgs A, int F, unsigned blkStride) {   // A.kf = F
    __builtin_amdgcn_s_setprio(3);
    const unsigned lane = threadIdx.x;
    if ((int)blockIdx.x < F) {
        const int f = (int)blockIdx.x;
        // keyframe f's counts: one per sub-block below the extent its regular waves worked on, and behind them (from index E0 / SUB_ITEMS + 1 on) one per
        // 256 new surfels of keyframe f - 1 that its spawn wave wrote and fused
        const long long E0 = f > 0 ? P.dc->ext[f - 1] : P.dc->ext[0], Kp = f > 0 ? P.dc->ext[f] - E0 : 0;
        const long long nblk = (E0 + SUB_ITEMS - 1) / SUB_ITEMS, x0 = E0 / SUB_ITEMS + 1, x1 = x0 + (Kp + SUB_ITEMS - 1) / SUB_ITEMS;
        const unsigned *bu = P.blockUpd + (size_t)f * blkStride;
        unsigned u = 0;
        for (long long b = lane; b < nblk; b += 64) u += bu[b];
        for (long long b = x0 + lane; b < x1; b += 64) u += bu[b];
        u = wave_incl_scan(u);
        if (lane == 63) {
            atomicAdd(reinterpret_cast<unsigned long long *>(&P.ctr[CTR_TOT_UPDATED]), (unsigned long long)u);
            if (f == F - 1) P.ctr[CTR_UPDATED] = u;
        }
        return;
    }
    const long long E0 = P.dc->ext[F - 1];
    const long long q = (long long)blockIdx.x - F, sb = E0 / SUB_ITEMS + q;
    if (sb * SUB_ITEMS >= E0 + P.nseeds) return;
    unsigned excl;
    const unsigned K = spawn_count(A, lane, excl);
    if (q == 0 && lane == 0) P.dc->ext[F] = E0 + (long long)K;
    if (K && sb * SUB_ITEMS < E0 + (long long)K) emit_records(A, E0, sb * SUB_ITEMS, SUB_ITEMS / 64, lane, K, excl);
}

// k_replay: the window's F compactions, replayed symbolically by ONE wave.
// Elements are named by their PHYSICAL slot (nothing moved during the window): base elements 0 .. n0 - 1, the k-th new surfel of keyframe
// f = ext[f] + k.  The reference's array ("virtual" order) differs from the identity only where a compaction put something:
//   loc64[p]  = element at virtual position p, with the keyframe (stamp) that put it there      -- only for explicit placements
//   vposD[e]  = virtual position of element e                                                   -- only for elements placed explicitly
//   run f     = the new surfels of keyframe f that were APPENDED: elements ext[f] + k0 + q at virtual positions runV + q, q < runCnt
// (a run is clipped when a later keyframe shortens the array; where a run and an explicit entry both cover a position the later stamp wins).
// Per keyframe: virtual positions of the logged slots -> ascending (LDS rank sort; a bitmap over the positions beyond RP_SORT entries) ->
// new surfel k to the k-th largest hole, else appended (SurfelMapping.cpp:372-384) -> if holes remain, the back-to-front loop (:386-390) as
// k_compact resolves it: the a-th smallest leftover hole below the new end receives resolve(nFinal + a).  At the end every virtual position
// whose element is not already in that physical slot becomes one move (source, destination); k_gather / k_scatter apply them.
// All table traffic is agent-scope (L2): one wave, but its own stores must be what its later loads see.
constexpr int RP_SORT = 1024;          // deleted positions of one keyframe ordered in the LDS up to here
constexpr int RP_HASH = 2048;          // slots of the LDS tables (explicit placements of a window with <= RP_HASH / 2 deletions in all)
constexpr unsigned RP_EMPTY = 0xFFFFFFFFu;
struct ReplayLds {
    unsigned v[RP_SORT + 4], d[RP_SORT];                      // a keyframe's deleted positions: as logged, ascending
    long long ext[DEFER_WIN + 1], runV[DEFER_WIN];
    unsigned runK0[DEFER_WIN], runCnt[DEFER_WIN];
    unsigned dcnt[DEFER_WIN];                                 // deletions per keyframe
    unsigned log[RP_HASH / 2];                                // LDS mode: the whole window's deletion log (fetched in one trip)
    unsigned locK[RP_HASH], locV[RP_HASH], vposK[RP_HASH], vposV[RP_HASH];   // LDS tables (open addressing; locV = element + 1 | stamp << 26)
};
__device__ __forceinline__ unsigned rp_hash(unsigned key) { return (key * 2654435761u) >> 21; }   // 11 bits
static_assert(RP_HASH == 2048, "rp_hash yields 11 bits");

// LDS = true: the window's explicit placements live in two LDS hash tables (few deletions: the steady state; no global round trips inside the
// keyframe loop).  LDS = false: dense global tables indexed by position / element (any number of deletions; agent-scope accesses).
template <bool LDS>
__device__ __forceinline__ void replay_body(const SfDev &P, int F, ReplayLds &S) {
    const unsigned lane = threadIdx.x;
    DeferCtl *dc = P.dc;
    const long long n0 = S.ext[0];
    long long n = n0;
    unsigned nLocKeys = 0, nVposKeys = 0, logBase = 0;
    long long totK = 0, totD = 0, totNb = 0, lastK = 0, lastD = 0, lastNb = 0;
    // ---- the two tables: virtual position -> (element, stamp), element -> virtual position ----
    auto loc_get = [&](unsigned p, unsigned &elem, unsigned &stampOut) -> bool {
        if constexpr (LDS) {
            for (unsigned s = rp_hash(p);; s = (s + 1) & (RP_HASH - 1)) {
                const unsigned k = S.locK[s];
                if (k == RP_EMPTY) return false;
                if (k == p) { const unsigned v = S.locV[s]; elem = (v & 0x3FFFFFFu) - 1u; stampOut = v >> 26; return true; }
            }
        } else {
            const unsigned long long v = ld_agent64(&P.loc64[p]);
            if (!v) return false;
            elem = (unsigned)v - 1u; stampOut = (unsigned)(v >> 32);
            return true;
        }
    };
    auto vpos_get = [&](unsigned id, unsigned &pos) -> bool {
        if constexpr (LDS) {
            for (unsigned s = rp_hash(id);; s = (s + 1) & (RP_HASH - 1)) {
                const unsigned k = S.vposK[s];
                if (k == RP_EMPTY) return false;
                if (k == id) { pos = S.vposV[s]; return true; }
            }
        } else {
            const unsigned v = ld_agent(&P.vposD[id]);
            if (!v) return false;
            pos = v - 1u;
            return true;
        }
    };
    // explicit placement (all lanes call; `on` lanes place): element `elem` now sits at virtual position `pos`
    auto put = [&](bool on, unsigned pos, unsigned elem, unsigned stampNo) {
        if constexpr (LDS) {
            if (on) {
                unsigned s = rp_hash(pos);
                for (;; s = (s + 1) & (RP_HASH - 1)) { const unsigned old = atomicCAS(&S.locK[s], RP_EMPTY, pos); if (old == RP_EMPTY || old == pos) break; }
                S.locV[s] = (elem + 1u) | (stampNo << 26);
                s = rp_hash(elem);
                for (;; s = (s + 1) & (RP_HASH - 1)) { const unsigned old = atomicCAS(&S.vposK[s], RP_EMPTY, elem); if (old == RP_EMPTY || old == elem) break; }
                S.vposV[s] = pos;
            }
        } else {
            if (on) { st_agent64(&P.loc64[pos], (unsigned long long)(elem + 1u) | ((unsigned long long)stampNo << 32)); st_agent(&P.vposD[elem], pos + 1u); }
            const unsigned long long m = __ballot(on);
            if (on) { const unsigned r = lane_rank(m); st_agent(&P.locKeys[nLocKeys + r], pos); st_agent(&P.vposKeys[nVposKeys + r], elem); }
            nLocKeys += (unsigned)__popcll(m); nVposKeys += (unsigned)__popcll(m);
        }
    };
    auto tables_sync = [&]() {   // a keyframe's (or phase's) table stores are complete before anything reads them
        if constexpr (LDS) __syncthreads();
        else { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); }
    };
    unsigned runMask = 0;   // bit g: keyframe g appended a run that still has entries (uniform)
    auto vpos_of = [&](unsigned id) -> unsigned {
        unsigned pos;
        if (vpos_get(id, pos)) return pos;
        if ((long long)id < n0) return id;
        int g = 0;
        for (int q = 1; q < F; q++) if ((long long)id >= S.ext[q]) g = q;   // the keyframe that spawned it
        return (unsigned)(S.runV[g] + ((long long)id - S.ext[g] - (long long)S.runK0[g]));
    };
    // newest run covering p: its keyframe (-1: none) and element
    auto run_of = [&](long long p, int upto, unsigned &elem) -> int {
        for (unsigned m = upto >= 31 ? runMask : (runMask & ((2u << upto) - 1u)); m;) {   // (newest first; the steady state has no runs at all)
            const int g = 31 - __builtin_clz(m);
            m &= ~(1u << g);
            const long long v0 = S.runV[g];
            if (p >= v0 && p < v0 + (long long)S.runCnt[g]) { elem = (unsigned)(S.ext[g] + (long long)S.runK0[g] + (p - v0)); return g; }
        }
        return -1;
    };
    auto loc_of = [&](long long p, int upto) -> unsigned {
        unsigned ee = 0, st = 0, er = 0;
        const bool have = loc_get((unsigned)p, ee, st);
        const int g = run_of(p, upto, er);
        if (have && (g < 0 || st > (unsigned)(g + 1))) return ee;
        return g >= 0 ? er : (unsigned)p;
    };
    for (int f = 0; f < F; f++) {
        const unsigned D = S.dcnt[f];
        const long long K = S.ext[f + 1] - S.ext[f];
        const unsigned stampNo = (unsigned)(f + 1);
        const bool inLds = D <= (unsigned)RP_SORT;
        lastK = K; lastD = D; lastNb = n; totK += K; totD += D; totNb += n;
        // ---- 1. virtual positions of the logged slots ----
        for (unsigned j0 = 0; j0 < D; j0 += 64) {
            const unsigned j = j0 + lane;
            if (j < D) {
                const unsigned vp = vpos_of(LDS ? S.log[logBase + j] : ld_agent(&P.delList[logBase + j]));
                if (inLds) S.v[j] = vp;
                else atomicOr(&P.bitmap[vp >> 5], 1u << (vp & 31u));
            }
        }
        if (inLds && lane < 4) S.v[D + lane] = 0xFFFFFFFFu;   // padding of the last 16-byte read
        __syncthreads();
        // ---- 2. ascending order ----
        if (inLds) {
            for (unsigned j0 = 0; j0 < D; j0 += 64) {
                const unsigned j = j0 + lane;
                const unsigned v = j < D ? S.v[j] : 0u;
                unsigned r = 0;
                for (unsigned q = 0; q < D; q += 4) {   // (the positions are distinct: the ranks are a permutation)
                    const uint4 x = *reinterpret_cast<const uint4 *>(&S.v[q]);
                    r += (x.x < v ? 1u : 0u) + (x.y < v ? 1u : 0u) + (x.z < v ? 1u : 0u) + (x.w < v ? 1u : 0u);
                }
                if (j < D) S.d[r] = v;
            }
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const long long nw = (n + 31) >> 5;
            unsigned base = 0;
            for (long long w0 = 0; w0 < nw; w0 += 64) {
                const long long w = w0 + lane;
                unsigned bits = w < nw ? ld_agent(&P.bitmap[w]) : 0u;
                const unsigned c = (unsigned)__popc(bits);
                const unsigned incl = wave_incl_scan(c);
                unsigned o = base + incl - c;
                if (bits) st_agent(&P.bitmap[w], 0u);   // clean for the next use
                for (; bits; bits &= bits - 1) st_agent(&P.dBig[o++], (unsigned)(w * 32 + __builtin_ctz(bits)));
                base += (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        auto DL = [&](long long j) -> unsigned { return inLds ? S.d[j] : ld_agent(&P.dBig[j]); };
        // ---- 3. new surfel k -> k-th largest hole (SurfelMapping.cpp:372-384) ----
        const long long nPl = K < (long long)D ? K : (long long)D;
        for (long long k0 = 0; k0 < nPl; k0 += 64) {
            const long long k = k0 + lane;
            const bool on = k < nPl;
            put(on, on ? DL((long long)D - 1 - k) : 0u, (unsigned)(S.ext[f] + k), stampNo);
        }
        if (K > (long long)D) {   // the others are appended: a run
            if (lane == 0) { S.runV[f] = n; S.runK0[f] = D; S.runCnt[f] = (unsigned)(K - (long long)D); }
            runMask |= 1u << f;
            n += K - (long long)D;
        } else if ((long long)D > K) {
            // ---- 4. leftover holes: the back-to-front loop of :386-390, per hole ----
            const long long R = (long long)D - K, nFinal = n - R;
            tables_sync();   // (a tail source may be a surfel placed just above)
            auto lower = [&](long long x) -> long long {   // first index in the R smallest holes with value >= x
                long long lo = 0, hi = R;
                while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)DL(mid) < x) lo = mid + 1; else hi = mid; }
                return lo;
            };
            const long long cntLow = lower(nFinal);   // holes below the new end: each receives a tail element
            for (long long a0 = 0; a0 < cntLow; a0 += 64) {
                const long long a = a0 + lane;
                const bool on = a < cntLow;
                long long p = nFinal + (on ? a : 0);
                bool chain = on;
                while (__ballot(chain)) {
                    if (chain) {
                        const long long lb = lower(p);
                        if (lb < R && (long long)DL(lb) == p) p = n - (R - lb);   // a hole inside the tail only relays: follow to where its content comes from
                        else chain = false;
                    }
                }
                const unsigned e = on ? loc_of(p, f) : 0u;
                if constexpr (LDS) __syncthreads();   // (every lane has read the tables before this chunk's placements go in: a destination < nFinal is never a source, but slots move)
                put(on, on ? DL(a) : 0u, e, stampNo);
            }
            __syncthreads();
            if (runMask) {   // runs that reach beyond the new end are clipped
                bool gone = false;
                if ((int)lane <= f && ((runMask >> lane) & 1u) && S.runV[lane] + (long long)S.runCnt[lane] > nFinal) {
                    S.runCnt[lane] = S.runV[lane] >= nFinal ? 0u : (unsigned)(nFinal - S.runV[lane]);
                    gone = S.runCnt[lane] == 0;
                }
                runMask &= ~(unsigned)__ballot(gone);
            }
            n = nFinal;
        }
        tables_sync();
        logBase += D;
    }
    // ---- the moves: every virtual position whose element is not already in that physical slot ----
    const long long nF = n;
    unsigned nMoves = 0;
    auto add_move = [&](bool on, unsigned dst, unsigned src) {
        const unsigned long long m = __ballot(on);
        if (on) { const unsigned r = nMoves + lane_rank(m); P.moveDst[r] = dst; P.srcOf[r] = src; }
        nMoves += (unsigned)__popcll(m);
    };
    for (int g = 0; g < F; g++) {   // appended runs first, while the explicit table is intact
        const unsigned cnt = ((runMask >> g) & 1u) ? S.runCnt[g] : 0u;
        for (unsigned q0 = 0; q0 < cnt; q0 += 64) {
            const unsigned q = q0 + lane;
            bool on = q < cnt;
            const long long p = S.runV[g] + q;
            const unsigned id = (unsigned)(S.ext[g] + (long long)S.runK0[g] + q);
            unsigned ee = 0, st = 0;
            if (on && loc_get((unsigned)p, ee, st) && st > (unsigned)(g + 1)) on = false;   // a later explicit placement owns p
            if (on && (long long)id == p) on = false;
            add_move(on, (unsigned)p, id);
        }
    }
    // explicit placements: a stale one (a later run covers its position) or one beyond the final end is dropped
    auto explicit_move = [&](bool on, unsigned p, unsigned id, unsigned st) {
        unsigned er = 0;
        if (on) { const int g = run_of((long long)p, F - 1, er); if (g >= 0 && (unsigned)(g + 1) > st) on = false; }
        if (on && (long long)p >= nF) on = false;
        if (on && id == p) on = false;
        add_move(on, p, id);
    };
    if constexpr (LDS) {
        for (unsigned s0 = 0; s0 < (unsigned)RP_HASH; s0 += 64) {
            const unsigned k = S.locK[s0 + lane], v = S.locV[s0 + lane];
            explicit_move(k != RP_EMPTY, k, (v & 0x3FFFFFFu) - 1u, v >> 26);
        }
    } else {
        for (unsigned j0 = 0; j0 < nLocKeys; j0 += 64) {   // (a position may be listed more than once: cleared at its first visit)
            const unsigned j = j0 + lane;
            bool on = j < nLocKeys;
            const unsigned p = on ? ld_agent(&P.locKeys[j]) : 0u;
            const unsigned long long v = on ? ld_agent64(&P.loc64[p]) : 0ull;
            on = on && v != 0ull;
            if (on) st_agent64(&P.loc64[p], 0ull);
            explicit_move(on, p, (unsigned)v - 1u, (unsigned)(v >> 32));
        }
        for (unsigned j0 = 0; j0 < nVposKeys; j0 += 64) { const unsigned j = j0 + lane; if (j < nVposKeys) st_agent(&P.vposD[ld_agent(&P.vposKeys[j])], 0u); }
    }
    if (lane < DEFER_WIN) dc->delCnt[lane] = 0;   // the next window starts with empty logs
    if (lane == 0) {
        dc->nMoves = nMoves;
        P.ctr[CTR_LIVE] = nF; P.ctr[CTR_NEW] = lastK; P.ctr[CTR_DELETED] = lastD; P.ctr[CTR_BEFORE] = lastNb; P.ctr[CTR_AFTER] = nF;
        P.ctr[CTR_TOT_NEW] += totK; P.ctr[CTR_TOT_DELETED] += totD; P.ctr[CTR_TOT_KF] += F; P.ctr[CTR_TOT_BEFORE] += totNb;
    }
}

// k_replay: the window's F compactions, replayed symbolically by ONE wave.
// Elements are named by their PHYSICAL slot (nothing moved during the window): base elements 0 .. n0 - 1, the k-th new surfel of keyframe
// f = ext[f] + k.  The reference's array ("virtual" order) differs from the identity only where a compaction put something:
//   loc   : virtual position -> element, with the keyframe (stamp) that put it there      -- only explicit placements
//   vpos  : element -> virtual position                                                   -- only elements placed explicitly
//   run f : the new surfels of keyframe f that were APPENDED: elements ext[f] + k0 + q at virtual positions runV + q, q < runCnt
// (a run is clipped when a later keyframe shortens the array; where a run and an explicit entry both cover a position the later stamp wins).
// Per keyframe: virtual positions of the logged slots -> ascending (LDS rank sort; a bitmap over the positions beyond RP_SORT entries) ->
// new surfel k to the k-th largest hole, else appended (SurfelMapping.cpp:372-384) -> if holes remain, the back-to-front loop (:386-390) as
// k_compact resolves it: the a-th smallest leftover hole below the new end receives resolve(nFinal + a).  At the end every virtual position
// whose element is not already in that physical slot becomes one move (source, destination); k_gather / k_scatter apply them.
// Checked against the literal loop by a host model of exactly this scheme (tests/test_replay_model.py) and by the GPU parity tests.
__global__ __launch_bounds__(64) void k_replay(SfDev P, int F) {
    __shared__ __attribute__((aligned(16))) ReplayLds S;
    __builtin_amdgcn_s_setprio(3);   // one wave on the latency-critical map stream, next to the throughput-oriented batched kernels
    const unsigned lane = threadIdx.x;
    DeferCtl *dc = P.dc;
    if ((int)lane <= F) S.ext[lane] = dc->ext[lane];
    if (lane < DEFER_WIN) { S.runCnt[lane] = 0; S.runV[lane] = 0; S.runK0[lane] = 0; }
    const unsigned dmine = (int)lane < F ? ld_agent(&dc->delCnt[lane]) : 0u;
    if (lane < DEFER_WIN) S.dcnt[lane] = dmine;
    const unsigned dsum = wave_incl_scan(dmine);
    const unsigned totalD = (unsigned)__builtin_amdgcn_readlane((int)dsum, 63);
    const bool useLds = totalD <= (unsigned)RP_HASH / 2 && P.cap < (1ull << 26) - 1;
    if (useLds) {
        for (unsigned j = lane; j < totalD; j += 64) S.log[j] = ld_agent(&P.delList[j]);   // (all requests leave together)
        for (unsigned s = lane; s < (unsigned)RP_HASH; s += 64) { S.locK[s] = RP_EMPTY; S.vposK[s] = RP_EMPTY; }
    }
    __syncthreads();
    if (useLds) replay_body<true>(P, F, S);
    else replay_body<false>(P, F, S);
}

// The window's moves: all sources first (a destination may be another move's source), then all destinations.
__global__ __launch_bounds__(256) void k_gather(SfDev P) {
    const MapSoA &M = P.map;
    const unsigned nM = P.dc->nMoves;
    for (unsigned j = blockIdx.x * 256 + threadIdx.x; j < nM; j += gridDim.x * 256) {
        const unsigned s = P.srcOf[j];
        const HotPk h = M.hot[s];
        const ColdRec c = cold_load(M.cold + s);
        P.stageHot[j] = h; cold_store(P.stageCold + j, c);
        if (h.tl == HOT_WIDE) { P.stageUtl[2 * (size_t)j] = M.utlWide[2 * (size_t)s]; P.stageUtl[2 * (size_t)j + 1] = M.utlWide[2 * (size_t)s + 1]; }
        if (c.rgbf & COLD_WIDE) for (int q = 0; q < 3; q++) P.stageRgb[3 * (size_t)j + q] = M.rgbWide[3 * (size_t)s + q];
    }
}
__global__ __launch_bounds__(256) void k_scatter(SfDev P) {
    const MapSoA &M = P.map;
    const unsigned nM = P.dc->nMoves;
    for (unsigned j = blockIdx.x * 256 + threadIdx.x; j < nM; j += gridDim.x * 256) {
        const unsigned d = P.moveDst[j];
        const HotPk h = P.stageHot[j];
        const ColdRec c = cold_load(P.stageCold + j);
        M.hot[d] = h; cold_store(M.cold + d, c);
        if (h.tl == HOT_WIDE) { M.utlWide[2 * (size_t)d] = P.stageUtl[2 * (size_t)j]; M.utlWide[2 * (size_t)d + 1] = P.stageUtl[2 * (size_t)j + 1]; }
        if (c.rgbf & COLD_WIDE) for (int q = 0; q < 3; q++) M.rgbWide[3 * (size_t)d + q] = P.stageRgb[3 * (size_t)j + q];
    }
}
}  // namespace

namespace msl {
namespace sf {
// Closes a deferred window of F keyframes (P.prevSlotAbs = the slot of its last keyframe, P.blockUpd = the window's first per-sub-block slice).
void map_launch_replay(KernelProfiler &prof, hipStream_t st, const SfDev &P, int F, unsigned blkStride) {
    const unsigned nFront = (unsigned)((P.nseeds + SUB_ITEMS - 1) / SUB_ITEMS) + 1u;
    hipLaunchKernelGGL(k_defer_tail, dim3((unsigned)F + nFront), dim3(64), 0, st, P, fuse_args(P, 0, true, blkStride), F, blkStride);
    MSL_SF_LAUNCH(prof, SK_COMPACT, st, k_replay, dim3(1), dim3(64), P, F);
    hipLaunchKernelGGL(k_gather, dim3(128), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_scatter, dim3(128), dim3(256), 0, st, P);
}
}  // namespace sf
}  // namespace msl
