// msl_assign.h -- the greedy, order-dependent hand-out of the reference's SearchByProjection loops, solved by one workgroup as a
// min-fixpoint (internal).  Used by k_match_assign, k_local_assign (msl_match.hip) and k_line_assign<> (msl_line_match.hip).
//
// The sequential loop.  Queries j = 0 .. nQ-1 (last-frame points, local map points, lines) run in order.  Query j looks at its candidate
// targets (keypoints / keylines of the current frame), SKIPS a target that is at that moment held by a query with Observations() > 0
// (src/ORBmatcher.cc:80-82 and :619-621, src/LSDmatcher.cpp:105-107 and :169-171), chooses among the rest by a rule of its own (best
// distance, best / second-best ratio, thresholds: the call site's pick function) and writes itself into the chosen target, overwriting
// whoever held it.
//
// The fixpoint.
//   * pick(j) is a function of the set of targets query j skips, and of nothing else: the call site's pick function sees every candidate
//     and the skip test, and its best / second-best updates are order-free minima of (distance, walk position) keys.
//   * Query j skips target i iff, when j runs, i is held by a query with observations.  Targets held with observations on entry are
//     skipped by every query: seed_t gives them t = -1.  Otherwise let t(i) = the first query WITH observations that picks i
//     (T_FREE = none): before t(i) only queries without observations (or a holder on entry without observations) can have written i, so
//     nobody skips it; from t(i) on it is held with observations, every later query skips it and nobody overwrites it.  Hence:
//     j skips i  <=>  t(i) < j.
//   * Uniqueness and equality with the sequential loop: pick(j) depends only on t restricted to queries < j, i.e. on pick(0 .. j-1).  By
//     induction over j exactly one assignment satisfies "pick(j) = choice of j given the t of the picks", and it is the sequential one.
//   * Round bound: each round recomputes every pick from the t of the previous round.  After round r the picks of queries 0 .. r-1 are
//     final (query 0's never depends on t; query r's only on queries < r), so at most nQ + 1 rounds run; the loop stops at the first
//     round that changes nothing (a few in practice, more in conflict-heavy windows).
//   * Holder of i = the last picker (later queries overwrite); with t(i) set nobody picks after it.  Every accepted pick counts as a match.
#pragma once

#include "msl_common.h"

namespace msl {

constexpr int T_FREE = 0x7FFFFFFF;                  // t(i): no query with observations picks target i

// The hand-out for one workgroup of NT threads.
//   pick_of(j)  the target query j chooses given the current s_t (it skips target i iff s_t[i] < j), or -1
//   has_obs(j)  whether query j has observations (its pick blocks the later queries)
//   seed_t(i)   t of target i before any pick: -1 when held with observations on entry, else T_FREE
//   s_t[nT], s_pick[nQ], s_nm: LDS.  Targets are < nT <= 32767.
// Returns behind a barrier with s_pick[j] = the pick of query j (-1 = none), s_t[i] = the holder of target i (-1 = none; t itself is no
// longer needed and its storage holds it) and *s_nm = the number of accepted picks.  The entry barrier also publishes whatever the
// caller put into LDS before the call.
template <int NT, class PickOf, class HasObs, class SeedT>
__device__ __forceinline__ void greedy_assign(int nQ, int nT, int *s_t, short *s_pick, int *s_nm, PickOf pick_of, HasObs has_obs, SeedT seed_t) {
    for (int i = threadIdx.x; i < nT; i += NT) s_t[i] = seed_t(i);
    for (int j = threadIdx.x; j < nQ; j += NT) s_pick[j] = -2;             // -2: not evaluated yet (forces a first round)
    if (threadIdx.x == 0) *s_nm = 0;
    __syncthreads();
    for (int round = 0; round <= nQ; round++) {
        bool changed = false;
        for (int j = threadIdx.x; j < nQ; j += NT) {
            const int np = pick_of(j);
            changed |= np != s_pick[j];
            s_pick[j] = (short)np;
        }
        if (!__syncthreads_or(changed ? 1 : 0)) break;
        for (int i = threadIdx.x; i < nT; i += NT) s_t[i] = seed_t(i);
        __syncthreads();
        for (int j = threadIdx.x; j < nQ; j += NT)
            if (s_pick[j] >= 0 && has_obs(j)) atomicMin(&s_t[s_pick[j]], j);
        __syncthreads();
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nT; i += NT) s_t[i] = -1;
    __syncthreads();
    int nm = 0;
    for (int j = threadIdx.x; j < nQ; j += NT) {
        const int pk = s_pick[j];
        if (pk >= 0) { atomicMax(&s_t[pk], j); nm++; }
    }
    if (nm) atomicAdd(s_nm, nm);
    __syncthreads();
}

}  // namespace msl
