// msl_sf_fuse.hip -- map stage of the surfel fusion, the fusion kernel: k_fuse replaces fuseSurfelsKernel (reference
// src/SurfelFusion.cpp:167-283); the spawn wave of a deferred launch also materialises the new surfels of the keyframe before
// (initializeSurfels, :285-331).  The stage's overview and the two ways through a keyframe: msl_sf_map_dev.h.

#include "msl_sf_map_dev.h"

namespace {
// mul4 / mul3 of msl_sf.h on the packed rows: the same products and the same association
__device__ __forceinline__ void mul4r(const float *m, float v0, float v1, float v2, float v3, float out[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = ((m[r] * v0 + m[3 + r] * v1) + m[6 + r] * v2) + m[9 + r] * v3;
}
__device__ __forceinline__ void mul3r(const float *m, float v0, float v1, float v2, float out[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = (m[r] * v0 + m[3 + r] * v1) + m[6 + r] * v2;
}

// k_fuse (:167-283): ONE WAVE per sub-block of SUB_ITEMS = 128 consecutive surfels, no LDS and no workgroup barrier, so a wave starts wherever
// a SIMD has a free slot and 64 registers -- next to the LDS-heavy frame-batched kernels workgroups with LDS waited for it.
//   Phase A (streaming): lane l owns the surfels l and 64 + l of the sub-block (16-byte hot records; a load instruction covers 64
//     consecutive records = 1 KB).  Stale / deleted / out of range / out of image surfels finish here; the in-view ones need ONE 8-byte
//     gather each ({depth, superpixel index} texel written by kb_seed_plane) for the occlusion test.  The gathers of a lane leave together
//     (branch-free, clamped addresses).
//   Hand-over inside the wave: survivor number s (rank by (k, lane) = array order) goes to lane s % 64, round s / 64, with one
//     ds_permute_b32 per k -- a push through the LDS crossbar that allocates no LDS.  Non-survivors push an empty word to the remaining
//     lanes, so every k is a permutation of the 64 lanes and no two lanes ever target the same destination.
//   Phase B (gathers): per round one survivor per lane, neighbouring lanes = neighbouring surfels; its hot record (just streamed: cache
//     hit), 32-byte cold record, the 48-byte record of its seed and the pose's rotation are requested together, so <= 64 survivors cost
//     one round trip and a sub-block wholly in view two.
// DEFER = false (classic): deleted slots are handed to k_compact in delU (one atomic per wave that deleted something), per-sub-block deleted /
//   updated counts go to blockSums / blockUpd with plain stores.
// DEFER = true: deleted slots become HOT_HOLE and go to the window's deletion log; the regular waves of keyframe kf > 0 work on the slots below
//   E0 (the extent keyframe kf - 1 worked on), the launch's spawn wave (spawnWave = true, its own instantiation) on the new surfels of kf - 1.
template <bool DEFER, bool spawnWave>
__device__ __forceinline__ void fuse_body(const FuseArgs &P, const FuseFrame &F, int nSubHint, unsigned waveIdx, int G) {
    constexpr int KPL = SUB_ITEMS / 64;        // records per lane; a wave owns WSPAN = SUB_ITEMS consecutive surfels (measurements: msl_sf.h)
    constexpr long long WSPAN = 64 * KPL;
    struct { HotPk *hot; ColdRec *cold; } M = {P.hot, P.cold};
    const FuseAux *aux = &P.dc->aux;
    const unsigned lane0 = threadIdx.x;
    const uint2 *tex = P.tex;
    const float4 *fuseRec = P.fuseRec;
    uint8_t *fused = P.fused;
    const int ref = F.ref;
    const float cameraF = (float)(((double)fabsf(P.fx) + (double)fabsf(P.fy)) / 2.0);
    const float halfF = 0.5f * cameraF;   // BASELINE * cameraF (:220), exact
    // deferred, keyframe kf > 0: E0 = the extent keyframe kf - 1 worked on; its new surfels follow from there
    const bool pending = DEFER && P.kf > 0;
    long long E0v = 0;   // (requested here, first used behind the hot records of the wave's first sub-block: the two travel together)
    if (pending) E0v = P.dc->ext[P.kf - 1];
    long long E0 = 0;
    if (DEFER && spawnWave) E0 = ((long long)__builtin_amdgcn_readfirstlane((int)(E0v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)E0v);
    if (spawnWave && !pending) return;   // (the first keyframe of a window has nothing to materialise)
    if (DEFER && !pending && waveIdx == 0 && lane0 == 0) P.dc->ext[0] = P.ctr[CTR_LIVE];
    if (DEFER && !spawnWave && waveIdx == 0 && lane0 == 0) P.dc->logBase[P.kf] = P.kf > 0 ? P.dc->logBase[P.kf - 1] + P.dc->delCnt[P.kf - 1] : 0u;   // where this keyframe's log entries start
    // The spawn wave (deferred, one per launch, dispatched first): the new surfels of keyframe kf - 1 go to the physical slots E0, E0 + 1, ...; this
    // wave counts them (one trip over the lattice's flag words), publishes the extent for the next launch, and -- only if there are any -- writes
    // them and fuses them itself, 256 at a time.  No other wave of the launch ever waits for the count: they work on the slots below E0.
    unsigned spK = 0;
    if (DEFER && spawnWave) {
        unsigned excl;
        spK = spawn_count(P, lane0, excl);
        if (lane0 == 0) P.dc->ext[P.kf] = E0 + (long long)spK;
        if (spK == 0) return;
    }
    // Wave g owns sub-block G - 1 - g (the newest surfels -- nearly all in view: most phase-B work -- are dispatched first) and, should the
    // map have outgrown the grid, G - 1 - g + G, ... (grid-stride; normally one iteration).  The grid covers the host's last KNOWN live count
    // plus a margin, not its upper bound.  Sub-blocks below nSubHint load at once; above it the wave reads the live count first and leaves if
    // there is nothing for it.  Capacity is a multiple of 4096 and every sub-block that loads speculatively lies below it.
    // Workgroups are dispatched round-robin over the 8 XCDs: give each XCD runs of FUSE_CHUNK consecutive sub-blocks (neighbouring surfels
    // project to neighbouring pixels, so an XCD's L2 fetches a part of the texel map instead of all of it; small enough runs keep the XCDs
    // balanced -- whole eighths of the map were 2 x slower).
#ifndef MSL_FUSE_CHUNK
#define MSL_FUSE_CHUNK 16
#endif
    constexpr unsigned FUSE_CHUNK = MSL_FUSE_CHUNK;
    // Round 6: when the launch before left screen keys, the sub-blocks are DEALT by screen position instead (P.deal, built by deal_subblocks below):
    // XCD x gets the sub-blocks whose in-view surfels project into the x-th band of image rows, top to bottom, then its share of the sub-blocks
    // with nothing in view -- its L2 then fetches one band of the texel map and of the seed records, not the whole screen (every XCD fetching the
    // whole 2.46 MB texel map was a third of the kernel's fabric traffic).  One scalar load on the head of the wave's chain.
    long long sb0;
    if (!spawnWave && P.deal != nullptr) {
        const unsigned gs = (unsigned)G >> 3;   // (G is a multiple of 8 whenever a table is handed over)
        // (a scalar load by hand: the compiler cannot prove that no store of the kernel aliases the table and would fetch the wave-uniform word
        // through the vector cache; the launch before wrote it, and the scalar cache is invalidated at every kernel start)
        const unsigned *dp = P.deal + ((waveIdx & 7u) * gs + (waveIdx >> 3));
        unsigned dv;
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(dv) : "s"(dp) : "memory");
        sb0 = (long long)dv;
    } else {
        long long lin = waveIdx;
        constexpr unsigned T = 8u * FUSE_CHUNK;
        const unsigned full = ((unsigned)G / T) * T;
        if (waveIdx < full) { const unsigned grp = waveIdx / T, r = waveIdx % T; lin = (long long)grp * T + (r & 7u) * FUSE_CHUNK + (r >> 3); }
        sb0 = (long long)G - 1 - lin;
    }
    for (long long it = 0;; it++) {
        // (the lane number is re-materialised per iteration: values derived from it are then not hoisted out of this -- normally single-trip --
        // loop and kept in registers / scratch for its whole body)
        unsigned lane = lane0;
        asm volatile("" : "+v"(lane));
#define REC_LOCAL(k) (64u * (unsigned)(k) + lane)
        const long long sb = sb0 + it * G;   // regular waves: the sub-block; grid-stride should the map have outgrown the grid
        long long c0, n = 0, cntIdx;
        if (DEFER && spawnWave) {
            c0 = E0 + it * WSPAN;
            n = E0 + (long long)spK;
            if (c0 >= n) return;
            unsigned excl;   // (the per-lane prefix again rather than a register kept through the whole body: this path runs when a keyframe spawned something)
            (void)spawn_count(P, lane, excl);
            emit_records(P, E0, c0, KPL, lane, spK, excl);
            cntIdx = E0 / SUB_ITEMS + 1 + it;   // its updated counts sit behind those of the sub-blocks below E0 (k_defer_tail adds them up)
        } else {
            c0 = sb * WSPAN; cntIdx = sb;
            if (pending) {
                // (the grid lies inside the capacity, so a wave's FIRST sub-block is requested before the extent has arrived; the slots from E0 on belong
                // to the spawn wave: sub-blocks wholly beyond E0 leave below, records beyond it inside a sub-block fail the `i < n` test)
                if (it > 0) {
                    E0 = ((long long)__builtin_amdgcn_readfirstlane((int)(E0v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)E0v);
                    if (c0 >= E0) return;
                }
            } else if (sb >= nSubHint && c0 >= __hip_atomic_load(&P.ctr[CTR_LIVE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        }
        // lane l owns records l, 64 + l, 128 + l, 192 + l of the sub-block: the survivors' rank order (k, lane) is then the array order, so
        // neighbouring lanes of phase B work on neighbouring records and their gathers and stores share cache lines
        HotPk hq[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) hq[k] = M.hot[c0 + REC_LOCAL(k)];
        if (!pending) n = P.ctr[CTR_LIVE];
        else if (!spawnWave) {
            E0 = ((long long)__builtin_amdgcn_readfirstlane((int)(E0v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)E0v);
            if (c0 >= E0) return;
            n = E0;
        }
        unsigned stp = 0;  // two bits per record: 0: nothing to do, 1: stale -> delete, 2: already deleted, 3: in view
        unsigned keyAcc = 0;   // bits 0..15: sum of the screen keys (image row scaled to 0 .. 253) of the lane's in-view records, bits 16..: their number
        float pzv[KPL];
        unsigned offT[KPL];
        // rare: a record with exact ints in the side array, or a slot the window has logged already -- ONE test for the lane's four records
        unsigned anyTl = 0;
#pragma unroll
        for (int k = 0; k < KPL; k++) anyTl |= hq[k].tl;
        const bool anyHi = __builtin_expect(__ballot(anyTl >> 31) != 0ull, 0);
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const long long i = c0 + REC_LOCAL(k);
            const float x = hq[k].px, y = hq[k].py, z = hq[k].pz;
            const unsigned tl = hq[k].tl;
            int ut = tl_ut(tl), lu = tl_lu(tl);
            bool hole = false;
            if (anyHi) {
                if (tl == HOT_WIDE) { const int *w = aux->map.utlWide; ut = w[2 * i]; lu = w[2 * i + 1]; }
                else if (tl & 0x80000000u) hole = true;
            }
            float pc[3];
            mul4r(F.inv, x, y, z, 1.0f, pc);
            const bool inRange = !(pc[2] < P.fuseNear || pc[2] > P.fuseFar);
            const bool live = i < n && !hole, stale = ref - lu > 5 && ut < 5;
            // what does not need the projection: stale -> delete (1), already deleted (2), out of range (0)
            int st = 0;
            if (live) st = stale ? (ut != 0 ? 1 : 2) : (ut == 0 ? 2 : 0);
            const bool cand = live && !stale && ut != 0 && inRange;
            unsigned off = 0;
            // (branch-free on purpose.  Skipping the two divisions, the roundings and the image test for 64-record groups that lie outside the frustum
            // as a whole -- `if (__ballot(cand))` -- measured 0.5 us SLOWER alone and no faster beside the frame-batched kernels: the kernel is
            // bound by its chain of memory round trips, not by these instructions)
            {
                const float zq = inRange ? pc[2] : 1.0f;   // keeps the (unused) quotients of skipped surfels finite
                const float projectU = pc[0] * P.fx / zq + P.cx, projectV = pc[1] * P.fy / zq + P.cy;  // :75-78
                const int pUInt = round_half_up_pixel(projectU), pVInt = round_half_up_pixel(projectV);   // int(projectU + 0.5) wherever it matters
                const bool inImage = !(pUInt < 1 || pUInt > P.W - 2 || pVInt < 1 || pVInt > P.H - 2);
                if (cand && inImage) { st = 3; keyAcc += (((unsigned)pVInt * (unsigned)P.rowScale) >> 16) | 0x10000u; }
                // a record that is not in view needs no texel: all such lanes read texel 0 (ONE line for the whole wave) instead of up to 64 scattered
                // border texels -- two thirds of the dense map's records, each a separate request to the vector cache (round 4 clamped the address
                // to the border texel nearest to the projection)
                off = st == 3 ? (unsigned)(pVInt * P.W + pUInt) : 0u;
            }
            stp |= (unsigned)st << (2 * k); pzv[k] = pc[2];
            offT[k] = off;
        }
        uint2 tx[KPL];
        {
#pragma unroll
            for (int k = 0; k < KPL; k++) tx[k] = tex[offT[k]];
            // a common use of all four results: keeps the compiler from sinking each load into its (conditional) consumer, which would turn one
            // round trip back into up to four dependent ones
            if constexpr (KPL == 4) asm volatile("" ::"v"(tx[0].x), "v"(tx[1].x), "v"(tx[2].x), "v"(tx[3].x), "v"(tx[0].y), "v"(tx[1].y), "v"(tx[2].y), "v"(tx[3].y));
            else asm volatile("" ::"v"(tx[0].x), "v"(tx[KPL - 1].x), "v"(tx[0].y), "v"(tx[KPL - 1].y));
        }
        // the sub-block's screen key for the next dealing: mean row of its in-view records (255: nothing in view) -- stored here, before phase B,
        // so that nothing of it stays live through the gathers (a hint: the approximate reciprocal is good enough)
        if (!(DEFER && spawnWave)) {
            const unsigned ks = (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan(keyAcc), 63);
            const unsigned kc = ks >> 16;
            const unsigned key = kc ? min((unsigned)((float)(ks & 0xFFFFu) * __builtin_amdgcn_rcpf((float)kc)), 254u) : 255u;
            if (lane == 0) P.sbKeys[cntIdx] = key;
        }
        // ---- classification: deletions of phase A, survivors ----
        // (one bit field per lane instead of eight lane masks: the masks would live in scalar registers, which this kernel is short of)
        unsigned fl = 0;   // bit k: record k deleted in phase A; bit 4 + k: record k survives into phase B
        unsigned cntDel = 0;
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const unsigned st = (stp >> (2 * k)) & 3u;
            const bool occluded = st == 3u && (double)pzv[k] < (double)__uint_as_float(tx[k].x) - 1.0;
            const bool del = st == 1u || st == 2u || occluded;
            if (DEFER) { if (del) M.hot[c0 + REC_LOCAL(k)].tl = HOT_HOLE; }
            else if (st == 1u || occluded) {   // updateTimes = 0, lastUpdate stays (:201; the host-vector drop-in hands the record back)
                if (__builtin_expect(hq[k].tl == HOT_WIDE, 0)) aux->map.utlWide[2 * (c0 + REC_LOCAL(k))] = 0;
                else M.hot[c0 + REC_LOCAL(k)].tl = hq[k].tl & 0xFFFFFu;
            }
            fl |= del ? (1u << k) : 0u;
            fl |= (st == 3u && !occluded) ? (16u << k) : 0u;
            cntDel += (unsigned)__popcll(__ballot(del));
        }
        // deleted slots: classic -> delU (k_compact's fast path), deferred -> the window's log behind the entries of the keyframes before
        // (a wave that deletes is rare but often among the last to finish: everything it needs travels in ONE round trip -- the count's atomic and, for
        // a deferred keyframe, the log position the keyframes before left, dc->logBase[kf - 1] + dc->delCnt[kf - 1])
        auto list_base = [&](unsigned c) -> unsigned {
            unsigned base = 0, prior = 0;
            if (DEFER && P.kf > 0) prior = P.dc->logBase[P.kf - 1] + P.dc->delCnt[P.kf - 1];
            if (lane == 0) base = atomicAdd(P.delCount, c);
            return (unsigned)__builtin_amdgcn_readfirstlane((int)base) + prior;
        };
        auto hand_over = [&](bool d, unsigned long long m, unsigned base, long long i) {
            if (d) {
                const unsigned j = base + lane_rank(m);
                if (DEFER || j < (unsigned)LIST_D) P.delOut[j] = (unsigned)i;   // (the log holds one entry per physical slot at most: it cannot overflow the capacity)
            }
        };
        if (cntDel) {   // rare: a handful of slots per keyframe
            unsigned base = list_base(cntDel);
#pragma unroll
            for (int k = 0; k < KPL; k++) {
                const bool d = (fl >> k) & 1u;
                const unsigned long long m = __ballot(d);
                hand_over(d, m, base, c0 + REC_LOCAL(k)); base += (unsigned)__popcll(m);
            }
        }
        // ---- survivors -> (round, lane): one push per k.  word = local index, valid bit, superpixel << 16 ----
        unsigned rcv[KPL], bk[KPL];
        unsigned total = 0;
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const bool sv = (fl >> (4 + k)) & 1u;
            const unsigned long long m = __ballot(sv);
            const unsigned c = (unsigned)__popcll(m), rs = lane_rank(m);
            const unsigned dest = (sv ? total + rs : total + c + (lane - rs)) & 63u;
            const unsigned payload = sv ? (REC_LOCAL(k) | 0x100u | (tx[k].y << 16)) : 0u;
            rcv[k] = (unsigned)__builtin_amdgcn_ds_permute((int)(dest * 4u), (int)payload);
            bk[k] = total;
            total += c;
        }
        const unsigned rounds = (total + 63u) >> 6;
        unsigned nupd = 0, cntDelB = 0;
        for (unsigned r = 0; r < rounds; r++) {   // one round for <= 64 survivors
            unsigned item = 0u;
#pragma unroll
            for (int k = 0; k < KPL; k++) {
                const unsigned rk = (bk[k] + ((lane - bk[k]) & 63u)) >> 6;   // round of the survivor this lane received from k (if any)
                if ((rcv[k] & 0x100u) && rk == r) item = rcv[k];
            }
            // branch-free loads: a lane without a survivor in this round reads record c0 / seed 0 (valid addresses, one line for all such
            // lanes) -- conditional loads made the compiler sink the first uses into the load block and wait there
            const long long i = c0 + (item & 0xFFu);
            const unsigned sp = item >> 16;
            const HotPk h = M.hot[i];
            // the update reads normal, size and weight of the cold record and overwrites the rest: two loads (a whole-struct copy became three)
            ColdRec c;
            {
                const float4 cn = *reinterpret_cast<const float4 *>(M.cold + i);
                c.nx = cn.x; c.ny = cn.y; c.nz = cn.z; c.size = cn.w; c.weight = M.cold[i].weight;
            }
            const float4 f0 = fuseRec[fuserec_index(P.nseeds, sp, 0)], f1 = fuseRec[fuserec_index(P.nseeds, sp, 1)], f2 = fuseRec[fuserec_index(P.nseeds, sp, 2)];
            // the rotation of the pose (only the update path needs it, to turn the fused normal back into the world): three 12-byte loads from the
            // keyframe's device record, requested HERE with the records -- left to the compiler they sat behind the tests, one more dependent round
            // trip in every round (k_fuse 18.1 against 16.5 us under rocprofv3); as kernel arguments they cost nine scalar registers this kernel lacks
            const float *poseM = F.frame->pose;
            const float r00 = poseM[0], r10 = poseM[1], r20 = poseM[2], r01 = poseM[4], r11 = poseM[5], r21 = poseM[6], r02 = poseM[8], r12 = poseM[9], r22 = poseM[10];
            // common use of one field per load instruction: all records are in flight together
            asm volatile("" ::"v"(h.px), "v"(h.tl), "v"(c.nx), "v"(c.weight), "v"(f0.x), "v"(f1.x), "v"(f2.x), "v"(r00), "v"(r01), "v"(r02));
            bool upd = false, delB = false;
            if (item && __float_as_uint(f2.w) != 0u) {   // seed tests of :214-219 (norm != 0, viewCos >= MAX_ANGLE_COS)
                const float seedDepth = f0.w;
                const float pz = ((F.inv[2] * h.px + F.inv[5] * h.py) + F.inv[8] * h.pz) + F.inv[11] * 1.0f;   // row 2 of mul4: as in phase A
                // :220-221 is (float)((double)(pz pz) / (0.5 (double)cameraF) * 4.0).  Both operands of the division are float values (0.5 cameraF
                // exactly), the multiplication by 4 is exact, and rounding a correctly rounded binary64 quotient of two binary32 numbers to
                // binary32 gives the correctly rounded binary32 quotient (53 >= 2 * 24 + 2: double rounding is innocuous for division), so one
                // IEEE float division yields the same bits as the double expression at a third of the instructions.
                float tolerateDiff = (pz * pz) / halfF * 4.0f;
                tolerateDiff = tolerateDiff < MIN_TOLERATE_DIFF ? (float)MIN_TOLERATE_DIFF : tolerateDiff;
                if (!(pz < seedDepth - tolerateDiff) && !(pz > seedDepth + tolerateDiff)) {
                    float nc[3];
                    mul3r(F.inv, c.nx, c.ny, c.nz, nc);
                    const float normDiffCos = nc[0] * f0.x + nc[1] * f0.y + nc[2] * f0.z;
                    if (normDiffCos < MAX_ANGLE_COS) {
                        if (DEFER) M.hot[i].tl = HOT_HOLE;
                        else if (__builtin_expect(h.tl == HOT_WIDE, 0)) aux->map.utlWide[2 * i] = 0;
                        else M.hot[i].tl = h.tl & 0xFFFFFu;
                        delB = true;
                    } else {
                        const float oldWeight = c.weight;
                        const float newWeight = f1.w;                      // getWeight(seed.meanDepth)
                        const float sumWeight = oldWeight + newWeight;
                        const float fusedPx = (h.px * oldWeight + newWeight * f1.x) / sumWeight;   // f1.xyz = pose * seed.pos
                        const float fusedPy = (h.py * oldWeight + newWeight * f1.y) / sumWeight;
                        const float fusedPz = (h.pz * oldWeight + newWeight * f1.z) / sumWeight;
                        float fusedNx = nc[0] * oldWeight + newWeight * f0.x;
                        float fusedNy = nc[1] * oldWeight + newWeight * f0.y;
                        float fusedNz = nc[2] * oldWeight + newWeight * f0.z;
                        // :254-257: newNormLength is a double that holds a float (std::sqrt(float)); float /= double is a binary64 division
                        // of two float values rounded to float = the IEEE float division (same argument as above)
                        const float newNormLength = sqrtf(fusedNx * fusedNx + fusedNy * fusedNy + fusedNz * fusedNz);
                        fusedNx = fusedNx / newNormLength; fusedNy = fusedNy / newNormLength; fusedNz = fusedNz / newNormLength;
                        float newNormW[3];
                        newNormW[0] = (r00 * fusedNx + r01 * fusedNy) + r02 * fusedNz;   // mul3(pose, ...): the same products, the same association
                        newNormW[1] = (r10 * fusedNx + r11 * fusedNy) + r12 * fusedNz;
                        newNormW[2] = (r20 * fusedNx + r21 * fusedNy) + r22 * fusedNz;
                        int ut = (int)(h.tl >> 20);   // (a survivor is never a hole; HOT_WIDE: the side array)
                        if (__builtin_expect(h.tl == HOT_WIDE, 0)) ut = aux->map.utlWide[2 * i];
                        unsigned tlNew = tl_pack(ut + 1, ref);             // updateTimes + 1, lastUpdate = reference index (:275-276)
                        if (__builtin_expect(!tl_fits(ut + 1, ref), 0)) {   // rare: exact ints to the side array (pointers fetched one at a time: no register tuples in a cold path)
                            int *w = aux->map.utlWide;
                            w[2 * i] = ut + 1; w[2 * i + 1] = ref;
                            asm volatile("" ::: "memory");
                            set_wide_flag_ptr(aux->map.wideFlag, 2ull);
                            tlNew = HOT_WIDE;
                        }
                        c.rgbf = __float_as_uint(f2.z);                    // r, g, b of the seed (bytes: never COLD_WIDE)
                        c.nx = newNormW[0]; c.ny = newNormW[1]; c.nz = newNormW[2];
                        c.weight = sumWeight;
                        c.color = f2.y;                                    // seed.meanIntensity
                        const float newSize = f2.x;                        // seed.size * fabs(meanDepth / (cameraF * viewCos))
                        if (newSize < c.size) c.size = newSize;
                        u32x4 hv = {__float_as_uint(fusedPx), __float_as_uint(fusedPy), __float_as_uint(fusedPz), tlNew};
                        u32x4 c0v = {__float_as_uint(c.nx), __float_as_uint(c.ny), __float_as_uint(c.nz), __float_as_uint(c.size)};
                        u32x4 c1v = {__float_as_uint(c.color), __float_as_uint(c.weight), c.rgbf, 0u};   // (_spare is 0 in every record: store_surfel)
                        st16(M.hot + i, hv);
                        st16(M.cold + i, c0v);
                        st16(reinterpret_cast<u32x4 *>(M.cold + i) + 1, c1v);
                        fused[sp] = 1;
                        upd = true;
                    }
                }
            }
            nupd += (unsigned)__popcll(__ballot(upd));
            const unsigned long long mb = __ballot(delB);
            if (mb) {   // rare
                const unsigned cb = (unsigned)__popcll(mb);
                hand_over(delB, mb, list_base(cb), i);
                cntDelB += cb;
            }
        }
        if (lane == 0) {   // per-sub-block counts: deleted (classic: the slow paths of k_compact, the host-vector download), updated (deferred: the keyframe's slice)
            if (!DEFER) P.blockSums[cntIdx] = cntDel + cntDelB;
            P.blockUpd[cntIdx] = nupd;
        }
        // (normally) nothing beyond the grid; a deferred launch decides at the head of the loop (the new surfels may reach into the next sub-block)
        if (!(DEFER && spawnWave) && (sb + G) * WSPAN >= n) return;   // (n = E0 for a pending launch's regular waves)
    }
#undef REC_LOCAL
}

template <bool DEFER>
// Register budget (round 6): at 8 waves per SIMD a wave has 80 scalar registers (800 per SIMD / 8 less the trap handler's 16) and the kernel spilled 41 of them to
// lanes of a VGPR: 147 v_readlane / v_writelane instructions, a fifth of its VALU count.  A minimum of 6 waves lets the compiler use 106 SGPRs: no spills, 59 VGPRs
// (the wave still fits the 64-register holes the frame-batched kernels leave), 7 waves per SIMD by the scalar file.  15.5 -> 15.0 us by rocprofv3 beside the
// (faster, round 6) superpixel stage, config 3 +1.2 %, front end +- 0; measured before the superpixel stage was trimmed: +- 0 everywhere.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_fuse(FuseArgs P, FuseFrame F, int nSubHint) {   // by value: kernarg -> SGPRs
    __builtin_amdgcn_s_setprio(3);   // the map chain is sequential per keyframe: issue ahead of the batched kernels' waves
    if (DEFER) {
        if (blockIdx.x == 0) fuse_body<DEFER, true>(P, F, nSubHint, 0u, (int)gridDim.x - 1);   // workgroup 0: the spawn wave (its own instantiation: what it
        else fuse_body<DEFER, false>(P, F, nSubHint, blockIdx.x - 1u, (int)gridDim.x - 1);     // carries through the loop costs the other waves no register)
    } else {
        fuse_body<false, false>(P, F, nSubHint, blockIdx.x, (int)gridDim.x);
    }
}
}  // namespace

namespace msl {
namespace sf {
void map_launch_fuse(KernelProfiler &prof, hipStream_t st, const SfDev &P, int slot, const FrameDev &F, int nSubGrid, int nSubHint, bool deferred, bool dealt, unsigned blkStride) {
    const FuseArgs A = fuse_args(P, slot, deferred, blkStride, dealt);
    const FuseFrame FF = fuse_frame(F, P.frames + slot);
    if (deferred) MSL_SF_LAUNCH(prof, SK_FUSE, st, k_fuse<true>, dim3((unsigned)nSubGrid + 1u), dim3(64), A, FF, nSubHint);
    else MSL_SF_LAUNCH(prof, SK_FUSE, st, k_fuse<false>, dim3((unsigned)nSubGrid), dim3(64), A, FF, nSubHint);
}
}  // namespace sf
}  // namespace msl
