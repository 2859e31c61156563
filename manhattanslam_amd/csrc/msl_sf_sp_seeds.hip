// msl_sf_sp_seeds.hip -- superpixel stage for gfx950 (MI355X): the seed update that follows every pixel pass (stage overview: msl_sf_superpixel.hip).
//     kb_update_seeds<STRADDLE>           16 lanes per seed: ordered window gather, Huber mean (reference src/SurfelFusion.cpp:428-515)
//     kb_commit_seeds                     one thread per seed: the per-seed scalar end; chunk-abort (`return`) semantics: restore-only
//     k_debug_chain                       test hook of the rotating chains
//     k_debug_newton                      test hook of the Newton quotient

#include "msl_sf_sp_dev.h"

namespace {

// kb_update_seeds (:428-515): 16 lanes per seed (lane = window row), 16 seeds per workgroup.
// Integer-valued sums are exact in any order; the float depth sum and the Huber/Newton sums run in window raster order as rotating DPP chains
// over the seed's 16 lanes (chain_block_f32 above), fed by terms each lane computes from its own elements of the ordered depth list.
// Round 5: 56 VGPRs and 17 KB of LDS (rounds 2-4: 80 and 35 KB -- the term list, the per-seed LDS scalars and their atomics are gone): 8 instead
// of 4 workgroups per CU for a kernel whose waves mostly wait (13.5 -> 6.9 us per frame beside the other stages, front end +3.7 %).
// What kb_update_seeds leaves for kb_commit_seeds in the seed's record of seedsTmp[] (round 6): the per-seed scalar rest of updateSeedsKernel -- three
// divisions, the colour fetch, the stability test, the new seed record and its AssignRec with an FP64 division: ~130 instructions that ONE lane of a
// seed's sixteen executed -- runs there, one thread per seed.
struct SeedUpd {
    int state;            // 0: skipped (unused or stable: kb_update_seeds wrote what changes); 1: no pixel owned, the seed ends its chunk (:473-474); 2: update
    int cnt, sumI, sumX, sumY;   // the integer-valued sums (:461-464)
    int depthLoop;        // the seed has valid depths: meanDepth below is the refined mean (:486-512), otherwise 0 goes to the record (:489-490)
    float meanDepth;
};
static_assert(sizeof(SeedUpd) <= sizeof(msl_seed), "the hand-over record fits a seedsTmp record");
constexpr int UPD_SEEDS = 16;   // seeds per workgroup (four per wave).  The waves share nothing (a seed's 16 lanes use their own row of s_depth and wave_barrier
                                // only), but one-wave workgroups (4 seeds, 4.3 KB of LDS) gain nothing: front end +- 0
constexpr int NEWTON_RB = 4;    // blocks (of 16 elements) of a seed's depth list that stay in registers for the Newton steps; the rest is re-read from s_depth.
                                // 4 / 6 / 8 measured alike (all 46 - 48 VGPRs: the gather holds more); 4 is the least code (the chains are unrolled per block)
__host__ __device__ constexpr int upd_blocks(int nseeds) { return (nseeds + UPD_SEEDS - 1) / UPD_SEEDS; }
template <bool STRADDLE>   // STRADDLE: W mod 8 in {1, 2, 3} (a window quad can stick out over the right edge)
__global__ __launch_bounds__(16 * UPD_SEEDS) void kb_update_seeds(SfDev P, int it, int nSlots) {
    // rows of 256 + 16 words: the two seeds of a 32-lane half read / write entry l + 16 t of their own row together (ds_*_b32: bank = word address mod
    // 32); with a row stride of 256 words both rows started on the same bank (round 4: 32 % of the kernel's LDS cycles were bank conflicts)
    __shared__ __attribute__((aligned(16))) float s_depth[UPD_SEEDS][272];   // the ordered depth lists (the only LDS of the kernel since round 5: 17 KB)
    int slot, blk;
    if (!xcd_slot(upd_blocks(P.nseeds), nSlots, slot, blk)) return;
#ifdef MSL_FUSE_STAMPS   // section cycle counts of the waves of slot 0, summed into delList[96 ..] (tools/fuse_stamps.py)
    unsigned long long ust[8]; int usn = 0;
#define USTAMP() ust[usn++] = __builtin_amdgcn_s_memtime()
#else
#define USTAMP()
#endif
    USTAMP();
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int seedI = blk * UPD_SEEDS + g;
    const FrameDev F = P.frames[slot];   // by value: one load up front instead of re-reading fields around every store
    const unsigned short *index = P.index + (size_t)slot * P.pxStride;
    msl_seed S;
    memset(&S, 0, sizeof(S));
    bool active = seedI < P.nseeds;
    bool stable = false;
    if (active) {
        S = P.seeds[(size_t)slot * P.nseeds + seedI];
        stable = it > 0 ? (P.tmin[(size_t)slot * P.nseeds + seedI] == T_INF) : (S.stable != 0);
        // The seed records themselves are written by kb_commit_seeds (from the SeedUpd this kernel leaves in seedsTmp[]), which also knows by then
        // whether the seed's chunk had ended earlier.
        if (!S.use || stable) {
            if (l == 0) {   // skipped: only the stable flag (as left by the pixel pass) and t(s) change
                P.seeds[(size_t)slot * P.nseeds + seedI].stable = stable;
                P.arec[(size_t)slot * P.nseeds + seedI].stable = stable ? 1u : 0u;
                reinterpret_cast<SeedUpd *>(P.seedsTmp + ((size_t)slot * P.nseeds + seedI))->state = 0;
                P.tmin[(size_t)slot * P.nseeds + seedI] = stable ? T_INF : 0u;
            }
            active = false;
        }
    }
    if (!__ballot(active)) return;   // all four seeds of the wave are skipped (stable or unused): nothing to gather
    const int spX = seedI % P.spW, spY = seedI / P.spW;
    const int xb0 = spX * SP + SP / 2 - SP, yb0 = spY * SP + SP / 2 - SP;
    const int xb = xb0 > 0 ? xb0 : 0, yb = yb0 > 0 ? yb0 : 0;
    const int xe = (xb0 + SP * 2) < P.W - 1 ? (xb0 + SP * 2) : P.W - 1, ye = (yb0 + SP * 2) < P.H - 1 ? (yb0 + SP * 2) : P.H - 1;
    int sumX = 0, sumY = 0, sumI = 0, cnt = 0, nd = 0;
    {
        // Lane = (row r of a group of four window rows, quad q of four window columns): 12 wide loads per lane (8 B of
        // index, 16 B of depth, 4 B of gray, four times) instead of 48 scalar ones.  Window columns start at a multiple
        // of 4: a quad lies left of the image as a whole (first lattice column) or starts inside it.  When W is not a multiple of 4 the last
        // quad of a window may stick out over the right edge: it is then loaded from W - 4 (inside the row) and its first elements, which
        // belong to the neighbouring lane's quad, are masked (col >= col0) -- no element-wise path, the window order is unchanged.  Raster
        // order of the window = (iteration, lane, element), which the ordered depth list below follows.
        const int rq = l >> 2, cq = l & 3;
        const int col0 = xb0 + 4 * cq;
        const bool quadIn = col0 >= 0 && (STRADDLE ? col0 < P.W : col0 + 3 < P.W);
        const int colc = quadIn ? (STRADDLE ? min(col0, P.W - 4) : col0) : 0;
        Quad<unsigned short> idq[4];
        Quad<float> dq[4];
        Quad<uint8_t> gq[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int jc = min(max(yb0 + 4 * m + rq, 0), P.H - 1);
            idq[m] = load_quad(byte_off(index, 2u * (unsigned)(jc * P.W + colc)));
            dq[m] = load_quad(byte_off(F.depthG(), (unsigned)jc * P.dsB + 4u * (unsigned)colc));
            gq[m] = load_quad(byte_off(F.grayG(), (unsigned)jc * P.gsB + (unsigned)colc));
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int j = yb0 + 4 * m + rq;
            const bool rowOk = active && quadIn && j >= yb && j < ye;
            bool hd[4];
            int c = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int col = colc + e;
                const bool own = rowOk && (!STRADDLE || col >= col0) && col >= xb && col < xe && idq[m].v[e] == seedI;
                hd[e] = own && dq[m].v[e] >= DEPTH_01_F;   // `> 0.1` (:452), float form (msl_sf_sp_dev.h)
                if (own) { sumX += col; sumY += j; sumI += gq[m].v[e]; cnt++; }
                c += hd[e] ? 1 : 0;
            }
            const int incl = row_incl_scan(c);
            int o = nd + incl - c;
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (hd[e]) s_depth[g][o++] = dq[m].v[e];
            nd += row_lane_i32<15>(incl);
        }
    }
    USTAMP();   // 1: seed record + window gather + ordered depth list
    sumX = row_sum_i32(sumX); sumY = row_sum_i32(sumY); sumI = row_sum_i32(sumI); cnt = row_sum_i32(cnt);
    __builtin_amdgcn_wave_barrier();
    const bool depthLoop = active && cnt != 0 && nd > 0;   // (uniform over the seed's 16 lanes)
    if (l == 0 && active && cnt == 0)   // `return`: ends the chunk (:473-474); the seed itself stays as it is, unstable (kb_commit_seeds)
        atomicMin(&P.chunkAbort[(slot * 2 + (it & 1)) * 16 + seed_chunk(seedI, P.nseeds)], seedI);
    // ---- mean depth and its Huber refinement (:486-512): the sequential sums as rotating chains (above); everything per seed is uniform over its
    // 16 lanes and lives in registers -- no LDS, no atomics, no barriers in the Newton loop ----
    const int ndL = depthLoop ? nd : 0;                 // a seed without a depth loop contributes empty lists
    const int nblk = rows_max_i32((ndL + 15) >> 4);    // blocks of the longest list of the wave's four seeds
    float meanDepth = 0.0f;
    // The first NEWTON_RB blocks of the list stay in registers once the depth sum has read them (dr[]; element l + 16 bq, +0.0f beyond the list's
    // end): a Newton step then computes each of their residuals ONCE and takes the in-band count, the tail flag and the chain term (tr[]) from that
    // one value.  Blocks beyond NEWTON_RB (a seed that owns more than 16 NEWTON_RB pixels with a valid depth) are walked in s_depth as before:
    // a counting pass in front of the chain, the chain pass recomputing the residual.
    float dr[NEWTON_RB > 0 ? NEWTON_RB : 1], tr[NEWTON_RB > 0 ? NEWTON_RB : 1];
    {
        float sd = 0.0f;
#pragma unroll
        for (int bq = 0; bq < NEWTON_RB; bq++) {
            dr[bq] = 0.0f;
            if (bq < nblk) {
                const int e = l + 16 * bq;
                dr[bq] = e < ndL ? s_depth[g][e] : 0.0f;
                sd = chain_block_f32(sd, dr[bq]);
            }
        }
        for (int bq = NEWTON_RB; bq < nblk; bq++) {
            const int e = l + 16 * bq;
            sd = chain_block_f32(sd, e < ndL ? s_depth[g][e] : 0.0f);
        }
        const float sumDepth = row_lane_f32<15>(sd);
        if (depthLoop) meanDepth = sumDepth / (float)nd;
    }
    USTAMP();   // 2: means, colour fetch, sequential depth sum
    bool open = depthLoop;
    for (int newtonI = 0; newtonI < 5; newtonI++) {
        if (!__ballot(open)) break;
        // in-range count (sumB) and whether any list of the wave has a Huber tail this step; the terms of the chain -- in range: 2*residual; a tail
        // element: the +-inf marker huber_term_add() turns into +-HUBER_RANGE; beyond the list's end or a closed seed: +0.0f
        int inr = 0;
        bool tail = false;
#pragma unroll
        for (int bq = 0; bq < NEWTON_RB; bq++) {   // the register-resident blocks: one residual per element and step
            tr[bq] = 0.0f;
            if (bq < nblk && open && l + 16 * bq < ndL) {
                const float residual = meanDepth - dr[bq];
                if (in_huber_band(residual)) { inr++; tr[bq] = 2 * residual; }
                else { tail = true; tr[bq] = residual > 0 ? __builtin_inff() : -__builtin_inff(); }
            }
        }
        for (int bq = NEWTON_RB; bq < nblk; bq++) {   // the rest of a long list: counted here, its terms recomputed in front of the chain below
            const int e = l + 16 * bq;
            if (open && e < ndL) {
                const float residual = meanDepth - s_depth[g][e];
                if (in_huber_band(residual)) inr++; else tail = true;
            }
        }
        inr = row_sum_i32(inr);
        const bool anyTail = __ballot(tail) != 0ull;
        // the chain over the terms, in list order
        float sa = 0.0f;
#pragma unroll
        for (int bq = 0; bq < NEWTON_RB; bq++)
            if (bq < nblk) sa = anyTail ? chain_block_huber(sa, tr[bq]) : chain_block_f32(sa, tr[bq]);
        for (int bq = NEWTON_RB; bq < nblk; bq++) {
            const int e = l + 16 * bq;
            float t = 0.0f;
            if (open && e < ndL) {
                const float residual = meanDepth - s_depth[g][e];
                if (in_huber_band(residual)) t = 2 * residual;
                else t = residual > 0 ? __builtin_inff() : -__builtin_inff();
            }
            // no Huber tails anywhere in the wave (the common case): a plain float chain, 1 VALU op per element instead of ~8
            sa = anyTail ? chain_block_huber(sa, t) : chain_block_f32(sa, t);
        }
        const float sumA = row_lane_f32<15>(sa);
        const float deltaDepth = sp_newton_delta(sumA, inr);   // (float)((double)(-sumA) / ((double)sumB + 10.0)), sumB = (float)(2 * inr): one float division (msl_sf_sp_arith.h)
        if (open) {
            meanDepth = meanDepth + deltaDepth;
            if ((sp_lt_001(deltaDepth) && sp_gt_neg001(deltaDepth)) || newtonI == 4) open = false;   // `deltaDepth < 0.01 && deltaDepth > -0.01` (:507), float form
        }
    }
    USTAMP();   // 3: Newton steps
    if (active && l == 0) {
        SeedUpd U;
        U.state = cnt == 0 ? 1 : 2; U.cnt = cnt; U.sumI = sumI; U.sumX = sumX; U.sumY = sumY; U.depthLoop = depthLoop ? 1 : 0; U.meanDepth = meanDepth;
        *reinterpret_cast<SeedUpd *>(P.seedsTmp + ((size_t)slot * P.nseeds + seedI)) = U;
    }
#ifdef MSL_FUSE_STAMPS
    USTAMP();   // 4: stores
    if (slot == 0 && (threadIdx.x & 63) == 0) {
        for (int q = 1; q < usn; q++) atomicAdd(&P.delList[96 + q], (unsigned)(ust[q] - ust[q - 1]));
        atomicAdd(&P.delList[96], 1u);
    }
#endif
}

// kb_commit_seeds: the per-seed end of updateSeedsKernel (:475-515), one thread per seed: means, colour fetch, stability test, the new seed record, t(s)
// and the AssignRec, from the sums kb_update_seeds left (SeedUpd) -- and the chunk-abort rule: a seed without a single owned pixel ends its chunk
// (`return`, :473-474), so the seeds BEHIND it in the chunk stay as they are, unstable.  That rule can never fire: a used seed (lattice position
// spX < W / 8, spY < H / 8) always owns the pixel at its lattice centre (8 spX + 4, 8 spY + 4).  That pixel is free (what `use` means, :541-545); its
// ONLY updatePixels candidate is this seed (|8 c + 4 - x| < 8 holds for c = spX alone when x mod 8 == 4, :384-389); pass 0 assigns it with cost
// 0 < 1e6 whatever intensity / depth are; no later pass can move it; and it lies inside the clipped window updateSeeds counts.  So the owned-pixel
// count is >= 1 and the abort path is kept for fidelity only (property-tested on adversarial inputs in the CPU suite).
__global__ __launch_bounds__(256) void kb_commit_seeds(SfDev P, int it) {
    const int slot = blockIdx.y;
    const int seedI = blockIdx.x * 256 + threadIdx.x;
    if (seedI >= P.nseeds) return;
    if (seedI == 0) P.wlCount[slot] = 0;   // the next pixel pass rebuilds the relaxation worklist
    const size_t si = (size_t)slot * P.nseeds + seedI;
    const SeedUpd U = *reinterpret_cast<const SeedUpd *>(P.seedsTmp + si);
    if (U.state == 0) return;   // skipped (unused or stable): already as it should be
    const int abortAt = P.chunkAbort[(slot * 2 + (it & 1)) * 16 + seed_chunk(seedI, P.nseeds)];   // first seed of the chunk without a pixel (0x7FFFFFFF: none)
    if (U.state == 1 || seedI > abortAt) {   // the seed that ended the chunk, or one behind it: values untouched, unstable
        P.seeds[si].stable = 0; P.arec[si].stable = 0u; P.tmin[si] = 0u;
        return;
    }
    const FrameDev &F = P.frames[slot];
    // the 64-byte record as four 16-byte words (nobody else writes it): words 0-1 x, y; 10-11 meanDepth, meanIntensity; 12-14 r, g, b;
    // 15 the bytes fused | stable << 8 | use << 16 | _pad << 24
    static_assert(sizeof(msl_seed) == 64 && offsetof(msl_seed, meanDepth) == 40 && offsetof(msl_seed, r) == 48 && offsetof(msl_seed, stable) == 61, "msl_seed layout");
    uint4 *rec = reinterpret_cast<uint4 *>(P.seeds + si);
    const uint4 w0o = rec[0], w2o = rec[2], w3o = rec[3];
    const float sumIntensityNum = (float)U.cnt;
    const float sumIntensity = (float)U.sumI / sumIntensityNum, mX = (float)U.sumX / sumIntensityNum, mY = (float)U.sumY / sumIntensityNum;
    const float preIntensity = __uint_as_float(w2o.w), preX = __uint_as_float(w0o.x), preY = __uint_as_float(w0o.y);
    int tR = 0, tG = 0, tB = 0;
    vec3b(P, F, mY, mX, tR, tG, tB);
    const float updateDiff = fabsf(preIntensity - sumIntensity) + fabsf(preX - mX) + fabsf(preY - mY);
    const bool tStable = sp_lt_02(updateDiff);   // `updateDiff < 0.2` (:489), float form
    const float tDepth = U.depthLoop ? U.meanDepth : 0.0f;   // no valid depth among the seed's pixels: 0 (:489-490)
    uint4 w0 = w0o, w2 = w2o, w3 = w3o;
    w0.x = __float_as_uint(mX); w0.y = __float_as_uint(mY);
    w2.z = __float_as_uint(tDepth); w2.w = __float_as_uint(sumIntensity);
    w3.x = (unsigned)tR; w3.y = (unsigned)tG; w3.z = (unsigned)tB;
    w3.w = (w3.w & 0x00FF00FFu) | (tStable ? 0x100u : 0u);
    rec[0] = w0; rec[2] = w2; rec[3] = w3;
    P.tmin[si] = tStable ? T_INF : 0u;
    AssignRec a;
    a.x = mX; a.y = mY; a.meanIntensity = sumIntensity; a.stable = tStable ? 1u : 0u;
    a.invDepth = arec_inv_depth(tDepth); a._pad = 0;   // (the one expression ever stored there: the invariant kb_assign's sign test rests on)
    P.arec[si] = a;
}

// Test hook of the rotating chains: list q (<= 256 floats at x + 256 q, n[q] of them valid) is summed by the 16 lanes of row q & 3 of wave q >> 2 exactly
// the way kb_update_seeds sums a seed's depth list (huber = 0) or its Huber terms (huber = 1: +-inf entries mark tail elements).
__global__ __launch_bounds__(64) void k_debug_chain(const float *x, const int *n, float *out, int lists, int huber) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 4), l = threadIdx.x & 15;
    const int nq = q < lists ? n[q] : 0;
    int nblk = (nq + 15) >> 4;
#pragma unroll
    for (int d = 32; d >= 16; d >>= 1) nblk = max(nblk, __shfl_xor(nblk, d, 64));
    nblk = __builtin_amdgcn_readfirstlane(nblk);
    float s = 0.0f;
    for (int bq = 0; bq < nblk; bq++) {
        const int e = l + 16 * bq;
        const float t = e < nq ? x[(size_t)q * 256 + e] : 0.0f;
        s = huber ? chain_block_huber(s, t) : chain_block_f32(s, t);
    }
    if (q < lists && l == 15) out[q] = s;
}

// Test hook of the Newton quotient: out[i] = kb_update_seeds' deltaDepth for the numerator sumA[i] and inr[i] in-band depths (the float division),
// literal[i] = the reference's float / double expression, both evaluated here.
__global__ __launch_bounds__(256) void k_debug_newton(const float *sumA, const int *inr, float *out, float *literal, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = sp_newton_delta(sumA[i], inr[i]);
    literal[i] = sp_newton_delta_literal(sumA[i], inr[i]);
}

}  // namespace

namespace msl {
namespace sf {

// Seed pass `it`.  kb_update_seeds runs uncapped, 8 workgroups per CU (17 KB of LDS, 56 VGPRs): capped at 7 / 6 / 5 by unused dynamic LDS the front end
// made 23.1 / 23.2 / 22.7 k frames/s against 23.1 k -- no sweet spot below the maximum, unlike kb_seed_plane (round 5).
void sp_launch_seed_pass(KernelProfiler &prof, hipStream_t sp, const SfDev &P, int n, int it) {
    if (sp_quad_straddles(P.W)) MSL_SF_LAUNCH(prof, SK_UPDATE_SEEDS, sp, kb_update_seeds<true>, dim3(xcd_grid(upd_blocks(P.nseeds), n)), dim3(16 * UPD_SEEDS), P, it, n);
    else MSL_SF_LAUNCH(prof, SK_UPDATE_SEEDS, sp, kb_update_seeds<false>, dim3(xcd_grid(upd_blocks(P.nseeds), n)), dim3(16 * UPD_SEEDS), P, it, n);
    MSL_SF_LAUNCH(prof, SK_COMMIT_SEEDS, sp, kb_commit_seeds, sp_seed_grid(P, n), dim3(256), P, it);
}

int sp_debug_chain(const float *x_host, const int32_t *n_host, int lists, int huber, float *out_host) {
    if (lists <= 0) return MSL_OK;
    if (!x_host || !n_host || !out_host) return MSL_ERR_INVALID;
    for (int q = 0; q < lists; q++) if (n_host[q] < 0 || n_host[q] > 256) return MSL_ERR_INVALID;
    DevBuf x, cnt, out;
    MSL_HIP_TRY(grow_all(0, {{x, sizeof(float) * 256 * (size_t)lists}, {cnt, sizeof(int) * (size_t)lists}, {out, sizeof(float) * (size_t)lists}}));
    MSL_HIP_TRY(hipMemcpy(x.p, x_host, sizeof(float) * 256 * (size_t)lists, hipMemcpyHostToDevice));
    MSL_HIP_TRY(hipMemcpy(cnt.p, n_host, sizeof(int) * (size_t)lists, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_chain, dim3((unsigned)((lists + 3) / 4)), dim3(64), 0, 0, (const float *)x.p, (const int *)cnt.p, (float *)out.p, lists, huber);
    MSL_HIP_TRY(hipMemcpy(out_host, out.p, sizeof(float) * (size_t)lists, hipMemcpyDeviceToHost));
    return MSL_OK;
}

int sp_debug_newton(const float *sumA_host, const int32_t *inr_host, size_t n, float *out_host, float *literal_host) {
    if (n == 0) return MSL_OK;
    if (!sumA_host || !inr_host || !out_host || !literal_host) return MSL_ERR_INVALID;
    for (size_t i = 0; i < n; i++) if (inr_host[i] < 0 || inr_host[i] > SP_NEWTON_MAX_INR) return MSL_ERR_INVALID;
    DevBuf a, c, out, lit;
    MSL_HIP_TRY(grow_all(0, {{a, sizeof(float) * n}, {c, sizeof(int) * n}, {out, sizeof(float) * n}, {lit, sizeof(float) * n}}));
    MSL_HIP_TRY(hipMemcpy(a.p, sumA_host, sizeof(float) * n, hipMemcpyHostToDevice));
    MSL_HIP_TRY(hipMemcpy(c.p, inr_host, sizeof(int) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_newton, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const float *)a.p, (const int *)c.p, (float *)out.p, (float *)lit.p, (long long)n);
    MSL_HIP_TRY(hipMemcpy(out_host, out.p, sizeof(float) * n, hipMemcpyDeviceToHost));
    MSL_HIP_TRY(hipMemcpy(literal_host, lit.p, sizeof(float) * n, hipMemcpyDeviceToHost));
    return MSL_OK;
}

}  // namespace sf
}  // namespace msl
