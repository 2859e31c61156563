// msl_sf_sp_assign.hip -- superpixel stage for gfx950 (MI355X): seed initialisation, pixel assignment and the relaxation that gives the passes
// after the first the reference's raster-order `stable` semantics (stage overview: msl_sf_superpixel.hip).
//     kb_seed_init                        one thread per 8x8 superpixel seed                  (reference src/SurfelFusion.cpp:528-584)
//     kb_assign                           one wave per three dual cells: argmin over <= 4 seeds (:333-415)
//     kb_prop_lds | kb_prop x 6 + kb_prop_finish    the min-fixpoint t(s) over the worklist kb_assign left
//     kb_commit_px                        a pixel takes its pick iff its seed was unstable before it in raster order
//     k_debug_div100                      test hook of sp_div100_of_float

#include "msl_sf_sp_dev.h"

namespace {

__global__ __launch_bounds__(256) void kb_seed_init(SfDev P) {
    const int slot = blockIdx.y;
    const int seedI = blockIdx.x * 256 + threadIdx.x;
    if (seedI >= P.nseeds) return;
    if (seedI == 0) P.wlCount[slot] = 0;
    const FrameDev F = P.frames[slot];   // by value: one load up front instead of re-reading fields around every store
    const int spX = seedI % P.spW, spY = seedI / P.spW;
    int imageX = spX * SP + SP / 2, imageY = spY * SP + SP / 2;
    imageX = imageX < (P.W - 1) ? imageX : (P.W - 1);
    imageY = imageY < (P.H - 1) ? imageY : (P.H - 1);
    msl_seed s;
    memset(&s, 0, sizeof(s));
    P.fused[(size_t)slot * P.flagStride + seedI] = 0;
    if (member_at(P, F, imageY, imageX) != -1) {
        P.seeds[(size_t)slot * P.nseeds + seedI] = s; P.arec[(size_t)slot * P.nseeds + seedI] = assign_rec(s);
        return;
    }
    s.use = 1;
    s.x = (float)imageX; s.y = (float)imageY;
    vec3b(P, F, (float)imageY, (float)imageX, s.r, s.g, s.b);
    s.meanIntensity = gray_at(P, F, imageY, imageX);
    s.meanDepth = depth_at(P, F, imageY, imageX);
    if (sp_lt_001(s.meanDepth)) {   // `< 0.01` (:559), float form (msl_sf_sp_arith.h)
        int xb = spX * SP + SP / 2 - SP, yb = spY * SP + SP / 2 - SP;
        int xe = xb + SP * 2, ye = yb + SP * 2;
        xb = xb > 0 ? xb : 0; yb = yb > 0 ? yb : 0;
        xe = xe < P.W - 1 ? xe : P.W - 1; ye = ye < P.H - 1 ? ye : P.H - 1;
        bool found = false;
        for (int j = yb; j < ye && !found; j++)
            for (int i = xb; i < xe; i++) {
                const float d = depth_at(P, F, j, i);
                if (sp_gt_001(d)) { s.meanDepth = d; found = true; break; }   // `> 0.01` (:572)
            }
    }
    P.seeds[(size_t)slot * P.nseeds + seedI] = s;
    P.arec[(size_t)slot * P.nseeds + seedI] = assign_rec(s);
}

// kb_assign: a(p) = argmin seed of pixel p (:357-415 without the `stable` gate).  it == 0: every seed is
// unstable, so every free pixel is processed: write the index map directly.  it > 0: store a(p) and run
// relaxation round 0 (pixels whose current seed is unstable at pass start are processed for sure).
//
// One wave per "dual cell" [8 bx + 4, 8 bx + 12) x [8 by + 4, 8 by + 12), bx / by from -1.  Of the 3x3 neighbourhood only the seeds with
// |8c + 4 - x| < 8 on both axes are candidates (:384-389): per axis the pixel's own cell plus the left / upper neighbour when (x mod 8) < 4 or
// the right / lower one when (x mod 8) > 4 -- so ALL pixels of a dual cell have the same candidates {bx, bx + 1} x {by, by + 1} (its first
// column / row, x mod 8 == 4, only the first of each pair).  The candidates are therefore wave-uniform: their fields are scalar operands, and
// the per-pixel work is the four cost evaluations and nothing else.  Enumeration in the reference's order (checkI outer, checkJ inner, ascending).
constexpr int ASSIGN_NY = 3;   // dual cells (one below the other) per wave.  Everything the wave reads -- the NY + 1 lattice rows of candidate records
                               // (scalar loads) and the pixels' member / gray / depth / index words -- is requested before the first use: with one
                               // pixel per lane and loads that wait for one another the kernel had too few bytes in flight to keep HBM busy while
                               // other waves computed (35 us of memory time and 43 us of cost arithmetic per pass simply added up).
                               // 3 instead of 2: the slot mapping, the FrameDev load and the column terms are paid once for 192 pixels (213 instead
                               // of 221 VALU per cell, 60 VGPRs; 4 would need 74).  A column's last wave may have cells below the image (inImg).
constexpr int ASSIGN_WAVES = 4;   // waves (dual-cell columns) per workgroup.  The waves share nothing (no barrier, no LDS), but one-wave workgroups
                                  // lose here: front end -1.7 %
__host__ __device__ constexpr int assign_blocks(int nbx, int nby) { return ((nbx + ASSIGN_WAVES - 1) / ASSIGN_WAVES) * ((nby + ASSIGN_NY - 1) / ASSIGN_NY); }
__global__ __launch_bounds__(64 * ASSIGN_WAVES) void kb_assign(SfDev P, int it, int nSlots, int nbx, int nby) {
    const int bpr = (nbx + ASSIGN_WAVES - 1) / ASSIGN_WAVES;   // workgroups per row of dual cells
    int slot, blk;
    if (!xcd_slot(assign_blocks(nbx, nby), nSlots, slot, blk)) return;
    if (blk == 0) {   // (lanes of the workgroup's first wave)
        if (it > 0 && threadIdx.x < 8) P.changed[slot * 8 + threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
        if (threadIdx.x >= 32 && threadIdx.x < 32 + NCHUNK) P.chunkAbort[(slot * 2 + (it & 1)) * 16 + threadIdx.x - 32] = 0x7FFFFFFF;
    }
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int byg = blk / bpr, bxi = (blk - byg * bpr) * ASSIGN_WAVES + wv;
    if (bxi >= nbx) return;
    const int bx = bxi - 1, by0 = byg * ASSIGN_NY - 1;
    // The candidates (wave-uniform): cell k uses lattice rows by0 + k and by0 + k + 1, in each the neighbours bx and bx + 1 -- two records that
    // are adjacent in memory.  Rows / columns outside the lattice are clamped for the address (the array has a record of padding either side)
    // and never evaluated (the range test of :384-389).
    const bool okx0 = bx >= 0 && bx < P.spW, okx1 = bx + 1 < P.spW;
    const int bxc = min(bx, P.spW - 1);
    const AssignRec *arec = P.arec + (unsigned)slot * (unsigned)P.nseeds;
    AssignRec cr[ASSIGN_NY + 1][2];
    int rowIdx[ASSIGN_NY + 1];
#pragma unroll
    for (int r = 0; r <= ASSIGN_NY; r++) {
        const int rc = min(max(by0 + r, 0), P.spH - 1);
        rowIdx[r] = rc * P.spW + bx;                       // seed index of (bx, by0 + r) when valid
        const AssignRec *rp = arec + (rc * P.spW + bxc);
        cr[r][0] = rp[0]; cr[r][1] = rp[1];
    }
    const FrameDev F = P.frames[slot];   // by value: one load up front instead of re-reading fields around every store
    unsigned short *index = P.index + (size_t)slot * P.pxStride, *amap = P.amap + (size_t)slot * P.pxStride;
    float *pxInv = P.pxInv + (size_t)slot * P.pxStride;
    unsigned *tmin = P.tmin + (size_t)slot * P.nseeds;
    const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
    const int colI = 8 * bx + 4 + lx;
    const float colF = (float)colI;
    const bool colIn = colI >= 0 && colI < P.W;
    // ---- all loads of the wave's pixels ----
    bool inImg[ASSIGN_NY];
    int mem[ASSIGN_NY], cur[ASSIGN_NY];
    float gI[ASSIGN_NY], dIn[ASSIGN_NY];
    unsigned tCur[ASSIGN_NY];
#pragma unroll
    for (int k = 0; k < ASSIGN_NY; k++) {
        const int rowI = 8 * (by0 + k) + 4 + ly;
        inImg[k] = colIn && rowI >= 0 && rowI < P.H && by0 + k + 1 < nby;
        const int rowC = min(max(rowI, 0), P.H - 1), colC = min(max(colI, 0), P.W - 1), pc = rowC * P.W + colC;   // (a clamped address: loaded, never used)
        mem[k] = member_at(P, F, rowC, colC);
        gI[k] = gray_at(P, F, rowC, colC);
        dIn[k] = it == 0 ? depth_at(P, F, rowC, colC) : *byte_off(pxInv, 4u * (unsigned)pc);
        cur[k] = it == 0 ? 0 : (int)*byte_off(index, 2u * (unsigned)pc);
    }
#pragma unroll
    for (int k = 0; k < ASSIGN_NY; k++)
        tCur[k] = it == 0 ? 0u : *byte_off(tmin, 4u * (unsigned)cur[k]);   // (a plain load: 0 stays 0 and non-zero stays non-zero during the pass, so a stale line answers the same)
    // ---- per cell: the four cost evaluations ----
#pragma unroll
    for (int k = 0; k < ASSIGN_NY; k++) {
        const int by = by0 + k;
        if (__ballot(inImg[k]) == 0) continue;
        const bool oky0 = by >= 0 && by < P.spH, oky1 = by + 1 < P.spH;
        const int rowI = 8 * by + 4 + ly;
        const int p = rowI * P.W + colI;
        const bool isPlane = mem[k] != -1;
        const float myIntensity = gI[k];
        // (float)(1.0 / (double)depth) is the same in all three passes: computed (one f64 divide) in pass 0, read back afterwards
        float myInvDepth = dIn[k];
        if (it == 0) {
            myInvDepth = 0.0f;
            if (sp_gt_001(dIn[k])) myInvDepth = (float)(1.0 / (double)dIn[k]);   // `> 0.01` (:373), float form
            if (inImg[k] && !isPlane) *byte_off_w(pxInv, 4u * (unsigned)p) = myInvDepth;
        }
        const bool pxHasDepth = myInvDepth > 0;
        const double myInvD = (double)myInvDepth;
        const float rowF = (float)rowI;
        float minDistDepth = 1e6f, minDistNodepth = 1e6f;
        int minSpIndexDepth = -1, minSpIndexNodepth = -1;
        bool allHasDepth = true;
        // calculateCost (:333-355) + the two running minima (:398-410) for one candidate; `use` = this pixel has the candidate (x mod 8 == 4:
        // the pixel's own cell only).  Selects instead of branches.
        auto consider = [&](const AssignRec &C, int spIndex, bool use) {
            // `C.invDepth >= 0` (:348) from the sign of the record's high word: the record is a scalar operand, so this is one s_cmp per candidate
            // where the f64 comparison was a v_cmp_ge_f64 per cost evaluation (the invariant: arec_has_depth, msl_sf.h)
            const bool candHas = arec_has_depth(C);
            float nodepthCost = 0;
            const float dist = (C.x - colF) * (C.x - colF) + (C.y - rowF) * (C.y - rowF);
            nodepthCost += dist / ((SP / 2) * (SP / 2));
            const float intensityDiff = C.meanIntensity - myIntensity;
            nodepthCost = sp_cost_add_intensity(nodepthCost, intensityDiff);   // (one correction step: the dividend is a float, msl_sf_sp_arith.h)
            const bool has = candHas && pxHasDepth;
            const float inverseDepthDiff = (float)(C.invDepth - myInvD);
            const float withDepth = sp_cost_add_depth(nodepthCost, inverseDepthDiff);   // (one FMA: float * 400.0 is exact in binary64)
            const float depthCost = has ? withDepth : nodepthCost;
            allHasDepth = allHasDepth && (has || !use);
            const bool bd = use && depthCost < minDistDepth, bn = use && nodepthCost < minDistNodepth;
            minDistDepth = bd ? depthCost : minDistDepth; minSpIndexDepth = bd ? spIndex : minSpIndexDepth;
            minDistNodepth = bn ? nodepthCost : minDistNodepth; minSpIndexNodepth = bn ? spIndex : minSpIndexNodepth;
        };
        const bool anyStable = (cr[k][0].stable | cr[k][1].stable | cr[k + 1][0].stable | cr[k + 1][1].stable) != 0;   // (wave-uniform; rare)
        // the reference's order: checkI (x) outer, checkJ (y) inner, ascending
        if (okx0 && oky0) consider(cr[k][0], rowIdx[k], true);
        if (okx0 && oky1) consider(cr[k + 1][0], rowIdx[k + 1], ly != 0);
        if (okx1 && oky0) consider(cr[k][1], rowIdx[k] + 1, lx != 0);
        if (okx1 && oky1) consider(cr[k + 1][1], rowIdx[k + 1] + 1, lx != 0 && ly != 0);
        const int pick = allHasDepth ? minSpIndexDepth : minSpIndexNodepth;
        if (!inImg[k]) continue;
        if (it == 0) { *byte_off_w(index, 2u * (unsigned)p) = isPlane ? (unsigned short)0 : (unsigned short)(pick >= 0 ? pick : 0); continue; }
        *byte_off_w(amap, 2u * (unsigned)p) = isPlane ? IDX_PLANE : (pick >= 0 ? (unsigned short)pick : IDX_NONE);
        if (!isPlane && pick >= 0) {
            // the current seed is unstable at pass start <=> t(cur) == 0 (kb_update_seeds / kb_commit_seeds left 0 or T_INF, and this pass
            // only ever lowers a t to p + 1 >= 1, so a value read at any time during the pass answers the same)
            if (tCur[k] == 0) {
                // processed for sure (round 0): t(pick) = min(t(pick), p + 1) -- only a candidate that entered the pass stable has a t above 0
                if (anyStable && tmin[pick] > (unsigned)p + 1u) atomicMin(&tmin[pick], (unsigned)p + 1u);
            } else if (pick != cur[k]) {
                // Only these pixels can extend a chain: p is processed iff its (stable) seed gets unstabilised before p, and it
                // then unstabilises a DIFFERENT seed.  (pick == cur would only re-lower t(cur) above its current value.)
                P.wl[(size_t)slot * P.pxStride + atomicAdd(&P.wlCount[slot], 1u)] = (unsigned)p;
            }
        }
    }
}

// t(s) = raster position from which seed s counts as unstable: 0 if unstable at pass start, else
// 1 + the first processed pixel that picked it (min-fixpoint).
__device__ __forceinline__ bool relax_pixel(unsigned *tmin, const unsigned short *index, const unsigned short *amap, int p) {
    const unsigned short a = amap[p];
    if (a >= IDX_PLANE) return false;
    const unsigned tc = __hip_atomic_load(&tmin[index[p]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tc == 0 || tc > (unsigned)p) return false;     // tc == 0: handled in round 0; tc > p: not processed (yet)
    if (__hip_atomic_load(&tmin[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned)p + 1u) return false;
    return atomicMin(&tmin[a], (unsigned)p + 1u) > (unsigned)p + 1u;
}

constexpr int PROP_BLOCKS = 16;   // workgroups per keyframe over the (small) worklist
__global__ __launch_bounds__(256) void kb_prop(SfDev P, int round, int nSlots) {
    int slot, blk;
    if (!xcd_slot(PROP_BLOCKS, nSlots, slot, blk)) return;
    if (!P.changed[slot * 8 + round]) return;
    unsigned *tmin = P.tmin + (size_t)slot * P.nseeds;
    const unsigned short *index = P.index + (size_t)slot * P.pxStride, *amap = P.amap + (size_t)slot * P.pxStride;
    const unsigned *wl = P.wl + (size_t)slot * P.pxStride;
    const unsigned nwl = P.wlCount[slot];
    bool any = false;
    for (unsigned e = blk * 256 + threadIdx.x; e < nwl; e += PROP_BLOCKS * 256) any |= relax_pixel(tmin, index, amap, (int)wl[e]);
    if (any) P.changed[slot * 8 + round + 1] = 1;
}

// Finisher: one workgroup per keyframe iterates the relaxation to its fixpoint (normally zero rounds).
__global__ __launch_bounds__(1024) void kb_prop_finish(SfDev P) {
    __shared__ int s_ch;
    const int slot = blockIdx.x;
    if (threadIdx.x == 0) s_ch = P.changed[slot * 8 + PROP_ROUNDS];
    __syncthreads();
    unsigned *tmin = P.tmin + (size_t)slot * P.nseeds;
    const unsigned short *index = P.index + (size_t)slot * P.pxStride, *amap = P.amap + (size_t)slot * P.pxStride;
    const unsigned *wl = P.wl + (size_t)slot * P.pxStride;
    const unsigned nwl = P.wlCount[slot];
    while (s_ch) {
        __syncthreads();
        if (threadIdx.x == 0) s_ch = 0;
        __syncthreads();
        bool any = false;
        for (unsigned e = threadIdx.x; e < nwl; e += 1024) any |= relax_pixel(tmin, index, amap, (int)wl[e]);
        if (any) s_ch = 1;
        __syncthreads();
    }
}

// The whole relaxation in ONE launch: one workgroup per keyframe keeps t(s) in LDS (4 B per seed) and its share of the
// worklist in registers, so a round costs a few LDS operations instead of a kernel boundary plus agent-scope round trips.
// The min-fixpoint is unique, so the evaluation order does not matter.  (kb_prop / kb_prop_finish remain as the fallback
// for seed counts whose t(s) does not fit the LDS.)
constexpr int PROP_LDS_MAX_SEEDS = 36 * 1024;   // 144 KB
__global__ __launch_bounds__(256) void kb_prop_lds(SfDev P) {
    extern __shared__ unsigned s_t[];
    const int slot = blockIdx.x;
    const unsigned nwl = P.wlCount[slot];
    if (nwl == 0) return;
    unsigned *tmin = P.tmin + (size_t)slot * P.nseeds;
    const unsigned short *index = P.index + (size_t)slot * P.pxStride, *amap = P.amap + (size_t)slot * P.pxStride;
    const unsigned *wl = P.wl + (size_t)slot * P.pxStride;
    constexpr int NT = 256, R = 16;   // a 256-thread workgroup finds room on a busy GPU; a 16-wave one waits for a whole CU
    unsigned ep[R];
    unsigned short ec[R], ea[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const unsigned e = threadIdx.x + r * NT;
        ep[r] = 0xFFFFFFFFu; ec[r] = 0; ea[r] = 0;
        if (e < nwl) { const unsigned p = wl[e]; ep[r] = p; ec[r] = index[p]; ea[r] = amap[p]; }
    }
    for (int i = threadIdx.x; i < P.nseeds; i += NT) s_t[i] = tmin[i];
    __syncthreads();
    auto relax = [&](unsigned p, unsigned short cur, unsigned short a) -> bool {
        if (a >= IDX_PLANE) return false;
        const unsigned tc = s_t[cur];
        if (tc == 0 || tc > p) return false;            // tc == 0: handled in round 0; tc > p: not processed (yet)
        if (s_t[a] <= p + 1u) return false;
        return atomicMin(&s_t[a], p + 1u) > p + 1u;
    };
    int any;
    do {
        bool ch = false;
#pragma unroll
        for (int r = 0; r < R; r++)
            if (ep[r] != 0xFFFFFFFFu) ch |= relax(ep[r], ec[r], ea[r]);
        for (unsigned e = threadIdx.x + R * NT; e < nwl; e += NT) { const unsigned p = wl[e]; ch |= relax(p, index[p], amap[p]); }
        any = __syncthreads_or(ch ? 1 : 0);
    } while (any);
    for (int i = threadIdx.x; i < P.nseeds; i += NT) {
        const unsigned t = s_t[i];
        if (t != tmin[i]) tmin[i] = t;
    }
}

__global__ __launch_bounds__(256) void kb_commit_px(SfDev P, int nSlots) {
    // 8 consecutive pixels per thread (16-byte loads of both maps; the slot stride is a multiple of 64).  A pixel whose pick equals its
    // current seed cannot change, so t(s) is only looked up for the few pixels that picked a different seed.
    int slot, blk;
    if (!xcd_slot(((P.npx + 7) / 8 + 255) / 256, nSlots, slot, blk)) return;
    const int p0 = (blk * 256 + threadIdx.x) * 8;
    if (p0 >= P.npx) return;
    unsigned short *index = P.index + (size_t)slot * P.pxStride;
    const uint4 a4 = *reinterpret_cast<const uint4 *>(P.amap + (size_t)slot * P.pxStride + p0);
    uint4 i4 = *reinterpret_cast<const uint4 *>(index + p0);
    const unsigned *tmin = P.tmin + (size_t)slot * P.nseeds;
    unsigned aw[4] = {a4.x, a4.y, a4.z, a4.w}, iw[4] = {i4.x, i4.y, i4.z, i4.w};
    bool changed = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const unsigned a = (aw[k >> 1] >> (16 * (k & 1))) & 0xFFFFu, cur = (iw[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        if (a >= IDX_PLANE || a == cur || p0 + k >= P.npx) continue;   // (the last group may reach into the slot's padding)
        if (tmin[cur] <= (unsigned)(p0 + k)) {
            iw[k >> 1] = (iw[k >> 1] & ~(0xFFFFu << (16 * (k & 1)))) | (a << (16 * (k & 1)));
            changed = true;
        }
    }
    if (changed) { i4.x = iw[0]; i4.y = iw[1]; i4.z = iw[2]; i4.w = iw[3]; *reinterpret_cast<uint4 *>(index + p0) = i4; }
}

__global__ void k_debug_div100(const float *x, double *out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sp_div100_of_float(x[i] * x[i]);   // (what kb_assign evaluates: the dividend is a float product)
}

}  // namespace

namespace msl {
namespace sf {

bool sp_init_attributes(int nseeds) {
    // the attribute belongs to the function, not to a handle: always ask for the largest size any handle may use
    if (nseeds > PROP_LDS_MAX_SEEDS) return false;
    return hipFuncSetAttribute((const void *)kb_prop_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(unsigned) * PROP_LDS_MAX_SEEDS)) == hipSuccess;
}

void sp_launch_seed_init(KernelProfiler &prof, hipStream_t sp, const SfDev &P, int n) {
    MSL_SF_LAUNCH(prof, SK_SEED_INIT, sp, kb_seed_init, sp_seed_grid(P, n), dim3(256), P);
}

// Pixel pass `it`: the assignment, then (it > 0) the relaxation in one launch (propLds) or in rounds, and the commit of the index map.
void sp_launch_pixel_pass(KernelProfiler &prof, hipStream_t sp, const SfDev &P, int n, int it, bool propLds) {
    const int W = P.W, H = P.H;
    const unsigned un = (unsigned)n;
    const int nbx = ((W - 5) >> 3) + 2, nby = ((H - 5) >> 3) + 2;   // dual cells [8 b + 4, 8 b + 12), b from -1, that meet the image
    const dim3 pxGrid(xcd_grid(assign_blocks(nbx, nby), n)), flatPx(xcd_grid(((P.npx + 7) / 8 + 255) / 256, n));
    MSL_SF_LAUNCH(prof, SK_ASSIGN, sp, kb_assign, pxGrid, dim3(64 * ASSIGN_WAVES), P, it, n, nbx, nby);
    if (it > 0) {
        prof.begin(SK_PROP, sp);
        if (propLds) {
            hipLaunchKernelGGL(kb_prop_lds, dim3(un), dim3(256), sizeof(unsigned) * P.nseeds, sp, P);
        } else {
            for (int r = 0; r < PROP_ROUNDS; r++) hipLaunchKernelGGL(kb_prop, dim3(xcd_grid(PROP_BLOCKS, n)), dim3(256), 0, sp, P, r, n);
            hipLaunchKernelGGL(kb_prop_finish, dim3(un), dim3(1024), 0, sp, P);
        }
        prof.end(sp);
        MSL_SF_LAUNCH(prof, SK_COMMIT_PX, sp, kb_commit_px, flatPx, dim3(256), P, n);
    }
}

int sp_debug_div100(const float *x_host, double *out_host, size_t n) {
    if (n == 0) return MSL_OK;
    if (!x_host || !out_host) return MSL_ERR_INVALID;
    DevBuf x, out;
    MSL_HIP_TRY(grow_all(0, {{x, sizeof(float) * n}, {out, sizeof(double) * n}}));
    MSL_HIP_TRY(hipMemcpy(x.p, x_host, sizeof(float) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_div100, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const float *)x.p, (double *)out.p, (long long)n);
    MSL_HIP_TRY(hipMemcpy(out_host, out.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return MSL_OK;
}

}  // namespace sf
}  // namespace msl
