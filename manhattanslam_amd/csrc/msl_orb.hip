// msl_orb.hip -- ORB extractor for gfx950 (MI355X): kernels + device driver (host plan, handle and C ABI: msl_orb_host.hip).
//
// Replaces ORB_SLAM2::ORBextractor (reference src/ORBextractor.cc).  Frame-batched pipeline, all
// integer/byte work, HBM/L2-bound; no MFMA (nothing here is a contraction).  Per batch of B frames:
//
//   k_pyramid  x1      all levels, tile chains through LDS (k_resize x(L-1) as fallback): OpenCV 11-bit fixed-point bilinear   (:872-893, cv::resize)
//   k_fast     x1      one wave per 30-px FAST cell: LDS-staged tile, packed quick test, FAST-9/16 score,
//                      in-cell 3x3 NMS, at iniTh and only then at minTh, ordered ballot compaction (:745-780)
//   k_octree   x1      one workgroup per (frame, level): quadtree distribution, LDS resident (:531-721)
//   k_blur     x1      7x7 sigma-2 fixed-point separable Gaussian, LDS tile             (:851-852)
//   k_describe x1      one wave per keypoint: IC_Angle + steered BRIEF-256, output assembly
//                                                                      (:75-149, :470-475, :829-869)
//
// Float expressions that feed a rounding (angle, rotated pattern coordinates) are written in the
// reference's order and this file is compiled with -ffp-contract=off.

#include "msl_orb_dev.h"
#include "msl_orb_fast.h"
#include "msl_orb_sums.h"

#include <type_traits>

#include <cfloat>
#include <cmath>
#include <cstdlib>

using namespace msl;
using namespace msl::orb;

namespace {

__constant__ int8_t c_pattern[1024] = {
#include "../../include/msl_orb_pattern.inc"
};

__device__ __forceinline__ const uint8_t *level_ptr(const OrbDev &P, int frame, int l, int &pitch) {
    if (l == 0) { pitch = (int)P.inRowStride; return P.in + (size_t)frame * P.inFrameStride; }
    pitch = P.lv[l].pitch;
    return P.pyr + (size_t)frame * P.pyrStride + P.lv[l].off;
}

// ---------------------------------------------------------------------------------------------
// k_resize: level l from level l-1.  One thread per output pixel; taps come from host-built tables
// so the coefficient arithmetic (double -> float -> cvRound) is the host's.
// ---------------------------------------------------------------------------------------------
// XCD-aware block -> (item, frame) mapping for the frame-batched kernels.  Workgroup g of a launch runs on XCD g % 8 (dispatch order; used for
// speed only) and every XCD has its own 4 MB L2.  With blockIdx.y = frame each frame's workgroups were spread over all eight L2s, so every
// pyramid line was fetched from HBM / Infinity Cache up to eight times (FAST cell rows of 36 bytes, blur tiles, descriptor patches: 15.2 MB per
// frame against 1.9 MB of algorithmic reads in round 3).  Launch a 1-D grid of xcd_grid1(nx * ny) workgroups instead: XCD x gets the contiguous
// run of virtual indices [x C, (x + 1) C), C = ceil(nx ny / 8), i.e. whole frames (and inside a frame neighbouring cells / tiles) share one L2.
__device__ __forceinline__ bool xcd_item(int nx, int ny, int &x, int &y) {
    const unsigned g = blockIdx.x, C = gridDim.x >> 3;
    const unsigned v = (g & 7u) * C + (g >> 3);
    if (v >= (unsigned)nx * (unsigned)ny) return false;
    x = (int)(v % (unsigned)nx); y = (int)(v / (unsigned)nx);
    return true;
}
inline unsigned xcd_grid1(long long items) { return (unsigned)(8 * ((items + 7) / 8)); }

__global__ __launch_bounds__(256) void k_resize(OrbDev P, int l) {
    const int frame = blockIdx.z;
    const LevelDev &D = P.lv[l];
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= D.w || dy >= D.h) return;
    int sp;
    const uint8_t *src = level_ptr(P, frame, l - 1, sp);
    const ResizeTap tx = P.taps[D.xtabOff + dx], ty = P.taps[D.ytabOff + dy];
    const uint8_t *r0 = src + (size_t)ty.s0 * sp, *r1 = src + (size_t)ty.s1 * sp;
    const int h0 = r0[tx.s0] * tx.c0 + r0[tx.s1] * tx.c1;
    const int h1 = r1[tx.s0] * tx.c0 + r1[tx.s1] * tx.c1;
    int v = (((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
    v = min(max(v, 0), 255);
    P.pyr[(size_t)frame * P.pyrStride + D.off + (size_t)dy * D.pitch + dx] = (uint8_t)v;
}

// ---------------------------------------------------------------------------------------------
// k_pyramid: ALL levels in one launch.  The pyramid is a chain (level l is resized from level l-1, :872-893), but a tile of level l
// only depends on a slightly larger tile of level l-1: every level is cut into the same pyrTX x pyrTY grid of tiles, workgroup (i, j)
// owns tile (i, j) on every level, loads its part of the input once, and walks down the chain in LDS (two ping-pong buffers),
// recomputing the few halo pixels its next level reads beyond its own tile (~1.3x the arithmetic, 1/7 of the launches and no
// level ever re-read from HBM by the resize chain).  Each pixel is computed with k_resize's expression and taps from
// the same source values, so the levels are the same bytes; every pixel of a level is written by exactly one workgroup.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pyramid(OrbDev P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_pyr[];
    int tileI, frame;
    if (!xcd_item(P.pyrTX * P.pyrTY, P.nFrames, tileI, frame)) return;
    const int ti = tileI % P.pyrTX, tj = tileI / P.pyrTX;
    const int L = P.nlevels;
    PyrRange rx = P.pyrX[ti], ry = P.pyrY[tj];   // level 0: the input region
    // The level held in the source buffer: pixel (x, y) at (y - soy) * spitch + (x - sox).  Every pitch is a multiple of four: the input region is
    // staged with whole dwords (round 6: four bytes per load -- the byte-wise loop was 40 trips of a 64-bit address computation and one byte per
    // thread), and a later level starts at the column needLo & ~3, so that a lane's run of four pixels is one aligned dword in LDS and in memory.
    int sox = rx.needLo, soy = ry.needLo, spitch = (rx.needHi - rx.needLo + 3) & ~3;
    // The column taps of a level's runs are read from LDS: staged (coalesced, once per workgroup) while the level before is computed, two rows of
    // PYR_TAPS entries in turn.  Fetched from the table by each lane, four adjacent entries at a lane stride of 32 bytes, they cost four times the
    // cache lines per load instruction of the one-pixel form, and the kernel took twice as long.
    ResizeTap *const s_tx = reinterpret_cast<ResizeTap *>(s_pyr + P.pyrTapOff);
    auto stage_taps = [&](int l) {   // level l's entries for the columns needLo & ~3 .. + 4 ng (those beyond the level's last column are the first of its row table)
        const PyrRange r = P.pyrX[l * P.pyrTX + ti];
        const int lo = r.needLo & ~3, n = (r.needHi - lo + 3) & ~3;
        const ResizeTap *xtab = P.taps + P.lv[l].xtabOff + lo;
        for (int c = threadIdx.x; c < n; c += 256) s_tx[(l & 1) * PYR_TAPS + c] = xtab[c];
    };
    if (L > 1) stage_taps(1);
    {
        const int sh = ry.needHi - ry.needLo;
        int pitch;
        const uint8_t *img = level_ptr(P, frame, 0, pitch);
        const int nw = spitch >> 2, imgW = P.lv[0].w;
        const unsigned m = ((1u << 22) + nw - 1) / nw;   // exact floor(i / nw) for i < 2^15, nw < 2^7
        for (int i = threadIdx.x; i < nw * sh; i += 256) {
            const int r = (int)__umulhi((unsigned)i << 10, m), q = i - r * nw;   // (i m) >> 22
            const int x = sox + 4 * q;
            const uint8_t *src = img + (unsigned)((soy + r) * pitch + x);
            unsigned v = 0;
            if (x + 3 < imgW) __builtin_memcpy(&v, src, 4);   // (bytes beyond the region but inside the image row: staged, never read)
            else
                for (int e = 0; e < 4 && x + e < imgW; e++) v |= (unsigned)src[e] << (8 * e);
            reinterpret_cast<unsigned *>(s_pyr)[i] = v;
        }
    }
    __syncthreads();
    for (int l = 1; l < L; l++) {
        const LevelDev &D = P.lv[l];
        const uint8_t *src = s_pyr + (((l - 1) & 1) ? P.pyrBuf0 : 0u);
        unsigned *dst = reinterpret_cast<unsigned *>(s_pyr + ((l & 1) ? P.pyrBuf0 : 0u));
        rx = P.pyrX[l * P.pyrTX + ti]; ry = P.pyrY[l * P.pyrTY + tj];
        // A lane computes a run of four adjacent pixels of one row (the needed rectangle, widened to whole runs): one row tap and four column taps
        // (adjacent entries of the staged table: 32 contiguous bytes of LDS) per run, the source bytes as aligned LDS words, one dword to LDS and -- where the run is
        // owned -- one to memory.  The pixels are k_resize's, by the same expression (resize_px, msl_orb_sums.h).
        const int dox = rx.needLo & ~3, doy = ry.needLo, ng = (rx.needHi - dox + 3) >> 2, dh = ry.needHi - ry.needLo;
        uint8_t *out = P.pyr + (size_t)frame * P.pyrStride + D.off;
        const ResizeTap *ytab = P.taps + D.ytabOff, *xtap = s_tx + (l & 1) * PYR_TAPS;
        if (l + 1 < L) stage_taps(l + 1);
        const unsigned m = ((1u << 22) + ng - 1) / ng;
        for (int i = threadIdx.x; i < ng * dh; i += 256) {
            const int r = (int)__umulhi((unsigned)i << 10, m), g = i - r * ng;   // (i m) >> 22 without the 64-bit product
            const int dx = dox + 4 * g, dy = doy + r;
            const ResizeTap ty = ytab[dy];
            ResizeTap tx[4];
            __builtin_memcpy(tx, xtap + 4 * g, sizeof tx);
            const int rb0 = (ty.s0 - soy) * spitch - sox, rb1 = (ty.s1 - soy) * spitch - sox;
            // All four pixels are computed, without a branch: the words of the eight source pairs leave together.  A column outside the needed range
            // (the run was widened to whole dwords) has its tap clamped into the source row, so that every address is a staged one; its byte is
            // never read by the next level and never stored to memory.
            unsigned pr0[4], pr1[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int s0 = min(max((int)tx[k].s0, sox), sox + spitch - 1);
                const int a0 = rb0 + s0, a1 = rb1 + s0;   // (the same byte offset in their words: the pitch is a multiple of four)
                const unsigned *w0 = reinterpret_cast<const unsigned *>(src + (a0 & ~3)), *w1 = reinterpret_cast<const unsigned *>(src + (a1 & ~3));
                pr0[k] = resize_pair(w0[0], w0[1], a0 & 3); pr1[k] = resize_pair(w1[0], w1[1], a0 & 3);
            }
            unsigned run = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned cx = (unsigned)(unsigned short)tx[k].c0 | ((unsigned)(unsigned short)tx[k].c1 << 16);
                run |= resize_px(pr0[k], pr1[k], cx, ty.c0, ty.c1) << (8 * k);
            }
            dst[i] = run;
            if (dy >= ry.ownLo && dy < ry.ownHi) {
                uint8_t *o = out + (size_t)dy * D.pitch + dx;   // (dx is a multiple of four, and so are the level's offset and pitch)
                if (dx >= rx.ownLo && dx + 3 < rx.ownHi) *reinterpret_cast<unsigned *>(o) = run;
                else
                    for (int k = 0; k < 4; k++) if (dx + k >= rx.ownLo && dx + k < rx.ownHi) o[k] = (uint8_t)(run >> (8 * k));
            }
        }
        sox = dox; soy = doy; spitch = 4 * ng;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// k_fast: one wave (64 threads) per FAST cell; the integer pieces are msl_orb_fast.h.  Nothing here waits for another wave: no __syncthreads(),
// no LDS atomics.  Orderings come from ballots and mbcnt ranks, and LDS written by other lanes is read behind wave_lds_sync().
//   tile     (cw + 6) x (ch + 6) pixels into LDS, four bytes per load and store
//   stage    at a threshold: quick test -> list -> score -> 3x3 suppression inside the cell -> keys
//     quick test   a lane owns groups of four horizontally adjacent pixels, enumerated over a row pitch padded to four (the columns >= cw are masked):
//                  13 word reads, byte offset and widening by one v_perm per 16-bit pair (fast_quick4_at).  The groups' (row, group, element) order is
//                  the cell's row-major order; four ballots give every passing pixel its place in the list
//     score        64 list entries at a time: full lanes whatever the candidates' density (fast_score16)
//     suppression  over the list again; a ballot orders the kept pixels, which go straight to cellKeys (row-major order, as k_octree reads them)
//   The stage runs at iniTh.  Only a cell that keeps nothing there -- no corner at iniTh, or none that is a strict local maximum, e.g. two adjacent
//   equal maxima -- runs it again at minTh (:766-769); the branch is uniform over the wave.  A cell with corners at iniTh therefore never scores
//   the pixels that pass at minTh only.  That is exact: a pixel kept at iniTh scores above any neighbour that fails the quick test at iniTh,
//   whether that neighbour's score is stored or left 0 (fast_quick4).
// LDS is dynamic and sized by the largest cell of the geometry (fast_lds, OrbLaunch::fastLds): 5.8 KB for a 640 x 480 frame (the 37 x 34 cells of its last level).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// number of set bits of m below this lane
__device__ __forceinline__ unsigned lanes_below(unsigned long long m, unsigned add = 0) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, add));
}

__global__ __launch_bounds__(64) void k_fast(OrbDev P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_fast[];
    int cellI, frame;
    if (!xcd_item(P.cellsPerFrame, P.nFrames, cellI, frame)) return;
    const CellDev C = P.cells[cellI];
    const int lane = threadIdx.x;
    uint32_t *cnt_out = P.cellCnt + (size_t)frame * P.cellsPerFrame + cellI;
    const int cw = C.cw, ch = C.ch;
    if (cw <= 0 || ch <= 0) { if (lane == 0) *cnt_out = 0; return; }
    int pitch;
    const uint8_t *img = level_ptr(P, frame, C.level, pitch);
    const FastLds F = fast_lds(cw, ch);
    const int tp = F.tp, sp = F.sp;
    uint8_t *const s_tile = s_fast;                                                           // rows y0-3.., cols x0-3..
    uint8_t *const s_score = s_fast + F.scoreOff;                                             // pixel (r, c) at (r + 1) * sp + c + 1
    unsigned short *const s_list = reinterpret_cast<unsigned short *>(s_fast + F.listOff);    // r << 8 | c

    {   // four bytes per load and LDS store (the tile's rows start at any byte; a row's last word may reach 3 bytes past the tile, still inside
        // the image row: the cells end 13 px before the level's right edge).  The words of a row beyond these are never written: only masked
        // columns read them.
        const int nw = (cw + 6 + 3) >> 2;
        const unsigned mNw = ((1u << 20) + nw - 1) / nw;   // exact floor(i / w) for i < 2^13, w <= 2^7 by multiply-shift
        const uint8_t *src = img + (size_t)(C.y0 - 3) * pitch + (C.x0 - 3);
        for (int i = lane; i < nw * (ch + 6); i += 64) {
            const int r = (int)(((unsigned)i * mNw) >> 20), q = i - r * nw;
            uint32_t w4;
            __builtin_memcpy(&w4, src + (size_t)r * pitch + 4 * q, 4);
            *reinterpret_cast<uint32_t *>(&s_tile[r * tp + 4 * q]) = w4;
        }
    }
    for (int i = lane; i < (sp * (ch + 2) + 3) >> 2; i += 64) reinterpret_cast<uint32_t *>(s_score)[i] = 0u;
    wave_lds_sync();

    const int ngr = (cw + 3) >> 2, nGroups = ngr * ch, wp = tp >> 2;
    const unsigned mG = ((1u << 20) + ngr - 1) / ngr;
    uint32_t *out = P.cellKeys + (size_t)frame * P.keysPerFrame + C.keyOff;

    // quick test at thQuick, score, suppression; keeps the strict 3x3 maxima that score >= thKeep and returns their number
    auto stage = [&](int thQuick, int thKeep) -> unsigned {
        unsigned nlist = 0;
        for (int g0 = 0; g0 < nGroups; g0 += 64) {
            const int g = g0 + lane;
            unsigned m4 = 0;
            int r = 0, c0 = 0;
            if (g < nGroups) {
                r = (int)(((unsigned)g * mG) >> 20); c0 = 4 * (g - r * ngr);
                // tile rows r .. r + 6 are the centre row - 3 .. + 3; the words start at tile column c0 = the centres' column - 3
                const uint32_t *w = reinterpret_cast<const uint32_t *>(s_tile + r * tp + c0);
                const uint32_t u0 = w[0], u1 = w[1];                                                    // 3 rows up
                const uint32_t a0 = w[wp], a1 = w[wp + 1], a2 = w[wp + 2];                              // 2 rows up
                const uint32_t b0 = w[3 * wp], b1 = w[3 * wp + 1], b2 = w[3 * wp + 2];                  // the centre row
                const uint32_t d0 = w[5 * wp], d1 = w[5 * wp + 1], d2 = w[5 * wp + 2];                  // 2 rows down
                const uint32_t e0 = w[6 * wp], e1 = w[6 * wp + 1];                                      // 3 rows down
                m4 = fast_quick4_at({b0, b1, 3}, /*0*/ {e0, e1, 3}, /*8*/ {u0, u1, 3}, /*4*/ {b1, b2, 2}, /*12*/ {b0, b1, 0},
                                    /*2*/ {d1, d2, 1}, /*10*/ {a0, a1, 1}, /*6*/ {a1, a2, 1}, /*14*/ {d0, d1, 1}, thQuick);
                if (cw - c0 < 4) m4 &= (1u << (cw - c0)) - 1u;
            }
            const unsigned long long q0 = __ballot(m4 & 1u), q1 = __ballot(m4 & 2u), q2 = __ballot(m4 & 4u), q3 = __ballot(m4 & 8u);
            if (q0 | q1 | q2 | q3) {
                unsigned pos = nlist + lanes_below(q3, lanes_below(q2, lanes_below(q1, lanes_below(q0))));
                const unsigned rc = ((unsigned)r << 8) | (unsigned)c0;
                if (m4 & 1u) s_list[pos++] = (unsigned short)rc;
                if (m4 & 2u) s_list[pos++] = (unsigned short)(rc + 1);
                if (m4 & 4u) s_list[pos++] = (unsigned short)(rc + 2);
                if (m4 & 8u) s_list[pos++] = (unsigned short)(rc + 3);
                nlist += (unsigned)(__popcll(q0) + __popcll(q1) + __popcll(q2) + __popcll(q3));
            }
        }
        wave_lds_sync();
        for (unsigned j = lane; j < nlist; j += 64) {
            const unsigned rc = s_list[j];
            const int r = (int)(rc >> 8), c = (int)(rc & 255u);
            const uint8_t *t = &s_tile[(r + 3) * tp + c + 3];
            const int ring[16] = {t[3 * tp], t[3 * tp + 1], t[2 * tp + 2], t[tp + 3], t[3], t[-tp + 3], t[-2 * tp + 2], t[-3 * tp + 1],
                                  t[-3 * tp], t[-3 * tp - 1], t[-2 * tp - 2], t[-tp - 3], t[-3], t[tp - 3], t[2 * tp - 2], t[3 * tp - 1]};
            s_score[(r + 1) * sp + c + 1] = (uint8_t)max(fast_score16((int)t[0], ring), 0);
        }
        wave_lds_sync();
        unsigned kept = 0;
        for (unsigned j0 = 0; j0 < nlist; j0 += 64) {
            const unsigned j = j0 + lane;
            bool keep = false;
            uint32_t key = 0;
            if (j < nlist) {
                const unsigned rc = s_list[j];
                const int r = (int)(rc >> 8), c = (int)(rc & 255u);
                const uint8_t *q = &s_score[(r + 1) * sp + c + 1];
                const int s = q[0];
                keep = s >= thKeep && s > q[-1] && s > q[1] && s > q[-sp - 1] && s > q[-sp] && s > q[-sp + 1] && s > q[sp - 1] && s > q[sp] && s > q[sp + 1];
                const unsigned kx = C.x0 + c - 16, ky = C.y0 + r - 16;  // border-frame coordinates (:773-774)
                key = kx | (ky << 12) | ((unsigned)s << 24);
            }
            const unsigned long long m = __ballot(keep);
            if (keep) out[kept + lanes_below(m)] = key;
            kept += (unsigned)__popcll(m);
        }
        return kept;
    };

    const int thIni = min(P.iniTh, 256), thMin = min(P.minTh, 256);   // (a score is at most 254)
    unsigned total = stage(thIni, thIni);
    if (total == 0) {   // fallback to minTh when nothing survives at iniTh (:766-769)
        wave_lds_sync();
        total = stage(min(thIni, thMin), thMin);
    }
    if (lane == 0) *cnt_out = total;
}

// ---------------------------------------------------------------------------------------------
// k_octree: DistributeOctTree for one (frame, level).  The reference's std::list semantics are
// expressed with prefix sums: after a full round the list is [children of the expanded nodes, last
// expanded first, each as n4,n3,n2,n1] ++ [the one-key nodes in their old order]; in "careful"
// mode nodes are expanded largest first (ties: later created first) until the list reaches N.
// Keys never move: each keeps the list position of its node; the winner per final node is the
// max-response key, earliest in input order on ties.
// ---------------------------------------------------------------------------------------------
struct Rect { short x0, y0, x1, y1; };

__device__ __forceinline__ int quadrant(const Rect r, int x, int y) {
    const int mx = r.x0 + ((r.x1 - r.x0 + 1) >> 1), my = r.y0 + ((r.y1 - r.y0 + 1) >> 1);
    return (x < mx ? 0 : 1) + (y < my ? 0 : 2);
}
__device__ __forceinline__ Rect child_rect(const Rect r, int q) {
    const short mx = r.x0 + ((r.x1 - r.x0 + 1) >> 1), my = r.y0 + ((r.y1 - r.y0 + 1) >> 1);
    Rect c;
    c.x0 = (q & 1) ? mx : r.x0; c.x1 = (q & 1) ? r.x1 : mx;
    c.y0 = (q & 2) ? my : r.y0; c.y1 = (q & 2) ? r.y1 : my;
    return c;
}

// Experiment builds (-DMSL_OCT_STAMPS): the level-0 workgroup of frame 0 parks (100 MHz clock, shader clock) pairs at its phase boundaries behind
// the error word; msl_orb_debug_stamps reads them.
#ifdef MSL_OCT_STAMPS
#define OCT_STAMP(P, level, frame, idx)                                                                                   \
    do {                                                                                                                  \
        const int i_ = (idx);                                                                                             \
        if ((level) == 0 && (frame) == 0 && threadIdx.x == 0 && i_ < 100) {                                               \
            unsigned long long *d_ = reinterpret_cast<unsigned long long *>(reinterpret_cast<unsigned char *>((P).err) + 128); \
            d_[2 * i_] = __builtin_amdgcn_s_memrealtime(); d_[2 * i_ + 1] = __builtin_amdgcn_s_memtime();                 \
        }                                                                                                                 \
    } while (0)
#else
#define OCT_STAMP(P, level, frame, idx) do { } while (0)
#endif
// Where a workgroup keeps the level's candidate keys and their node ids while the list is subdivided.  REG: in registers (OCT_KPT per thread:
// <= 8192 candidates per level, which covers every frame but synthetic noise) -- a key never moves, only its node id changes, so no round
// touches memory for them; otherwise in the global keys / knode arrays as in rounds 1-3 (slower: every pass is a chain of L2 round trips).
// KPT = keys per thread held in registers (16: <= 8192 candidates per level, 32: <= 16384 -- level 0 of a 1280 x 960 frame has ~14 k); 0 = global arrays.
template <int KPT> struct OctKeys {
    static constexpr bool REG = KPT > 0;
    static constexpr int OCT_KPT = KPT > 0 ? KPT : 1;
    uint32_t key[OCT_KPT];
    unsigned node[OCT_KPT], quad[OCT_KPT];
    uint32_t *gkeys; uint16_t *gnode; unsigned n; int tid;
    unsigned per;   // REG: a thread owns the `per` CONSECUTIVE keys k = tid * per + j -- neighbours in FAST-cell order, i.e. mostly in the same node
    unsigned cnt;   // REG: how many of them exist: min(per, n - tid * per), 0 beyond the list's end
    // The number of keys this thread holds, as a value the compiler takes for new in every pass.  `j < cnt` is then one compare where it is used;
    // as loop invariants the sixteen (thirty-two) lane masks of `j < per && k < n` stayed in SGPRs across the whole kernel (k_octree<32>: 47
    // SGPRs spilled into VGPR lanes for them).
    __device__ __forceinline__ unsigned held() const { unsigned c = cnt; asm volatile("" : "+v"(c)); return c; }
    // f(k, key, node&, quad&): quad is scratch that survives between two passes of one round (REG only; recomputed otherwise)
    template <typename F> __device__ __forceinline__ void for_each(F f) {
        if constexpr (REG) {
            const unsigned c = held(), k0 = (unsigned)tid * per;
#pragma unroll
            for (int j = 0; j < OCT_KPT; j++)
                if ((unsigned)j < c) f(k0 + (unsigned)j, key[j], node[j], quad[j]);
        } else {
            for (unsigned k = tid; k < n; k += OCT_NT) {
                unsigned nd = gnode[k], q = 0xFFFFFFFFu;
                const unsigned nd0 = nd;
                f(k, gkeys[k], nd, q);
                if (nd != nd0) gnode[k] = (uint16_t)nd;
            }
        }
    }
};

// Exclusive scans over the quadtree workgroup (OCT_NT threads, a compile-time number of waves).  As msl_common.h's block_excl_scan, but the
// wave totals are folded by one more wave scan and two lane reads instead of sixteen selects per thread: written for any block size, those
// selects kept 32 lane masks (`i < waves`, `i < my wave`) alive in SGPRs for the whole kernel, the larger part of its 249 spilled SGPRs.
// Integer sums: the same values.  s_wave: 32 entries (the pair form keeps its second row from entry 16 on).
constexpr int OCT_NW = OCT_NT / 64;
static_assert(OCT_NW <= 8, "the pair scan folds both rows of wave totals in lanes 0 .. 15");
__device__ __forceinline__ unsigned oct_excl_scan(unsigned v, unsigned *s_wave, unsigned *total) {
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const unsigned inc = wave_incl_scan(v);
    __syncthreads();  // protect s_wave reuse
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    const unsigned ts = wave_incl_scan(lane < OCT_NW ? s_wave[lane] : 0u);
    *total = (unsigned)__builtin_amdgcn_readlane((int)ts, OCT_NW - 1);
    const unsigned before = (unsigned)__builtin_amdgcn_readlane((int)ts, max(w - 1, 0));
    return (w ? before : 0u) + inc - v;
}
__device__ __forceinline__ void oct_excl_scan_pair(unsigned a, unsigned b, unsigned *s_wave, unsigned *totalA, unsigned *totalB, unsigned &exA, unsigned &exB) {
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const unsigned ia = wave_incl_scan(a), ib = wave_incl_scan(b);
    __syncthreads();
    if (lane == 63) { s_wave[w] = ia; s_wave[16 + w] = ib; }
    __syncthreads();
    // lanes 0 .. 7: the first row's totals, lanes 8 .. 15: the second row's; one scan over both
    const unsigned ts = wave_incl_scan(lane < OCT_NW ? s_wave[lane] : lane < 8 + OCT_NW && lane >= 8 ? s_wave[8 + lane] : 0u);
    const unsigned allA = (unsigned)__builtin_amdgcn_readlane((int)ts, 7), endB = (unsigned)__builtin_amdgcn_readlane((int)ts, 15);
    const unsigned beforeA = (unsigned)__builtin_amdgcn_readlane((int)ts, max(w - 1, 0)), uptoB = (unsigned)__builtin_amdgcn_readlane((int)ts, 7 + w);
    *totalA = allA; *totalB = endB - allA;
    exA = (w ? beforeA : 0u) + ia - a; exB = (uptoB - allA) + ib - b;
}

// The fields of its level's LevelDev record that k_octree reads, fetched once (scalar loads: the level is the workgroup's).
struct OctLevel { int h, quota, nIni, nCells, cellBase, keyBase; float hX; };

template <int KPT>
__device__ __forceinline__ void octree_body(const OctArgs &P, const OctLevel &G, OctKeys<KPT> &K, unsigned char *s_dyn, unsigned *s_wave, int *s_misc, int frame,
                                            int level) {
    constexpr bool REG = KPT > 0;
    constexpr int OCT_KPT = KPT > 0 ? KPT : 1;
    const int M = P.maxNode, tid = threadIdx.x, N = G.quota;
    const unsigned n = K.n;
    Rect *const s_rectB = reinterpret_cast<Rect *>(s_dyn);                         // [2][M]
    unsigned *const s_cntB = reinterpret_cast<unsigned *>(s_rectB + 2 * M);        // [2][M]
    unsigned *const s_cc = s_cntB + 2 * M;                                         // [4 M] child key counts
    short *const s_crankB = reinterpret_cast<short *>(s_cc + 4 * M);               // [2][M] creation rank among the nodes recorded for careful mode, -1 = none
    unsigned *const s_FG = reinterpret_cast<unsigned *>(s_crankB + 2 * M);         // [4 M] scans of "child exists" (low half) and "child expandable" (high half)
    unsigned short *const s_L = reinterpret_cast<unsigned short *>(s_FG + 4 * M);  // [M] scan of kept old nodes
    unsigned short *const s_order = s_L + M;                                       // [M] careful mode: sorted candidates
    unsigned short *const s_rankOf = s_order + M;                                  // [M] careful mode: node -> sorted rank (0xFFFF = not a candidate)
    int *nsel = P.nsel + frame * P.nlevels + level;
    uint32_t *sel = P.sel + ((size_t)frame * P.nlevels + level) * P.selCap;

    const unsigned lane = (unsigned)tid & 63u;
    // Histogram update by whole waves: ctr[q] += number of lanes that hold q (q = 0xFFFFFFFF: no item).  The keys arrive in FAST-cell order, so
    // the lanes of a wave sit in the same one or two nodes round after round, and plain LDS atomics would send all 64 lanes to the same counter,
    // which the LDS serialises (measured: 78 of the kernel's 124 us went into the full rounds).  Here the lanes that share a counter are found
    // with a ballot and their leader issues ONE atomic with the count: as many steps as the wave has distinct counters.
    auto hist_add = [&](unsigned *ctr, unsigned q) {
        unsigned long long todo = __ballot(q != 0xFFFFFFFFu);
        while (todo) {
            const unsigned leader = (unsigned)__builtin_ctzll(todo);
            const unsigned qq = (unsigned)__builtin_amdgcn_readlane((int)q, (int)leader);
            const unsigned long long mm = __ballot(q == qq);
            if (lane == leader) atomicAdd(&ctr[qq], (unsigned)__popcll(mm));
            todo &= ~mm;
        }
    };
    // f(k, key, node&, quad&) -> counter index or 0xFFFFFFFF, for every key.  REG: a thread's consecutive keys mostly share a counter, so it counts
    // runs and issues one atomic per run (different lanes sit in different cells: few of them meet in a counter at the same time).
    auto for_each_hist = [&](unsigned *ctr, auto f) {
        if constexpr (REG) {
            unsigned curQ = 0xFFFFFFFFu, curC = 0;
            const unsigned c = K.held();
#pragma unroll
            for (int j = 0; j < OCT_KPT; j++) {
                const unsigned k = (unsigned)tid * K.per + (unsigned)j;
                if ((unsigned)j < c) {
                    const unsigned q = f(k, K.key[j], K.node[j], K.quad[j]);
                    if (q != curQ) {
                        if (curQ != 0xFFFFFFFFu) atomicAdd(&ctr[curQ], curC);
                        curQ = q; curC = 0;
                    }
                    curC++;
                }
            }
            if (curQ != 0xFFFFFFFFu) atomicAdd(&ctr[curQ], curC);
        } else {
            for (unsigned k0 = (unsigned)tid - lane; k0 < n; k0 += OCT_NT) {
                const unsigned k = k0 + lane;
                unsigned q = 0xFFFFFFFFu;
                if (k < n) {
                    unsigned nd = K.gnode[k], qd = 0xFFFFFFFFu;
                    const unsigned nd0 = nd;
                    q = f(k, K.gkeys[k], nd, qd);
                    if (nd != nd0) K.gnode[k] = (uint16_t)nd;
                }
                hist_add(ctr, q);
            }
        }
    };

    int stampNo = 2;
    OCT_STAMP(P, level, frame, 1);
    // ---- root nodes (:536-572) ----
    int cur = 0, S = 0;
    const int H = G.h - 32;
    for (int i = tid; i < M; i += OCT_NT) { s_cntB[i] = 0; s_crankB[i] = -1; }
    for (int j = tid; j < 4 * M; j += OCT_NT) s_cc[j] = 0;
    __syncthreads();
    for_each_hist(s_cntB, [&](unsigned, uint32_t key, unsigned &node, unsigned &) {
        node = (unsigned)(int)((float)(key & 0xFFF) / G.hX);
        return node;
    });
    __syncthreads();
    if (tid == 0) {
        int sN = 0;
        for (int i = 0; i < G.nIni; i++) {
            const unsigned c = s_cntB[i];
            s_L[i] = (unsigned short)sN;
            if (c) {
                Rect r; r.x0 = (short)(int)(G.hX * (float)i); r.x1 = (short)(int)(G.hX * (float)(i + 1)); r.y0 = 0; r.y1 = (short)H;
                s_rectB[M + sN] = r; s_cntB[M + sN] = c; s_crankB[M + sN] = -1;
                sN++;
            }
        }
        s_misc[0] = sN;
    }
    __syncthreads();
    S = s_misc[0];
    K.for_each([&](unsigned, uint32_t, unsigned &node, unsigned &) { node = s_L[node]; });
    cur = 1;
    __syncthreads();

    // Child counts of the nodes that are being divided: s_cc[4 i + quadrant] += 1 for every key of a divided node i (s_cc is zero on entry).
    auto count_children = [&](const Rect *rect, auto is_divided) {
        for_each_hist(s_cc, [&](unsigned, uint32_t key, unsigned &node, unsigned &quad) {
            quad = is_divided(node) ? (unsigned)(4 * node + quadrant(rect[node], key & 0xFFF, (key >> 12) & 0xFFF)) : 0xFFFFFFFFu;
            return quad;
        });
    };

    bool careful = false;
    // ---- full rounds (:580-640).  Five barriers per round: the scans of "child exists" / "child expandable" / "old node kept" run as ONE pair of
    // block scans over register values (each thread owns `per` consecutive child slots), the new node records are written by the thread that scanned
    // them, and the counters of the next round are cleared while the keys move to their new nodes. ----
    while (true) {
        const int prevS = S;
        Rect *rect = (s_rectB + cur * M); unsigned *cnt = (s_cntB + cur * M);
        Rect *nrect = (s_rectB + (cur ^ 1) * M); unsigned *ncnt = (s_cntB + (cur ^ 1) * M); short *ncrank = (s_crankB + (cur ^ 1) * M);
        OCT_STAMP(P, level, frame, stampNo++);
        count_children(rect, [&](unsigned i) { return cnt[i] > 1; });
        __syncthreads();
        OCT_STAMP(P, level, frame, stampNo++);
        const int per = (4 * S + OCT_NT - 1) / OCT_NT, j0 = tid * per;
        unsigned sumFG = 0, sumL = 0;
        for (int p = 0; p < per; p++) {
            const int j = j0 + p;
            if (j < 4 * S) {
                const unsigned ci = cnt[j >> 2], c = ci > 1 ? s_cc[j] : 0;
                sumFG += (c > 0 ? 1u : 0u) | (c > 1 ? 0x10000u : 0u);
                sumL += ((j & 3) == 0 && ci == 1) ? 1u : 0u;
            }
        }
        unsigned totFG, totL, exFG, exL;
        oct_excl_scan_pair(sumFG, sumL, s_wave, &totFG, &totL, exFG, exL);
        OCT_STAMP(P, level, frame, stampNo++);
        const int Ctot = (int)(totFG & 0xFFFFu), nToExpand = (int)(totFG >> 16), Ltot = (int)totL;
        const int S2 = Ctot + Ltot;
        if (S2 > M) { if (tid == 0) { atomicExch(P.err, 1); *nsel = 0; } return; }
        for (int p = 0; p < per; p++) {
            const int j = j0 + p;
            if (j < 4 * S) {
                const int i = j >> 2;
                const unsigned ci = cnt[i], c = ci > 1 ? s_cc[j] : 0;
                exFG += (c > 0 ? 1u : 0u) | (c > 1 ? 0x10000u : 0u);      // inclusive from here
                s_FG[j] = exFG;
                if (c) {
                    const int pos = Ctot - (int)(exFG & 0xFFFFu);
                    nrect[pos] = child_rect(rect[i], j & 3);
                    ncnt[pos] = c;
                    ncrank[pos] = c > 1 ? (short)((exFG >> 16) - 1) : (short)-1;
                }
                if ((j & 3) == 0) {
                    exL += ci == 1 ? 1u : 0u;
                    s_L[i] = (unsigned short)exL;
                    if (ci == 1) { const int pos = Ctot + (int)exL - 1; nrect[pos] = rect[i]; ncnt[pos] = 1; ncrank[pos] = -1; }
                }
            }
        }
        __syncthreads();
        OCT_STAMP(P, level, frame, stampNo++);
        K.for_each([&](unsigned, uint32_t key, unsigned &node, unsigned &quad) {
            const unsigned i = node;
            if (cnt[i] > 1) {
                const unsigned j = REG ? quad : (unsigned)(4 * i + quadrant(rect[i], key & 0xFFF, (key >> 12) & 0xFFF));
                node = (unsigned)(Ctot - (int)(s_FG[j] & 0xFFFFu));
            } else {
                node = (unsigned)(Ctot + s_L[i] - 1);
            }
        });
        for (int j = tid; j < 4 * S2; j += OCT_NT) s_cc[j] = 0;
        __syncthreads();
        OCT_STAMP(P, level, frame, stampNo++);
        cur ^= 1; S = S2;
        if (S >= N || S == prevS) break;
        if (S + 3 * nToExpand > N) { careful = true; break; }
    }

    // ---- careful mode (:641-700) ----
    stampNo = 40;
    while (careful) {
        OCT_STAMP(P, level, frame, stampNo++);
        const int prevS = S;
        Rect *rect = (s_rectB + cur * M); unsigned *cnt = (s_cntB + cur * M); short *crank = (s_crankB + cur * M);
        Rect *nrect = (s_rectB + (cur ^ 1) * M); unsigned *ncnt = (s_cntB + (cur ^ 1) * M); short *ncrank = (s_crankB + (cur ^ 1) * M);
        count_children(rect, [&](unsigned i) { return crank[i] >= 0; });
        OCT_STAMP(P, level, frame, stampNo++);
        // rank of a candidate = number of candidates that sort before it: larger (size, creation rank) first.  The sort keys go to LDS first
        // (0 = not a candidate; s_FG is free until the scan below) so that the comparison loop is branch-free and its loads pipeline: as a loop
        // over cnt[] / crank[] with a short-circuit test it took 6.5 of the careful round's 12 us.
        unsigned long long *const pk = reinterpret_cast<unsigned long long *>(s_FG);
        for (int i = tid; i < S; i += OCT_NT) pk[i] = crank[i] >= 0 ? ((((unsigned long long)cnt[i] << 16) | (unsigned)crank[i]) + 1ull) : 0ull;
        __syncthreads();
        unsigned nMine = 0;
        for (int i = tid; i < S; i += OCT_NT) {
            const unsigned long long me = pk[i];
            if (me == 0) { s_rankOf[i] = 0xFFFF; continue; }
            int r = 0;
#pragma unroll 8
            for (int i2 = 0; i2 < S; i2++) r += pk[i2] > me ? 1 : 0;
            s_order[r] = (unsigned short)i;
            s_rankOf[i] = (unsigned short)r;
            nMine++;
        }
        if (tid == 0) s_misc[2] = 0x7FFFFFFF;
        unsigned mTot, exUnused;
        exUnused = oct_excl_scan(nMine, s_wave, &mTot);   // (its barriers also complete s_cc, s_order, s_rankOf)
        (void)exUnused;
        const int m = (int)mTot;
        OCT_STAMP(P, level, frame, stampNo++);
        if (m == 0) break;  // nothing to expand: size unchanged -> finish
        // growth prefix in sorted order -> number of expansions J: the first r + 1 with S + (children of the first r + 1 expansions) - (r + 1) >= N
        const int perR = (m + OCT_NT - 1) / OCT_NT, r0 = tid * perR;
        unsigned sumG = 0;
        for (int p = 0; p < perR; p++) {
            const int r = r0 + p;
            if (r < m) { const int i = s_order[r]; sumG += (s_cc[4 * i] > 0) + (s_cc[4 * i + 1] > 0) + (s_cc[4 * i + 2] > 0) + (s_cc[4 * i + 3] > 0); }
        }
        unsigned totG, exG;
        exG = oct_excl_scan(sumG, s_wave, &totG);
        for (int p = 0; p < perR; p++) {
            const int r = r0 + p;
            if (r < m) {
                const int i = s_order[r];
                exG += (s_cc[4 * i] > 0) + (s_cc[4 * i + 1] > 0) + (s_cc[4 * i + 2] > 0) + (s_cc[4 * i + 3] > 0);
                if (S + (int)exG - (r + 1) >= N) atomicMin(&s_misc[2], r + 1);
            }
        }
        __syncthreads();
        const int J = min(s_misc[2], m);
        OCT_STAMP(P, level, frame, stampNo++);
        // children of the J expanded nodes, flat index jj = 4 r + q in sorted order; kept nodes in their old order
        const int perC = (4 * J + OCT_NT - 1) / OCT_NT, jj0 = tid * perC, perS = (S + OCT_NT - 1) / OCT_NT, i0 = tid * perS;
        unsigned sumFG = 0, sumL = 0;
        for (int p = 0; p < perC; p++) {
            const int jj = jj0 + p;
            if (jj < 4 * J) { const unsigned c = s_cc[4 * s_order[jj >> 2] + (jj & 3)]; sumFG += (c > 0 ? 1u : 0u) | (c > 1 ? 0x10000u : 0u); }
        }
        for (int p = 0; p < perS; p++) { const int i = i0 + p; if (i < S) sumL += !(s_rankOf[i] < J) ? 1u : 0u; }
        unsigned totFG, totL, exFG, exL;
        oct_excl_scan_pair(sumFG, sumL, s_wave, &totFG, &totL, exFG, exL);
        OCT_STAMP(P, level, frame, stampNo++);
        const int Ctot = (int)(totFG & 0xFFFFu);
        const int S2 = Ctot + (S - J);
        if (S2 > M) { if (tid == 0) { atomicExch(P.err, 1); *nsel = 0; } return; }
        for (int p = 0; p < perC; p++) {
            const int jj = jj0 + p;
            if (jj < 4 * J) {
                const int i = s_order[jj >> 2];
                const unsigned c = s_cc[4 * i + (jj & 3)];
                exFG += (c > 0 ? 1u : 0u) | (c > 1 ? 0x10000u : 0u);
                s_FG[jj] = exFG;
                if (c) {
                    const int pos = Ctot - (int)(exFG & 0xFFFFu);
                    nrect[pos] = child_rect(rect[i], jj & 3);
                    ncnt[pos] = c;
                    ncrank[pos] = c > 1 ? (short)((exFG >> 16) - 1) : (short)-1;
                }
            }
        }
        for (int p = 0; p < perS; p++) {
            const int i = i0 + p;
            if (i < S) {
                const bool keep = !(s_rankOf[i] < J);
                exL += keep ? 1u : 0u;
                s_L[i] = (unsigned short)exL;
                if (keep) { const int pos = Ctot + (int)exL - 1; nrect[pos] = rect[i]; ncnt[pos] = cnt[i]; ncrank[pos] = -1; }
            }
        }
        __syncthreads();
        K.for_each([&](unsigned, uint32_t key, unsigned &node, unsigned &quad) {
            const unsigned i = node;
            const int r = s_rankOf[i];
            if (r < J) {
                const unsigned q = REG ? (quad & 3u) : (unsigned)quadrant(rect[i], key & 0xFFF, (key >> 12) & 0xFFF);
                node = (unsigned)(Ctot - (int)(s_FG[4 * r + q] & 0xFFFFu));
            } else {
                node = (unsigned)(Ctot + s_L[i] - 1);
            }
        });
        __syncthreads();   // every key has read s_rankOf / s_FG / s_L / the old s_cc: they may be overwritten
        OCT_STAMP(P, level, frame, stampNo++);
        for (int j = tid; j < 4 * max(S, S2); j += OCT_NT) s_cc[j] = 0;
        cur ^= 1; S = S2;
        if (S >= N || S == prevS) break;
        __syncthreads();
    }

    __syncthreads();
    OCT_STAMP(P, level, frame, 80);
    // ---- keep the best key of every node (:703-718) ----
    unsigned *best = s_cc;
    for (int i = tid; i < S; i += OCT_NT) best[i] = 0;
    __syncthreads();
    K.for_each([&](unsigned k, uint32_t key, unsigned &node, unsigned &) { atomicMax(&best[node], (key & 0xFF000000u) | (0xFFFFFFu - k)); });   // (final lists are long: few lanes share a node)
    __syncthreads();
    if (S > P.selCap) { if (tid == 0) { atomicExch(P.err, 2); *nsel = 0; } return; }
    // the winner's key: (score, index) identifies it; its thread hands it over (REG) or it is read back (global)
    if constexpr (REG) {
        K.for_each([&](unsigned k, uint32_t key, unsigned &node, unsigned &) {
            if ((best[node] & 0xFFFFFFu) == 0xFFFFFFu - k) sel[node] = key;
        });
    } else {
        for (int i = tid; i < S; i += OCT_NT) sel[i] = K.gkeys[0xFFFFFFu - (best[i] & 0xFFFFFFu)];
    }
    if (tid == 0) *nsel = S;
    OCT_STAMP(P, level, frame, 81);
}

// MAXKPT: the largest register-resident form this instantiation carries.  The 32-keys-per-thread form needs 239 VGPRs (a 512-thread workgroup then
// fills its CU's register files), so launches for ordinary frame sizes use k_octree<16> (133 VGPRs) and only large frames k_octree<32>.
template <int MAXKPT>
__global__ __launch_bounds__(OCT_NT) void k_octree(OctArgs P) {
    // Node arrays sized for THIS extractor's longest possible list (P.maxNode = max over levels of max(quota, 4 nIni) + 2, rounded up to 64, plus
    // one block of slack; 66 bytes per node: 21 KB for 1000 features instead of a fixed 66 KB for MAXNODE = 1024), so that the frame-batched kernels
    // of the other streams keep their LDS -- and with it their occupancy -- while this latency-bound kernel runs.  The same memory first holds
    // the exclusive scan of the level's per-cell candidate counts (P.octLds covers both uses).
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    __shared__ unsigned s_wave[33];   // (block_excl_scan_pair keeps two rows of 16 wave totals)
    __shared__ int s_misc[8];
    const int tid = threadIdx.x;
    int level, frame;
    if (!xcd_item(P.nlevels, P.nFrames, level, frame)) return;
    OCT_STAMP(P, level, frame, 0);
    OctLevel G;
    {
        const LevelDev &T = P.lv[level];
        G.h = T.h; G.quota = T.quota; G.nIni = T.nIni; G.nCells = T.nCells; G.cellBase = T.cellBase; G.keyBase = T.keyBase; G.hX = T.hX;
    }
    uint32_t *keys = P.keys + (size_t)frame * P.keysPerFrame + G.keyBase;
    uint16_t *knode = P.knode + (size_t)frame * P.keysPerFrame + G.keyBase;

    // ---- the cell lists in cell order (vToDistributeKeys, :757-779): key slot k belongs to the cell c with off[c] <= k < off[c + 1] ----
    const uint32_t *cellCnt = P.cellCnt + (size_t)frame * P.cellsPerFrame + G.cellBase;
    const uint32_t *cellKeys = P.cellKeys + (size_t)frame * P.keysPerFrame;
    unsigned *const s_off = reinterpret_cast<unsigned *>(s_dyn);     // [nCells + 1] exclusive scan of the cells' candidate counts
    unsigned *const s_koff = s_off + (G.nCells + 1);                 // [nCells] where each cell's list starts in cellKeys (a geometry constant)
    unsigned n = 0;
    {
        unsigned carry = 0;
        for (int c0 = 0; c0 < G.nCells; c0 += OCT_NT) {
            const int c = c0 + tid;
            const unsigned cnt = c < G.nCells ? cellCnt[c] : 0;
            const unsigned ko = c < G.nCells ? P.cells[G.cellBase + c].keyOff : 0;   // (in flight together with the count)
            unsigned tot;
            const unsigned off = carry + oct_excl_scan(cnt, s_wave, &tot);
            if (c < G.nCells) { s_off[c] = off; s_koff[c] = ko; }
            carry += tot;
        }
        n = carry;
        if (tid == 0) s_off[G.nCells] = n;
    }
    if (tid == 0) P.ncand[frame * P.nlevels + level] = (int)n;
    __syncthreads();
    if (n == 0) { if (tid == 0) P.nsel[frame * P.nlevels + level] = 0; return; }
    auto cell_of = [&](unsigned k) -> int {   // largest c with off[c] <= k (empty cells share their successor's offset: the search skips them)
        int lo = 0, hi = G.nCells;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] <= k) lo = mid; else hi = mid; }
        return lo;
    };
    auto run_in_registers = [&](auto kptTag) {
        constexpr int OCT_KPT = decltype(kptTag)::value;
        OctKeys<OCT_KPT> K;
        K.n = n; K.tid = tid; K.gkeys = keys; K.gnode = knode; K.per = (n + OCT_NT - 1) / OCT_NT;
        K.cnt = (unsigned)tid * K.per < n ? min(K.per, n - (unsigned)tid * K.per) : 0u;
        int c = 0;
#pragma unroll
        for (int j = 0; j < OCT_KPT; j++) {
            const unsigned k = (unsigned)tid * K.per + (unsigned)j;
            K.key[j] = 0; K.node[j] = 0; K.quad[j] = 0xFFFFFFFFu;
            if ((unsigned)j < K.per && k < n) {
                // one search for the thread's first key, then a walk: its keys are consecutive, so they sit in one or two cells, and their loads
                // leave together instead of each waiting for its own search and cell record
                if (j == 0) c = cell_of(k);
                else while (k >= s_off[c + 1]) c++;
                K.key[j] = cellKeys[s_koff[c] + (k - s_off[c])];
            }
        }
#pragma unroll
        for (int j = 0; j < OCT_KPT; j++) {
            const unsigned k = (unsigned)tid * K.per + (unsigned)j;
            if ((unsigned)j < K.per && k < n) keys[k] = K.key[j];     // (the global copy is what msl_orb_debug_candidates reads)
        }
        __syncthreads();   // s_off is dead from here on: the node arrays take its place
        octree_body<OCT_KPT>(P, G, K, s_dyn, s_wave, s_misc, frame, level);
    };
    if (n <= 16u * OCT_NT) {
        run_in_registers(std::integral_constant<int, 16>{});
    } else if (MAXKPT >= 32 && n <= 32u * OCT_NT) {   // level 0 of a 1280 x 960 frame: ~14 k candidates
        if constexpr (MAXKPT >= 32) run_in_registers(std::integral_constant<int, 32>{});
    } else {
        OctKeys<0> K;
        K.n = n; K.tid = tid; K.gkeys = keys; K.gnode = knode; K.per = 0; K.cnt = 0;
        for (unsigned k = tid; k < n; k += OCT_NT) { const int c = cell_of(k); keys[k] = cellKeys[s_koff[c] + (k - s_off[c])]; knode[k] = 0; }
        __syncthreads();
        octree_body<0>(P, G, K, s_dyn, s_wave, s_misc, frame, level);
    }
}

// ---------------------------------------------------------------------------------------------
// k_blur: GaussianBlur 7x7 sigma 2 (integer kernel {18,34,49,55,49,34,18} by default, >>16 with rounding),
// reflect-101 on the level's own borders.  Tile 64 x 32 outputs per workgroup.
// ---------------------------------------------------------------------------------------------
// Which OpenCV generation's 8-bit Gaussian kernel is pinned: 0 = per-coefficient rounding {18,34,49,55,..}
// (OpenCV 3.x, sum 257), 1 = error-diffused "bit-exact" kernel {18,34,48,56,..} (later releases, sum 256).  Row sums stay <= 65535.
#ifndef MSL_BLUR_VARIANT
#define MSL_BLUR_VARIANT 0
#endif
#if MSL_BLUR_VARIANT == 1
constexpr int GK0 = 18, GK1 = 34, GK2 = 48, GK3 = 56;
#else
constexpr int GK0 = 18, GK1 = 34, GK2 = 49, GK3 = 55;
#endif

__device__ __forceinline__ int reflect101(int p, int len) {
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

__global__ __launch_bounds__(256) void k_blur(OrbDev P) {
    // 64 x 32 output tile, four horizontally adjacent pixels per thread in both passes: dword traffic to LDS and memory
    // instead of bytes.  Arithmetic as before: u16 row sums (<= 65535), 32-bit column sums, (acc + 32768) >> 16.
    constexpr int IP = BT_W + 8;                                   // staged bytes per row: x = tx0 - 4 .. tx0 + 67
    __shared__ __attribute__((aligned(16))) uint8_t s_in[(BT_H + 6) * IP];
    __shared__ __attribute__((aligned(16))) unsigned short s_row[(BT_H + 6) * BT_W];
    const int tid = threadIdx.x;
    int tileI, frame;
    if (!xcd_item(P.blurTiles, P.nFrames, tileI, frame)) return;
    int l = 0;
    while (l + 1 < P.nlevels && tileI >= P.lv[l + 1].tileBase) l++;
    const LevelDev &D = P.lv[l];
    const int t = tileI - D.tileBase;
    const int tx0 = (t % D.tilesX) * BT_W, ty0 = (t / D.tilesX) * BT_H;
    int pitch;
    const uint8_t *img = level_ptr(P, frame, l, pitch);
    if (tx0 >= 4 && tx0 + BT_W + 4 <= D.w && ty0 >= 3 && ty0 + BT_H + 3 <= D.h) {
        // interior tile: 18 dwords per row, no reflection
        for (int i = tid; i < (BT_H + 6) * (IP / 4); i += 256) {
            const int r = i / (IP / 4), q = i - r * (IP / 4);
            unsigned v;
            __builtin_memcpy(&v, img + (size_t)(ty0 - 3 + r) * pitch + (tx0 - 4 + 4 * q), 4);
            reinterpret_cast<unsigned *>(s_in)[r * (IP / 4) + q] = v;
        }
    } else {
        for (int i = tid; i < (BT_H + 6) * IP; i += 256) {
            const int r = i / IP, c = i - r * IP;
            const int y = reflect101(ty0 + r - 3, D.h), x = reflect101(tx0 + c - 4, D.w);
            s_in[i] = img[(size_t)y * pitch + x];
        }
    }
    __syncthreads();
    // Row pass with v_dot4_u32_u8 (round 6): the seven taps of an output are two dot products of four staged bytes each -- the 8-byte window that starts
    // one byte behind the output's first staged byte, cut out of the thread's three dwords with v_alignbyte -- instead of twelve byte extractions and ten
    // multiply / adds per output.  A thread computes the same four columns of TWO consecutive staged rows and stores them as one dword per column,
    // {row 2 p, row 2 p + 1}: the column pass then takes two taps per v_dot2_u32_u16.  Integer arithmetic throughout: the same sums as before.
    constexpr unsigned TAPS_LO = (unsigned)GK0 | ((unsigned)GK1 << 8) | ((unsigned)GK2 << 16) | ((unsigned)GK3 << 24);   // staged bytes k + 1 .. k + 4
    constexpr unsigned TAPS_HI = (unsigned)GK2 | ((unsigned)GK1 << 8) | ((unsigned)GK0 << 16);                           // staged bytes k + 5 .. k + 7
    auto row4 = [&](int r, int j, unsigned (&o)[4]) {
        const unsigned *p = reinterpret_cast<const unsigned *>(s_in) + r * (IP / 4) + j;
        const unsigned w0 = p[0], w1 = p[1], w2 = p[2];
        o[0] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 1), TAPS_HI, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 1), TAPS_LO, 0u, false), false);
        o[1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 2), TAPS_HI, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 2), TAPS_LO, 0u, false), false);
        o[2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 3), TAPS_HI, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 3), TAPS_LO, 0u, false), false);
        o[3] = __builtin_amdgcn_udot4(w2, TAPS_HI, __builtin_amdgcn_udot4(w1, TAPS_LO, 0u, false), false);   // output column 4 j + k reads staged bytes 4 j + k + 1 .. + 7
    };
    static_assert((BT_H + 6) % 2 == 0, "whole row pairs");
    unsigned *const s_pair = reinterpret_cast<unsigned *>(s_row);   // [(BT_H + 6) / 2][BT_W]: low half = row 2 p, high half = row 2 p + 1 (row sums <= 65535)
    for (int i = tid; i < ((BT_H + 6) / 2) * (BT_W / 4); i += 256) {
        const int rp = i / (BT_W / 4), j = i - rp * (BT_W / 4);
        unsigned oa[4], ob[4];
        row4(2 * rp, j, oa); row4(2 * rp + 1, j, ob);
        uint4 pk; pk.x = oa[0] | (ob[0] << 16); pk.y = oa[1] | (ob[1] << 16); pk.z = oa[2] | (ob[2] << 16); pk.w = oa[3] | (ob[3] << 16);
        *reinterpret_cast<uint4 *>(&s_pair[rp * BT_W + 4 * j]) = pk;
    }
    __syncthreads();
    uint8_t *out = P.blur + (size_t)frame * P.blurStride + D.boff;
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    for (int i = tid; i < BT_H * (BT_W / 4); i += 256) {
        const int r = i / (BT_W / 4), j = i - r * (BT_W / 4);
        const int x = tx0 + 4 * j, y = ty0 + r;
        if (x >= D.w || y >= D.h) continue;
        // output row r = staged rows r .. r + 6 with the taps K0 K1 K2 K3 K2 K1 K0: four row pairs from pair r / 2 on; an even r starts on a pair
        // (taps K0 K1 | K2 K3 | K2 K1 | K0 0), an odd r in the middle of one (0 K0 | K1 K2 | K3 K2 | K1 K0)
        const bool odd = r & 1;
        const unsigned t0 = odd ? ((unsigned)GK0 << 16) : ((unsigned)GK0 | ((unsigned)GK1 << 16));
        const unsigned t1 = odd ? ((unsigned)GK1 | ((unsigned)GK2 << 16)) : ((unsigned)GK2 | ((unsigned)GK3 << 16));
        const unsigned t2 = odd ? ((unsigned)GK3 | ((unsigned)GK2 << 16)) : ((unsigned)GK2 | ((unsigned)GK1 << 16));
        const unsigned t3 = odd ? ((unsigned)GK1 | ((unsigned)GK0 << 16)) : (unsigned)GK0;
        const uint4 *q = reinterpret_cast<const uint4 *>(&s_pair[(r >> 1) * BT_W + 4 * j]);
        const uint4 q0 = q[0], q1 = q[BT_W / 4], q2 = q[2 * (BT_W / 4)], q3 = q[3 * (BT_W / 4)];
        auto col = [&](unsigned a0, unsigned a1, unsigned a2, unsigned a3) -> unsigned {
            unsigned acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a0), __builtin_bit_cast(u16x2, t0), 32768u, false);   // (acc + 32768) >> 16
            acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a1), __builtin_bit_cast(u16x2, t1), acc, false);
            acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a2), __builtin_bit_cast(u16x2, t2), acc, false);
            acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a3), __builtin_bit_cast(u16x2, t3), acc, false);
            return min(acc >> 16, 255u);
        };
        const unsigned res = col(q0.x, q1.x, q2.x, q3.x) | (col(q0.y, q1.y, q2.y, q3.y) << 8) | (col(q0.z, q1.z, q2.z, q3.z) << 16) | (col(q0.w, q1.w, q2.w, q3.w) << 24);
        uint8_t *dst = out + (size_t)y * D.pitch + x;
        if (x + 3 < D.w) __builtin_memcpy(dst, &res, 4);
        else
            for (int k = 0; k < 4 && x + k < D.w; k++) dst[k] = (uint8_t)(res >> (8 * k));
    }
}

// ---------------------------------------------------------------------------------------------
// k_describe: one wave per selected keypoint: IC_Angle, pinned sincos, steered BRIEF, output.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    const float p1 = 0.9997878412794807f * (float)(180 / M_PI);
    const float p3 = -0.3258083974640975f * (float)(180 / M_PI);
    const float p5 = 0.1555786518463281f * (float)(180 / M_PI);
    const float p7 = -0.04432655554792128f * (float)(180 / M_PI);
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// Pinned replacement for cosf/sinf at src/ORBextractor.cc:108 (DESIGN.md "pinned sincos").
__device__ __forceinline__ void sincos_pinned(float angle, float *s_out, float *c_out) {
    const double x = (double)angle;
    const double kd = floor(x * 6.36619772367581382433e-01 + 0.5);
    const int k = (int)kd;
    const double r = (x - kd * 1.57079632673412561417e+00) - kd * 6.07710050650619224932e-11;
    const double z = r * r;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double v = z * r;
    const double sr = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double sn = r + v * (S1 + z * sr);
    const double cr = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double cs = 1.0 - (0.5 * z - z * cr);
    double s, c;
    switch (k & 3) {
        case 0: s = sn; c = cs; break;
        case 1: s = cs; c = -sn; break;
        case 2: s = -sn; c = -cs; break;
        default: s = -cs; c = sn; break;
    }
    *s_out = (float)s;
    *c_out = (float)c;
}

// cv::undistortPoints(K, dist, P = K) for one point, OpenCV 3.x cvUndistortPoints plain C path (double arithmetic, 5
// fixed-point iterations); src/Frame.cc:437-463.  The zero terms of the 12-coefficient model are kept so that the
// operation order is the library's.
__device__ __forceinline__ void undistort_point(const msl_frame_params &p, float xin, float yin, float *xo, float *yo) {
    const double fx = p.fx, fy = p.fy, cx = p.cx, cy = p.cy, ifx = 1. / fx, ify = 1. / fy;
    const double k0 = p.k1, k1 = p.k2, k2 = p.p1, k3 = p.p2, k4 = p.k3, kz = 0.0;
    double x = xin, y = yin;
    x = (x - cx) * ifx;
    y = (y - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((kz * r2 + kz) * r2 + kz) * r2) / (1 + ((k4 * r2 + k1) * r2 + k0) * r2);
        const double deltaX = 2 * k2 * x * y + k3 * (r2 + 2 * x * x) + kz * r2 + kz * r2 * r2;
        const double deltaY = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y + kz * r2 + kz * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = fx * x + 0.0 * y + cx, yy = 0.0 * x + fy * y + cy, ww = 1. / (0.0 * x + 0.0 * y + 1.0);
    *xo = (float)(xx * ww);
    *yo = (float)(yy * ww);
}

__global__ __launch_bounds__(256) void k_describe(OrbDev P) {
    // The grid is indexed by OUTPUT keypoint: wave o of a frame (four per workgroup, ceil(outCap / 4) workgroups) finds its level and its index
    // in the level's selection from the running sums of the frame's nsel[] (scalar loads: <= 12 values), so the waves that exist are the
    // keypoints that exist, rounded up to a workgroup -- not selCap slots on every level.  The output order is the levels' order, as before.
    int blockX, frame;
    if (!xcd_item((P.outCap + 3) / 4, P.nFrames, blockX, frame)) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int outIdx = blockX * 4 + wv;
    const int *nsel = P.nsel + frame * P.nlevels;
    int tot = 0, level = 0, idx = outIdx;
    for (int l = 0; l < P.nlevels; l++) {
        const int c = nsel[l];
        if (outIdx >= tot + c) { level = l + 1; idx = outIdx - (tot + c); }
        tot += c;
    }
    if (blockX == 0 && threadIdx.x == 0) {
        P.nout[frame] = min(tot, P.outCap);
        if (tot > P.outCap) atomicExch(P.err, 3);
    }
    if (outIdx >= min(tot, P.outCap)) return;
    const LevelDev &D = P.lv[level];
    const unsigned key = P.sel[((size_t)frame * P.nlevels + level) * P.selCap + idx];
    const int x = (int)(key & 0xFFF) + 16, y = (int)((key >> 12) & 0xFFF) + 16;  // :793-794
    const int score = key >> 24;
    int pitch;
    const uint8_t *img = level_ptr(P, frame, level, pitch);
    // Fetch the keypoint's neighbourhoods with row-wise dword loads (10 per lane) instead of ~20 scattered byte gathers per lane: the
    // 31 x 31 patch of the level (IC_Angle, |u|, |v| <= 15; columns x-16 .. x+15 are read), which is summed where it lands, in registers, and
    // the 37 x 37 patch of the blurred level (rotated BRIEF samples, |offset| <= 18; columns x-20 .. x+19), which goes to LDS.  A keypoint
    // lies at least 19 px inside the level (FAST cells start 16 + 3 px in), so every byte exists.
    constexpr int PW = 4 * IC_ROW_WORDS, PH = IC_ROWS, BW = 40, BH = 37;
    __shared__ __attribute__((aligned(16))) uint8_t s_blurp[4][BH * BW];
    const uint8_t *bl = P.blur + (size_t)frame * P.blurStride + D.boff + (size_t)y * D.pitch + x;
    int m10 = 0, m01 = 0;
    {
        unsigned pv[4], bv[6];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = lane + 64 * k;   // dword i of the patch: row i / 8, dword i % 8
            pv[k] = 0;
            if (i < PH * (PW / 4)) __builtin_memcpy(&pv[k], img + (size_t)(y - 15 + i / (PW / 4)) * pitch + (x - 16 + 4 * (i % (PW / 4))), 4);
        }
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const int i = lane + 64 * k;
            bv[k] = 0;
            if (i < BH * (BW / 4)) __builtin_memcpy(&bv[k], bl + (i / (BW / 4) - 18) * D.pitch + (4 * (i % (BW / 4)) - 20), 4);
        }
#pragma unroll
        for (int k = 0; k < 6; k++) { const int i = lane + 64 * k; if (i < BH * (BW / 4)) reinterpret_cast<unsigned *>(s_blurp[wv])[i] = bv[k]; }
        // IC_Angle (:75-99): m10 = sum u*I, m01 = sum v*I over the circular patch, from the patch words in registers (msl_orb_sums.h): two
        // v_dot4_u32_u8 per word against weight words built from umax[], instead of one byte per lane and trip through LDS.  The missing words
        // (i >= 248) are 0.
        const uint64_t umaxNib = ic_pack_umax(P.umax);
        uint32_t sI = 0, sCI = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) ic_add_word(pv[k], min(lane + 64 * k, IC_WORDS - 1), umaxNib, sI, sCI, m01);
        m10 = ic_m10(sI, sCI);
        // wave totals in the VALU (DPP row scan + row broadcasts, msl_common.h) instead of six rounds of ds_bpermute per sum; integer sums: any order
        m10 = __builtin_amdgcn_readlane((int)wave_incl_scan((unsigned)m10), 63);
        m01 = __builtin_amdgcn_readlane((int)wave_incl_scan((unsigned)m01), 63);
    }
    __builtin_amdgcn_wave_barrier();
    const float angle = fast_atan2_deg((float)m01, (float)m10);
    const float factorPI = (float)(M_PI / 180.f);
    float a, b;
    sincos_pinned(angle * factorPI, &b, &a);
    // steered BRIEF (:104-149): lane handles test pairs 4*lane .. 4*lane+3
    unsigned nib = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int8_t *pp = &c_pattern[(4 * lane + j) * 4];
        const float x0 = (float)pp[0], y0 = (float)pp[1], x1 = (float)pp[2], y1 = (float)pp[3];
        const int r0 = __float2int_rn(x0 * b + y0 * a), c0 = __float2int_rn(x0 * a - y0 * b);
        const int r1 = __float2int_rn(x1 * b + y1 * a), c1 = __float2int_rn(x1 * a - y1 * b);
        const int t0 = s_blurp[wv][(r0 + 18) * BW + c0 + 20], t1 = s_blurp[wv][(r1 + 18) * BW + c1 + 20];
        nib |= (t0 < t1 ? 1u : 0u) << j;
    }
    // lane 8 q collects the nibbles of lanes 8 q .. 8 q + 7 (inside one DPP row): row_shl:n hands lane i the value of lane i + n
    unsigned w = nib | ((unsigned)__builtin_amdgcn_update_dpp(0, (int)nib, 0x101, 0xF, 0xF, true) << 4);
    w |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0x102, 0xF, 0xF, true) << 8;
    w |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0x104, 0xF, 0xF, true) << 16;
    msl_keypoint *kp = P.kps + (size_t)frame * P.outCap + outIdx;
    uint32_t *dsc = (uint32_t *)(P.desc + ((size_t)frame * P.outCap + outIdx) * 32);
    if ((lane & 7) == 0) dsc[lane >> 3] = w;
    if (lane == 0) {
        float fx = (float)x, fy = (float)y;
        if (level != 0) { fx *= D.scale; fy *= D.scale; }  // :861-866
        kp->x = fx; kp->y = fy; kp->size = (float)D.patch; kp->angle = angle;
        kp->response = (float)score; kp->octave = level; kp->class_id = -1;
        if (P.frameOn) {
            // UndistortKeyPoints (src/Frame.cc:437-463), ComputeStereoFromRGBD (:495-513), PosInGrid (:418-427)
            const size_t o = (size_t)frame * P.outCap + outIdx;
            float ux = fx, uy = fy;
            if (P.fp.k1 != 0.0) undistort_point(P.fp, fx, fy, &ux, &uy);
            P.unXY[2 * o] = ux; P.unXY[2 * o + 1] = uy;
            const float d = *(const float *)((const uint8_t *)P.depth + (size_t)frame * P.depthFrameStride + (size_t)(int)fy * P.depthRowStride +
                                             sizeof(float) * (size_t)(int)fx);
            P.depthOut[o] = d > 0 ? d : -1.0f;
            P.uRight[o] = d > 0 ? ux - P.fp.bf / d : -1.0f;
            const int posX = (int)roundf((ux - P.fp.minX) * P.gridWInv), posY = (int)roundf((uy - P.fp.minY) * P.gridHInv);
            P.gridCell[o] = (posX < 0 || posX >= MSL_FRAME_GRID_COLS || posY < 0 || posY >= MSL_FRAME_GRID_ROWS) ? -1 : posX * MSL_FRAME_GRID_ROWS + posY;
        }
    }
}

const char *kKernelNames[MSL_ORB_NKERNELS] = {"k_pyramid", "k_fast", "k_octree", "k_blur", "k_describe", "copy"};

}  // namespace

// =============================================================================================
// Device driver
// =============================================================================================
namespace msl {
namespace orb {

const char *kernel_name(int kid) { return kKernelNames[kid]; }

int allow_octree_lds(int octLds) {
    if (octLds <= 32 * 1024) return MSL_OK;
    MSL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_octree<16>), hipFuncAttributeMaxDynamicSharedMemorySize, octLds));
    MSL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_octree<32>), hipFuncAttributeMaxDynamicSharedMemorySize, octLds));
    return MSL_OK;
}

}  // namespace orb
}  // namespace msl

int orb_launch_pipeline(const OrbDev *dev, OrbLaunch *launch, const uint8_t *d_gray, size_t rowStride, size_t frameStride, int n,
                        msl_keypoint *d_kps, uint8_t *d_desc, int *d_nout, const FrameEpilogue *ep) {
    OrbLaunch &q = *launch;
    OrbDev P = *dev;
    P.in = d_gray; P.inRowStride = rowStride; P.inFrameStride = frameStride;
    P.kps = d_kps; P.desc = d_desc; P.nout = d_nout;
    P.frameOn = ep ? 1 : 0;
    P.nFrames = n;
    if (ep) {
        P.fp = ep->fp;
        P.gridWInv = (float)MSL_FRAME_GRID_COLS / (float)(ep->fp.maxX - ep->fp.minX);   // src/Frame.cc:137-138
        P.gridHInv = (float)MSL_FRAME_GRID_ROWS / (float)(ep->fp.maxY - ep->fp.minY);
        P.depth = ep->depth; P.depthRowStride = ep->depthRowStride; P.depthFrameStride = ep->depthFrameStride;
        P.unXY = ep->unXY; P.depthOut = ep->depthOut; P.uRight = ep->uRight; P.gridCell = ep->gridCell;
    }
    hipStream_t s = q.stream;
    const int L = P.nlevels;
    static const bool perLevel = getenv("MSL_ORB_PYRAMID") && !strcmp(getenv("MSL_ORB_PYRAMID"), "levels");
    if (P.pyrTX && !perLevel) {
        q.prof.begin(KID_RESIZE, s);
        hipLaunchKernelGGL(k_pyramid, dim3(xcd_grid1((long long)P.pyrTX * P.pyrTY * n)), dim3(256), q.pyrLds, s, P);
        q.prof.end(s);
    } else {
        for (int l = 1; l < L; l++) {
            const LevelDev &G = P.lv[l];
            q.prof.begin(KID_RESIZE, s);
            hipLaunchKernelGGL(k_resize, dim3((G.w + 63) / 64, (G.h + 3) / 4, n), dim3(256), 0, s, P, l);
            q.prof.end(s);
        }
    }
    // One frame cannot fill the GPU and every kernel is a dependent launch: the blur (needs the pyramid only) then runs on a side stream beside
    // FAST + quadtree instead of behind them.  Batched calls keep one stream: their kernels fill the GPU and the order keeps each frame's data warm.
    const bool fork = n == 1 && q.sideStream && !q.prof.on;
    if (fork) {
        MSL_HIP_TRY(hipEventRecord(q.evFork, s));
        MSL_HIP_TRY(hipStreamWaitEvent(q.sideStream, q.evFork, 0));
        hipLaunchKernelGGL(k_blur, dim3(xcd_grid1((long long)P.blurTiles * n)), dim3(256), 0, q.sideStream, P);
        MSL_HIP_TRY(hipEventRecord(q.evJoin, q.sideStream));
    }
    q.prof.begin(KID_FAST, s);
    hipLaunchKernelGGL(k_fast, dim3(xcd_grid1((long long)P.cellsPerFrame * n)), dim3(64), q.fastLds, s, P);
    q.prof.end(s);
    q.prof.begin(KID_OCTREE, s);
    OctArgs A;
    A.cellCnt = P.cellCnt; A.cellKeys = P.cellKeys; A.cells = P.cells; A.lv = P.lvDev; A.keys = P.keys; A.knode = P.knode; A.sel = P.sel;
    A.nsel = P.nsel; A.ncand = P.ncand; A.err = P.err;
    A.cellsPerFrame = P.cellsPerFrame; A.keysPerFrame = P.keysPerFrame; A.nlevels = L; A.nFrames = n; A.selCap = P.selCap; A.maxNode = P.maxNode;
    if (q.octBig) hipLaunchKernelGGL(k_octree<32>, dim3(xcd_grid1((long long)L * n)), dim3(OCT_NT), (size_t)P.octLds, s, A);
    else hipLaunchKernelGGL(k_octree<16>, dim3(xcd_grid1((long long)L * n)), dim3(OCT_NT), (size_t)P.octLds, s, A);
    q.prof.end(s);
    if (fork) {
        MSL_HIP_TRY(hipStreamWaitEvent(s, q.evJoin, 0));
    } else {
        q.prof.begin(KID_BLUR, s);
        hipLaunchKernelGGL(k_blur, dim3(xcd_grid1((long long)P.blurTiles * n)), dim3(256), 0, s, P);
        q.prof.end(s);
    }
    q.prof.begin(KID_DESCRIBE, s);
    hipLaunchKernelGGL(k_describe, dim3(xcd_grid1((long long)((P.outCap + 3) / 4) * n)), dim3(256), 0, s, P);
    q.prof.end(s);
    MSL_HIP_TRY(hipGetLastError());
    return MSL_OK;
}
