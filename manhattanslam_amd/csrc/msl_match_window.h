// msl_match_window.h -- the pieces every point search on the matcher handle shares (internal): the current frame's 64 x 48 feature grid
// as a cell-sorted item list (k_match_grid), Frame::GetFeaturesInArea's window (src/Frame.cc:332-381) walked by one thread or one wave, the
// candidate keys (dist << 16 | item position) and their staging.  Used by msl_match.hip (last-frame and local-map search),
// msl_reloc.hip (keyframe search) and msl_fuse.hip (the grid of a keyframe table); each translation unit gets its own copy of k_match_grid.
#pragma once

#include "msl_match_handle.h"
#include "msl_match_math.h"

namespace msl {
namespace {
constexpr int GRID_ROWS = MSL_FRAME_GRID_ROWS, GRID_COLS = MSL_FRAME_GRID_COLS, NCELLS = GRID_ROWS * GRID_COLS;
constexpr int CMAX = 32;                            // stored candidates per point; more are re-enumerated by k_match_assign
constexpr unsigned KEY_NONE = 0xFFFFFFFFu;          // no candidate key (dist << 16 | item position)
constexpr int DIST_ANY = 257, DIST_BELOW_256 = 256; // distance caps of a candidate: the local search drops 256 (never best nor second)

struct MatchDev {
    int nPairs, cap;
    msl_match_params prm;
    float gridWInv, gridHInv, mb;
    const msl_keypoint *curKps; const float *curUn; const float *curUright; const int32_t *curCell; const uint8_t *curDesc; const int32_t *nCur;
    const float *lastXyz; const uint8_t *lastDesc; const uint8_t *lastFlags; const int32_t *lastOctave; const float *lastAngle; const int32_t *nLast;
    const float *TcwCur, *TcwLast;
    // scratch
    unsigned short *items;     // [nPairs][cap]      keypoint indices sorted by (cell, index)
    unsigned *cellStart;       // [nPairs][NCELLS+1]
    int *mode;                 // [nPairs]           0: octave +-1, 1: forward, 2: backward
    unsigned *cand;            // [nPairs][cap][CMAX] dist << 16 | item position
    unsigned *candCnt;         // [nPairs][cap]      total candidates of the point (may exceed CMAX)
    int32_t *matchOut, *nmatches;
};

// ---- k_match_grid ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_match_grid(MatchDev P) {
    __shared__ unsigned s_start[NCELLS + 1];
    __shared__ unsigned s_fill[NCELLS];
    __shared__ unsigned s_wave[17];
    extern __shared__ unsigned short s_items[];   // [cap]
    const int pair = blockIdx.x;
    const int n = min(P.nCur[pair], P.cap);
    const int32_t *cell = P.curCell + (size_t)pair * P.cap;
    for (int c = threadIdx.x; c <= NCELLS; c += 256) { s_start[c] = 0; if (c < NCELLS) s_fill[c] = 0; }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = cell[i];
        if (c >= 0 && c < NCELLS) atomicAdd(&s_start[c + 1], 1u);
    }
    __syncthreads();
    block_scan_array_incl(s_start + 1, NCELLS, s_wave);     // s_start[c] = first item of cell c, s_start[NCELLS] = total
    for (int i = threadIdx.x; i < n; i += 256) {            // unordered placement inside each cell ...
        const int c = cell[i];
        if (c >= 0 && c < NCELLS) s_items[s_start[c] + atomicAdd(&s_fill[c], 1u)] = (unsigned short)i;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < NCELLS; c += 256) {       // ... then ascending keypoint index per cell (cells hold a few items)
        const unsigned b = s_start[c], e = s_start[c + 1];
        for (unsigned a = b + 1; a < e; a++) {
            const unsigned short v = s_items[a];
            unsigned j = a;
            while (j > b && s_items[j - 1] > v) { s_items[j] = s_items[j - 1]; j--; }
            s_items[j] = v;
        }
    }
    __syncthreads();
    const unsigned total = s_start[NCELLS];
    for (unsigned i = threadIdx.x; i < total; i += 256) P.items[(size_t)pair * P.cap + i] = s_items[i];
    for (int c = threadIdx.x; c <= NCELLS; c += 256) P.cellStart[(size_t)pair * (NCELLS + 1) + c] = s_start[c];
    if (threadIdx.x == 0 && P.mode) {   // bForward / bBackward (:560-571); the local-map search has no last frame (mode == nullptr)
        P.mode[pair] = search_mode(P.TcwCur + (size_t)pair * 12, P.TcwLast + (size_t)pair * 12, P.mb);
    }
}

// ---- shared pieces of the candidate test ---------------------------------------------------------------------------------
struct Query {
    float u, v, ur, radius;           // ur: abscissa of the projection in the right image (u - mbf * invz)
    int minLevel, maxLevel;
    int minCX, maxCX, minCY, maxCY;   // window in grid cells (empty when minCX > maxCX)
};

// Frame::GetFeaturesInArea window (src/Frame.cc:337-351) of (u, v, radius) into Q's cell range; false = no cell.  The float -> int
// conversions are clamped so that they stay defined (a NaN coordinate gives an empty window, as the reference's conversion does on x86-64).
__device__ __forceinline__ bool grid_window(const MatchDev &P, float u, float v, float radius, Query &Q) {
    const float fx0 = floorf((u - P.prm.minX - radius) * P.gridWInv), fx1 = ceilf((u - P.prm.minX + radius) * P.gridWInv);
    const float fy0 = floorf((v - P.prm.minY - radius) * P.gridHInv), fy1 = ceilf((v - P.prm.minY + radius) * P.gridHInv);
    const int nMinCellX = max(0, (int)fminf(fmaxf(fx0, -1.0e6f), 1.0e6f));
    const int nMaxCellX = min(GRID_COLS - 1, (int)fminf(fmaxf(fx1, -1.0e6f), 1.0e6f));
    const int nMinCellY = max(0, (int)fminf(fmaxf(fy0, -1.0e6f), 1.0e6f));
    const int nMaxCellY = min(GRID_ROWS - 1, (int)fminf(fmaxf(fy1, -1.0e6f), 1.0e6f));
    if (nMinCellX >= GRID_COLS || nMaxCellX < 0 || nMinCellY >= GRID_ROWS || nMaxCellY < 0) return false;
    Q.minCX = nMinCellX; Q.maxCX = nMaxCellX; Q.minCY = nMinCellY; Q.maxCY = nMaxCellY;
    return nMinCellX <= nMaxCellX && nMinCellY <= nMaxCellY;
}

__device__ __forceinline__ bool project_query(const MatchDev &P, int pair, int q, int mode, Query &Q) {
    const float *Tc = P.TcwCur + (size_t)pair * 12;
    const float tcw[3] = {Tc[3], Tc[7], Tc[11]};
    const float *xw = P.lastXyz + ((size_t)pair * P.cap + q) * 3;
    const float x3Dw[3] = {xw[0], xw[1], xw[2]};
    float x3Dc[3];
    gemm3(Tc, false, 1.0, x3Dw, tcw, x3Dc);            // x3Dc = Rcw * x3Dw + tcw (:577)
    const float xc = x3Dc[0], yc = x3Dc[1];
    const float invzc = (float)(1.0 / (double)x3Dc[2]);
    if (invzc < 0) return false;
    const float u = P.prm.fx * xc * invzc + P.prm.cx;
    const float v = P.prm.fy * yc * invzc + P.prm.cy;
    if (!(u >= P.prm.minX && u <= P.prm.maxX)) return false;   // NaN: GetFeaturesInArea would find no feature
    if (!(v >= P.prm.minY && v <= P.prm.maxY)) return false;
    const int nLastOctave = P.lastOctave[(size_t)pair * P.cap + q];
    if (nLastOctave < 0 || nLastOctave >= P.prm.nlevels) return false;   // not an octave of this pyramid (the reference would index out of bounds): no candidates
    const float radius = P.prm.th * P.prm.scale_factors[nLastOctave];
    Q.u = u; Q.v = v; Q.ur = u - P.prm.bf * invzc; Q.radius = radius;   // ur: :626
    if (mode == 1) { Q.minLevel = nLastOctave; Q.maxLevel = -1; }
    else if (mode == 2) { Q.minLevel = 0; Q.maxLevel = nLastOctave; }
    else { Q.minLevel = nLastOctave - 1; Q.maxLevel = nLastOctave + 1; }
    return grid_window(P, u, v, radius, Q);
}

// filters of GetFeaturesInArea (:353-376) + the mvuRight test (:625-630) for item position p; returns the Hamming distance or -1.
// RIGHT = false: a search without the mvuRight test (the keyframe search; curUright is not read).
template <bool RIGHT = true>
__device__ __forceinline__ int eval_item(const MatchDev &P, int pair, const Query &Q, unsigned i2, const uint4 &d0, const uint4 &d1) {
    const size_t base = (size_t)pair * P.cap + i2;
    const int octave = P.curKps[base].octave;
    const bool bCheckLevels = (Q.minLevel > 0) || (Q.maxLevel >= 0);
    if (bCheckLevels) {
        if (octave < Q.minLevel) return -1;
        if (Q.maxLevel >= 0 && octave > Q.maxLevel) return -1;
    }
    const float2 pt = *reinterpret_cast<const float2 *>(P.curUn + 2 * base);
    const float distx = pt.x - Q.u, disty = pt.y - Q.v;
    if (!(fabsf(distx) < Q.radius && fabsf(disty) < Q.radius)) return -1;
    if (RIGHT) {
        const float uRight = P.curUright[base];
        if (uRight > 0) {
            const float er = fabsf(Q.ur - uRight);
            if (er > Q.radius) return -1;
        }
    }
    uint4 e0, e1;
    load_desc(P.curDesc + base * 32, e0, e1);
    return hamming256(d0, d1, e0, e1);
}

// The window of Q holds window_cells(Q) cells; cell c of them in the reference's walk order (ascending ix, then iy) holds the item
// positions [b, e), which ascend in that order too (a cell's items in mGrid insertion order).
__device__ __forceinline__ int window_cells(const Query &Q) { return (Q.maxCX - Q.minCX + 1) * (Q.maxCY - Q.minCY + 1); }
__device__ __forceinline__ void window_cell(const MatchDev &P, int pair, const Query &Q, int c, unsigned &b, unsigned &e) {
    const int ny = Q.maxCY - Q.minCY + 1;
    const unsigned *cs = P.cellStart + (size_t)pair * (NCELLS + 1) + (Q.minCX + c / ny) * GRID_ROWS + Q.minCY + c % ny;
    b = cs[0]; e = cs[1];
}

// The window walked by one thread in reference order: item(p) for every item position p.
template <class Item>
__device__ __forceinline__ void walk_window(const MatchDev &P, int pair, const Query &Q, Item item) {
    const int C = window_cells(Q);
    for (int c = 0; c < C; c++) {
        unsigned b, e;
        window_cell(P, pair, Q, c, b, e);
        for (unsigned p = b; p < e; p++) item(p);
    }
}

// The window of Q walked by one wave (cells spread over the lanes): every item that passes eval_item with a distance below distCap is
// stored as (dist << 16 | item position), the first CMAX of them in cand; *cnt (wave-shared, zero on entry) ends as the total.
template <bool RIGHT = true>
__device__ __forceinline__ void wave_candidates(const MatchDev &P, int pair, const Query &Q, const uint8_t *desc32, int distCap, unsigned *cand,
                                                unsigned *cnt, int lane) {
    uint4 d0, d1;
    load_desc(desc32, d0, d1);
    const unsigned short *items = P.items + (size_t)pair * P.cap;
    const int C = window_cells(Q);
    for (int c = lane; c < C; c += 64) {
        unsigned b, e;
        window_cell(P, pair, Q, c, b, e);
        for (unsigned p = b; p < e; p++) {
            const int dist = eval_item<RIGHT>(P, pair, Q, items[p], d0, d1);
            if (dist < 0 || dist >= distCap) continue;
            const unsigned slot = atomicAdd(cnt, 1u);
            if (slot < CMAX) cand[slot] = ((unsigned)dist << 16) | p;
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// Every candidate key (dist << 16 | item position) of query q (row qi of cand / candCnt) that q does not skip under s_t (msl_assign.h),
// to offer(key): the stored candidates, or, when the wave found more than the CMAX it stored, the window of make_query(Q) walked again
// with the filters of wave_candidates (rare; any count stays exact).
template <bool RIGHT = true, class MakeQuery, class Offer>
__device__ __forceinline__ void unskipped_candidates(const MatchDev &P, int pair, size_t qi, int q, const uint8_t *desc32, int distCap, const int *s_t,
                                                     MakeQuery make_query, Offer offer) {
    const unsigned short *items = P.items + (size_t)pair * P.cap;
    const unsigned cnt = P.candCnt[qi];
    if (cnt <= CMAX) {
        const unsigned *cand = P.cand + qi * CMAX;
        for (unsigned k = 0; k < cnt; k++) {
            const unsigned key = cand[k];
            if (s_t[items[key & 0xFFFFu]] < q) continue;
            offer(key);
        }
        return;
    }
    Query Q;
    if (!make_query(Q)) return;
    uint4 d0, d1;
    load_desc(desc32, d0, d1);
    walk_window(P, pair, Q, [&](unsigned p) {
        const unsigned i2 = items[p];
        if (s_t[i2] < q) return;
        const int dist = eval_item<RIGHT>(P, pair, Q, i2, d0, d1);
        if (dist >= 0 && dist < distCap) offer(((unsigned)dist << 16) | p);
    });
}

// The current-frame part of a point search (both of them): sizes, parameters, the grid pitch and the six current-frame arrays.
void stage_current_frame(Stage &S, MatchDev &P, int n_frames, int cap, const msl_match_params &prm, const msl_keypoint *cur_kps, const float *cur_un_xy,
                         const float *cur_uright, const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur) {
    const size_t n = (size_t)n_frames * cap;
    P.nPairs = n_frames; P.cap = cap; P.prm = prm;
    P.gridWInv = static_cast<float>(GRID_COLS) / static_cast<float>(prm.maxX - prm.minX);   // src/Frame.cc:137-138
    P.gridHInv = static_cast<float>(GRID_ROWS) / static_cast<float>(prm.maxY - prm.minY);
    P.curKps = S.in(cur_kps, n); P.curUn = S.in(cur_un_xy, 2 * n); P.curUright = S.in(cur_uright, n); P.curCell = S.in(cur_grid_cell, n);
    P.curDesc = S.in(cur_desc, 32 * n); P.nCur = S.in(n_cur, (size_t)n_frames);
}

}  // namespace
}  // namespace msl
