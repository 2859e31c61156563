// msl_orb_host.hip -- ORB extractor, host side: the handle, the geometry plan of a frame size and its commit to the device, staging and
// copy-out of a call, the C ABI, the debug and profile hooks.  No kernel lives here: the device side is msl_orb.hip, reached through
// msl_orb_dev.h.  Compiled with -ffp-contract=off like the kernels: the resize coefficients below feed a rounding.

#include "msl_orb_dev.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

using namespace msl;
using namespace msl::orb;

namespace {

inline int cv_round_f(float v) { return (int)lrintf(v); }
inline int cv_round_d(double v) { return (int)lrint(v); }
inline int cv_floor_d(double v) { int i = (int)v; return i - (i > v); }
inline int cv_ceil_d(double v) { int i = (int)v; return i + (i < v); }

}  // namespace

// What msl_orb_create fixes; all that planning reads of the handle.
struct OrbConfig {
    int nfeatures = 0, nlevels = 0, iniTh = 0, minTh = 0, maxBatch = 0;
    int outCap = 0;   // keypoints per frame the outputs are sized for: fixed by the creation geometry (msl_orb_capacity); 0 until that is committed
    std::vector<float> scale, invScale;
    std::vector<int> perLevel;
    int umax[16];
};

struct msl_orb : OrbConfig, OrbLaunch {
    int device = 0;
    int maxW = 0, maxH = 0;
    double scaleFactor = 0;
    std::vector<float> sigma2, invSigma2;
    // geometry is committed for one frame size at a time (planned and committed again if the size changes)
    int geomW = 0, geomH = 0;
    OrbDev dev{};
    bool ownStream = true;
    // device allocations of the current geometry (commit_geometry); outBlock = [nout[B] | kps[B][cap] | desc[B][cap]], d_nout / d_kps / d_desc point into it
    struct Geometry { DevBuf in, pyr, blur, cells, levels, taps, pyrRanges, cellCnt, cellKeys, keys, knode, sel, nsel, ncand, outBlock; } geo;
    size_t inPitch = 0, outKpsOff = 0, outDescOff = 0;
    msl_keypoint *d_kps = nullptr; uint8_t *d_desc = nullptr; int *d_nout = nullptr;
    DevBuf d_err; PinBuf h_err;
    PinBuf h_pinIn, h_pinOut;   // staging of the single-frame drop-in call
    DevBuf d_depthIn;           // staged depth frames (host input)
    DevBuf d_unXY, d_depthOut, d_uRight, d_gridCell;   // outputs of the frame epilogue
    int lastFrames = 0;
};

namespace {

// ---------------------------------------------------------------------------------------------
// Plan: everything a W x H frame needs, worked out on the host.  No HIP call, no handle: a size that is rejected costs nothing.
// ---------------------------------------------------------------------------------------------
struct OrbPlan {
    int W = 0, H = 0;
    OrbDev dev{};   // every field but the device pointers
    std::vector<CellDev> cells;
    std::vector<ResizeTap> taps;
    std::vector<PyrRange> pyrX, pyrY;
    size_t pyrLds = 0, fastLds = 0, inPitch = 0, outKpsOff = 0, outDescOff = 0;
    int needCap = 0, outCap = 0;
    bool octBig = false;
    // running totals of the level loop
    size_t pyrOff = 0, blurOff = 0;
    unsigned keyOff = 0;
    int tileBase = 0, maxList = 0, maxSel = 0;
};

// Level l: size, offsets in the pyramid and blurred stores, FAST cell grid (:728-743), blur tiles.
int plan_level_grid(const OrbConfig *h, OrbPlan &P, int l) {
    LevelDev &G = P.dev.lv[l];
    const float s = h->invScale[l];
    G.w = cv_round_f((float)P.W * s); G.h = cv_round_f((float)P.H * s);    // src/ORBextractor.cc:875
    G.pitch = (G.w + 63) & ~63;
    G.scale = h->scale[l];
    G.patch = (int)(31 * h->scale[l]);                                  // :788
    G.quota = h->perLevel[l];
    if (l > 0) { G.off = (unsigned)P.pyrOff; P.pyrOff += (size_t)G.pitch * G.h; }
    G.boff = (unsigned)P.blurOff; P.blurOff += (size_t)G.pitch * G.h;
    const int minB = 16, maxBX = G.w - 16, maxBY = G.h - 16;
    const float width = (float)(maxBX - minB), height = (float)(maxBY - minB);
    const float Wc = 30;
    G.nCols = (int)(width / Wc); G.nRows = (int)(height / Wc);
    if (G.nCols < 1 || G.nRows < 1) {
        set_error("level %d (%dx%d) is too small for the 30-px FAST grid", l, G.w, G.h);
        return MSL_ERR_INVALID;
    }
    G.wCell = (int)ceilf(width / G.nCols); G.hCell = (int)ceilf(height / G.nRows);
    if (G.wCell > MAXCELL || G.hCell > MAXCELL || G.w > 4095 + 16 || G.h > 4095 + 16) {
        set_error("unsupported level geometry %dx%d (cell %dx%d)", G.w, G.h, G.wCell, G.hCell);
        return MSL_ERR_INVALID;
    }
    P.fastLds = std::max(P.fastLds, (size_t)fast_lds(G.wCell, G.hCell).bytes);   // (a cell is at most wCell x hCell)
    G.cellBase = (int)P.cells.size(); G.nCells = G.nRows * G.nCols;
    G.keyBase = (int)P.keyOff;
    for (int i = 0; i < G.nRows; i++)
        for (int j = 0; j < G.nCols; j++) {
            // view = rows [iniY,maxY) x cols [iniX,maxX); cv::FAST computes its inner 3-px-inset region
            const float iniY = (float)(minB + i * G.hCell), iniX = (float)(minB + j * G.wCell);
            float maxY = iniY + G.hCell + 6, maxX = iniX + G.wCell + 6;
            CellDev c{}; c.level = (short)l; c.keyOff = P.keyOff;
            const bool skip = (iniY >= maxBY - 3) || (iniX >= maxBX - 6);
            if (maxY > maxBY) maxY = (float)maxBY;
            if (maxX > maxBX) maxX = (float)maxBX;
            const int cw = (int)maxX - (int)iniX - 6, chh = (int)maxY - (int)iniY - 6;
            if (!skip && cw > 0 && chh > 0) {
                c.x0 = (short)((int)iniX + 3); c.y0 = (short)((int)iniY + 3); c.cw = (short)cw; c.ch = (short)chh;
                P.keyOff += (unsigned)(((cw + 1) / 2) * ((chh + 1) / 2));  // strict 3x3 maxima are non-adjacent
            }
            P.cells.push_back(c);
        }
    G.keyCap = (int)P.keyOff - G.keyBase;
    if (G.keyCap >= (1 << 24)) { set_error("level too large"); return MSL_ERR_INVALID; }
    G.tilesX = (G.w + BT_W - 1) / BT_W; G.tilesY = (G.h + BT_H - 1) / BT_H;
    G.tileBase = P.tileBase; P.tileBase += G.tilesX * G.tilesY;
    return MSL_OK;
}

// Level l: quadtree roots (:536-552) and what they bound: the longest node list and the keypoints the level can return.
int plan_level_quadtree(OrbPlan &P, int l) {
    LevelDev &G = P.dev.lv[l];
    const int minB = 16, maxBX = G.w - 16, maxBY = G.h - 16;
    G.nIni = (int)roundf((float)(maxBX - minB) / (maxBY - minB));
    if (G.nIni < 1) { set_error("unsupported aspect ratio (nIni = 0)"); return MSL_ERR_INVALID; }
    G.hX = (float)(maxBX - minB) / G.nIni;
    // longest quadtree list of this level: a full round only runs when its outcome stays <= quota (the first one makes <= 4 nIni nodes), the
    // one-by-one phase stops at the first length >= quota and every expansion adds <= 3
    if (std::max(G.quota, 4 * G.nIni) + 2 > MAXNODE) { set_error("per-level quota %d exceeds %d", G.quota, MAXNODE - 2); return MSL_ERR_INVALID; }
    P.maxList = std::max(P.maxList, std::max(G.quota, 4 * G.nIni) + 2);
    // keypoints this level can return: quota + 2 from the one-by-one phase (:691-696), or the <= 4 nIni nodes of the first full round when
    // that already reaches the quota (wide images with a small budget: nIni = round(width / height) roots, :536-552)
    P.needCap += std::max(G.quota + 2, 4 * G.nIni); P.maxSel = std::max(P.maxSel, std::max(G.quota + 2, 4 * G.nIni));
    return MSL_OK;
}

// Level l >= 1 from level l - 1: resize taps (cv::resize INTER_LINEAR 8U tables).  The two axes clamp differently, as cv::resize
// does: x zeroes the fraction at both borders and overrides the last tap, y only clamps the indices.
void plan_level_taps(OrbPlan &P, int l) {
    LevelDev &G = P.dev.lv[l];
    std::vector<ResizeTap> &taps = P.taps;
    const int sw = P.dev.lv[l - 1].w, sh = P.dev.lv[l - 1].h;
    const double scale_x = 1. / ((double)G.w / sw), scale_y = 1. / ((double)G.h / sh);
    G.xtabOff = (unsigned)taps.size();
    for (int dx = 0; dx < G.w; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor_d(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        ResizeTap t;
        t.s0 = (short)sx; t.s1 = (short)std::min(sx + 1, sw - 1);
        t.c0 = (short)std::min(std::max(cv_round_f((1.f - fx) * 2048), -32768), 32767);
        t.c1 = (short)std::min(std::max(cv_round_f(fx * 2048), -32768), 32767);
        if (sx + 1 >= sw) { t.c0 = 2048; t.c1 = 0; }
        taps.push_back(t);
    }
    G.ytabOff = (unsigned)taps.size();
    for (int dy = 0; dy < G.h; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor_d(fy);
        fy -= sy;
        ResizeTap t;
        t.s0 = (short)std::min(std::max(sy, 0), sh - 1); t.s1 = (short)std::min(std::max(sy + 1, 0), sh - 1);
        t.c0 = (short)std::min(std::max(cv_round_f((1.f - fy) * 2048), -32768), 32767);
        t.c1 = (short)std::min(std::max(cv_round_f(fy * 2048), -32768), 32767);
        taps.push_back(t);
    }
}

// Fused pyramid (k_pyramid): one tile grid for all levels, ranges per axis; left off (pyrTX == 0: one k_resize per level) when a tile chain
// does not fit k_pyramid's LDS budget or its multiply-shift row index.
void plan_pyramid(OrbPlan &P) {
    OrbDev &D = P.dev;
    const int L = D.nlevels;
    const std::vector<ResizeTap> &taps = P.taps;
    D.pyrTX = D.pyrTY = 0;
    if (L < 2) return;
    const int TX = std::max(1, D.lv[L - 1].w / 22), TY = std::max(1, D.lv[L - 1].h / 22);
    auto axis = [&](int T, bool isX, std::vector<PyrRange> &out, std::vector<int> &extent) {
        out.assign((size_t)L * T, PyrRange{0, 0, 0, 0});
        extent.assign(L, 0);
        for (int i = 0; i < T; i++) {
            for (int l = 1; l < L; l++) {
                const int n = isX ? D.lv[l].w : D.lv[l].h;
                PyrRange &r = out[(size_t)l * T + i];
                r.ownLo = (short)((long long)i * n / T); r.ownHi = (short)((long long)(i + 1) * n / T);
            }
            int lo = out[(size_t)(L - 1) * T + i].ownLo, hi = out[(size_t)(L - 1) * T + i].ownHi;
            for (int l = L - 1; l >= 1; l--) {
                PyrRange &r = out[(size_t)l * T + i];
                r.needLo = (short)lo; r.needHi = (short)hi;
                extent[l] = std::max(extent[l], hi - lo);
                const ResizeTap *tab = taps.data() + (isX ? D.lv[l].xtabOff : D.lv[l].ytabOff);
                int slo = tab[lo].s0, shi = tab[hi - 1].s1 + 1;   // source pixels of level l-1 this range reads (taps are monotone)
                for (int q = lo; q < hi; q++) { slo = std::min(slo, (int)std::min(tab[q].s0, tab[q].s1)); shi = std::max(shi, (int)std::max(tab[q].s0, tab[q].s1) + 1); }
                if (l - 1 >= 1) { const PyrRange &o = out[(size_t)(l - 1) * T + i]; lo = std::min(slo, (int)o.ownLo); hi = std::max(shi, (int)o.ownHi); }
                else { lo = slo; hi = shi; }
            }
            PyrRange &r0 = out[i];
            r0.ownLo = r0.ownHi = 0; r0.needLo = (short)lo; r0.needHi = (short)hi;
            extent[0] = std::max(extent[0], hi - lo);
        }
    };
    std::vector<int> ex, ey;
    axis(TX, true, P.pyrX, ex); axis(TY, false, P.pyrY, ey);
    // k_pyramid's row pitches: the input region rounded up to whole dwords; a later level starts at the column needLo & ~3 and ends on a whole run of four
    ex[0] = (ex[0] + 3) & ~3;
    for (int l = 1; l < L; l++) {
        ex[l] = 0;
        for (int i = 0; i < TX; i++) { const PyrRange &r = P.pyrX[(size_t)l * TX + i]; ex[l] = std::max(ex[l], ((r.needHi - (r.needLo & ~3)) + 3) & ~3); }
    }
    size_t b0 = 0, b1 = 0;
    bool ok = true;
    for (int l = 0; l < L; l++) {
        const size_t a = (size_t)ex[l] * ey[l] + 8;   // (+ 8: a pixel's source pair is cut from two aligned words, the second of which may lie past the last row)
        if (l & 1) b1 = std::max(b1, a); else b0 = std::max(b0, a);
        if (l >= 1 && (D.lv[l].w < TX || D.lv[l].h < TY)) ok = false;
    }
    b0 = (b0 + 15) & ~(size_t)15;
    for (int l = 0; l < L; l++) if (ex[l] >= 128 || (size_t)ex[l] * ey[l] >= (1u << 15)) ok = false;   // k_pyramid's multiply-shift row index
    // k_pyramid reads a pixel's two source columns as one pair of adjacent bytes and multiplies unsigned 16-bit fields (resize_px): true of every
    // column tap cv::resize's rule makes (s1 = s0 + 1, or the clamped last column with c1 = 0); a table that broke it would fall back to k_resize
    for (int l = 1; l < L && ok; l++)
        for (int x = 0; x < D.lv[l].w; x++) {
            const ResizeTap &t = taps[D.lv[l].xtabOff + x];
            if (t.c0 < 0 || t.c1 < 0 || !(t.s1 == t.s0 + 1 || t.c1 == 0)) ok = false;
        }
    b1 = (b1 + 15) & ~(size_t)15;
    const size_t tapBytes = 2 * PYR_TAPS * sizeof(ResizeTap);   // two levels' column taps in turn (ex[l] < 128 = PYR_TAPS)
    if (ok && b0 + b1 + tapBytes <= 48 * 1024) { D.pyrTX = TX; D.pyrTY = TY; D.pyrBuf0 = (unsigned)b0; D.pyrTapOff = (unsigned)(b0 + b1); P.pyrLds = b0 + b1 + tapBytes; }
}

int plan_geometry(const OrbConfig *h, int W, int H, OrbPlan &P) {
    P.W = W; P.H = H;
    OrbDev &D = P.dev;
    const int L = h->nlevels, B = h->maxBatch;
    D.nlevels = L; D.iniTh = h->iniTh; D.minTh = h->minTh;
    for (int i = 0; i < 16; i++) D.umax[i] = h->umax[i];
    for (int l = 0; l < L; l++) {
        int rc = plan_level_grid(h, P, l);
        if (rc == MSL_OK) rc = plan_level_quadtree(P, l);
        if (rc != MSL_OK) return rc;
        if (l > 0) plan_level_taps(P, l);
    }
    plan_pyramid(P);
    D.cellsPerFrame = (int)P.cells.size();
    D.keysPerFrame = (int)P.keyOff;
    D.selCap = P.maxSel;
    D.maxNode = ((P.maxList + 63) & ~63) + 64;   // the analytic bound, rounded up, plus one 64-node block of slack (4 KB): an overrun would zero a whole level (P.err)
    {
        int maxCells = 0;
        for (int l = 0; l < L; l++) maxCells = std::max(maxCells, D.lv[l].nCells);
        D.octLds = (int)((std::max<size_t>((size_t)OCT_NODE_BYTES * D.maxNode, 2 * sizeof(unsigned) * (size_t)(maxCells + 1)) + 15) & ~(size_t)15);
    }
    P.outCap = h->outCap ? h->outCap : std::max(h->nfeatures + 2 * L, P.needCap);   // creation: the handle's capacity follows its (max_width, max_height) geometry
    if (P.needCap > P.outCap) {
        set_error("frame %dx%d can return %d keypoints (aspect ratio: %d quadtree roots), the extractor was created for %d; create it with this frame size", W, H,
                  P.needCap, D.lv[0].nIni, P.outCap);
        return MSL_ERR_INVALID;
    }
    D.outCap = P.outCap;
    P.octBig = (long long)W * H > 640ll * 480 * 3 / 2;
    D.blurTiles = P.tileBase;
    D.pyrStride = (P.pyrOff + 255) & ~(size_t)255;
    D.blurStride = (P.blurOff + 255) & ~(size_t)255;
    P.inPitch = (size_t)((W + 63) & ~63);
    // outputs of a call in ONE allocation, counts first: the single-frame drop-in call fetches everything with one copy
    P.outKpsOff = (sizeof(int) * (size_t)B + 255) & ~(size_t)255;
    P.outDescOff = P.outKpsOff + ((sizeof(msl_keypoint) * (size_t)D.outCap * B + 255) & ~(size_t)255);
    return MSL_OK;
}

// ---------------------------------------------------------------------------------------------
// Commit: the planned geometry replaces the handle's.  The only place that writes h->dev.
// ---------------------------------------------------------------------------------------------
int commit_geometry(msl_orb *h, const OrbPlan &P) {
    // the work that may still use the old buffers (the side stream's is joined into h->stream by evJoin)
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    h->geomW = h->geomH = 0;   // (a failure below leaves the handle without a geometry: the next call plans again)
    msl_orb::Geometry &g = h->geo;
    g = msl_orb::Geometry();
    OrbDev &D = h->dev;
    D = P.dev;
    const size_t B = (size_t)h->maxBatch, L = (size_t)D.nlevels, nCells = P.cells.size(), nKeys = P.keyOff;
    MSL_HIP_TRY(grow_all(h->stream, {{g.in, P.inPitch * P.H * B}, {g.pyr, std::max<size_t>(D.pyrStride, 256) * B}, {g.blur, D.blurStride * B},
                                     {g.cells, sizeof(CellDev) * nCells}, {g.levels, sizeof(LevelDev) * L}, {g.taps, sizeof(ResizeTap) * std::max<size_t>(P.taps.size(), 1)},
                                     {g.pyrRanges, D.pyrTX ? sizeof(PyrRange) * (P.pyrX.size() + P.pyrY.size()) : 0},
                                     {g.cellCnt, sizeof(uint32_t) * nCells * B}, {g.cellKeys, sizeof(uint32_t) * nKeys * B},
                                     {g.keys, sizeof(uint32_t) * nKeys * B}, {g.knode, sizeof(uint16_t) * nKeys * B},
                                     {g.sel, sizeof(uint32_t) * (size_t)D.selCap * L * B}, {g.nsel, sizeof(int) * L * B}, {g.ncand, sizeof(int) * L * B},
                                     {g.outBlock, P.outDescOff + (size_t)32 * D.outCap * B}}));
    MSL_HIP_TRY(hipMemcpy(g.cells.p, P.cells.data(), sizeof(CellDev) * nCells, hipMemcpyHostToDevice));
    MSL_HIP_TRY(hipMemcpy(g.levels.p, D.lv, sizeof(LevelDev) * L, hipMemcpyHostToDevice));   // (the level table is complete in the plan: no field of it is a device pointer)
    if (!P.taps.empty())
        MSL_HIP_TRY(hipMemcpy(g.taps.p, P.taps.data(), sizeof(ResizeTap) * P.taps.size(), hipMemcpyHostToDevice));
    if (D.pyrTX) {
        PyrRange *ranges = (PyrRange *)g.pyrRanges.p;
        MSL_HIP_TRY(hipMemcpy(ranges, P.pyrX.data(), sizeof(PyrRange) * P.pyrX.size(), hipMemcpyHostToDevice));
        MSL_HIP_TRY(hipMemcpy(ranges + P.pyrX.size(), P.pyrY.data(), sizeof(PyrRange) * P.pyrY.size(), hipMemcpyHostToDevice));
        D.pyrX = ranges; D.pyrY = ranges + P.pyrX.size();
    }
    D.pyr = (uint8_t *)g.pyr.p; D.blur = (uint8_t *)g.blur.p; D.cells = (const CellDev *)g.cells.p; D.lvDev = (const LevelDev *)g.levels.p; D.taps = (const ResizeTap *)g.taps.p;
    D.cellCnt = (uint32_t *)g.cellCnt.p; D.cellKeys = (uint32_t *)g.cellKeys.p; D.keys = (uint32_t *)g.keys.p; D.knode = (uint16_t *)g.knode.p;
    D.sel = (uint32_t *)g.sel.p; D.nsel = (int *)g.nsel.p; D.ncand = (int *)g.ncand.p; D.err = (int *)h->d_err.p;
    uint8_t *out = (uint8_t *)g.outBlock.p;
    h->d_nout = reinterpret_cast<int *>(out);
    h->d_kps = reinterpret_cast<msl_keypoint *>(out + P.outKpsOff);
    h->d_desc = out + P.outDescOff;
    h->outCap = P.outCap; h->inPitch = P.inPitch; h->outKpsOff = P.outKpsOff; h->outDescOff = P.outDescOff;
    h->pyrLds = P.pyrLds; h->fastLds = P.fastLds; h->octBig = P.octBig;
    { const int rc = allow_octree_lds(D.octLds); if (rc != MSL_OK) return rc; }
    h->geomW = P.W; h->geomH = P.H;
    return MSL_OK;
}

// The handle's geometry is the one of W x H frames.  A size that plan_geometry rejects leaves the handle as it was.
int ensure_geometry(msl_orb *h, int W, int H) {
    if (h->geomW == W && h->geomH == H) return MSL_OK;
    OrbPlan plan;
    const int rc = plan_geometry(h, W, H, plan);
    return rc != MSL_OK ? rc : commit_geometry(h, plan);
}

int check_device_error(msl_orb *h) {
    MSL_HIP_TRY(hipMemcpyAsync(h->h_err.p, h->d_err.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    h->prof.drain();
    const int e = *(const int *)h->h_err.p;
    if (e) {
        (void)hipMemsetAsync(h->d_err.p, 0, sizeof(int), h->stream);
        set_error("device-side bound exceeded in ORB pipeline (code %d)", e);
        return MSL_ERR_OVERFLOW;
    }
    return MSL_OK;
}

// ---------------------------------------------------------------------------------------------
// One batched call: gray frames in, pipeline, output arrays out
// ---------------------------------------------------------------------------------------------
struct GrayOnDevice { const uint8_t *p; size_t rowStride, frameStride; };

// Host frames go to the handle's input buffer (profiler slot `copy`); device frames are used where they are.
int stage_gray(msl_orb *h, const uint8_t *gray, int n, int W, int H, size_t rowStride, size_t frameStride, msl_mem mem, GrayOnDevice &out) {
    out = {gray, rowStride, frameStride};
    if (mem != MSL_MEM_HOST) return MSL_OK;
    uint8_t *d_in = (uint8_t *)h->geo.in.p;
    h->prof.begin(KID_COPY, h->stream);
    if (rowStride == (size_t)W && h->inPitch == (size_t)W && frameStride == (size_t)W * H) {
        // tightly packed frames (the streaming case): one copy for the whole batch
        MSL_HIP_TRY(hipMemcpyAsync(d_in, gray, (size_t)W * H * n, hipMemcpyHostToDevice, h->stream));
    } else {
        for (int f = 0; f < n; f++)
            MSL_HIP_TRY(hipMemcpy2DAsync(d_in + (size_t)f * h->inPitch * H, h->inPitch, gray + (size_t)f * frameStride, rowStride, W, H, hipMemcpyHostToDevice, h->stream));
    }
    h->prof.end(h->stream);
    out = {d_in, h->inPitch, h->inPitch * H};
    return MSL_OK;
}

// One output array of a call: [frames][cap] at the caller's, [frames][outCap] in the handle.  In order: keypoints, descriptors and -- frame
// batch -- undistorted xy, depth, uRight, grid cell.
struct OutArray { void *user; void *own; size_t bytesPerKey; };

// Runs the pipeline on staged frames and delivers its outputs.  The kernels write straight into device buffers of the handle's own row length
// (direct); every other caller gets row-pitched copies out of the handle's buffers, and a host caller the deferred device error with them.
int run_batch(msl_orb *h, const GrayOnDevice &g, int n, FrameEpilogue *ep, const OutArray *outs, int nOuts, int cap, int32_t *n_out, msl_mem out_mem) {
    const int outCap = h->outCap;
    const bool direct = out_mem == MSL_MEM_DEVICE && cap == outCap;
    void *dst[6];
    for (int i = 0; i < nOuts; i++) dst[i] = direct ? outs[i].user : outs[i].own;
    if (ep) { ep->unXY = (float *)dst[2]; ep->depthOut = (float *)dst[3]; ep->uRight = (float *)dst[4]; ep->gridCell = (int *)dst[5]; }
    const int rc = orb_launch_pipeline(&h->dev, h, g.p, g.rowStride, g.frameStride, n, (msl_keypoint *)dst[0], (uint8_t *)dst[1], direct ? n_out : h->d_nout, ep);
    if (rc != MSL_OK) return rc;
    h->lastFrames = n;
    if (direct) return MSL_OK;
    const hipMemcpyKind kind = out_mem == MSL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    MSL_HIP_TRY(hipMemcpyAsync(n_out, h->d_nout, sizeof(int) * n, kind, h->stream));
    for (int i = 0; i < nOuts; i++) {
        const size_t b = outs[i].bytesPerKey;
        MSL_HIP_TRY(hipMemcpy2DAsync(outs[i].user, b * cap, outs[i].own, b * outCap, b * outCap, n, kind, h->stream));
    }
    return out_mem == MSL_MEM_HOST ? check_device_error(h) : MSL_OK;
}

}  // namespace

extern "C" {

msl_orb *msl_orb_create(int nfeatures, float scaleFactorF, int nlevels, int iniThFAST, int minThFAST, int max_width,
                        int max_height, int max_batch, int device) noexcept {
    try {
    if (nfeatures < 1 || nlevels < 1 || nlevels > ML || !(scaleFactorF > 1.0f) || iniThFAST < 1 || iniThFAST > 255 ||
        minThFAST < 1 || minThFAST > 255 || max_width < 1 || max_height < 1 || max_batch < 1) {
        set_error("msl_orb_create: invalid argument");
        return nullptr;
    }
    if (bind_device(device) != MSL_OK) return nullptr;
    // (owned by a guard until the handle is complete: an exception from the containers below -- std::bad_alloc -- lands in the catch barrier, and the
    // streams, events and device buffers created so far must go with it)
    std::unique_ptr<msl_orb, void (*)(msl_orb *)> guard(new msl_orb, [](msl_orb *p) { msl_orb_destroy(p); });
    msl_orb *h = guard.get();
    h->device = device; h->nfeatures = nfeatures; h->nlevels = nlevels; h->iniTh = iniThFAST; h->minTh = minThFAST;
    h->maxW = max_width; h->maxH = max_height; h->maxBatch = max_batch;
    h->scaleFactor = scaleFactorF;  // include/ORBextractor.h:97 keeps it as double
    // scale tables and per-level quotas, src/ORBextractor.cc:416-445
    h->scale.resize(nlevels); h->sigma2.resize(nlevels); h->invScale.resize(nlevels); h->invSigma2.resize(nlevels);
    h->scale[0] = 1.0f; h->sigma2[0] = 1.0f;
    for (int i = 1; i < nlevels; i++) {
        h->scale[i] = (float)(h->scale[i - 1] * h->scaleFactor);
        h->sigma2[i] = h->scale[i] * h->scale[i];
    }
    for (int i = 0; i < nlevels; i++) { h->invScale[i] = 1.0f / h->scale[i]; h->invSigma2[i] = 1.0f / h->sigma2[i]; }
    h->perLevel.resize(nlevels);
    const float factor = (float)(1.0f / h->scaleFactor);
    float nDesired = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int level = 0; level < nlevels - 1; level++) {
        h->perLevel[level] = cv_round_f(nDesired);
        sum += h->perLevel[level];
        nDesired *= factor;
    }
    h->perLevel[nlevels - 1] = std::max(nfeatures - sum, 0);
    // circular patch row ends, :453-467
    {
        int v, v0;
        const int vmax = cv_floor_d(15 * sqrtf(2.f) / 2 + 1), vmin = cv_ceil_d(15 * sqrtf(2.f) / 2);
        for (v = 0; v < 16; v++) h->umax[v] = 0;
        for (v = 0; v <= vmax; ++v) h->umax[v] = cv_round_d(sqrt(225.0 - v * v));
        for (v = 15, v0 = 0; v >= vmin; --v) {
            while (h->umax[v0] == h->umax[v0 + 1]) ++v0;
            h->umax[v] = v0;
            ++v0;
        }
    }
    int prLo = 0, prHi = 0;   // frame-batched throughput work: lowest priority, so latency-critical streams of the process go first
    (void)hipDeviceGetStreamPriorityRange(&prLo, &prHi);
    if (hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prLo) != hipSuccess ||
        h->d_err.grow(2048, h->stream) != hipSuccess || hipMemset(h->d_err.p, 0, 2048) != hipSuccess ||   // [0] deferred error; from byte 128: 200 device-clock stamps of experiment builds
        h->h_err.grow(sizeof(int), h->stream) != hipSuccess ||
        hipStreamCreateWithPriority(&h->sideStream, hipStreamNonBlocking, prLo) != hipSuccess ||
        hipEventCreateWithFlags(&h->evFork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&h->evJoin, hipEventDisableTiming) != hipSuccess) {
        set_error("msl_orb_create: HIP resource allocation failed");
        return nullptr;
    }
    h->prof.nk = MSL_ORB_NKERNELS;
    if (ensure_geometry(h, max_width, max_height) != MSL_OK) return nullptr;
    return guard.release();
    } MSL_ABI_CATCH_PTR
}

void msl_orb_destroy(msl_orb *h) noexcept {
    try {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->sideStream) (void)hipStreamSynchronize(h->sideStream);
    h->prof.destroy();
    if (h->evFork) (void)hipEventDestroy(h->evFork);
    if (h->evJoin) (void)hipEventDestroy(h->evJoin);
    const hipStream_t streams[2] = {h->sideStream, h->ownStream ? h->stream : nullptr};
    delete h;   // frees the buffers
    for (hipStream_t st : streams) if (st) (void)hipStreamDestroy(st);
    } MSL_ABI_CATCH_VOID
}

int msl_orb_scale_tables(const msl_orb *h, float *sf, float *isf, float *s2, float *is2) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    for (int i = 0; i < h->nlevels; i++) {
        if (sf) sf[i] = h->scale[i];
        if (isf) isf[i] = h->invScale[i];
        if (s2) s2[i] = h->sigma2[i];
        if (is2) is2[i] = h->invSigma2[i];
    }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_orb_features_per_level(const msl_orb *h, int32_t *out) noexcept {
    try {
    if (!h || !out) return MSL_ERR_INVALID;
    for (int i = 0; i < h->nlevels; i++) out[i] = h->perLevel[i];
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_orb_capacity(const msl_orb *h) noexcept { try { return h ? h->outCap : MSL_ERR_INVALID; } MSL_ABI_CATCH_INT }
int msl_orb_levels(const msl_orb *h) noexcept { try { return h ? h->nlevels : MSL_ERR_INVALID; } MSL_ABI_CATCH_INT }

int msl_orb_set_stream(msl_orb *h, void *hip_stream) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->ownStream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)hip_stream; h->ownStream = false;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_orb_wait_event(msl_orb *h, void *hip_event) noexcept {
    try {
    if (!h || !hip_event) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    MSL_HIP_TRY(hipStreamWaitEvent(h->stream, (hipEvent_t)hip_event, 0));   // (the side stream forks from this one inside every call)
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_orb_sync(msl_orb *h) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    return check_device_error(h);
    } MSL_ABI_CATCH_INT
}

int msl_orb_extract_batch(msl_orb *h, const uint8_t *gray, int n_frames, int width, int height, size_t row_stride,
                          size_t frame_stride, msl_mem in_mem, msl_keypoint *kps, uint8_t *desc32, int cap,
                          int32_t *n_out, msl_mem out_mem) noexcept {
    try {
    if (!h || !n_out || n_frames < 0) { set_error("msl_orb_extract_batch: invalid argument"); return MSL_ERR_INVALID; }
    if (n_frames == 0) return MSL_OK;
    if (!gray || width == 0 || height == 0) {  // empty image: silent return (src/ORBextractor.cc:815-816)
        if (out_mem == MSL_MEM_HOST) for (int f = 0; f < n_frames; f++) n_out[f] = 0;
        else { MSL_HIP_TRY(hipSetDevice(h->device)); MSL_HIP_TRY(hipMemsetAsync(n_out, 0, sizeof(int) * n_frames, h->stream)); }
        return MSL_OK;
    }
    if (n_frames > h->maxBatch || width > h->maxW || height > h->maxH || row_stride < (size_t)width || !kps || !desc32) {
        set_error("msl_orb_extract_batch: frame %dx%d x%d exceeds the handle's limits (%dx%d x%d) or bad pointers", width,
                  height, n_frames, h->maxW, h->maxH, h->maxBatch);
        return MSL_ERR_INVALID;
    }
    const int outCap = h->outCap;
    if (cap < outCap) { set_error("msl_orb_extract_batch: cap %d < required %d", cap, outCap); return MSL_ERR_CAPACITY; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    GrayOnDevice g;
    int rc = ensure_geometry(h, width, height);
    if (rc == MSL_OK) rc = stage_gray(h, gray, n_frames, width, height, row_stride, frame_stride, in_mem, g);
    if (rc != MSL_OK) return rc;
    const OutArray outs[2] = {{kps, h->d_kps, sizeof(msl_keypoint)}, {desc32, h->d_desc, 32}};
    return run_batch(h, g, n_frames, nullptr, outs, 2, cap, n_out, out_mem);
    } MSL_ABI_CATCH_INT
}

// The reference's call pattern: one frame per call, host buffers in and out, the result needed before the caller goes on (src/Frame.cc:100,
// 175-177).  Latency is everything here, so this form avoids every pageable-memory transfer: the frame goes through a pinned staging buffer
// (one CPU copy, one DMA), the counts, keypoints and descriptors come back as ONE copy of the output block into pinned memory next to the
// error word, and a single stream synchronisation ends the call (the batch form issues four device-to-host copies into pageable memory).
static int extract_one_host(msl_orb *h, const uint8_t *gray, int width, int height, size_t stride, msl_keypoint *kps, uint8_t *desc32, int cap, int *n_out) {
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = ensure_geometry(h, width, height);
    if (rc != MSL_OK) return rc;
    const int outCap = h->outCap;
    if (cap < outCap) { set_error("msl_orb_extract: cap %d < required %d", cap, outCap); return MSL_ERR_CAPACITY; }
    const size_t inBytes = h->inPitch * (size_t)height;
    // frame 0's share of the output block: counts (all B of them: a few bytes), its keypoints and -- B == 1 only -- its descriptors contiguous
    const size_t outBytes = h->maxBatch == 1 ? h->geo.outBlock.cap : 0;
    hipStream_t s = h->stream;
    MSL_HIP_TRY(h->h_pinIn.grow(inBytes, s));
    MSL_HIP_TRY(h->h_pinOut.grow(h->outKpsOff + sizeof(msl_keypoint) * (size_t)outCap + (size_t)32 * outCap + 256, s));
    uint8_t *pinIn = (uint8_t *)h->h_pinIn.p, *pinOut = (uint8_t *)h->h_pinOut.p, *d_in = (uint8_t *)h->geo.in.p;
    h->prof.begin(KID_COPY, s);
    // (one copy: splitting it so that the DMA of the first half overlaps the CPU copy of the second measured 6 us SLOWER -- an enqueue costs more than it hides)
    if (stride == h->inPitch) memcpy(pinIn, gray, stride * (size_t)(height - 1) + width);
    else for (int y = 0; y < height; y++) memcpy(pinIn + (size_t)y * h->inPitch, gray + (size_t)y * stride, (size_t)width);
    MSL_HIP_TRY(hipMemcpyAsync(d_in, pinIn, inBytes, hipMemcpyHostToDevice, s));
    h->prof.end(s);
    rc = orb_launch_pipeline(&h->dev, h, d_in, h->inPitch, inBytes, 1, h->d_kps, h->d_desc, h->d_nout, nullptr);
    if (rc != MSL_OK) return rc;
    h->lastFrames = 1;
    const size_t kpsBytes = sizeof(msl_keypoint) * (size_t)outCap, descBytes = (size_t)32 * outCap;
    uint8_t *hk = pinOut + h->outKpsOff, *hd = hk + ((kpsBytes + 255) & ~(size_t)255);
    if (outBytes) {   // a one-frame handle: counts | keypoints | descriptors are one contiguous block
        MSL_HIP_TRY(hipMemcpyAsync(pinOut, h->geo.outBlock.p, outBytes, hipMemcpyDeviceToHost, s));
        hd = pinOut + h->outDescOff;
    } else {
        MSL_HIP_TRY(hipMemcpyAsync(pinOut, h->d_nout, sizeof(int), hipMemcpyDeviceToHost, s));
        MSL_HIP_TRY(hipMemcpyAsync(hk, h->d_kps, kpsBytes, hipMemcpyDeviceToHost, s));
        MSL_HIP_TRY(hipMemcpyAsync(hd, h->d_desc, descBytes, hipMemcpyDeviceToHost, s));
    }
    rc = check_device_error(h);   // error word into pinned memory, then the call's only synchronisation
    if (rc != MSL_OK) { *n_out = 0; return rc; }
    const int n = *reinterpret_cast<const int *>(pinOut);
    memcpy(kps, hk, sizeof(msl_keypoint) * (size_t)n);
    memcpy(desc32, hd, (size_t)32 * n);
    *n_out = n;
    return MSL_OK;
}

int msl_orb_extract(msl_orb *h, const uint8_t *gray, int width, int height, size_t stride, msl_keypoint *kps,
                    uint8_t *desc32, int cap, int *n_out) noexcept {
    try {
    if (!n_out) { set_error("msl_orb_extract: n_out is NULL"); return MSL_ERR_INVALID; }
    if (h && gray && width > 0 && height > 0 && width <= h->maxW && height <= h->maxH && stride >= (size_t)width && kps && desc32)
        return extract_one_host(h, gray, width, height, stride, kps, desc32, cap, n_out);
    int32_t n = 0;
    const int rc = msl_orb_extract_batch(h, gray, 1, width, height, stride, stride * (size_t)height, MSL_MEM_HOST, kps, desc32,
                                         cap, &n, MSL_MEM_HOST);
    *n_out = n;
    return rc;
    } MSL_ABI_CATCH_INT
}

// host twin of the device undistortion (same expression order), used by ComputeImageBounds only
static void undistort_point_host(const msl_frame_params &p, float xin, float yin, float *xo, float *yo) {
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

int msl_frame_image_bounds(msl_frame_params *p, int width, int height) noexcept {
    try {   // ComputeImageBounds, src/Frame.cc:465-494
    if (!p || width < 1 || height < 1 || p->fx == 0 || p->fy == 0) { set_error("msl_frame_image_bounds: invalid argument"); return MSL_ERR_INVALID; }
    if (p->k1 != 0.0) {
        const float c[4][2] = {{0.f, 0.f}, {(float)width, 0.f}, {0.f, (float)height}, {(float)width, (float)height}};
        float u[4][2];
        for (int i = 0; i < 4; i++) undistort_point_host(*p, c[i][0], c[i][1], &u[i][0], &u[i][1]);
        p->minX = std::min(u[0][0], u[2][0]); p->maxX = std::max(u[1][0], u[3][0]);
        p->minY = std::min(u[0][1], u[1][1]); p->maxY = std::max(u[2][1], u[3][1]);
    } else {
        p->minX = 0.0f; p->maxX = (float)width; p->minY = 0.0f; p->maxY = (float)height;
    }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_orb_extract_frame_batch(msl_orb *h, const uint8_t *gray, const float *depth, int n_frames, int width, int height,
                                size_t gray_row_stride, size_t gray_frame_stride, size_t depth_row_stride, size_t depth_frame_stride,
                                msl_mem in_mem, const msl_frame_params *params, msl_keypoint *kps, uint8_t *desc32, float *kps_un_xy,
                                float *depth_out, float *uright_out, int32_t *grid_cell, int cap, int32_t *n_out, msl_mem out_mem) noexcept {
    try {
    if (!h || !gray || !depth || !params || !kps || !desc32 || !kps_un_xy || !depth_out || !uright_out || !grid_cell || !n_out ||
        n_frames < 1 || n_frames > h->maxBatch || width < 1 || height < 1 || width > h->maxW || height > h->maxH ||
        gray_row_stride < (size_t)width || depth_row_stride < (size_t)width * 4 || (depth_row_stride & 3) ||
        !(params->maxX > params->minX) || !(params->maxY > params->minY) || params->fx == 0 || params->fy == 0) {
        set_error("msl_orb_extract_frame_batch: invalid argument (call msl_frame_image_bounds first?)");
        return MSL_ERR_INVALID;
    }
    const int outCap = h->outCap;
    if (cap < outCap) { set_error("msl_orb_extract_frame_batch: cap %d < required %d", cap, outCap); return MSL_ERR_CAPACITY; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = ensure_geometry(h, width, height);
    if (rc != MSL_OK) return rc;
    const size_t B = (size_t)h->maxBatch;
    MSL_HIP_TRY(grow_all(h->stream, {{h->d_unXY, sizeof(float) * 2 * outCap * B}, {h->d_depthOut, sizeof(float) * outCap * B},   // (sized once: outCap and B are fixed)
                                     {h->d_uRight, sizeof(float) * outCap * B}, {h->d_gridCell, sizeof(int) * outCap * B}}));
    GrayOnDevice g;
    rc = stage_gray(h, gray, n_frames, width, height, gray_row_stride, gray_frame_stride, in_mem, g);
    if (rc != MSL_OK) return rc;
    FrameEpilogue ep{};
    ep.fp = *params; ep.depth = depth; ep.depthRowStride = depth_row_stride; ep.depthFrameStride = depth_frame_stride;
    if (in_mem == MSL_MEM_HOST) {
        const size_t dpitch = (size_t)width * 4, dframe = dpitch * height;
        MSL_HIP_TRY(h->d_depthIn.grow(dframe * B, h->stream));
        uint8_t *d_depthIn = (uint8_t *)h->d_depthIn.p;
        for (int f = 0; f < n_frames; f++)
            MSL_HIP_TRY(hipMemcpy2DAsync(d_depthIn + (size_t)f * dframe, dpitch, (const uint8_t *)depth + (size_t)f * depth_frame_stride,
                                         depth_row_stride, dpitch, height, hipMemcpyHostToDevice, h->stream));
        ep.depth = (const float *)d_depthIn; ep.depthRowStride = dpitch; ep.depthFrameStride = dframe;
    }
    const OutArray outs[6] = {{kps, h->d_kps, sizeof(msl_keypoint)}, {desc32, h->d_desc, 32}, {kps_un_xy, h->d_unXY.p, sizeof(float) * 2},
                              {depth_out, h->d_depthOut.p, sizeof(float)}, {uright_out, h->d_uRight.p, sizeof(float)}, {grid_cell, h->d_gridCell.p, sizeof(int)}};
    return run_batch(h, g, n_frames, &ep, outs, 6, cap, n_out, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_orb_debug_stamps(msl_orb *h, uint64_t *out, int n) noexcept {
    try {
    if (!h || !out || n < 0 || n > 200) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    MSL_HIP_TRY(hipMemcpy(out, (const uint8_t *)h->d_err.p + 128, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_orb_debug_level_size(const msl_orb *h, int level, int *w, int *h_out) noexcept {
    try {
    if (!h || level < 0 || level >= h->nlevels) return MSL_ERR_INVALID;
    *w = h->dev.lv[level].w; *h_out = h->dev.lv[level].h;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_orb_debug_level(msl_orb *h, int frame, int level, int blurred, uint8_t *out) noexcept {
    try {
    if (!h || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->lastFrames) return MSL_ERR_INVALID;
    if (level == 0 && !blurred) { set_error("level 0 is the caller's image"); return MSL_ERR_INVALID; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    const LevelDev &G = h->dev.lv[level];
    const uint8_t *src = blurred ? h->dev.blur + (size_t)frame * h->dev.blurStride + G.boff
                                 : h->dev.pyr + (size_t)frame * h->dev.pyrStride + G.off;
    MSL_HIP_TRY(hipMemcpy2D(out, G.w, src, G.pitch, G.w, G.h, hipMemcpyDeviceToHost));
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_orb_debug_candidates(msl_orb *h, int frame, int level, int32_t *xys, int cap, int *n_out) noexcept {
    try {
    if (!h || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->lastFrames) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    int n = 0;
    MSL_HIP_TRY(hipMemcpy(&n, h->dev.ncand + frame * h->nlevels + level, sizeof(int), hipMemcpyDeviceToHost));
    *n_out = n;
    if (n > cap) return MSL_ERR_CAPACITY;
    std::vector<uint32_t> k(n);
    if (n) MSL_HIP_TRY(hipMemcpy(k.data(), h->dev.keys + (size_t)frame * h->dev.keysPerFrame + h->dev.lv[level].keyBase,
                                 sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        xys[3 * i] = (int)(k[i] & 0xFFF) + 16; xys[3 * i + 1] = (int)((k[i] >> 12) & 0xFFF) + 16; xys[3 * i + 2] = (int)(k[i] >> 24);
    }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_orb_profile_enable(msl_orb *h, int on) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    h->prof.drain();
    h->prof.set_mode(on);
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_orb_profile_read(msl_orb *h, float *ms, int32_t *launches) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    h->prof.drain();
    for (int i = 0; i < MSL_ORB_NKERNELS; i++) { if (ms) ms[i] = h->prof.ms[i]; if (launches) launches[i] = h->prof.launches[i]; }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
const char *msl_orb_kernel_name(int k) noexcept { try { return (k >= 0 && k < MSL_ORB_NKERNELS) ? kernel_name(k) : ""; } MSL_ABI_CATCH_PTR }

}  // extern "C"
