// msl_orb_dev.h -- what the ORB extractor's kernels and device driver (msl_orb.hip) and its host side (msl_orb_host.hip) share: the limits, the
// structs the kernels take by value, and the driver's entry points (internal).
#pragma once

#include "msl_common.h"

namespace msl {
namespace orb {

constexpr int ML = 12;          // max pyramid levels
constexpr int MAXCELL = 64;     // max FAST cell extent (pixels)
constexpr int MAXNODE = 1024;   // max quadtree list length per level
constexpr int OCT_NT = 512;     // threads of the quadtree workgroup
constexpr int OCT_NODE_BYTES = 66;   // k_octree's LDS per node slot
constexpr int BT_W = 64, BT_H = 32;  // k_blur's output tile
constexpr int PYR_TAPS = 128;       // k_pyramid: column taps staged per level (a tile's row pitch is below 128 pixels)

// The frame epilogue of one call: intrinsics, the depth frames on the device, and where its four outputs go.
struct FrameEpilogue {
    msl_frame_params fp; const float *depth; size_t depthRowStride, depthFrameStride;
    float *unXY, *depthOut, *uRight; int *gridCell;
};

enum { KID_RESIZE = 0, KID_FAST, KID_OCTREE, KID_BLUR, KID_DESCRIBE, KID_COPY };
const char *kernel_name(int kid);   // the profiler slot's name

// Where a launch sequence runs, and the two launch parameters of the current geometry that are not kernel arguments (the handle's base).
struct OrbLaunch {
    hipStream_t stream = nullptr;
    hipStream_t sideStream = nullptr; hipEvent_t evFork = nullptr, evJoin = nullptr;   // single-frame calls: the blur runs beside FAST + quadtree
    KernelProfiler prof;
    size_t pyrLds = 0;     // k_pyramid: dynamic LDS bytes
    size_t fastLds = 0;    // k_fast: dynamic LDS bytes (the largest cell of the geometry)
    bool octBig = false;   // frames of more than 640 x 480 x 1.5 pixels: level 0 may hold more than 8192 FAST candidates -> k_octree<32>
};

// k_fast's LDS for one cw x ch cell (one wave): the (ch + 6)-row pixel tile with a word pitch of tp bytes, the (cw + 2) x (ch + 2) score image
// with its zero border, and the list of the pixels that pass the quick test (two bytes each, at most all of them).  tp leaves two words beyond
// the last group of four pixels: the quick test reads three words per row.  Every part grows with cw and ch, so the level's wCell x hCell bounds
// all of its cells.
struct FastLds { int tp, sp, scoreOff, listOff, bytes; };
__host__ __device__ inline FastLds fast_lds(int cw, int ch) {
    FastLds f;
    f.tp = 4 * ((cw + 3) >> 2) + 8; f.sp = cw + 2;
    f.scoreOff = f.tp * (ch + 6);
    f.listOff = (f.scoreOff + f.sp * (ch + 2) + 3) & ~3;
    f.bytes = f.listOff + 2 * cw * ch;
    return f;
}

// k_octree's dynamic LDS beyond what a launch gets by default (a large feature budget); called when a geometry is committed.
int allow_octree_lds(int octLds);

}  // namespace orb
}  // namespace msl

// The structs the kernels take.  They stay in an unnamed namespace, where they were while kernels and host code were one file: a kernel's symbol
// carries the name of its parameter type, and with the same symbols the gfx950 code object stays what it was, byte for byte (profiles/README.md).
// Both files see this one definition; the driver's entry point that takes an OrbDev therefore has C linkage (a C++ one would be local to its file).
namespace {

struct LevelDev {
    int w, h, pitch;
    unsigned off;       // byte offset inside one frame's pyramid store (levels >= 1)
    unsigned boff;      // byte offset inside one frame's blurred store
    int nCols, nRows, wCell, hCell;
    int cellBase, nCells;
    int keyBase, keyCap;
    int quota;
    int nIni; float hX;
    float scale; int patch;
    unsigned xtabOff, ytabOff;  // element offsets into the resize tables
    int tileBase, tilesX, tilesY;  // blur tiling
};

struct CellDev {
    short level, x0, y0, cw, ch, _pad;
    unsigned keyOff;  // first key slot of the cell (frame relative)
};

struct alignas(8) ResizeTap { short s0, s1, c0, c1; };   // (8-byte loads: k_pyramid fetches four adjacent entries per lane)
// one axis of one tile on one level of the fused pyramid: the pixels the tile owns (writes to HBM) and the pixels it has to compute
// because its share of the next level reads them (level 0: the input pixels it loads)
struct PyrRange { short ownLo, ownHi, needLo, needHi; };

struct OrbDev {
    int nlevels, iniTh, minTh;
    int cellsPerFrame, keysPerFrame, selCap, outCap, blurTiles;
    unsigned long long pyrStride, blurStride;
    LevelDev lv[msl::orb::ML];
    int umax[16];
    const uint8_t *in; unsigned long long inRowStride, inFrameStride;
    uint8_t *pyr, *blur;
    const CellDev *cells;
    const ResizeTap *taps;
    const PyrRange *pyrX, *pyrY;   // fused pyramid: [level][tile column] / [level][tile row] ranges (pyrTX == 0: one launch per level)
    int pyrTX, pyrTY; unsigned pyrBuf0, pyrTapOff;   // bytes of the first LDS buffer; where the staged column taps start (behind the second)
    uint32_t *cellCnt, *cellKeys, *keys;
    uint16_t *knode;
    uint32_t *sel; int *nsel, *ncand;
    msl_keypoint *kps; uint8_t *desc; int *nout; int *err;
    // Frame post-ORB epilogue; frameOn == 0: plain extractor
    int frameOn;
    msl_frame_params fp; float gridWInv, gridHInv;
    const float *depth; unsigned long long depthRowStride, depthFrameStride;   // bytes
    float *unXY, *depthOut, *uRight; int *gridCell;
    int nFrames;   // frames of this launch sequence (the kernels run 1-D, XCD-aware grids: xcd_item)
    int maxNode;   // k_octree: node-array length
    int octLds;    // k_octree: dynamic LDS bytes = max(OCT_NODE_BYTES * maxNode, 8 * (cells of the largest level + 1))
    const LevelDev *lvDev;   // lv[] on the device (uploaded once per geometry): for kernels that take slim arguments
};

// What k_octree takes instead of the whole OrbDev (1.3 KB): the arrays it touches and a few scalars.  A workgroup reads its level's record from
// lv with scalar loads.
struct OctArgs {
    const uint32_t *cellCnt, *cellKeys; const CellDev *cells; const LevelDev *lv;
    uint32_t *keys; uint16_t *knode; uint32_t *sel; int *nsel, *ncand, *err;
    int cellsPerFrame, keysPerFrame, nlevels, nFrames, selCap, maxNode;
};

}  // namespace

// Launch the whole pipeline for n frames whose pixels are already on the device.
extern "C" int orb_launch_pipeline(const OrbDev *dev, msl::orb::OrbLaunch *q, const uint8_t *d_gray, size_t rowStride, size_t frameStride, int n,
                                       msl_keypoint *d_kps, uint8_t *d_desc, int *d_nout, const msl::orb::FrameEpilogue *ep);
