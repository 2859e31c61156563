// msl_peac_host.h -- what the plane extractor's device driver (msl_peac.hip) and its host stage (msl_peac_host.hip) share: the description of
// one call, the packed hand-over of k_peac_cluster, and the frame-parallel host steps (internal).
#pragma once

#include "msl_common.h"

namespace msl {
namespace peac {

// The images of one call as the caller handed them over, and the geometry check_call derives from them.
struct PeacImages {
    int device = 0;                          // (the *_from_blocks forms have none)
    const uint16_t *depth = nullptr;
    size_t stride = 0, frameStride = 0;      // bytes
    int width = 0, height = 0, n_frames = 0;
    msl_mem mem = MSL_MEM_HOST;
    float fx = 0, fy = 0, cx = 0, cy = 0, factor = 0;
    // derived: the half-resolution cloud is ceil(cols / 2.0) x ceil(rows / 2.0) (src/PlaneExtractor.cpp:51-52), cut into Nw x Nh windows
    int cw = 0, ch = 0, Nw = 0, Nh = 0;
    size_t nBlocks = 0, nVert = 0;           // per frame
};

// Where the host stage's results go: the membership image and the plane counts, and -- optionally -- what PlaneDetection hands on beyond them
// (extractedPlanes: planes [frames][maxPlanes]; plane_vertices_: offsets [frames][maxPlanes + 1], indices [frames][ch * cw])
struct PeacOutputs {
    int32_t *membership = nullptr, *nPlanes = nullptr;
    int maxPlanes = 0;
    msl_peac_plane *planes = nullptr;
    int32_t *offsets = nullptr, *indices = nullptr;
};

// Every argument test of a call, and the derived fields of I.  hostEntry: the name of a *_from_blocks entry point, or nullptr for a call that runs
// the device kernels (those also refuse what k_peac_fit cannot take).  O: nullptr for the entry points without a membership image.
int check_call(PeacImages &I, const msl_peac_params *prm, const PeacOutputs *O, const char *hostEntry);

// One plane k_peac_cluster extracted
struct PlaneOut { double st[9], center[3], normal[3], mse; int32_t id, N, rid, _pad; };

// The packed hand-over of k_peac_cluster, as offsets in ints.  Input: [frames][nB] initial heap, [frames] heap sizes, [frames][maxE][2] initial
// edges, [frames] edge counts.  Output: [frames] plane counts (-1: more than maxPl), [frames][nB] disjoint-set parents, [frames][nB] set sizes,
// then -- 8-byte aligned -- [frames][maxPl] PlaneOut.
struct ClusterLayout {
    size_t nB; int maxE, maxPl;
    size_t heap, heapCount, edges, edgeCount, inInts;
    size_t nPlanes, parent, setSize, outInts, planes /* rounded up to an even number of ints */, outBytes;
    ClusterLayout(int n_frames, size_t nBlocks, int maxE_, int maxPl_) : nB(nBlocks), maxE(maxE_), maxPl(maxPl_) {
        const size_t F = (size_t)n_frames;
        heap = 0; heapCount = heap + F * nB; edges = heapCount + F; edgeCount = edges + F * 2 * (size_t)maxE; inInts = edgeCount + F;
        nPlanes = 0; parent = nPlanes + F; setSize = parent + F * nB; outInts = setSize + F * nB;
        planes = (outInts + 1) & ~(size_t)1; outBytes = sizeof(int) * planes + sizeof(PlaneOut) * F * (size_t)maxPl;
    }
};

// The PEAC environment switches, read once per process.
struct PeacEnv {
    int timing;            // MSL_PEAC_TIMING: 0 = unset, 1 = per-call lines on stderr, 2 = per-frame lines as well
    int simd;              // MSL_PEAC_SIMD = 0 / 2 / 4 / 8 lowers the instruction set the SIMD lanes may use; -1: unset
    int lanes;             // MSL_PEAC_LANES = 2 / 4 / 8 caps the candidates per group; 16 otherwise
    bool threadsSet; int threads;   // MSL_PEAC_THREADS overrides the worker count (1 = everything on the calling thread)
    int localRanks;        // LOCAL_WORLD_SIZE (set by torch.distributed.run): the ranks that share the node's CPUs, at least 1
    bool strictThreads;    // MSL_PEAC_STRICT_THREADS: a worker thread that cannot be started fails the call
    bool poolReport;       // MSL_PEAC_POOL_REPORT: the pool prints its worker count when it is created
};
const PeacEnv &peac_env();

int peac_workers();   // threads the host stage runs a call's frames on (the caller included)

// The frame-parallel host steps; blocks [frames][nBlocks], half [frames][ch][cw] (raw depth of the cloud vertices).
// The whole host stage: graph initialisation, clustering, erosion, region growing.  Returns a status (MSL_ERR_CAPACITY: more than maxPlanes planes).
int segment_frames(const PeacImages &I, const msl_peac_params &prm, const msl_peac_block *blocks, const uint16_t *half, const PeacOutputs &O);
// Device clustering, before: graph initialisation only, the initial heaps and edge lists packed into cin [L.inInts].  False when a frame's edge
// list does not fit.
bool graphs_for_device(const PeacImages &I, const msl_peac_params &prm, const msl_peac_block *blocks, const ClusterLayout &L, int *cin);
// Device clustering, after: erosion, region growing and the final merge on the planes and disjoint sets k_peac_cluster left (cout [L.outInts]).
int finish_from_device(const PeacImages &I, const msl_peac_params &prm, const uint16_t *half, const ClusterLayout &L, const int *cout, const PlaneOut *planes,
                       const PeacOutputs &O);

}  // namespace peac
}  // namespace msl
