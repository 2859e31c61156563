// msl_peac.hip -- the PEAC plane extractor, producer of SurfelFusion's plane-membership image: the device kernels, the
// per-device state and the driver of the entry points that take a device.
//
// Replaces PlaneDetection::readDepthImage + runPlaneDetection (reference src/PlaneExtractor.cpp:44-81), i.e.
// ahc::PlaneFitter<ImagePointCloud>::run (include/peac/AHCPlaneFitter.hpp:218-262) with the reference's default parameters.
//
//   GPU (frame-batched, FP64; the same operations in the same order as the host arithmetic of the reference, ties among exactly equal merge costs
//   resolved by node creation order where the reference depends on heap addresses -- DESIGN.md section 3):
//     k_peac_cloud  organised half-resolution cloud (src/PlaneExtractor.cpp:60-74), only when the caller asks for it
//     k_peac_half   the raw depth of the cloud's vertices, packed: what the host stage reads
//     k_peac_fit    ONE WAVE PER WINDOW: the lanes evaluate the window's points in parallel -- missing data, depth discontinuity
//                   towards the right / lower neighbour (include/peac/AHCPlaneSeg.hpp:237-285, :41-43), the nine products of
//                   Stats::push (:81-92) -- and stage the products in LDS; nine lanes then add one statistic each in window
//                   raster order (the reference's summation order, so the FP64 sums are the reference's bit for bit); one lane
//                   runs the PCA plane fit (Stats::compute, :148-183) with the 3x3 symmetric eigen-solve of
//                   include/peac/eig33sym.hpp:71-75 (Eigen::SelfAdjointEigenSolver, restated in msl_peac_math.h).
//     k_peac_cluster ONE WAVE PER FRAME: the agglomerative clustering (AHCPlaneFitter.hpp:939-1143).  A sequential chain of pops, but every pop fits a
//                   plane for each neighbour of the popped node (one per lane); binary heap and disjoint set in LDS, neighbour sets as a bit matrix.
//   Host (msl_peac_host.hip): graph initialisation, then -- after the device clustering -- erosion, region growing, final merge and relabelling; and
//   the whole clustering for the calls that do not cluster on the device (cluster_on_device below says which).
//
// A call is fit_and_fetch (block fits, half depth and the optional cloud to the host), cluster_on_device where it applies, and one of the two host
// finishes.  All device state lives in one PeacState per device, behind one mutex and one lookup (peac_state).
#include "msl_peac_host.h"
#include "msl_peac_math.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

namespace {
using namespace msl;
using namespace msl::peac;

struct PeacDev {
    const uint16_t *depth;
    size_t strideBytes, frameStrideBytes;
    int width, height, cw, ch;             // full-resolution image, half-resolution cloud
    float fx, fy, cx, cy, factor;
    int winW, winH, Nw, Nh, loose;
    double alpha, tol;
    double *cloud;                         // [frames][ch * cw][3] or nullptr
    msl_peac_block *blocks;                // [frames][Nh * Nw]
};

__global__ __launch_bounds__(256) void k_peac_cloud(PeacDev P) {
    const int frame = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.cw * P.ch) return;
    const int row = i / P.cw, col = i - row * P.cw;
    const uint16_t *img = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(P.depth) + (size_t)frame * P.frameStrideBytes);
    const double z = vertex_z(img, P.strideBytes, P.factor, row, col);
    double x, y;
    vertex_xy(P.fx, P.fy, P.cx, P.cy, row, col, z, x, y);
    double *o = P.cloud + ((size_t)frame * P.cw * P.ch + i) * 3;
    o[0] = x; o[1] = y; o[2] = z;
}

// Raw depth of the cloud's vertices (even rows / columns) packed to [frames][ch][cw]: what the host-side region growing reads --
// a quarter of the image, so device-resident input costs one small copy instead of the whole frame.
__global__ __launch_bounds__(256) void k_peac_half(PeacDev P, uint16_t *out) {
    const int frame = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.cw * P.ch) return;
    const int row = i / P.cw, col = i - row * P.cw;
    const uint8_t *img = reinterpret_cast<const uint8_t *>(P.depth) + (size_t)frame * P.frameStrideBytes;
    out[(size_t)frame * P.cw * P.ch + i] = *reinterpret_cast<const uint16_t *>(img + (size_t)(2 * row) * P.strideBytes + 2 * (size_t)(2 * col));
}

// One wave per window.  LDS: nine arrays of winW * winH products (a missing point contributes +0.0, which leaves every partial
// sum unchanged, so the additions that matter happen in the reference's raster order).
__global__ __launch_bounds__(64) void k_peac_fit(PeacDev P) {
    extern __shared__ double s_term[];   // [9][win]
    const int frame = blockIdx.y, b = blockIdx.x, lane = threadIdx.x;
    const uint16_t *img = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(P.depth) + (size_t)frame * P.frameStrideBytes);
    const int seedRow = (b / P.Nw) * P.winH, seedCol = (b % P.Nw) * P.winW, win = P.winW * P.winH;
    int nMissing = 0, nPushed = 0;
    bool broken = false;   // a valid point with a depth discontinuity towards its right / lower neighbour
    for (int p = lane; p < win; p += 64) {
        const int i = seedRow + p / P.winW, j = seedCol + p % P.winW;
        const double z = vertex_z(img, P.strideBytes, P.factor, i, j);
        double x = 0, y = 0;
        const bool has = z != 0;   // ImagePointCloud::get (include/PlaneExtractor.h:47-55): a 16-bit depth times a float is never NaN
        if (has) {
            vertex_xy(P.fx, P.fy, P.cx, P.cy, i, j, z, x, y);
            if (j + 1 < P.cw) { const double zn = vertex_z(img, P.strideBytes, P.factor, i, j + 1); if (zn != 0 && fabs(z - zn) > P.alpha * fabs(z) + P.tol) broken = true; }
            if (i + 1 < P.ch) { const double zn = vertex_z(img, P.strideBytes, P.factor, i + 1, j); if (zn != 0 && fabs(z - zn) > P.alpha * fabs(z) + P.tol) broken = true; }
            nPushed++;
        } else {
            nMissing++;
        }
        const double zz = has ? z : 0.0;
        s_term[0 * win + p] = x; s_term[1 * win + p] = y; s_term[2 * win + p] = zz;
        s_term[3 * win + p] = x * x; s_term[4 * win + p] = y * y; s_term[5 * win + p] = zz * zz;
        s_term[6 * win + p] = x * y; s_term[7 * win + p] = y * zz; s_term[8 * win + p] = x * zz;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { nMissing += __shfl_xor(nMissing, d, 64); nPushed += __shfl_xor(nPushed, d, 64); }
    // INIT_STRICT: any missing point rejects the window; INIT_LOOSE: the nanCntTh-th missing point does (AHCPlaneSeg.hpp:245-257)
    const bool valid = !__any(broken) && (P.loose ? nMissing < win / 2 : nMissing == 0);
    __builtin_amdgcn_wave_barrier();
    double sum = 0.0;
    if (valid && lane < 9) {
        const double *t = s_term + lane * win;
        for (int p = 0; p < win; p++) sum += t[p];   // Stats::push order (:81-92)
    }
    msl_peac_stats S;
    S.sx = __shfl(sum, 0, 64); S.sy = __shfl(sum, 1, 64); S.sz = __shfl(sum, 2, 64);
    S.sxx = __shfl(sum, 3, 64); S.syy = __shfl(sum, 4, 64); S.szz = __shfl(sum, 5, 64);
    S.sxy = __shfl(sum, 6, 64); S.syz = __shfl(sum, 7, 64); S.sxz = __shfl(sum, 8, 64);
    S.N = valid ? nPushed : 0; S.nouse = valid ? 0 : 1;
    if (lane != 0) return;
    msl_peac_block B;
    B.stats = S;
    B.center[0] = B.center[1] = B.center[2] = B.normal[0] = B.normal[1] = B.normal[2] = 0;
    if (S.N < 4) B.mse = B.curvature = __longlong_as_double(0x7FF8000000000000ll);   // quiet NaN (:279-280)
    else plane_fit(S, B.center, B.normal, B.mse, B.curvature);
    P.blocks[(size_t)frame * P.Nw * P.Nh + b] = B;
}

// ---- agglomerative clustering on the device: one wave per frame ----------------------------------------------------------------------------
// ahCluster (AHCPlaneFitter.hpp:939-1143) is a sequential chain of pops, but every pop evaluates ALL neighbours of the popped node (a plane fit
// each: ~30 000 3x3 eigen-solves per 640x480 frame) -- that part is data parallel, and frames are independent.  One wave per frame: lane 0 keeps the
// reference's binary heap (libstdc++ push_heap / pop_heap spelled out, so the pop order is the reference's even among equal keys) and the disjoint
// set in LDS; the neighbours of the popped node are fitted one per lane with the same __host__ __device__ code the host uses (so the same bits),
// the reference's first-minimum rule picks the merge, and the adjacency -- a bit matrix, whose ascending bit order is the reference's ordered
// neighbour set -- is updated by all lanes.  The host supplies the initial heap and edges (graph initialisation needs cos()) and continues with the
// extracted planes (erosion, FIFO region growing: order dependent pixel work that stays on the host).
struct ClusterDev {
    int nB, maxN, words, minSupport, maxStep, maxE, maxPl;
    double depthSigma, stdTolMerge, simMerge;
    const msl_peac_block *blocks;   // [frames][nB]
    unsigned *rows;                 // [frames][maxN][words] adjacency bit matrix
    double *gst;                    // [frames][maxN][9] statistics of every node
    double *gcxy;                   // [frames][maxN][2] centre x, y (output only)
    const int *heap0, *heapCount;   // [frames][nB], [frames] initial heap
    const int *edges, *edgeCount;   // [frames][maxE][2], [frames] initial edges
    int *nPlanes; PlaneOut *planes; // [frames] (-1: more than maxPl), [frames][maxPl] extracted planes in extraction order
    int *parent, *setSize;          // [frames][nB] disjoint set after the clustering
};
__device__ __forceinline__ unsigned ld_ag(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_ag(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_agd(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agd(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Minimum of a double over the 64 lanes (DPP row shifts and row broadcasts, as msl::wave_incl_scan; lanes without a source see +inf); every lane gets it.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_min_step(double v) {
    const unsigned long long u = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, ROWMASK, 0xF, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)0x7FF00000, (int)(unsigned)(u >> 32), CTRL, ROWMASK, 0xF, false);
    return fmin(v, __longlong_as_double(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave_min_d(double v) {
    v = dpp_min_step<0x111, 0xF>(v); v = dpp_min_step<0x112, 0xF>(v); v = dpp_min_step<0x114, 0xF>(v); v = dpp_min_step<0x118, 0xF>(v);
    v = dpp_min_step<0x142, 0xA>(v);   // row_bcast:15 -> rows 1, 3
    v = dpp_min_step<0x143, 0xC>(v);   // row_bcast:31 -> rows 2, 3
    return __shfl(v, 63, 64);
}

__global__ __launch_bounds__(64) void k_peac_cluster(ClusterDev C) {
    extern __shared__ double s_mem[];
    const int f = blockIdx.x, lane = threadIdx.x, nB = C.nB, maxN = C.maxN, words = C.words;
    double *s_mse = s_mem, *s_nx = s_mse + maxN, *s_ny = s_nx + maxN, *s_nz = s_ny + maxN, *s_cz = s_nz + maxN;
    double *s_hkey = s_cz + maxN;   // MSE of the node in heap slot i (saves the dependent s_mse[s_heap[i]] read on every comparison)
    int *s_N = reinterpret_cast<int *>(s_hkey + maxN), *s_rid = s_N + maxN, *s_heap = s_rid + maxN, *s_cand = s_heap + maxN;
    int *s_parent = s_cand + maxN, *s_size = s_parent + nB;
    uint8_t *s_nouse = reinterpret_cast<uint8_t *>(s_size + nB);
    unsigned *rows = C.rows + (size_t)f * maxN * words;
    double *gst = C.gst + (size_t)f * maxN * 9, *gcxy = C.gcxy + (size_t)f * maxN * 2;
    const msl_peac_block *blocks = C.blocks + (size_t)f * nB;
    PlaneOut *planes = C.planes + (size_t)f * C.maxPl;
    for (int b = lane; b < nB; b += 64) {
        const msl_peac_block &B = blocks[b];
        const bool nouse = B.stats.nouse != 0;
        s_mse[b] = B.mse; s_nx[b] = B.normal[0]; s_ny[b] = B.normal[1]; s_nz[b] = B.normal[2]; s_cz[b] = B.center[2];
        s_nouse[b] = nouse ? 1 : 0; s_N[b] = nouse ? 0 : B.stats.N; s_rid[b] = b; s_parent[b] = b; s_size[b] = 1;
        double *g = gst + (size_t)b * 9;
        g[0] = B.stats.sx; g[1] = B.stats.sy; g[2] = B.stats.sz; g[3] = B.stats.sxx; g[4] = B.stats.syy; g[5] = B.stats.szz; g[6] = B.stats.sxy; g[7] = B.stats.syz; g[8] = B.stats.sxz;
        gcxy[2 * b] = B.center[0]; gcxy[2 * b + 1] = B.center[1];
    }
    int hcount = C.heapCount[f];
    for (int i = lane; i < hcount; i += 64) { const int id = C.heap0[(size_t)f * nB + i]; s_heap[i] = id; s_hkey[i] = blocks[id].mse; }
    {
        const int ne = C.edgeCount[f];
        const int *E = C.edges + (size_t)f * C.maxE * 2;
        for (int e = lane; e < ne; e += 64) {
            const int a = E[2 * e], b = E[2 * e + 1];
            atomicOr(&rows[(size_t)a * words + (b >> 5)], 1u << (b & 31));
            atomicOr(&rows[(size_t)b * words + (a >> 5)], 1u << (a & 31));
        }
    }
    __threadfence();   // (once: the plain initialisation stores above become visible to the agent-scope accesses below)
    __syncthreads();
    int nNodes = nB, nPl = 0, step = 0;
    // the set bits of `words` words held one per lane (chunks of 64 words), ascending, into s_cand; returns their number
    auto list_bits = [&](auto word_of) -> int {
        int base = 0;
        for (int w0 = 0; w0 < words; w0 += 64) {
            const int w = w0 + lane;
            unsigned bits = w < words ? word_of(w) : 0u;
            const unsigned cnt = (unsigned)__popc(bits);
            const unsigned incl = wave_incl_scan(cnt);
            int o = base + (int)(incl - cnt);
            while (bits) { const int b = __ffs((int)bits) - 1; bits &= bits - 1; s_cand[o++] = w * 32 + b; }
            base += __shfl((int)incl, 63, 64);
        }
        __syncthreads();
        return base;
    };
    // PlaneSegMinMSECmp(a, b) = mse[b] < mse[a]; comp(parent, value) in __push_heap reads "value's key < parent's key"
    auto heap_push = [&](int id, double key) {   // std::push_heap (libstdc++ __push_heap), lane 0
        int hole = hcount++;
        int parent = (hole - 1) / 2;
        while (hole > 0 && key < s_hkey[parent]) { s_heap[hole] = s_heap[parent]; s_hkey[hole] = s_hkey[parent]; hole = parent; parent = (hole - 1) / 2; }
        s_heap[hole] = id; s_hkey[hole] = key;
    };
    auto heap_pop = [&]() -> int {   // top, then std::pop_heap (libstdc++ __pop_heap / __adjust_heap) + pop_back, lane 0
        const int top = s_heap[0];
        const int len = --hcount;
        if (len > 0) {
            const int value = s_heap[len];
            const double vkey = s_hkey[len];
            int hole = 0, child = 0;
            while (child < (len - 1) / 2) {
                child = 2 * (child + 1);
                if (s_hkey[child - 1] < s_hkey[child]) child--;   // comp(first[child], first[child - 1])
                s_heap[hole] = s_heap[child]; s_hkey[hole] = s_hkey[child]; hole = child;
            }
            if ((len & 1) == 0 && child == (len - 2) / 2) { child = 2 * (child + 1); s_heap[hole] = s_heap[child - 1]; s_hkey[hole] = s_hkey[child - 1]; hole = child - 1; }
            int parent = (hole - 1) / 2;
            while (hole > 0 && vkey < s_hkey[parent]) { s_heap[hole] = s_heap[parent]; s_hkey[hole] = s_hkey[parent]; hole = parent; parent = (hole - 1) / 2; }
            s_heap[hole] = value; s_hkey[hole] = vkey;
        }
        return top;
    };
    auto ds_find = [&](int x) { while (s_parent[x] != x) { s_parent[x] = s_parent[s_parent[x]]; x = s_parent[x]; } return x; };
    auto emit_plane = [&](int p) {   // extractedPlanes.push_back
        if (nPl >= C.maxPl) { nPl++; return; }
        PlaneOut &O = planes[nPl];
        if (lane < 9) O.st[lane] = ld_agd(&gst[(size_t)p * 9 + lane]);
        if (lane == 9) { O.center[0] = ld_agd(&gcxy[2 * p]); O.center[1] = ld_agd(&gcxy[2 * p + 1]); O.center[2] = s_cz[p]; }
        if (lane == 10) { O.normal[0] = s_nx[p]; O.normal[1] = s_ny[p]; O.normal[2] = s_nz[p]; O.mse = s_mse[p]; }
        if (lane == 11) { O.id = p; O.N = s_N[p]; O.rid = s_rid[p]; O._pad = 0; }
        nPl++;
    };
    // Rows, statistics and centres are read and written at agent scope (L2) only, so program order within the wave plus completion of
    // the outstanding stores / atomics is all the ordering the next step needs -- no cache write-back or invalidation.
    auto drain = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
    auto isolate = [&](int p, int nc) {   // the neighbours of p are s_cand[0..nc)
        const unsigned clr = ~(1u << (p & 31));
        for (int i = lane; i < nc; i += 64) atomicAnd(&rows[(size_t)s_cand[i] * words + (p >> 5)], clr);
        for (int w = lane; w < words; w += 64) st_ag(&rows[(size_t)p * words + w], 0u);
        drain();
    };
    while (hcount > 0 && step <= C.maxStep) {
        int p = 0;
        if (lane == 0) p = heap_pop();
        p = __shfl(p, 0, 64);
        hcount = __shfl(hcount, 0, 64);
        __syncthreads();
        if (s_nouse[p]) continue;
        const int nc = list_bits([&](int w) { return ld_ag(&rows[(size_t)p * words + w]); });
        // every candidate merge fitted by one lane; the reference's rule (first strict minimum of the MSE, ascending neighbour order) picks one
        bool have = false;
        double bMse = 0, bC0 = 0, bC1 = 0, bC2 = 0, bN0 = 0, bN1 = 0, bN2 = 0;
        int bNb = -1, bN = 0;
        const double pnx = s_nx[p], pny = s_ny[p], pnz = s_nz[p];
        double ps[9];
#pragma unroll
        for (int k = 0; k < 9; k++) ps[k] = ld_agd(&gst[(size_t)p * 9 + k]);
        const int pN = s_N[p];
        for (int c0 = 0; c0 < nc; c0 += 64) {
            const int ci = c0 + lane;
            const bool in = ci < nc;
            const int nb = in ? s_cand[ci] : p;
            const bool pass = in && fabs(pnx * s_nx[nb] + pny * s_ny[nb] + pnz * s_nz[nb]) >= C.simMerge;
            double mMse = 0, cen[3] = {0, 0, 0}, nrm[3] = {0, 0, 0};
            int mN = 0;
            if (pass) {
                msl_peac_stats t;
                double y[9];
#pragma unroll
                for (int k = 0; k < 9; k++) y[k] = ld_agd(&gst[(size_t)nb * 9 + k]);
                t.sx = ps[0] + y[0]; t.sy = ps[1] + y[1]; t.sz = ps[2] + y[2]; t.sxx = ps[3] + y[3]; t.syy = ps[4] + y[4]; t.szz = ps[5] + y[5];
                t.sxy = ps[6] + y[6]; t.syz = ps[7] + y[7]; t.sxz = ps[8] + y[8]; t.N = pN + s_N[nb]; t.nouse = 0;
                double curv;
                plane_fit(t, cen, nrm, mMse, curv);
                mN = t.N;
            }
            const unsigned long long pm = __ballot(pass);
            const int lim = min(64, nc - c0);
            int jBest = -1;
            // The rule walks the candidates in order and keeps the first strict minimum.  Without NaNs and without ties that is the lane of the
            // wave-wide minimum; anything else (never seen on real data) replays the walk literally.
            const double minv = wave_min_d(pass ? mMse : __builtin_inf());
            const unsigned long long eq = __ballot(pass && mMse == minv), nanm = __ballot(pass && mMse != mMse);
            if (pm && !nanm && __popcll(eq) == 1 && !(have && (bMse == minv || bMse != bMse))) {
                if (!have || bMse > minv) { jBest = __ffsll((long long)eq) - 1; have = true; bMse = minv; bN = __shfl(mN, jBest, 64); }
            } else {
                for (int j = 0; j < lim; j++) {
                    if (!((pm >> j) & 1ull)) continue;
                    const double m = __shfl(mMse, j, 64);
                    if (!have || bMse > m || (bMse == m && (double)bN < m)) { have = true; bMse = m; bN = __shfl(mN, j, 64); jBest = j; }   // (sic: N against mse, :1005)
                }
            }
            if (jBest >= 0) {   // the best so far lies in this chunk: fetch the rest of its fit
                bNb = __shfl(nb, jBest, 64);
                bC0 = __shfl(cen[0], jBest, 64); bC1 = __shfl(cen[1], jBest, 64); bC2 = __shfl(cen[2], jBest, 64);
                bN0 = __shfl(nrm[0], jBest, 64); bN1 = __shfl(nrm[1], jBest, 64); bN2 = __shfl(nrm[2], jBest, 64);
            }
        }
        const double tm = C.depthSigma * bC2 * bC2 + C.stdTolMerge;   // ParamSet::T_mse(P_MERGING): pow(.., 2) is the product
        if (have && bMse < tm * tm) {
            const int id = nNodes++, nb = bNb;
            if (lane < 9) st_agd(&gst[(size_t)id * 9 + lane], ld_agd(&gst[(size_t)p * 9 + lane]) + ld_agd(&gst[(size_t)nb * 9 + lane]));
            if (lane == 0) {
                s_mse[id] = bMse; s_nx[id] = bN0; s_ny[id] = bN1; s_nz[id] = bN2; s_cz[id] = bC2; s_N[id] = bN; s_nouse[id] = 0;
                s_rid[id] = s_N[p] >= s_N[nb] ? s_rid[p] : s_rid[nb];
                st_agd(&gcxy[2 * id], bC0); st_agd(&gcxy[2 * id + 1], bC1);
                heap_push(id, bMse);
                // mergeNbsFrom (AHCPlaneSeg.hpp:398-436): union of the two disjoint sets
                const int xr = ds_find(s_rid[p]), yr = ds_find(s_rid[nb]);
                if (xr != yr) {
                    if (s_size[xr] < s_size[yr]) { s_parent[xr] = yr; s_size[yr] += s_size[xr]; }
                    else { s_parent[yr] = xr; s_size[xr] += s_size[yr]; }
                }
                s_nouse[p] = 1; s_nouse[nb] = 1;
            }
            hcount = __shfl(hcount, 0, 64);
            // neighbours of the new node = union of both neighbour sets without the two merged nodes; both old rows are cleared
            const int nu = list_bits([&](int w) {
                unsigned u = ld_ag(&rows[(size_t)p * words + w]) | ld_ag(&rows[(size_t)nb * words + w]);
                if (w == (p >> 5)) u &= ~(1u << (p & 31));
                if (w == (nb >> 5)) u &= ~(1u << (nb & 31));
                st_ag(&rows[(size_t)id * words + w], u);
                st_ag(&rows[(size_t)p * words + w], 0u); st_ag(&rows[(size_t)nb * words + w], 0u);
                return u;
            });
            for (int i = lane; i < nu; i += 64) {
                unsigned *r = rows + (size_t)s_cand[i] * words;
                atomicOr(&r[id >> 5], 1u << (id & 31));
                atomicAnd(&r[p >> 5], ~(1u << (p & 31)));
                atomicAnd(&r[nb >> 5], ~(1u << (nb & 31)));
            }
            drain();
        } else {
            if (s_N[p] >= C.minSupport) emit_plane(p);
            isolate(p, nc);
        }
        __syncthreads();
        ++step;
    }
    while (hcount > 0) {   // (only reached when max_step stopped the loop above; the reference does not test nouse here either)
        int p = 0;
        if (lane == 0) p = heap_pop();
        p = __shfl(p, 0, 64);
        hcount = __shfl(hcount, 0, 64);
        __syncthreads();
        if (s_N[p] >= C.minSupport) emit_plane(p);
        const int nc = list_bits([&](int w) { return ld_ag(&rows[(size_t)p * words + w]); });
        isolate(p, nc);
        __syncthreads();
    }
    if (lane == 0) C.nPlanes[f] = nPl <= C.maxPl ? nPl : -1;
    for (int b = lane; b < nB; b += 64) { C.parent[(size_t)f * nB + b] = s_parent[b]; C.setSize[(size_t)f * nB + b] = s_size[b]; }
}

// ---- per-device state ----------------------------------------------------------------------------------------------------------------------
// What a device keeps between calls.  One per device, created by its first call and never destroyed (see DevBuf in msl_common.h); every use is
// under g_stateMutex.
struct PeacState {
    // The extractor's own stream (non-blocking, highest priority): its few small kernels and copies must neither wait for nor hold up the frame-batched
    // ORB / surfel work queued on the device.  Work the caller enqueued on the legacy default stream before the call is still ordered first (event).
    hipStream_t stream = nullptr; hipEvent_t ev = nullptr;
    DevBuf depth, blocks, cloud, half;      // staged host images, block fits, organised cloud, packed vertex depths
    DevBuf rows, gst, gcxy, cin, cout;      // device clustering (k_peac_cluster)
    bool clusterLdsSet = false;             // k_peac_cluster's dynamic-LDS limit is raised
};
PeacState *g_state[16];
std::mutex g_stateMutex;

// The state of `device`, with the device bound and the stream and event created: the one place that indexes the table and binds a device.
// g_stateMutex held.
int peac_state(int device, PeacState **out) {
    if (device < 0 || device >= 16) { set_error("msl_peac: device %d out of range (the extractor keeps state for devices 0 .. 15)", device); return MSL_ERR_INVALID; }
    const int rc = bind_device(device);
    if (rc != MSL_OK) return rc;
    PeacState *&S = g_state[device];
    if (!S) S = new PeacState;
    if (!S->ev) MSL_HIP_TRY(hipEventCreateWithFlags(&S->ev, hipEventDisableTiming));
    if (!S->stream) {
        int lo = 0, hi = 0;
        MSL_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        MSL_HIP_TRY(hipStreamCreateWithPriority(&S->stream, hipStreamNonBlocking, hi));
    }
    *out = S;
    return MSL_OK;
}

// Copies into host memory of the caller or of the call itself may still run when a call fails half-way: every return drains the stream first, unless
// the call got to its own last synchronisation (done).  Declared after the host memory it protects.
struct DrainUnlessDone {
    hipStream_t st; bool done = false;
    ~DrainUnlessDone() { if (!done) (void)hipStreamSynchronize(st); }
};

// ---- the steps of a call -------------------------------------------------------------------------------------------------------------------
// cloud (optional) + block fit + (optional) packed vertex depths of the call's frames, enqueued; *dBlocksOut receives the device pointer of the
// [frames][nBlocks] blocks, S.half the vertex depths.
int device_fit(PeacState &S, const PeacImages &I, const msl_peac_params &prm, double *cloudDev, msl_peac_block *blocksUser /* device output buffer or nullptr */,
               bool wantHalf, msl_peac_block **dBlocksOut) {
    PeacDev P;
    P.width = I.width; P.height = I.height; P.cw = I.cw; P.ch = I.ch;
    P.fx = I.fx; P.fy = I.fy; P.cx = I.cx; P.cy = I.cy; P.factor = I.factor;
    P.winW = prm.window_w; P.winH = prm.window_h; P.Nw = I.Nw; P.Nh = I.Nh; P.loose = prm.init_loose ? 1 : 0;
    P.alpha = prm.depth_alpha; P.tol = prm.depth_change_tol;
    P.strideBytes = I.stride; P.frameStrideBytes = I.frameStride;
    const int n_frames = I.n_frames;
    const hipStream_t st = S.stream;
    if (I.mem == MSL_MEM_DEVICE) { MSL_HIP_TRY(hipEventRecord(S.ev, 0)); MSL_HIP_TRY(hipStreamWaitEvent(st, S.ev, 0)); }
    if (I.mem == MSL_MEM_HOST) {
        // bytes actually present in the caller's buffer: the last row carries no stride padding
        const size_t frameBytes = I.stride * (size_t)(I.height - 1) + (size_t)I.width * 2, slot = (frameBytes + 255) & ~(size_t)255;
        MSL_HIP_TRY(S.depth.grow(slot * n_frames, st));
        for (int f = 0; f < n_frames; f++)
            MSL_HIP_TRY(hipMemcpyAsync((uint8_t *)S.depth.p + f * slot, (const uint8_t *)I.depth + f * I.frameStride, frameBytes, hipMemcpyHostToDevice, st));
        P.depth = (const uint16_t *)S.depth.p; P.frameStrideBytes = slot;
    } else {
        P.depth = I.depth;
    }
    if (blocksUser) P.blocks = blocksUser;
    else { MSL_HIP_TRY(S.blocks.grow(sizeof(msl_peac_block) * I.nBlocks * n_frames, st)); P.blocks = (msl_peac_block *)S.blocks.p; }
    P.cloud = cloudDev;
    const dim3 perVertex((unsigned)((I.nVert + 255) / 256), (unsigned)n_frames);
    if (cloudDev) {
        hipLaunchKernelGGL(k_peac_cloud, perVertex, dim3(256), 0, st, P);
        MSL_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_peac_fit, dim3((unsigned)I.nBlocks, (unsigned)n_frames), dim3(64), sizeof(double) * 9 * prm.window_w * prm.window_h, st, P);
    MSL_HIP_TRY(hipGetLastError());
    if (wantHalf) {
        MSL_HIP_TRY(S.half.grow(sizeof(uint16_t) * I.nVert * n_frames, st));
        hipLaunchKernelGGL(k_peac_half, perVertex, dim3(256), 0, st, P, (uint16_t *)S.half.p);
        MSL_HIP_TRY(hipGetLastError());
    }
    *dBlocksOut = P.blocks;
    return MSL_OK;
}

// What the host stage needs from the device, on the host: the block fits and the raw depth of the cloud vertices ([frames][ch][cw])
struct Fetched { std::vector<msl_peac_block> blocks; std::vector<uint16_t> half; msl_peac_block *dBlocks = nullptr; };

// device_fit, then the blocks, the half depth and -- when the caller wants the organised cloud of PlaneDetection::readDepthImage -- the cloud copied
// to the host; returns with the stream drained
int fit_and_fetch(PeacState &S, const PeacImages &I, const msl_peac_params &prm, double *cloud_out, Fetched &H) {
    const hipStream_t st = S.stream;
    const size_t cloudBytes = sizeof(double) * 3 * I.nVert * I.n_frames;
    double *dCloud = nullptr;
    if (cloud_out) { MSL_HIP_TRY(S.cloud.grow(cloudBytes, st)); dCloud = (double *)S.cloud.p; }
    const int rc = device_fit(S, I, prm, dCloud, nullptr, true, &H.dBlocks);
    if (rc != MSL_OK) return rc;
    H.blocks.resize(I.nBlocks * I.n_frames);
    H.half.resize(I.nVert * I.n_frames);
    MSL_HIP_TRY(hipMemcpyAsync(H.blocks.data(), H.dBlocks, sizeof(msl_peac_block) * H.blocks.size(), hipMemcpyDeviceToHost, st));
    MSL_HIP_TRY(hipMemcpyAsync(H.half.data(), S.half.p, sizeof(uint16_t) * H.half.size(), hipMemcpyDeviceToHost, st));
    if (cloud_out) MSL_HIP_TRY(hipMemcpyAsync(cloud_out, dCloud, cloudBytes, hipMemcpyDeviceToHost, st));
    MSL_HIP_TRY(hipStreamSynchronize(st));
    return MSL_OK;
}

// The hand-over of the device clustering on the host: the packed input graphs_for_device fills, and what k_peac_cluster left -- plane counts and
// disjoint sets (out), the planes.  A frame hands over at most 4 edges per window and min(nBlocks, 256) planes.
struct Clustered {
    ClusterLayout L;
    std::vector<int> in, out;
    std::vector<PlaneOut> planes;
    explicit Clustered(const PeacImages &I) : L(I.n_frames, I.nBlocks, 4 * (int)I.nBlocks, (int)std::min<size_t>(I.nBlocks, 256)) {}
};

// Agglomerative clustering on the device (one wave per frame) when a frame's node data fits the LDS and the call is large enough;
// MSL_PEAC_CLUSTER=host / device forces one side (same results: tests/test_peac_gpu.py runs both).  usable: R holds the call's planes and
// disjoint sets; otherwise the host clusters (also when a frame's edges or planes do not fit the hand-over).
int cluster_on_device(PeacState &S, const PeacImages &I, const msl_peac_params &prm, const Fetched &H, Clustered &R, bool &usable) {
    usable = false;
    const ClusterLayout &L = R.L;
    const int n_frames = I.n_frames, maxN = 2 * (int)I.nBlocks, words = (maxN + 31) / 32;
    const size_t ldsBytes = (size_t)maxN * (6 * sizeof(double) + 4 * sizeof(int) + 1) + 2 * I.nBlocks * sizeof(int) + 64;
    // auto: the device clusters any number of frames in the time of one (~13-20 ms, one latency-bound wave per frame), a host worker needs ~2 ms
    // per frame (candidate merges evaluated 16 at a time, plane_mse_lanes): the device wins once a call holds more than about eight frames per
    // usable CPU (measured: 64 frames on 16 workers, host 25.5 k frames/s of configuration 4 against 22.9 k with the device clustering).
    const bool wantDevice = msl_debug_peac_cluster_on_device(n_frames) != 0;
    if (ldsBytes > 150 * 1024 || !wantDevice) return MSL_OK;
    // graph initialisation on the host workers -> initial heap + edge list per frame
    R.in.resize(L.inInts);
    if (!graphs_for_device(I, prm, H.blocks.data(), L, R.in.data())) return MSL_OK;
    const hipStream_t st = S.stream;
    const size_t rowsB = sizeof(unsigned) * (size_t)n_frames * maxN * words, gstB = sizeof(double) * 9 * (size_t)n_frames * maxN,
                 gcxyB = sizeof(double) * 2 * (size_t)n_frames * maxN;
    MSL_HIP_TRY(grow_all(st, {{S.rows, rowsB}, {S.gst, gstB}, {S.gcxy, gcxyB}, {S.cin, sizeof(int) * L.inInts}, {S.cout, L.outBytes}}));
    MSL_HIP_TRY(hipMemcpyAsync(S.cin.p, R.in.data(), sizeof(int) * L.inInts, hipMemcpyHostToDevice, st));
    MSL_HIP_TRY(hipMemsetAsync(S.rows.p, 0, rowsB, st));
    ClusterDev C;
    C.nB = (int)I.nBlocks; C.maxN = maxN; C.words = words; C.minSupport = prm.min_support; C.maxStep = prm.max_step; C.maxE = L.maxE; C.maxPl = L.maxPl;
    C.depthSigma = prm.depth_sigma; C.stdTolMerge = prm.std_tol_merge; C.simMerge = prm.similarity_th_merge;
    C.blocks = H.dBlocks; C.rows = (unsigned *)S.rows.p; C.gst = (double *)S.gst.p; C.gcxy = (double *)S.gcxy.p;
    const int *dIn = (const int *)S.cin.p;
    C.heap0 = dIn + L.heap; C.heapCount = dIn + L.heapCount; C.edges = dIn + L.edges; C.edgeCount = dIn + L.edgeCount;
    int *dOut = (int *)S.cout.p;
    C.nPlanes = dOut + L.nPlanes; C.parent = dOut + L.parent; C.setSize = dOut + L.setSize;
    C.planes = reinterpret_cast<PlaneOut *>(dOut + L.planes);
    if (!S.clusterLdsSet) {
        MSL_HIP_TRY(hipFuncSetAttribute((const void *)k_peac_cluster, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        S.clusterLdsSet = true;
    }
    hipLaunchKernelGGL(k_peac_cluster, dim3((unsigned)n_frames), dim3(64), ldsBytes, st, C);
    MSL_HIP_TRY(hipGetLastError());
    R.out.resize(L.outInts); R.planes.resize((size_t)n_frames * L.maxPl);
    MSL_HIP_TRY(hipMemcpyAsync(R.out.data(), dOut, sizeof(int) * L.outInts, hipMemcpyDeviceToHost, st));
    MSL_HIP_TRY(hipMemcpyAsync(R.planes.data(), C.planes, sizeof(PlaneOut) * R.planes.size(), hipMemcpyDeviceToHost, st));
    MSL_HIP_TRY(hipStreamSynchronize(st));
    usable = true;
    for (int f = 0; f < n_frames; f++) if (R.out[L.nPlanes + f] < 0) usable = false;   // more planes than the hand-over holds: host path for this call
    return MSL_OK;
}

// msl_peac_membership_batch / msl_peac_extract_batch: the device steps under the state's lock, then one of the two host finishes
int membership_impl(PeacImages I, const msl_peac_params *params, const PeacOutputs &O, double *cloud_out) {
    int rc = check_call(I, params, &O, nullptr);
    if (rc != MSL_OK) return rc;
    Fetched H;
    Clustered R(I);
    bool usedDevice = false;
    const bool timing = peac_env().timing != 0;
    const auto tb0 = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lock(g_stateMutex);
        PeacState *S = nullptr;
        rc = peac_state(I.device, &S);
        if (rc != MSL_OK) return rc;
        DrainUnlessDone drain{S->stream};
        rc = fit_and_fetch(*S, I, *params, cloud_out, H);
        if (rc == MSL_OK) rc = cluster_on_device(*S, I, *params, H, R, usedDevice);
        if (rc != MSL_OK) return rc;
        drain.done = true;
    }
    const auto tb1 = std::chrono::steady_clock::now();
    rc = usedDevice ? finish_from_device(I, *params, H.half.data(), R.L, R.out.data(), R.planes.data(), O)
                    : segment_frames(I, *params, H.blocks.data(), H.half.data(), O);
    if (timing) {
        const auto tb2 = std::chrono::steady_clock::now();
        auto us = [](auto a, auto b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
        fprintf(stderr, "[msl_peac] batch of %d: device fit%s + copies %ld us, host stage %ld us\n", I.n_frames, usedDevice ? " + device clustering" : "", us(tb0, tb1),
                us(tb1, tb2));
    }
    return rc;
}

}  // namespace

extern "C" {

int msl_peac_block_fit(int device, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width, int height, int n_frames,
                       msl_mem mem, float fx, float fy, float cx, float cy, float depth_map_factor, const msl_peac_params *params,
                       msl_peac_block *blocks_out, msl_mem out_mem) noexcept {
    try {
    if (!params || !blocks_out) { set_error("msl_peac_block_fit: invalid argument"); return MSL_ERR_INVALID; }
    PeacImages I{device, depth, depth_stride_bytes, frame_stride_bytes, width, height, n_frames, mem, fx, fy, cx, cy, depth_map_factor};
    int rc = check_call(I, params, nullptr, nullptr);
    if (rc != MSL_OK) return rc;
    std::lock_guard<std::mutex> lock(g_stateMutex);
    PeacState *S = nullptr;
    rc = peac_state(device, &S);
    if (rc != MSL_OK) return rc;
    const hipStream_t st = S->stream;
    DrainUnlessDone drain{st};
    msl_peac_block *dBlocks = nullptr;
    rc = device_fit(*S, I, *params, nullptr, out_mem == MSL_MEM_DEVICE ? blocks_out : nullptr, false, &dBlocks);
    if (rc != MSL_OK) return rc;
    if (out_mem == MSL_MEM_HOST) MSL_HIP_TRY(hipMemcpyAsync(blocks_out, dBlocks, sizeof(msl_peac_block) * I.nBlocks * n_frames, hipMemcpyDeviceToHost, st));
    MSL_HIP_TRY(hipStreamSynchronize(st));
    drain.done = true;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_peac_block_stats(int device, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width, int height, int n_frames,
                         msl_mem mem, float fx, float fy, float cx, float cy, float depth_map_factor, int window_w, int window_h, double depth_alpha,
                         double depth_change_tol, int init_loose, double *cloud_out, msl_peac_stats *stats_out, msl_mem out_mem) noexcept {
    try {
    if (!stats_out) { set_error("msl_peac_block_stats: invalid argument"); return MSL_ERR_INVALID; }
    msl_peac_params prm;
    msl_peac_default_params(&prm);
    prm.window_w = window_w; prm.window_h = window_h; prm.depth_alpha = depth_alpha; prm.depth_change_tol = depth_change_tol; prm.init_loose = init_loose;
    PeacImages I{device, depth, depth_stride_bytes, frame_stride_bytes, width, height, n_frames, mem, fx, fy, cx, cy, depth_map_factor};
    int rc = check_call(I, &prm, nullptr, nullptr);
    if (rc != MSL_OK) return rc;
    std::vector<msl_peac_block> hb;
    std::vector<msl_peac_stats> hs;
    std::lock_guard<std::mutex> lock(g_stateMutex);
    PeacState *S = nullptr;
    rc = peac_state(device, &S);
    if (rc != MSL_OK) return rc;
    const hipStream_t st = S->stream;
    DrainUnlessDone drain{st};
    const size_t cloudBytes = sizeof(double) * 3 * I.nVert * n_frames;
    double *dCloud = nullptr;
    if (cloud_out) {
        if (out_mem == MSL_MEM_HOST) { MSL_HIP_TRY(S->cloud.grow(cloudBytes, st)); dCloud = (double *)S->cloud.p; }
        else dCloud = cloud_out;
    }
    msl_peac_block *dBlocks = nullptr;
    rc = device_fit(*S, I, prm, dCloud, nullptr, false, &dBlocks);
    if (rc != MSL_OK) return rc;
    // this entry point returns the Stats part only
    hb.resize(I.nBlocks * n_frames);
    MSL_HIP_TRY(hipMemcpyAsync(hb.data(), dBlocks, sizeof(msl_peac_block) * hb.size(), hipMemcpyDeviceToHost, st));
    MSL_HIP_TRY(hipStreamSynchronize(st));
    hs.resize(hb.size());
    for (size_t i = 0; i < hb.size(); i++) hs[i] = hb[i].stats;
    if (out_mem == MSL_MEM_HOST) {
        memcpy(stats_out, hs.data(), sizeof(msl_peac_stats) * hs.size());
        if (cloud_out) { MSL_HIP_TRY(hipMemcpyAsync(cloud_out, dCloud, cloudBytes, hipMemcpyDeviceToHost, st)); MSL_HIP_TRY(hipStreamSynchronize(st)); }
    } else {
        MSL_HIP_TRY(hipMemcpyAsync(stats_out, hs.data(), sizeof(msl_peac_stats) * hs.size(), hipMemcpyHostToDevice, st));
        MSL_HIP_TRY(hipStreamSynchronize(st));
    }
    drain.done = true;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_peac_membership_batch(int device, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width, int height, int n_frames,
                              msl_mem mem, float fx, float fy, float cx, float cy, float depth_map_factor, const msl_peac_params *params,
                              int32_t *membership_out, int32_t *n_planes_out) noexcept {
    try {
    const PeacImages I{device, depth, depth_stride_bytes, frame_stride_bytes, width, height, n_frames, mem, fx, fy, cx, cy, depth_map_factor};
    return membership_impl(I, params, PeacOutputs{membership_out, n_planes_out}, nullptr);
    } MSL_ABI_CATCH_INT
}
int msl_peac_extract_batch(int device, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width, int height, int n_frames,
                           msl_mem mem, float fx, float fy, float cx, float cy, float depth_map_factor, const msl_peac_params *params,
                           int32_t *membership_out, int32_t *n_planes_out, int max_planes, msl_peac_plane *planes_out, int32_t *vertex_offsets_out,
                           int32_t *vertex_indices_out, double *cloud_out) noexcept {
    try {
    if (!planes_out) { set_error("msl_peac_extract_batch: planes_out is NULL (use msl_peac_membership_batch for the image alone)"); return MSL_ERR_INVALID; }
    const PeacImages I{device, depth, depth_stride_bytes, frame_stride_bytes, width, height, n_frames, mem, fx, fy, cx, cy, depth_map_factor};
    return membership_impl(I, params, PeacOutputs{membership_out, n_planes_out, max_planes, planes_out, vertex_offsets_out, vertex_indices_out}, cloud_out);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
