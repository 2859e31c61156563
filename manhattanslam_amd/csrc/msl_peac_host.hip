// msl_peac_host.hip -- the host stage of the PEAC plane extractor: everything that never touches the device.
//
// ahc::PlaneFitter<ImagePointCloud>::run (reference include/peac/AHCPlaneFitter.hpp:218-262) after the per-window plane fits: graph initialisation
// (:756-928; needs cos()), the agglomerative clustering (:939-1143), block erosion + seeds (:490-596), the FIFO region growing (:422-471), final
// merge and relabelling (:296-372).  Order-dependent pixel work, one frame per worker thread at a time, index based (node pool + sorted adjacency
// vectors instead of shared_ptr / std::set<PlaneSeg*>).  The clustering is here in full (cluster()): it is the path of small calls -- a single
// frame, the reference's call pattern, in ~2 ms: the candidate merges of a pop are fitted 16 at a time in SIMD lanes (plane_mse_lanes) -- of frames
// whose node data does not fit the LDS, of MSL_PEAC_CLUSTER=host, and of the *_from_blocks entry points (no device).  For large calls msl_peac.hip
// clusters on the device between graphs_for_device and finish_from_device.
//
// Also here: the argument check of every PEAC entry point (check_call), the environment switches (peac_env), the worker pool, and the debug hooks
// that need them -- msl_debug_throw among them, whose kind 3 throws inside a pool worker.
//
// The membership image keeps every quirk a consumer can observe: rid2plid[] default-inserts plane 0 for an
// unknown set id, pixels whose plane was eroded keep their old id, rejected pixels keep their visit counters -2..-6.
#include "msl_peac_host.h"
#include "msl_peac_math.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <iterator>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <sched.h>
#include <stdexcept>
#include <thread>
#include <vector>

namespace {
using namespace msl;
using namespace msl::peac;

// ---- host side: agglomerative clustering over the block graph -----------------------------------------------------------------
struct Thresholds {
    msl_peac_params p;
    double t_mse_init(double z) const { return std::pow(p.depth_sigma * z * z + p.std_tol_init, 2); }     // ParamSet::T_mse (AHCParamSet.hpp:87-99)
    double t_mse_merge(double z) const { return std::pow(p.depth_sigma * z * z + p.std_tol_merge, 2); }
    double t_ang_init(double z) const {                                                                   // ParamSet::T_ang (:111-131)
        double clipped_z = z;
        clipped_z = std::max(clipped_z, p.z_near);
        clipped_z = std::min(clipped_z, p.z_far);
        const double factor = (p.angle_far - p.angle_near) / (p.z_far - p.z_near);
        return std::cos(factor * clipped_z + p.angle_near - factor * p.z_near);
    }
};

// ---- the MSE of several candidate merges at once (host SIMD) ------------------------------------------------------------------------------
// ahCluster fits a plane to every neighbour's merged statistics before it picks one (AHCPlaneFitter.hpp:985-1010): for a frame that is ~30 000
// 3x3 eigenvalue problems, all but ~1 500 of them discarded, and the whole latency of a single-frame call.  The lanes below run plane_mse() for
// VW candidates in lock-step: every lane performs exactly the scalar sequence of IEEE double operations of eig33sym_t<false> (same expressions,
// same association, no contraction; divisions and square roots are correctly rounded in either form), branches become selects, and a lane whose
// QR iteration has finished is masked, so the result is the scalar result bit for bit (tests/test_peac_host.py compares both on random and
// degenerate matrices, and the whole segmentation against the oracle with every width).
template <int VW> struct Lanes {
    typedef double D __attribute__((ext_vector_type(VW)));
    typedef long M __attribute__((ext_vector_type(VW)));   // comparison results: all ones / zero per lane
};
#define MSL_SEL(m, a, b) ((m) ? (a) : (b))

// in: 10 rows of VW doubles (sx sy sz sxx syy szz sxy syz sxz N); out: VW MSEs
template <int VW>
__attribute__((always_inline)) inline void plane_mse_lanes(const double *in, double *out) {
    typedef typename Lanes<VW>::D D;
    typedef typename Lanes<VW>::M M;
    D r[10];
    for (int i = 0; i < 10; i++) __builtin_memcpy(&r[i], in + (size_t)i * VW, sizeof(D));
    const D zero = 0.0, one = 1.0;
    const M izero = 0, ione = 1, itwo = 2;
    const D sc = one / r[9];
    D a00 = r[3] - r[0] * r[0] * sc, a10 = r[6] - r[0] * r[1] * sc, a20 = r[8] - r[0] * r[2] * sc;
    D a11 = r[4] - r[1] * r[1] * sc, a21 = r[7] - r[1] * r[2] * sc, a22 = r[5] - r[2] * r[2] * sc;
    // The helpers take and return 256- to 1024-bit vectors by value, and a lambda's call operator does not inherit the target("avx2" / "avx512f")
    // attribute of the wrapper this template is inlined into: if the inliner ever declined, the call would cross an ABI boundary between feature
    // sets (-Wpsabi) and could silently change the bits.  always_inline removes the dependence on heuristics; the build adds -Werror=psabi.
    auto vabs = [](D v) __attribute__((always_inline)) { return __builtin_elementwise_abs(v); };
    auto vmax = [](D a, D b) __attribute__((always_inline)) { return __builtin_elementwise_max(a, b); };   // fmax: a NaN operand is ignored
    auto vsqrt = [](D v) __attribute__((always_inline)) { return __builtin_elementwise_sqrt(v); };
    D scale = vmax(vmax(vmax(vabs(a00), vabs(a10)), vmax(vabs(a11), vabs(a20))), vmax(vabs(a21), vabs(a22)));
    scale = MSL_SEL(scale == zero, one, scale);
    a00 /= scale; a10 /= scale; a11 /= scale; a20 /= scale; a21 /= scale; a22 /= scale;
    const D tiny = 2.2250738585072014e-308, precision = 2.0 * 2.220446049250313e-16;
    const D v1norm2 = a20 * a20;
    const M small = v1norm2 <= tiny;
    const D beta = vsqrt(a10 * a10 + v1norm2), invBeta = one / beta, m01 = a10 * invBeta, m02 = a20 * invBeta;
    const D qq = (D)2.0 * m01 * a21 + m02 * (a22 - a11);
    D dg0 = a00, dg1 = MSL_SEL(small, a11, a11 + m02 * qq), dg2 = MSL_SEL(small, a22, a22 - m02 * qq);
    D sb0 = MSL_SEL(small, a10, beta), sb1 = MSL_SEL(small, a21, a21 - m01 * qq);
    M end = itwo, start = izero, iter = izero, active = ~izero;
    // Givens rotation that annihilates z against x: the three scalar cases share one division, one square root and one reciprocal
    auto givens = [&](D x, D z, D &c, D &sn) __attribute__((always_inline)) {
        const M big = vabs(x) > vabs(z);
        const D num = MSL_SEL(big, z, x), den = MSL_SEL(big, x, z);
        const D t = num / den;
        D u = vsqrt(one + t * t);
        u = MSL_SEL(den < zero, -u, u);
        const D rr = MSL_SEL(big, one, -one) / u, oo = -t * rr;   // |x| > |z|: c = 1 / u, sn = -t c; otherwise sn = -1 / u, c = -t sn
        c = MSL_SEL(big, rr, oo); sn = MSL_SEL(big, oo, rr);
        const M x0 = x == zero;
        c = MSL_SEL(x0, zero, c); sn = MSL_SEL(x0, MSL_SEL(z < zero, one, -one), sn);
    };
    for (;;) {
        const M c0 = active & (start <= izero) & (end > izero) & ((vabs(sb0) <= (vabs(dg0) + vabs(dg1)) * precision) | (vabs(sb0) <= tiny));
        sb0 = MSL_SEL(c0, zero, sb0);
        const M c1 = active & (start <= ione) & (end > ione) & ((vabs(sb1) <= (vabs(dg1) + vabs(dg2)) * precision) | (vabs(sb1) <= tiny));
        sb1 = MSL_SEL(c1, zero, sb1);
        end = MSL_SEL(active & (end == itwo) & (sb1 == zero), ione, end);
        end = MSL_SEL(active & (end == ione) & (sb0 == zero), izero, end);
        active &= end > izero;
        iter = MSL_SEL(active, iter + ione, iter);
        active &= ~(iter > (M)90);
        if (!__builtin_reduce_or(active)) break;
        start = end - ione;
        start = MSL_SEL((start == ione) & (sb0 != zero), izero, start);
        const M e2m = end == itwo;
        const D dEnd = MSL_SEL(e2m, dg2, dg1), dEm1 = MSL_SEL(e2m, dg1, dg0), e = MSL_SEL(e2m, sb1, sb0);
        const D td = (dEm1 - dEnd) * (D)0.5;
        const D ax = vabs(td), ay = vabs(e);
        const M gt = ax > ay;
        const D pp = MSL_SEL(gt, ax, ay), qp = MSL_SEL(gt, ay, ax) / pp;
        const D h = MSL_SEL(pp == zero, zero, pp * vsqrt(one + qp * qp));
        const D e2 = e * e, denom = td + MSL_SEL(td > zero, h, -h);
        const D muA = dEnd - vabs(e), muC = dEnd - e2 / denom;
        D mu = MSL_SEL(td == zero, muA, MSL_SEL(e != zero, muC, dEnd));
        const M under = active & (td != zero) & (e != zero) & (e2 == zero);   // e * e underflowed: the scalar code divides twice instead
        if (__builtin_reduce_or(under)) mu = MSL_SEL(under, dEnd - e / (denom / e), mu);
        const M s0 = start == izero;
        D x = MSL_SEL(s0, dg0, dg1) - mu, z = MSL_SEL(s0, sb0, sb1);
        const M doK0 = active & s0 & (z != zero);
        if (__builtin_reduce_or(doK0)) {   // k = 0
            const M doK = doK0;
            D c, sn;
            givens(x, z, c, sn);
            const D sdk = sn * dg0 + c * sb0, dkp1 = sn * sb0 + c * dg1;
            const D n0 = c * (c * dg0 - sn * sb0) - sn * (c * sb0 - sn * dg1), n1 = sn * sdk + c * dkp1, nsb = c * sdk - sn * dkp1;
            dg0 = MSL_SEL(doK, n0, dg0); dg1 = MSL_SEL(doK, n1, dg1); sb0 = MSL_SEL(doK, nsb, sb0);
            x = MSL_SEL(doK, nsb, x);
            const M more = doK & e2m;                      // k < end - 1
            const D nz = -sn * sb1, nsb1 = c * sb1;
            // a lane that ran k = 0 with end == 1 has left the scalar loop: end > 1 below keeps it out of k = 1
            z = MSL_SEL(more, nz, z); sb1 = MSL_SEL(more, nsb1, sb1);
        }
        const M doK1 = active & e2m & (z != zero);
        if (__builtin_reduce_or(doK1)) {   // k = 1 (a lane that skipped k = 0 at start == 0 did so with z == 0, which also ends its loop here)
            const M doK = doK1;
            D c, sn;
            givens(x, z, c, sn);
            const D sdk = sn * dg1 + c * sb1, dkp1 = sn * sb1 + c * dg2;
            const D n1 = c * (c * dg1 - sn * sb1) - sn * (c * sb1 - sn * dg2), n2 = sn * sdk + c * dkp1, nsb = c * sdk - sn * dkp1;
            sb0 = MSL_SEL(doK & s0, c * sb0 - sn * z, sb0);    // k > start
            dg1 = MSL_SEL(doK, n1, dg1); dg2 = MSL_SEL(doK, n2, dg2); sb1 = MSL_SEL(doK, nsb, sb1);
        }
    }
    const D lo01 = MSL_SEL(dg1 < dg0, dg1, dg0), lo = MSL_SEL(dg2 < lo01, dg2, lo01);   // s[0] of the selection sort
    const D mse = lo * scale * sc;
    __builtin_memcpy(out, &mse, sizeof(D));
}

#if defined(__HIP_DEVICE_COMPILE__)
#define MSL_TARGET(t)
inline int host_simd_level() { return 2; }
#else
#define MSL_TARGET(t) __attribute__((target(t)))
// instruction set the lanes may use: 8 = AVX-512F, 4 = AVX2, 2 = the x86-64 baseline (SSE2), 0 = the scalar code; MSL_PEAC_SIMD lowers it
inline int host_simd_level() {
    static const int w = [] {
        int best = __builtin_cpu_supports("avx512f") ? 8 : __builtin_cpu_supports("avx2") ? 4 : 2;
        if (peac_env().simd >= 0) best = std::min(best, peac_env().simd);
        return best;
    }();
    return w;
}
#endif
inline int host_lane_cap() { return peac_env().lanes; }   // MSL_PEAC_LANES = 2 / 4 / 8 / 16 caps the candidates per group (tests run every width)
// The solver is a single dependent chain of divisions and square roots, so a group twice as wide as the registers (two independent chains the
// core interleaves) costs little more than one register's worth: 16 lanes on AVX-512, 8 on AVX2.
void plane_mse_x2(const double *in, double *out) { plane_mse_lanes<2>(in, out); }
MSL_TARGET("avx2") void plane_mse_x4(const double *in, double *out) { plane_mse_lanes<4>(in, out); }
MSL_TARGET("avx2") void plane_mse_x8_avx2(const double *in, double *out) { plane_mse_lanes<8>(in, out); }
MSL_TARGET("avx512f") void plane_mse_x8(const double *in, double *out) { plane_mse_lanes<8>(in, out); }
MSL_TARGET("avx512f") void plane_mse_x16(const double *in, double *out) { plane_mse_lanes<16>(in, out); }
// lanes for a group when `left` candidates remain (0: scalar)
inline int lanes_for(size_t left) {
    const int simd = host_simd_level(), cap = host_lane_cap();
    if (left < 2 || simd == 0) return 0;
    int vw = 2;
    if (simd >= 4 && left > 2) vw = 4;
    if (simd >= 4 && left > 4) vw = 8;
    if (simd >= 8 && left > 8) vw = 16;
    return std::min(vw, cap);
}
inline void plane_mse_group(int vw, const double *in, double *out) {
    if (vw == 16) plane_mse_x16(in, out);
    else if (vw == 8) { if (host_simd_level() >= 8) plane_mse_x8(in, out); else plane_mse_x8_avx2(in, out); }
    else if (vw == 4) plane_mse_x4(in, out);
    else plane_mse_x2(in, out);
}

struct Node {
    msl_peac_stats st;
    double center[3], normal[3], mse, curvature;
    int N, rid;
    bool nouse;
    std::vector<int> nbs;   // adjacent node ids, ascending (= the reference's std::set<PlaneSeg*> with addresses pinned to creation order)
};

// One object per worker thread, reused for every frame that thread segments: all containers keep their capacity, so the steady state allocates
// nothing (64 threads that each mmap / munmap a few hundred KB per frame serialise on the process's address-space lock).
// Optional per-frame outputs beyond the membership image: what PlaneDetection hands on (extractedPlanes, plane_vertices_)
struct PlaneSink { msl_peac_plane *planes; int32_t *offsets, *indices; int maxPlanes; bool overflow; };

class alignas(128) FrameSegmenter {   // own cache lines: the vectors' end pointers inside the object change on every push
public:
    void set_sink(PlaneSink *s) { sink_ = s; }
    void configure(const PeacImages &I, const msl_peac_params &prm, const uint16_t *halfDepth /* [ch][cw] raw depth of the cloud vertices */) {
        T.p = prm; img_ = halfDepth; W = I.cw; H = I.ch; fx_ = I.fx; fy_ = I.fy; cx_ = I.cx; cy_ = I.cy; factor_ = I.factor;
        winW = prm.window_w; winH = prm.window_h; Nw = I.Nw; Nh = I.Nh;
    }

    // returns the number of extracted planes; member[H * W] receives PlaneFitter::membershipImg
    // Device-clustering path, phase 1: graph initialisation only (AHCPlaneFitter.hpp:756-928); the initial heap (in the order the pushes left
    // it) and the edge list go to k_peac_cluster.  Returns false if the edge list does not fit.
    bool graph_for_device(const msl_peac_block *blocks, int *heapOut, int *heapCount, int *edgesOut, int *edgeCount, int maxE) {
        parent_.resize((size_t)Nw * Nh); setSize_.assign((size_t)Nw * Nh, 1);
        for (size_t i = 0; i < parent_.size(); i++) parent_[i] = (int)i;
        nNodes_ = 0; planes_.clear(); growQ_.clear(); heap_.clear();
        edges_.clear(); recordEdges_ = true;
        build_graph(blocks);
        recordEdges_ = false;
        if ((int)edges_.size() / 2 > maxE) return false;
        std::copy(heap_.begin(), heap_.end(), heapOut); *heapCount = (int)heap_.size();
        std::copy(edges_.begin(), edges_.end(), edgesOut); *edgeCount = (int)edges_.size() / 2;
        return true;
    }
    // Phase 2: the planes k_peac_cluster extracted (extraction order) and its disjoint set; erosion, region growing and the final merge follow as
    // in run().  Only the plane nodes exist here; their ids keep the order of the original ids (the neighbour sets iterate in id order).
    int finish_from_device(const PlaneOut *pl, int np, const int *parent, const int *setSize, int32_t *member) {
        parent_.assign(parent, parent + (size_t)Nw * Nh); setSize_.assign(setSize, setSize + (size_t)Nw * Nh);
        nNodes_ = 0; planes_.clear(); growQ_.clear(); heap_.clear();
        std::vector<int> &order = relabel_, &newId = oldPlanes_;
        order.resize(np); newId.resize(np);
        for (int i = 0; i < np; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [pl](int a, int b) { return pl[a].id < pl[b].id; });
        for (int k = 0; k < np; k++) {
            const PlaneOut &O = pl[order[k]];
            Node nd;
            nd.st.sx = O.st[0]; nd.st.sy = O.st[1]; nd.st.sz = O.st[2]; nd.st.sxx = O.st[3]; nd.st.syy = O.st[4]; nd.st.szz = O.st[5];
            nd.st.sxy = O.st[6]; nd.st.syz = O.st[7]; nd.st.sxz = O.st[8]; nd.st.N = O.N; nd.st.nouse = 0;
            for (int c = 0; c < 3; c++) { nd.center[c] = O.center[c]; nd.normal[c] = O.normal[c]; }
            nd.mse = O.mse; nd.curvature = 0; nd.N = O.N; nd.rid = O.rid; nd.nouse = false;
            newId[order[k]] = add_node(nd);
        }
        for (int i = 0; i < np; i++) planes_.push_back(newId[i]);
        std::sort(planes_.begin(), planes_.end(), [this](int a, int b) { return nodes_[b].N < nodes_[a].N; });   // PlaneSegSizeCmp, as at the end of cluster()
        member_ = member;
        std::fill(member, member + (size_t)W * H, -1);
        if (T.p.do_refine) refine();
        emit_planes();
        return (int)planes_.size();
    }

    int run(const msl_peac_block *blocks, int32_t *member) {
        const bool timing = peac_env().timing >= 2;
        auto now = []() { return std::chrono::steady_clock::now(); };
        auto t0 = now();
        parent_.resize((size_t)Nw * Nh); setSize_.assign((size_t)Nw * Nh, 1);
        for (size_t i = 0; i < parent_.size(); i++) parent_[i] = (int)i;
        nNodes_ = 0; planes_.clear(); growQ_.clear(); heap_.clear();
        build_graph(blocks);
        auto t1 = now();
        cluster();
        auto t2 = now();
        member_ = member;
        std::fill(member, member + (size_t)W * H, -1);
        if (T.p.do_refine) refine();
        auto t3 = now();
        if (timing) {
            auto us = [](auto a, auto b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
            fprintf(stderr, "[msl_peac] graph %ld us, cluster %ld us (%zu nodes), refine %ld us (queue %zu)\n", us(t0, t1), us(t1, t2), (size_t)nNodes_, us(t2, t3), growQ_.size());
        }
        emit_planes();
        return (int)planes_.size();
    }

private:
    struct MseGreater {   // PlaneSegMinMSECmp: the queue's top is the node with the smallest MSE
        const FrameSegmenter *f;
        bool operator()(int a, int b) const { return f->nodes_[b].mse < f->nodes_[a].mse; }
    };
    // std::priority_queue<int, std::vector<int>, MseGreater> spelled out (push_heap / pop_heap on a member vector: the same sequence of
    // comparisons, hence the same order among equal keys, without a fresh container per run)
    std::vector<int> heap_;
    void heap_push(int id) { heap_.push_back(id); std::push_heap(heap_.begin(), heap_.end(), MseGreater{this}); }
    int heap_pop() { std::pop_heap(heap_.begin(), heap_.end(), MseGreater{this}); const int id = heap_.back(); heap_.pop_back(); return id; }

    Thresholds T;
    const uint16_t *img_ = nullptr;
    int W = 0, H = 0; float fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0, factor_ = 0;
    int winW = 0, winH = 0, Nw = 0, Nh = 0;
    std::vector<Node> nodes_;                 // node pool: [0, nNodes_) are live; the rest keep their neighbour vectors' capacity for the next frame
    int nNodes_ = 0;
    std::vector<int> G_, u_, oldPlanes_, relabel_, edges_;
    bool recordEdges_ = false;
    PlaneSink *sink_ = nullptr;
    void emit_planes() {   // plane_filter.extractedPlanes as Frame::ExtractPlanes reads them (src/Frame.cc:626-632)
        if (!sink_) return;
        if ((int)planes_.size() > sink_->maxPlanes) { sink_->overflow = true; return; }
        for (size_t j = 0; j < planes_.size(); j++) {
            const Node &nd = nodes_[planes_[j]];
            msl_peac_plane &o = sink_->planes[j];
            for (int c = 0; c < 3; c++) { o.normal[c] = nd.normal[c]; o.center[c] = nd.center[c]; }
            o.mse = nd.mse; o.N = nd.N; o._pad = 0;
        }
        if (sink_->offsets && !T.p.do_refine) for (size_t j = 0; j <= planes_.size(); j++) sink_->offsets[j] = 0;
    }
    std::vector<char> validPlane_;
    std::vector<float> distMap_;
    int add_node(const Node &src) {
        if ((size_t)nNodes_ == nodes_.size()) nodes_.emplace_back();
        nodes_[nNodes_] = src;                // (src.nbs is empty: the slot's vector is cleared, not reallocated)
        return nNodes_++;
    }
    std::vector<int> parent_, setSize_;       // disjoint set over the windows (DisjointSet.hpp)
    std::vector<int> planes_;                 // extractedPlanes, node ids
    std::vector<int> blkMap_;
    std::vector<std::pair<int, int>> growQ_;  // rfQueue: (pixel, plane)
    int32_t *member_ = nullptr;

    int find(int x) { while (parent_[x] != x) { parent_[x] = parent_[parent_[x]]; x = parent_[x]; } return x; }   // (path halving: same roots as Find())
    void unite(int x, int y) {
        const int xr = find(x), yr = find(y);
        if (xr == yr) return;
        if (setSize_[xr] < setSize_[yr]) { parent_[xr] = yr; setSize_[yr] += setSize_[xr]; }
        else { parent_[yr] = xr; setSize_[xr] += setSize_[yr]; }
    }
    static double similarity(const Node &a, const Node &b) { return std::abs(a.normal[0] * b.normal[0] + a.normal[1] * b.normal[1] + a.normal[2] * b.normal[2]); }
    static void link_one(std::vector<int> &v, int id) { auto it = std::lower_bound(v.begin(), v.end(), id); if (it == v.end() || *it != id) v.insert(it, id); }
    static void unlink_one(std::vector<int> &v, int id) { auto it = std::lower_bound(v.begin(), v.end(), id); if (it != v.end() && *it == id) v.erase(it); }
    void connect(int a, int b) {
        link_one(nodes_[a].nbs, b); link_one(nodes_[b].nbs, a);
        if (recordEdges_) { edges_.push_back(a); edges_.push_back(b); }
    }
    void isolate(int a) { for (int nb : nodes_[a].nbs) unlink_one(nodes_[nb].nbs, a); nodes_[a].nbs.clear(); }

    void build_graph(const msl_peac_block *blocks) {
        std::vector<int> &G = G_;   // node id of an accepted window
        G.assign((size_t)Nw * Nh, -1);
        for (int b = 0; b < Nw * Nh; b++) {
            const msl_peac_block &B = blocks[b];
            Node nd;
            nd.st = B.stats; nd.mse = B.mse; nd.curvature = B.curvature; nd.rid = b; nd.nouse = B.stats.nouse != 0; nd.N = nd.nouse ? 0 : B.stats.N;
            for (int k = 0; k < 3; k++) { nd.center[k] = B.center[k]; nd.normal[k] = B.normal[k]; }
            add_node(nd);
            if (nd.mse < T.t_mse_init(nd.center[2]) && !nd.nouse) { G[b] = b; heap_push(b); }
        }
        // edges between horizontally / vertically adjacent accepted windows whose two outer neighbours agree in normal (:849-927)
        auto sweep = [&](int outerN, int innerN, int outerStride, int innerStride) {
            for (int o = 0; o < outerN; ++o)
                for (int k = 1; k < innerN; k += 2) {
                    const int c = o * outerStride + k * innerStride, prev = c - innerStride, next = c + innerStride;
                    if (G[prev] < 0) { --k; continue; }
                    if (G[c] < 0) continue;
                    if (k < innerN - 1 && G[next] < 0) { ++k; continue; }
                    const double th = T.t_ang_init(nodes_[G[c]].center[2]);
                    const bool ok = k < innerN - 1 ? similarity(nodes_[G[prev]], nodes_[G[next]]) >= th : similarity(nodes_[G[c]], nodes_[G[prev]]) >= th;
                    if (ok) { connect(G[c], G[prev]); if (k < innerN - 1) connect(G[c], G[next]); }
                    else --k;
                }
        };
        sweep(Nh, Nw, Nw, 1);
        sweep(Nw, Nh, 1, Nw);
    }

    double merged_mse(int a, int b) const {
        msl_peac_stats t;
        const msl_peac_stats &x = nodes_[a].st, &y = nodes_[b].st;
        t.sx = x.sx + y.sx; t.sy = x.sy + y.sy; t.sz = x.sz + y.sz; t.sxx = x.sxx + y.sxx; t.syy = x.syy + y.syy; t.szz = x.szz + y.szz;
        t.sxy = x.sxy + y.sxy; t.syz = x.syz + y.syz; t.sxz = x.sxz + y.sxz; t.N = x.N + y.N; t.nouse = 0;
        return plane_mse(t);
    }
    // candMse_[i] = merged_mse(p, cand_[i]), the candidates taken VW at a time (a short last group is padded with its first candidate)
    std::vector<int> cand_;
    std::vector<double> candMse_;
    void candidate_mses(int p) {
        const size_t n = cand_.size();
        candMse_.resize(n);
        const msl_peac_stats &x = nodes_[p].st;
        alignas(64) double in[10 * 16], out[16];
        for (size_t i0 = 0; i0 < n;) {
            const size_t left = n - i0;
            const int vw = lanes_for(left);
            if (vw == 0) { candMse_[i0] = merged_mse(p, cand_[i0]); ++i0; continue; }
            for (int l = 0; l < vw; l++) {
                const msl_peac_stats &y = nodes_[cand_[i0 + ((size_t)l < left ? l : 0)]].st;
                in[0 * vw + l] = x.sx + y.sx; in[1 * vw + l] = x.sy + y.sy; in[2 * vw + l] = x.sz + y.sz;
                in[3 * vw + l] = x.sxx + y.sxx; in[4 * vw + l] = x.syy + y.syy; in[5 * vw + l] = x.szz + y.szz;
                in[6 * vw + l] = x.sxy + y.sxy; in[7 * vw + l] = x.syz + y.syz; in[8 * vw + l] = x.sxz + y.sxz;
                in[9 * vw + l] = (double)(x.N + y.N);
            }
            plane_mse_group(vw, in, out);
            for (int l = 0; l < vw && (size_t)l < left; l++) candMse_[i0 + l] = out[l];
            i0 += vw;
        }
    }
    Node merged_node(int a, int b) const {   // PlaneSeg(pa, pb) (AHCPlaneSeg.hpp:299-322)
        Node nd;
        const msl_peac_stats &x = nodes_[a].st, &y = nodes_[b].st;
        nd.st.sx = x.sx + y.sx; nd.st.sy = x.sy + y.sy; nd.st.sz = x.sz + y.sz; nd.st.sxx = x.sxx + y.sxx; nd.st.syy = x.syy + y.syy; nd.st.szz = x.szz + y.szz;
        nd.st.sxy = x.sxy + y.sxy; nd.st.syz = x.syz + y.syz; nd.st.sxz = x.sxz + y.sxz; nd.st.N = x.N + y.N; nd.st.nouse = 0;
        nd.nouse = false;
        nd.rid = nodes_[a].N >= nodes_[b].N ? nodes_[a].rid : nodes_[b].rid;
        nd.N = nd.st.N;
        plane_fit(nd.st, nd.center, nd.normal, nd.mse, nd.curvature);
        return nd;
    }

    void cluster() {   // ahCluster (:939-1143) on heap_
        int step = 0;
        while (!heap_.empty() && step <= T.p.max_step) {
            const int p = heap_pop();
            if (nodes_[p].nouse) continue;
            // try to merge with every neighbour (ascending id), keep the merge with the smallest MSE
            // (only the MSE of every candidate is needed to choose; the full node -- centre, normal, curvature -- is built for the winner alone)
            bool have = false;
            double bestMse = 0;
            int bestN = 0, bestNb = -1;
            cand_.clear();
            for (int nb : nodes_[p].nbs)
                if (!(similarity(nodes_[p], nodes_[nb]) < T.p.similarity_th_merge)) cand_.push_back(nb);
            candidate_mses(p);
            for (size_t ci = 0; ci < cand_.size(); ci++) {
                const int nb = cand_[ci];
                const double mse = candMse_[ci];
                if (!have || bestMse > mse || (bestMse == mse && bestN < mse)) { bestMse = mse; bestN = nodes_[p].st.N + nodes_[nb].st.N; bestNb = nb; have = true; }   // (sic: N against mse, :1005)
            }
            Node best;
            if (have) best = merged_node(p, bestNb);
            if (have && best.mse < T.t_mse_merge(best.center[2])) {
                const int id = add_node(best);   // accepted merges get ascending ids: the newest node sorts last among neighbours
                heap_push(id);
                // mergeNbsFrom (AHCPlaneSeg.hpp:398-436)
                unite(nodes_[p].rid, nodes_[bestNb].rid);
                std::vector<int> &u = u_;
                u.clear();
                std::set_union(nodes_[p].nbs.begin(), nodes_[p].nbs.end(), nodes_[bestNb].nbs.begin(), nodes_[bestNb].nbs.end(), std::back_inserter(u));
                unlink_one(u, p); unlink_one(u, bestNb);
                isolate(p); isolate(bestNb);
                for (int nb : u) link_one(nodes_[nb].nbs, id);
                nodes_[id].nbs.assign(u.begin(), u.end());
                nodes_[p].nouse = nodes_[bestNb].nouse = true;
            } else {
                if (nodes_[p].N >= T.p.min_support) planes_.push_back(p);
                isolate(p);
            }
            ++step;
        }
        while (!heap_.empty()) {
            const int p = heap_pop();
            if (nodes_[p].N >= T.p.min_support) planes_.push_back(p);
            isolate(p);
        }
        std::sort(planes_.begin(), planes_.end(), [this](int a, int b) { return nodes_[b].N < nodes_[a].N; });   // PlaneSegSizeCmp
    }

    bool point(int row, int col, double pt[3]) const {   // ImagePointCloud::get on the fly, from the packed vertex depths
        const double z = (double)img_[(size_t)row * W + col] * factor_;
        pt[2] = z;
        if (z == 0) return false;
        vertex_xy(fx_, fy_, cx_, cy_, row, col, z, pt[0], pt[1]);
        return true;
    }
    static int neighbours4(int i, int j, int Hh, int Ww, int nbs[4]) {
        const int id = i * Ww + j;
        int cnt = 0;
        if (j > 0) nbs[cnt++] = id - 1;
        if (j < Ww - 1) nbs[cnt++] = id + 1;
        if (i > 0) nbs[cnt++] = id - Ww;
        if (i < Hh - 1) nbs[cnt++] = id + Ww;
        return cnt;
    }

    void erode_blocks(std::vector<char> &validPlane) {   // findBlockMembership(isValidExtractedPlane) (:490-596)
        std::map<int, int> rid2plid;
        for (int plid = 0; plid < (int)planes_.size(); ++plid) rid2plid.insert(std::make_pair(nodes_[planes_[plid]].rid, plid));
        const int perBlk = winW * winH;
        blkMap_.assign((size_t)Nw * Nh, -1);
        validPlane.assign(planes_.size(), 0);
        for (int i = 0, blk = 0; i < Nh; ++i)
            for (int j = 0; j < Nw; ++j, ++blk) {
                const int setid = find(blk);
                if (setSize_[setid] * perBlk >= T.p.min_support) {
                    int nb4[4] = {-1, -1, -1, -1};
                    const int nNb = neighbours4(i, j, Nh, Nw, nb4);
                    bool interior = true;
                    for (int k = 0; k < nNb && T.p.erode_type != 0; ++k)
                        if (find(nb4[k]) != setid && (T.p.erode_type == 2 || setSize_[find(nb4[k])] * perBlk >= T.p.min_support)) { interior = false; break; }
                    const int plid = rid2plid[setid];   // default-inserts plane 0 for a set whose root is no extracted plane's rid, as the reference does
                    if (interior) {
                        blkMap_[blk] = plid;
                        for (int y = i * winH; y < (i + 1) * winH; y++) std::fill(member_ + (size_t)y * W + j * winW, member_ + (size_t)y * W + (j + 1) * winW, plid);
                        validPlane[plid] = 1;
                    }
                }
                // seeds of the region growing: the pixels of a plane window that face a window of another (or no) plane
                if (blkMap_[blk] < 0) {
                    if (i > 0 && blkMap_[blk - Nw] >= 0)
                        for (int k = 1; k < winW; ++k) growQ_.push_back(std::make_pair((i * winH - 1) * W + j * winW + k, blkMap_[blk - Nw]));
                    if (j > 0 && blkMap_[blk - 1] >= 0)
                        for (int k = 0; k < winH - 1; ++k) growQ_.push_back(std::make_pair((i * winH) * W + j * winW - 1 + k * W, blkMap_[blk - 1]));
                } else {
                    const int plid = blkMap_[blk];
                    if (i > 0 && blkMap_[blk - Nw] != plid)
                        for (int k = 0; k < winW - 1; ++k) growQ_.push_back(std::make_pair((i * winH) * W + j * winW + k, plid));
                    if (j > 0 && blkMap_[blk - 1] != plid)
                        for (int k = 1; k < winH; ++k) growQ_.push_back(std::make_pair((i * winH) * W + j * winW + k * W, plid));
                }
            }
    }

    void grow_regions() {   // floodFill (:422-471)
        std::vector<float> &distMap = distMap_;
        distMap.assign((size_t)H * W, std::numeric_limits<float>::max());
        for (size_t k = 0; k < growQ_.size(); ++k) {
            const int seed = growQ_[k].first, plid = growQ_[k].second;
            const int sy = seed / W, sx = seed - sy * W;
            const Node &pl = nodes_[planes_[plid]];
            int nb4[4] = {-1, -1, -1, -1};
            const int nNb = neighbours4(sy, sx, H, W, nb4);
            for (int t = 0; t < nNb; ++t) {
                const int c = nb4[t];
                int32_t &trail = member_[c];
                if (trail <= -6) continue;
                if (trail >= 0 && trail == plid) continue;
                const int cy = c / W, cx = c - cy * W;
                const int by = cy / winH, bx = cx / winW;
                if (by < Nh && bx < Nw && blkMap_[by * Nw + bx] >= 0) continue;   // only pixels outside the plane windows
                double pt[3] = {0, 0, 0};
                float cdist = -1;
                bool close = false;
                if (point(cy, cx, pt)) {
                    cdist = (float)std::abs(pl.normal[0] * (pt[0] - pl.center[0]) + pl.normal[1] * (pt[1] - pl.center[1]) + pl.normal[2] * (pt[2] - pl.center[2]));
                    close = std::pow(cdist, 2) < 9 * pl.mse + 1e-5;   // point-plane distance within 3 sigma
                }
                if (close) {
                    if (trail >= 0 && similarity(pl, nodes_[planes_[trail]]) >= T.p.similarity_th_refine) connect(planes_[trail], planes_[plid]);
                    float &old = distMap[c];
                    if (cdist < old) { trail = plid; old = cdist; growQ_.push_back(std::make_pair(c, plid)); }
                    else if (trail < 0) trail -= 1;
                } else if (trail < 0) {
                    trail -= 1;
                }
            }
        }
    }

    void refine() {   // refineDetails (:296-372)
        std::vector<char> &validPlane = validPlane_;
        erode_blocks(validPlane);
        grow_regions();
        std::vector<int> &old = oldPlanes_;
        old.assign(planes_.begin(), planes_.end());
        planes_.clear();
        heap_.clear();
        for (size_t i = 0; i < old.size(); ++i)
            if (validPlane[i]) heap_push(old[i]);
        cluster();
        std::vector<int> &relabel = relabel_;
        relabel.assign(old.size(), -1);
        for (size_t i = 0; i < old.size(); ++i) {
            if (!validPlane[i]) continue;
            const int root = find(nodes_[old[i]].rid);
            for (size_t j = 0; j < planes_.size(); ++j)
                if (root == nodes_[planes_[j]].rid) { relabel[i] = (int)j; break; }
        }
        const bool lists = sink_ && sink_->offsets && sink_->indices && (int)planes_.size() <= sink_->maxPlanes;
        if (lists) {   // pMembership (:341-361): sizes first, so every plane's pixels land contiguously and in raster order
            std::vector<int> &cur = u_;
            cur.assign(planes_.size() + 1, 0);
            for (size_t i = 0, nPx = (size_t)W * H; i < nPx; ++i) {
                const int32_t plid = member_[i];
                if (plid >= 0 && relabel[plid] >= 0) cur[relabel[plid] + 1]++;
            }
            for (size_t j = 0; j < planes_.size(); j++) cur[j + 1] += cur[j];
            for (size_t j = 0; j <= planes_.size(); j++) sink_->offsets[j] = cur[j];
        }
        for (size_t i = 0, nPx = (size_t)W * H; i < nPx; ++i) {
            int32_t &plid = member_[i];
            if (plid >= 0 && relabel[plid] >= 0) {   // anything else keeps its value (old id or visit counter), as in the reference
                plid = relabel[plid];
                if (lists) sink_->indices[u_[plid]++] = (int32_t)i;
            }
        }
    }
};

// CPUs this process may actually use: hardware threads, limited by the affinity mask and by the cgroup CPU quota (cpu.max of cgroup v2 /
// cpu.cfs_quota_us of v1).  More runnable threads than that only burn the quota early in each period and are then throttled together
// (measured on a 256-thread host with a 16-CPU quota: 64 workers -> every third call stalled for 60-80 ms).
int usable_cpus() {
    int n = std::max(1, (int)std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(n, std::max(1, CPU_COUNT(&set)));
    long long quota = -1, period = 0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64] = {0};
        if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
        fclose(f);
    } else if (FILE *fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        if (fscanf(fq, "%lld", &quota) != 1) quota = -1;
        fclose(fq);
        if (FILE *fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(fp, "%lld", &period) != 1) period = 0; fclose(fp); }
    }
    if (quota > 0 && period > 0) n = std::min(n, (int)std::max(1ll, (quota + period - 1) / period));
    return n;
}

// Host workers for the per-frame clustering (frames are independent).  The WORKSPACES persist between calls (no allocation, no page faults in
// the steady state); the threads are started per call (freshly created threads are spread over idle cores at once; ~20 us each).  The caller
// takes part with its own workspace, so a one-frame call starts no thread at all.
class SegPool {
public:
    static SegPool &get() { static SegPool p; return p; }
    int workers() const { return maxWorkers_ + 1; }   // the caller takes part
    long long thread_shortfall() const { return threadShortfall_.load(); }   // worker threads that could not be started since the process began
    // fn(frame, workspace) for frame = 0 .. nFrames-1, each exactly once; returns when all are done
    void run(int nFrames, const std::function<void(int, FrameSegmenter &)> &fn) {
        std::lock_guard<std::mutex> one(callMutex_);   // one batch at a time
        if (nFrames <= 0) return;
        const int nWorkers = std::min(nFrames - 1, maxWorkers_);
        while ((int)ws_.size() < nWorkers + 1) ws_.emplace_back(new FrameSegmenter);
        std::atomic<int> next{0};
        // An exception inside a worker (std::bad_alloc in a workspace, ...) must not terminate the process: the first one is kept, the other
        // frames are abandoned, every started thread is joined, and the caller's thread rethrows it -- into the C ABI's exception barrier.
        std::exception_ptr failure;
        std::mutex failMutex;
        auto work = [&](FrameSegmenter &ws) {
            try {
                for (;;) {
                    const int f = next.fetch_add(1);
                    if (f >= nFrames) break;
                    fn(f, ws);
                }
            } catch (...) {
                std::lock_guard<std::mutex> g(failMutex);
                if (!failure) failure = std::current_exception();
                next.store(nFrames);
            }
        };
        std::vector<std::thread> threads;
        threads.reserve(nWorkers);
        try {
            for (int t = 0; t < nWorkers; t++) threads.emplace_back([&, t]() { work(*ws_[t + 1]); });
        } catch (...) {   // thread creation failed (std::system_error): the threads that did start finish the work together with the caller
            std::lock_guard<std::mutex> g(failMutex);
            if (peac_env().strictThreads && !failure) failure = std::current_exception();
            // the degradation is recorded, not silent: a counter the debug hook reads, and -- once per process -- a line in msl_last_error()'s
            // buffer (the call still succeeds) and on stderr
            const int miss = nWorkers - (int)threads.size();
            if (threadShortfall_.fetch_add(miss) == 0) {
                set_error("msl_peac: only %d of %d worker threads could be started (resource limit?); the call continues with fewer", (int)threads.size(), nWorkers);
                fprintf(stderr, "[msl_peac] warning: only %d of %d worker threads could be started; continuing with fewer\n", (int)threads.size(), nWorkers);
            }
        }
        work(*ws_[0]);
        for (auto &th : threads) th.join();
        if (failure) std::rethrow_exception(failure);
    }

private:
    // MSL_PEAC_THREADS overrides the worker count (1 = everything on the calling thread)
    // and one process per GPU shares the node's CPUs with its sibling ranks: LOCAL_WORLD_SIZE (set by torch.distributed.run) divides the budget,
    // so 8 ranks do not start 8 x usable_cpus() workers
    static int worker_budget() {
        if (peac_env().threadsSet) return peac_env().threads;
        return std::max(1, usable_cpus() / peac_env().localRanks);
    }
    SegPool() : maxWorkers_(std::max(0, std::min(64, worker_budget()) - 1)) {
        if (peac_env().poolReport) fprintf(stderr, "[msl_peac] pool workers = %d (usable CPUs %d)\n", maxWorkers_ + 1, usable_cpus());
    }
    const int maxWorkers_;
    std::atomic<long long> threadShortfall_{0};
    std::mutex callMutex_;
    std::vector<std::unique_ptr<FrameSegmenter>> ws_;
};

}  // namespace

namespace msl {
namespace peac {

const PeacEnv &peac_env() {
    static const PeacEnv env = [] {
        PeacEnv e;
        const char *v = getenv("MSL_PEAC_TIMING");
        e.timing = !v ? 0 : atoi(v) >= 2 ? 2 : 1;
        v = getenv("MSL_PEAC_SIMD");
        e.simd = v ? atoi(v) : -1;
        if (e.simd != 0 && e.simd != 2 && e.simd != 4 && e.simd != 8) e.simd = -1;
        v = getenv("MSL_PEAC_LANES");
        e.lanes = v ? atoi(v) : 16;
        if (e.lanes != 2 && e.lanes != 4 && e.lanes != 8) e.lanes = 16;
        v = getenv("MSL_PEAC_THREADS");
        e.threadsSet = v != nullptr; e.threads = v ? atoi(v) : 0;
        v = getenv("LOCAL_WORLD_SIZE");
        e.localRanks = v ? std::max(1, atoi(v)) : 1;
        e.strictThreads = getenv("MSL_PEAC_STRICT_THREADS") != nullptr;
        e.poolReport = getenv("MSL_PEAC_POOL_REPORT") != nullptr;
        return e;
    }();
    return env;
}

int peac_workers() { return SegPool::get().workers(); }

int check_call(PeacImages &I, const msl_peac_params *prm, const PeacOutputs *O, const char *hostEntry) {
    if (O && (!prm || !O->membership || prm->min_support < 1 || (O->planes && O->maxPlanes < 1) || ((O->offsets || O->indices) && !O->planes) ||
              ((O->offsets != nullptr) != (O->indices != nullptr)) || (O->indices && !prm->do_refine))) {
        if (hostEntry) set_error("%s: invalid argument", hostEntry);
        else set_error("msl_peac: invalid argument (plane outputs need max_planes >= 1; vertex lists need planes_out, both list arrays and do_refine)");
        return MSL_ERR_INVALID;
    }
    bool bad = !prm || !I.depth || I.width < 2 || I.height < 2 || prm->window_w < 1 || prm->window_h < 1 || I.stride < (size_t)I.width * 2;
    if (hostEntry) bad = bad || I.n_frames < 0;
    else   // k_peac_fit stages 72 bytes per window point in dynamic LDS: up to 900 points (e.g. 30 x 30) fit the 64 KB a launch may ask for
        bad = bad || I.n_frames < 1 || prm->window_w * prm->window_h > 900 ||
              (I.n_frames > 1 && I.frameStride < I.stride * (size_t)(I.height - 1) + (size_t)I.width * 2) || I.fx == 0 || I.fy == 0;
    if (bad) { set_error("%s: invalid argument", hostEntry ? hostEntry : "msl_peac"); return MSL_ERR_INVALID; }
    I.cw = (I.width + 1) / 2; I.ch = (I.height + 1) / 2;
    I.Nw = I.cw / prm->window_w; I.Nh = I.ch / prm->window_h;
    I.nBlocks = (size_t)I.Nw * I.Nh; I.nVert = (size_t)I.cw * I.ch;
    if (!hostEntry && I.nBlocks == 0) { set_error("msl_peac: image smaller than one window"); return MSL_ERR_INVALID; }
    return MSL_OK;
}

}  // namespace peac
}  // namespace msl

namespace {
// per-frame sinks over the caller's arrays (none when no plane output is wanted)
std::vector<PlaneSink> make_sinks(const PeacImages &I, const PeacOutputs &O) {
    std::vector<PlaneSink> sinks;
    if (!O.planes) return sinks;
    sinks.resize(I.n_frames);
    for (int f = 0; f < I.n_frames; f++) {
        sinks[f].planes = O.planes + (size_t)f * O.maxPlanes;
        sinks[f].offsets = O.offsets ? O.offsets + (size_t)f * (O.maxPlanes + 1) : nullptr;
        sinks[f].indices = O.indices ? O.indices + (size_t)f * I.nVert : nullptr;
        sinks[f].maxPlanes = O.maxPlanes; sinks[f].overflow = false;
    }
    return sinks;
}
int check_sinks(const std::vector<PlaneSink> &sinks, int max_planes) {
    for (const PlaneSink &k : sinks)
        if (k.overflow) { set_error("msl_peac: a frame has more than max_planes = %d planes", max_planes); return MSL_ERR_CAPACITY; }
    return MSL_OK;
}
}  // namespace

namespace msl {
namespace peac {

int segment_frames(const PeacImages &I, const msl_peac_params &prm, const msl_peac_block *blocks, const uint16_t *half, const PeacOutputs &O) {
    std::vector<PlaneSink> sinks = make_sinks(I, O);
    const int n_frames = I.n_frames;
    const bool timing = peac_env().timing != 0;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<long> startUs(timing ? n_frames : 0), durUs(timing ? n_frames : 0);
    SegPool::get().run(n_frames, [&](int f, FrameSegmenter &seg) {
        const auto a = std::chrono::steady_clock::now();
        seg.configure(I, prm, half + (size_t)f * I.nVert);
        seg.set_sink(sinks.empty() ? nullptr : &sinks[f]);
        const int n = seg.run(blocks + (size_t)f * I.nBlocks, O.membership + (size_t)f * I.nVert);
        seg.set_sink(nullptr);
        if (O.nPlanes) O.nPlanes[f] = n;
        if (timing) {
            startUs[f] = (long)std::chrono::duration_cast<std::chrono::microseconds>(a - t0).count();
            durUs[f] = (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - a).count();
        }
    });
    if (timing && n_frames > 1) {
        long ms = 0, md = 0, sd = 0;
        for (int f = 0; f < n_frames; f++) { ms = std::max(ms, startUs[f]); md = std::max(md, durUs[f]); sd += durUs[f]; }
        fprintf(stderr, "[msl_peac] pool: latest frame start %ld us, longest frame %ld us, mean frame %ld us\n", ms, md, sd / n_frames);
    }
    return check_sinks(sinks, O.maxPlanes);
}

bool graphs_for_device(const PeacImages &I, const msl_peac_params &prm, const msl_peac_block *blocks, const ClusterLayout &L, int *cin) {
    std::atomic<int> bad{0};
    SegPool::get().run(I.n_frames, [&](int f, FrameSegmenter &seg) {
        seg.configure(I, prm, nullptr);   // (graph initialisation reads the block fits only)
        if (!seg.graph_for_device(blocks + (size_t)f * L.nB, cin + L.heap + (size_t)f * L.nB, cin + L.heapCount + f, cin + L.edges + (size_t)f * L.maxE * 2,
                                  cin + L.edgeCount + f, L.maxE))
            bad++;
    });
    return bad.load() == 0;
}

int finish_from_device(const PeacImages &I, const msl_peac_params &prm, const uint16_t *half, const ClusterLayout &L, const int *cout, const PlaneOut *planes,
                       const PeacOutputs &O) {
    std::vector<PlaneSink> sinks = make_sinks(I, O);
    SegPool::get().run(I.n_frames, [&](int f, FrameSegmenter &seg) {
        seg.configure(I, prm, half + (size_t)f * I.nVert);
        seg.set_sink(sinks.empty() ? nullptr : &sinks[f]);
        const int n = seg.finish_from_device(planes + (size_t)f * L.maxPl, cout[L.nPlanes + f], cout + L.parent + (size_t)f * L.nB, cout + L.setSize + (size_t)f * L.nB,
                                             O.membership + (size_t)f * I.nVert);
        seg.set_sink(nullptr);
        if (O.nPlanes) O.nPlanes[f] = n;
    });
    return check_sinks(sinks, O.maxPlanes);
}

}  // namespace peac
}  // namespace msl

extern "C" {

void msl_peac_default_params(msl_peac_params *p) noexcept {
    try {   // ahc::ParamSet / ahc::PlaneFitter defaults (AHCParamSet.hpp:68-76, AHCPlaneFitter.hpp:157-161)
    if (!p) return;
    p->window_w = 10; p->window_h = 10; p->min_support = 3000; p->max_step = 100000; p->do_refine = 1; p->erode_type = 2; p->init_loose = 0; p->_pad = 0;
    p->depth_sigma = 1.6e-6; p->std_tol_init = 5; p->std_tol_merge = 8; p->z_near = 500; p->z_far = 4000;
    p->angle_near = ((15.0) * M_PI / 180.0); p->angle_far = ((90.0) * M_PI / 180.0);
    p->similarity_th_merge = std::cos(((60.0) * M_PI / 180.0)); p->similarity_th_refine = std::cos(((30.0) * M_PI / 180.0));
    p->depth_alpha = 0.04; p->depth_change_tol = 0.02;
    } MSL_ABI_CATCH_VOID
}

int msl_peac_extract_from_blocks(const msl_peac_block *blocks, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width, int height,
                                 int n_frames, float fx, float fy, float cx, float cy, float depth_map_factor, const msl_peac_params *params,
                                 int32_t *membership_out, int32_t *n_planes_out, int max_planes, msl_peac_plane *planes_out, int32_t *vertex_offsets_out,
                                 int32_t *vertex_indices_out) noexcept {
    try {
    if (!blocks) { set_error("msl_peac_extract_from_blocks: invalid argument"); return MSL_ERR_INVALID; }
    PeacImages I{0, depth, depth_stride_bytes, frame_stride_bytes, width, height, n_frames, MSL_MEM_HOST, fx, fy, cx, cy, depth_map_factor};
    const PeacOutputs O{membership_out, n_planes_out, max_planes, planes_out, vertex_offsets_out, vertex_indices_out};
    const int rc = check_call(I, params, &O, "msl_peac_extract_from_blocks");
    if (rc != MSL_OK) return rc;
    std::vector<uint16_t> half(I.nVert * n_frames);   // raw depth of the cloud vertices (even rows / columns), as k_peac_half packs it
    for (int f = 0; f < n_frames; f++)
        for (int r = 0; r < I.ch; r++) {
            const uint16_t *row = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(depth) + (size_t)f * frame_stride_bytes + (size_t)(2 * r) * depth_stride_bytes);
            uint16_t *o = half.data() + ((size_t)f * I.ch + r) * I.cw;
            for (int c = 0; c < I.cw; c++) o[c] = row[2 * c];
        }
    return segment_frames(I, *params, blocks, half.data(), O);
    } MSL_ABI_CATCH_INT
}
int msl_peac_membership_from_blocks(const msl_peac_block *blocks, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width,
                                    int height, int n_frames, float fx, float fy, float cx, float cy, float depth_map_factor,
                                    const msl_peac_params *params, int32_t *membership_out, int32_t *n_planes_out) noexcept {
    try {
    return msl_peac_extract_from_blocks(blocks, depth, depth_stride_bytes, frame_stride_bytes, width, height, n_frames, fx, fy, cx, cy, depth_map_factor, params,
                                        membership_out, n_planes_out, 0, nullptr, nullptr, nullptr);
    } MSL_ABI_CATCH_INT
}

// Where a call of n_frames keyframes clusters: 1 = on the device (one wave per frame, ~13-20 ms per call whatever the number of frames), 0 = on
// the host workers (~2 ms per frame and worker).  The device wins once a call holds more than about eight frames per worker this process may
// use -- and the worker count is the CPU budget divided by LOCAL_WORLD_SIZE, so the 8 ranks of a node (2 workers each on a 16-CPU allowance)
// take the device path for config 4's 128-keyframe calls instead of collapsing onto shared host cores.  MSL_PEAC_CLUSTER=host / device forces one side.
int msl_debug_peac_cluster_on_device(int n_frames) noexcept {
    try {
    const char *mode = getenv("MSL_PEAC_CLUSTER");
    if (mode && !strcmp(mode, "host")) return 0;
    if (mode && !strcmp(mode, "device")) return 1;
    return n_frames > 8 * SegPool::get().workers() ? 1 : 0;
    } MSL_ABI_CATCH_INT
}

long long msl_debug_peac_thread_shortfall(void) noexcept { try { return SegPool::get().thread_shortfall(); } MSL_ABI_CATCH_(return -1) }

int msl_debug_peac_mse(const msl_peac_stats *stats, size_t n, int lanes, double *mse_out) noexcept {
    try {
    if (n == 0) return MSL_OK;
    const int level = host_simd_level();
    if (!stats || !mse_out || !(lanes == 0 || lanes == 2 || lanes == 4 || lanes == 8 || lanes == 16)) { set_error("msl_debug_peac_mse: invalid argument"); return MSL_ERR_INVALID; }
    if ((lanes == 16 && level < 8) || (lanes >= 4 && level < 4) || (lanes >= 2 && level < 2)) { set_error("msl_debug_peac_mse: %d lanes need a wider instruction set than this CPU (or MSL_PEAC_SIMD) allows", lanes); return MSL_ERR_INVALID; }
    if (lanes == 0) { for (size_t i = 0; i < n; i++) mse_out[i] = plane_mse(stats[i]); return MSL_OK; }
    alignas(64) double in[10 * 16], out[16];
    for (size_t i0 = 0; i0 < n; i0 += lanes) {
        for (int l = 0; l < lanes; l++) {
            const msl_peac_stats &y = stats[i0 + l < n ? i0 + l : i0];
            const double v[10] = {y.sx, y.sy, y.sz, y.sxx, y.syy, y.szz, y.sxy, y.syz, y.sxz, (double)y.N};
            for (int k = 0; k < 10; k++) in[k * lanes + l] = v[k];
        }
        plane_mse_group(lanes, in, out);
        for (int l = 0; l < lanes && i0 + l < n; l++) mse_out[i0 + l] = out[l];
    }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}


// Test hook of the exception barrier (tests/test_abi.py): raises the given failure INSIDE the library, behind the boundary.
//   0: std::bad_alloc  1: std::runtime_error  2: a non-standard exception  3: std::bad_alloc in a worker thread of the plane extractor's pool
int msl_debug_throw(int kind) noexcept {
    try {
        if (kind == 0) throw std::bad_alloc();
        if (kind == 1) throw std::runtime_error("msl_debug_throw");
        if (kind == 2) throw 42;
        if (kind == 3) SegPool::get().run(4, [](int f, FrameSegmenter &) { if (f == 2) throw std::bad_alloc(); });
        return MSL_OK;
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
