// msl_match_handle.h -- the matcher handle, its staging of caller arrays (Stage), the forwarder of the *_batch entry points, the two forms of
// an entry that checks before it touches a device (handle_form, batch_form: every entry on the handle but msl_match_descriptor_distance)
// with the list of its NULLs (none_null), the limits that several entry points share (MAX_CAP .. MAX_MCAP, in_range, at_least_one, table_limits,
// line_table_limits, levels_ok, frame_ok, log_scale_ok; the plane chain's are in msl_plane_tables.h) and the row readback of the debug entry points (last_call_row); shared by msl_match.hip,
// msl_line_match.hip, msl_pose.hip, msl_plane.hip, msl_bow.hip, msl_reloc.hip, msl_pnp.hip, msl_line3d.hip, msl_triangulate.hip, msl_fuse.hip,
// msl_mappoint.hip, msl_line_fuse.hip, msl_local_map.hip, msl_cull.hip, msl_plane_cloud.hip, msl_keyframe.hip, msl_keyframe_planes.hip, msl_observations.hip and msl_connections.hip (internal).
#pragma once

#include "msl_common.h"

#include <initializer_list>
#include <vector>

namespace msl {
// What msl_pnp_ransac's table N -> (minInliers, maxIts) was built from (no padding: compared bytewise).
struct PnpKey { double probability; int32_t min_inliers, max_iterations, min_set; float epsilon; int32_t cap, zero; };

// Limits that several entry points share: keypoints of a frame or keyframe (feature indices fit 13 bits, item positions 16), keyframes of
// a keyframe table, points of a point table; keylines of a frame or keyframe (indices fit 8 bits), lines of a line table; local map points
// or local map lines of a frame (positions fit the 16-bit picks of the hand-out).
constexpr int MAX_CAP = 8192, MAX_TAB = 4096, MAX_PTS = 1 << 20;
constexpr int MAX_KLCAP = 256, MAX_LINES = 1 << 20;
constexpr int MAX_MCAP = 32768;

// An int argument inside lo .. hi; false with the error set ("who: name value outside lo .. hi").
inline bool in_range(const char *who, const char *name, int value, int lo, int hi) {
    if (value < lo || value > hi) { set_error("%s: %s %d outside %d .. %d", who, name, value, lo, hi); return false; }
    return true;
}

// An int argument with no upper limit, such as the frames or pairs of a call; false with the error set ("who: name value below 1").
inline bool at_least_one(const char *who, const char *name, int n) {
    if (n < 1) { set_error("%s: %s %d below 1", who, name, n); return false; }
    return true;
}

// The limits of a call that takes a keyframe table and a point table; false with the error set.
inline bool table_limits(const char *who, int n_tab, int cap, int n_pts) {
    if (n_tab < 1 || n_tab > MAX_TAB) { set_error("%s: n_tab %d outside 1 .. %d", who, n_tab, MAX_TAB); return false; }
    if (cap < 1 || cap > MAX_CAP) { set_error("%s: cap %d outside 1 .. %d", who, cap, MAX_CAP); return false; }
    if (n_pts < 1 || n_pts > MAX_PTS) { set_error("%s: n_pts %d outside 1 .. %d", who, n_pts, MAX_PTS); return false; }
    return true;
}

// The same for a keyframe table of keylines and a line table
inline bool line_table_limits(const char *who, int n_tab, int klcap, int n_lines) {
    if (n_tab < 1 || n_tab > MAX_TAB) { set_error("%s: n_tab %d outside 1 .. %d", who, n_tab, MAX_TAB); return false; }
    if (klcap < 1 || klcap > MAX_KLCAP) { set_error("%s: klcap %d outside 1 .. %d", who, klcap, MAX_KLCAP); return false; }
    if (n_lines < 1 || n_lines > MAX_LINES) { set_error("%s: n_lines %d outside 1 .. %d", who, n_lines, MAX_LINES); return false; }
    return true;
}

// The length of a call's scale tables; false with the error set.
inline bool levels_ok(const char *who, int nlevels) {
    if (nlevels < 1 || nlevels > MSL_MATCH_MAX_LEVELS) { set_error("%s: nlevels %d outside 1 .. %d", who, nlevels, MSL_MATCH_MAX_LEVELS); return false; }
    return true;
}

// The frame a search projects into: the length of its scale tables, image bounds that are not empty (a NaN bound is refused) and a focal
// length to divide by; false with the error set.
inline bool frame_ok(const char *who, const msl_match_params &p) {
    if (!levels_ok(who, p.nlevels)) return false;
    if (!(p.maxX > p.minX)) { set_error("%s: image bounds minX %g .. maxX %g are empty", who, (double)p.minX, (double)p.maxX); return false; }
    if (!(p.maxY > p.minY)) { set_error("%s: image bounds minY %g .. maxY %g are empty", who, (double)p.minY, (double)p.maxY); return false; }
    if (p.fx == 0) { set_error("%s: fx is 0", who); return false; }
    return true;
}

// log_scale_factor = log(scaleFactor) of a search that predicts a scale level (a NaN is refused); false with the error set.
inline bool log_scale_ok(const char *who, float log_scale_factor) {
    if (!(log_scale_factor > 0)) { set_error("%s: log_scale_factor %g is not above 0", who, (double)log_scale_factor); return false; }
    return true;
}

// The refusal of a call whose host-side check (msl_index_check.h) left its reason in why
inline int refuse(const char *who, const char *why) { set_error("%s: %s", who, why); return MSL_ERR_INVALID; }

// The arrays a call requires, by name: the first that is NULL is the refusal; false with the error set.  An optional array is left out of the
// list, and arrays that a condition makes required are a second call under that condition.
struct Named { const char *name; const void *p; };
inline bool none_null(const char *who, std::initializer_list<Named> args) {
    for (const Named &a : args)
        if (!a.p) { set_error("%s: %s is NULL", who, a.name); return false; }
    return true;
}
#define MSL_NAMED(x) Named{#x, x}
}  // namespace msl

// One matcher object = one ORBmatcher of the reference (src/ORBmatcher.cc:41): its own stream and its own scratch, used by one thread at a time;
// the device is re-bound at every entry like the other handles.  The line searches (= the tracker's LSDmatcher), msl_pose_optimize, the
// plane association and the bag-of-words calls run on it too.
struct msl_match {
    // The most arrays one entry point stages: msl_keyframe_decision (14 inputs, 2 in/out, 12 outputs).
    static constexpr int STAGE_SLOTS = 28;
    int device = 0;
    hipStream_t stream = nullptr; bool ownStream = true;
    // Scratch the kernels of a call hand to one another.  Device-memory calls are asynchronous and ordered only by the stream, so each
    // buffer keeps its one role.
    msl::DevBuf items, cellStart, mode, cand, candCnt;                 // the point searches: grid, search mode, candidates
    msl::DevBuf trk, inView;                                           // msl_match_local_points: per-point track / in-view
    msl::DevBuf lineQ, lineTrk, lineView;                              // the line searches: per-line queries / tracks / in-view
    msl::DevBuf planeDis;                                              // msl_plane_associate: [frame][map plane][64] distances
    msl::DevBuf bowW;                                                  // msl_bow_transform: per-feature word weights
    msl::DevBuf relocCnt, relocFirst, relocScore;                      // msl_reloc_candidates: [frame][slot] shared words / first shared word / L1 score
    // msl_pnp_ransac: the compacted correspondences, per-hypothesis counts / masks / poses and Refine()'s lists in one buffer (the offsets of
    // the last call's per-hypothesis arrays are kept for msl_pnp_debug_hypotheses); the SetRansacParameters table and what it was built from.
    msl::DevBuf pnp, pnpTable;
    msl::PnpKey pnpKey{}; bool pnpTableValid = false;
    int pnpPairs = 0, pnpKmax = 0; size_t pnpOffK = 0, pnpOffCnt = 0, pnpOffRt = 0, pnpOffBr = 0;
    msl::DevBuf line3d;                                                // msl_lines_3d: per keyline the record msl_lines_3d_debug reads
    int line3dFrames = 0, line3dLcap = 0;                              // the shape of the last call
    // msl_triangulate_new_points: per table keyframe the sorted (node, feature) keys, per (item, neighbour) the pair geometry, per
    // (item, neighbour, idx1) the candidate with its verdict (msl_debug_triangulate reads the last two)
    msl::DevBuf triKeys, triPair, triRec;
    int triItems = 0, triNcap = 0, triCap = 0;                         // the shape of the last call
    // msl_fuse_map_points: per table keyframe the sorted ids its slots hold, per (item, candidate) the projection msl_debug_fuse reads;
    // msl_fuse_candidates: per item in flight the first position of every point id
    msl::DevBuf fuseHeld, fuseRec, fuseFirst;
    int fuseItems = 0, fuseLcap = 0;                                   // the shape of the last msl_fuse_map_points call
    msl::DevBuf lfuseRec;                                              // msl_fuse_map_lines: per (item, candidate) the query, which msl_debug_line_fuse reads
    int lfuseItems = 0, lfuseLcap = 0;                                 // the shape of the last msl_fuse_map_lines call
    // msl_local_points / msl_local_lines: per (frame in flight, table row) the stamp of the ordered compaction, per (frame in flight, list
    // position) the kept count and its scan; the stamps of one group of frames stay under lmBudget bytes (msl_debug_local_map_budget)
    msl::DevBuf lmStamp, lmCount;
    size_t lmBudget = (size_t)256 << 20;
    // msl_plane_clouds / msl_map_plane_merge: per resident workgroup the int64 sums, counts and colour sums of the voxels of a cloud too
    // large to accumulate in LDS; per item ((frame, detector plane) or (frame, frame plane)) the coarse cloud, its count, status and
    // coefficients
    msl::DevBuf pcSlab, pcWork;
    // msl_manhattan_observe: per frame the merged tail of each Manhattan table and the lower bounds of its new keys, built before the copy back
    msl::DevBuf kfpScratch;
    // msl_observations_apply: the work slot of every point (-1: none) and the block sums of the rebuild; per work slot the point's arrays
    // and its list of at most MSL_OBS_MAX observations; the slot writes in execution order
    msl::DevBuf obsIndex, obsSlots, obsWrites;
    // msl_connections_apply: per keyframe how its ordered row is to be rebuilt and whether an op wrote it; the two counters of the walk
    msl::DevBuf connWork;
    // Device copies of host-memory arguments, one pool for every entry point (msl::Stage deals the slots out in declaration order).
    // Sharing is sound because every call that touches the pool returns with the stream drained (Stage::finish synchronises whenever
    // either side is host memory, and only then is a slot used), so no slot is live when the next call starts.
    msl::DevBuf stage[STAGE_SLOTS];
    unsigned ldsSet = 0;                                               // bit k: kernel k's dynamic-LDS limit is raised (msl::allow_lds)
};

namespace msl {

// The device-indexed convenience entry points share one lazily created handle per device, serialised by one mutex.  The handles are
// never destroyed (see DevBuf).
extern msl_match *g_default[16];
extern std::mutex g_default_mutex;

inline msl_match *default_handle(int device) {   // g_default_mutex held
    msl_match *&h = g_default[device & 15];
    if (!h) h = msl_match_create(device);
    return h;
}

// The body of a *_batch form: run_x(h, args...) on the device's shared handle, synchronous.  sync_legacy: the call reads device memory
// that is complete, or enqueued on the legacy default stream, when the call is made (as before the handle existed).
template <class Run, class... A>
int abi_call_default(Run run, int device, bool sync_legacy, A... a) {
    std::lock_guard<std::mutex> lock(g_default_mutex);
    msl_match *h = default_handle(device);
    if (!h) return MSL_ERR_NO_DEVICE;
    if (sync_legacy) { if (bind_device(device) == MSL_OK) (void)hipStreamSynchronize(0); }
    int rc = run(h, a...);
    if (rc == MSL_OK) rc = msl_match_sync(h);
    return rc;
}

// The two forms of an entry: check_x(args...) makes no HIP call and comes first, so a refusal is made before the handle, or
// the device's shared one, is touched; launch_x(h, args...) starts at bind_device.
template <class Check, class Launch, class... A>
int handle_form(const char *who, Check check, Launch launch, msl_match *h, A... a) {
    if (!h) { set_error("%s: h is NULL", who); return MSL_ERR_INVALID; }
    const int rc = check(a...);
    return rc != MSL_OK ? rc : launch(h, a...);
}
template <class Check, class Launch, class... A>
int batch_form(Check check, Launch launch, int device, bool sync_legacy, A... a) {
    const int rc = check(a...);
    return rc != MSL_OK ? rc : abi_call_default(launch, device, sync_legacy, a...);
}

// What a debug entry point reads of the handle's last call: row `row` of the scratch `buf`, n records long, once the stream is drained.
template <class Rec>
int last_call_row(msl_match *h, const DevBuf &buf, size_t row, size_t n, std::vector<Rec> &rec) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    rec.resize(n);
    MSL_HIP_TRY(hipMemcpy(rec.data(), (const Rec *)buf.p + row * n, n * sizeof(Rec), hipMemcpyDeviceToHost));
    return MSL_OK;
}

// Kernels that ask for more dynamic LDS than the default limit: the limit is raised once per handle (= per device) and kernel.
enum LdsKernel { LDS_MATCH_ASSIGN, LDS_LOCAL_ASSIGN, LDS_LINE_ASSIGN_LAST, LDS_LINE_ASSIGN_LOCAL, LDS_BOW_VECTOR, LDS_MATCH_BOW, LDS_KF_ASSIGN, LDS_RELOC_SELECT, LDS_TRI_GROUP, LDS_FUSE_HELD, LDS_FUSE_RESOLVE, LDS_PC_VOXEL, LDS_PC_MERGE, LDS_POINTS3D };
template <class K>
hipError_t allow_lds(msl_match *h, LdsKernel k, K kernel, size_t max_bytes) {
    if (h->ldsSet >> k & 1u) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes);
    if (e == hipSuccess) h->ldsSet |= 1u << k;
    return e;
}

// The caller's arrays of one entry point as device pointers.  Each array is declared once, with its element count: inputs live in `mem`
// memory, in/out arrays and outputs in `out_mem` memory.  Device memory: the declaration returns the caller's own pointer.  Host memory:
// a slot of the handle's pool, grown to the array's size; inputs and in/outs are already enqueued for copy, in/outs and outputs are
// copied back by finish().  A null (optional) array returns null.  Errors are kept: check error() once before launching.
class Stage {
  public:
    Stage(msl_match *h, msl_mem mem, msl_mem out_mem) : h_(h), mem_(mem), outMem_(out_mem) {}
    template <class T> const T *in(const T *user, size_t count) { return (const T *)take(const_cast<T *>(user), sizeof(T) * count, mem_, true, false); }
    template <class T> T *inout(T *user, size_t count) { return (T *)take(user, sizeof(T) * count, outMem_, true, true); }
    template <class T> T *out(T *user, size_t count) { return (T *)take(user, sizeof(T) * count, outMem_, false, true); }
    // An in/out array that the ABI lists before `mem` (msl_observations_apply's tables, edited in place)
    template <class T> T *inout_in_mem(T *user, size_t count) { return (T *)take(user, sizeof(T) * count, mem_, true, true); }
    // An optional output the kernels always write to the handle's scratch `dev`: the pointer they write as well (device memory: the
    // caller's array, or null), while a host-memory array is copied back from the scratch by finish().
    template <class T> T *out_of_scratch(T *user, const T *dev, size_t count) {
        if (outMem_ != MSL_MEM_HOST) return user;
        if (user) copy_back(user, dev, sizeof(T) * count);
        return nullptr;
    }
    hipError_t error() const { return err_; }
    // The end of the entry point.  Host-memory outputs are copied back; with host memory on either side the stream is drained, so the
    // caller's host arrays are theirs again (and the pool is free) on return.
    hipError_t finish();

  private:
    void *take(void *user, size_t bytes, msl_mem side, bool copy_in, bool back);
    void copy_back(void *user, const void *dev, size_t bytes);
    struct Back { void *user; const void *dev; size_t bytes; };
    msl_match *h_; msl_mem mem_, outMem_;
    hipError_t err_ = hipSuccess;
    int used_ = 0, nBack_ = 0;
    Back back_[msl_match::STAGE_SLOTS];
};

}  // namespace msl
