// msl_sf_handle.h -- the surfel handle, and what the host units of the surfel path share (internal, host only): msl_surfel.hip (lifecycle, staging,
// batch driver), msl_sf_store.hip (the resident map), msl_sf_hostvec.hip (the host-vector drop-in), msl_sf_debug.hip.  None of them holds a kernel.
#pragma once

#include "msl_sf.h"

struct msl_sf {
    int device = 0;
    msl::sf::SfDev dev{};
    int maxBatch = 1;              // keyframes per batch; slots = 2 * maxBatch (double-buffered sets)
    hipStream_t preStream = nullptr, mapStream = nullptr; bool ownStreams = true;
    size_t blkStride = 0;          // entries per per-sub-block count slice (blockSums: one slice; blockUpd: DEFER_WIN slices, one per keyframe of a window)
    unsigned long long kfClassic = 0, kfDeferred = 0;   // keyframes that went through the classic pair of launches / through deferred windows (msl_sf_debug_scratch, which = 5)
    int dealG = 0;                 // the k_fuse grid SfDev::deal currently is a permutation for (0: none yet) -- screen-position dealing, msl_sf_compact.hip
    hipStream_t copyStream = nullptr;   // host-image mode: the H2D copies of slot set i + 1 run beside the superpixel kernels of set i
    // Synchronisation state of one of the two slot sets.  h2d: the set's staged images have arrived (recorded by every host-image batch; msl_sf_staged_gray
    // hands it to other handles); pre / map: the set's last superpixel stage / map stage is done; copy: its pinned FrameDev staging has been read
    struct SlotSet { hipEvent_t h2d = nullptr, pre = nullptr, map = nullptr, copy = nullptr; bool preValid = false, mapValid = false, copyValid = false; } sets[2];
    unsigned long long batchNo = 0;
    int stagedSet = -1; size_t stagedGs = 0;   // slot set / row stride of the gray images the last host-image batch staged (msl_sf_staged_gray); -1: none
    int lastSlot = 0;
    // One image kind of host-image calls, staged per slot: 2 * maxBatch slots of `stride` bytes each
    struct ImageSlots {
        msl::DevBuf buf; size_t stride = 0;
        uint8_t *at(size_t slot) const { return (uint8_t *)buf.p + slot * stride; }
    };
    // The slot set, allocated to exactly 2 * maxBatch slots by alloc_slots: the per-slot arrays behind SfDev's bases, the pinned FrameDev staging,
    // and the images of host-image calls (allocated by the first such call; depth16: the raw 16-bit depth of msl_sf_fuse_resident_batch_d16)
    struct Slots {
        msl::DevBuf frames, seeds, seedsTmp, cand, candOk, fused, tex, fuseRec, index, amap, tmin, arec, pxInv, wl, wlCount, chunkAbort, changed;
        msl::PinBuf hFrames;
        ImageSlots gray, depth, member, depth16;
    } slot;
    msl::DevBuf d_ctr; msl::PinBuf h_ctr;   // the map's counters, and the CTR_COUNT of them read_ctr last read (host_ctr, live_count)
    msl::DevBuf d_tickets, d_delU, d_dc, d_projTab;
    bool propLds = false;        // t(s) of one keyframe fits the LDS: single-launch relaxation
    bool classicNext = true;     // the map was replaced from outside the keyframe chain (upload / restore / append / detach): its first keyframe takes the classic
                                 // pair of launches, whose compaction handles any number of stale or deleted slots at full speed
    msl::DevBuf d_new;
    // The resident map, replaced as a whole by map_realloc (layout: msl_sf_store.hip; its capacity in surfels: dev.cap).  rp: deferred compaction's
    // move lists, dense replay tables and staging
    struct MapBufs { msl::DevBuf store, blockSums, blockUpd, delList, srcOf, rp; } map;
    size_t liveBound = 0;        // host-side upper bound of the live count: last known count + nseeds per keyframe enqueued since
    size_t liveKnown = 0;        // the most recent live count the host has seen (exact at that time; only a hint for k_fuse's speculative loads)
    unsigned long long liveKnownKf = 0;   // ... and the number of keyframes that had been enqueued when it was exact: an older snapshot never replaces a newer one
    // asynchronous refresh of that bound: after every batch the live count is copied to pinned memory behind an event; a later call picks
    // up whatever has arrived, so the bound follows the real count a couple of batches late instead of forcing a pipeline drain
    // every capacity / nseeds keyframes
    static constexpr int NSNAP = 4;
    static constexpr int SNAPW = msl::sf::CTR_COUNT;   // counters per snapshot
    msl::PinBuf h_snap; hipEvent_t snapEv[NSNAP] = {}; unsigned long long snapKf[NSNAP] = {}; bool snapBusy[NSNAP] = {};
    bool snapLive[NSNAP] = {};   // the snapshot's live count still describes the resident map (no upload / restore since it was taken)
    unsigned long long kfEnq = 0; int snapNext = 0;
    // churn = surfels spawned + deleted per keyframe over the most recent batch the host has seen (from the running totals of two snapshots):
    // the deferred compaction is built for the steady state (a replay by ONE wave per window); under heavy churn the classic chain, whose
    // compaction works with all its workgroups, is faster
    long long churnNew = -1, churnDel = 0, churnKf = 0; unsigned long long churnAt = 0; double churn = 0.0;
    msl::DevBuf d_aos;           // staging of every AoS transfer (aos_in, aos_out)
    msl::DevBuf d_snapStore; size_t snapN = 0; bool snapValid = false; long long snapWide = 0;   // msl_sf_map_snapshot / _restore (same layout as the map store)
    // host-vector mode (msl_sf_fuse_ex): the device map equals the caller's vector as the last call left it
    bool mirrorValid = false; size_t mirrorN = 0;
    msl::PinBuf h_blk;    // per-sub-block deleted / updated counts of the call's k_fuse launch: two halves of h_blk.cap / 8 entries
    msl::PinBuf h_list;   // {count | indices | records} of the sparse download
    msl::KernelProfiler prof;
};

namespace msl {
namespace sf {

// ---- msl_surfel.hip ----
int sync_all(msl_sf *h);   // every stream of the handle is idle
int alloc_slots(msl_sf *h, int maxBatch);
// The staged gray, depth and member images go together (a later host-image call allocates all three anew), and msl_sf_staged_gray has
// nothing to hand out until that call has run.  The only path that frees them.
void release_staged_images(msl_sf *h);
// The images of one batch as the caller handed them over.  Per kind: base pointer, row stride and frame stride in bytes, and (from check_images) the
// bytes actually present in one image -- the last row carries no stride padding.
struct ImageArg { const void *p = nullptr; size_t row = 0, frame = 0, bytes = 0; };
struct BatchImages {
    ImageArg gray, depth, depth16, member;   // (a frame stride left out is 0: one keyframe)
    msl_mem mem = MSL_MEM_HOST; float depthFactor = 1.0f;
    // the depth images are raw 16-bit values that become metres on the device, (float)raw * depthFactor (src/Frame.cc:96-97); `depth` is ignored then
    bool d16() const { return depth16.p != nullptr; }
};
// One batch of n keyframes: their images staged in the slot set of this batch, the superpixel stage for all of them on the pre stream, then the
// map stage per keyframe on the map stream.  compact: the resident map (false: the host-vector drop-in, whose map is the caller's vector).
int run_batch(msl_sf *h, int n, const int32_t *refs, const float *poses, BatchImages I, bool compact);

// ---- msl_sf_store.hip ----
// Both streams drained and the counters read into pinned memory: the live count is exact, every pending live-count snapshot consumed.
int read_ctr(msl_sf *h);
int check_err(msl_sf *h);   // the device-side error code read_ctr brought along: reported and cleared
inline int settle(msl_sf *h) { const int rc = read_ctr(h); return rc != MSL_OK ? rc : check_err(h); }
inline long long host_ctr(const msl_sf *h, SfCtr i) { return ((const long long *)h->h_ctr.p)[i]; }   // counter i as read_ctr last read it
inline size_t live_count(const msl_sf *h) { return (size_t)host_ctr(h, CTR_LIVE); }
// (Re)allocate the resident map for `cap` surfels, preserving the first `keep` entries.  The new set is built beside the old one: a failed
// attempt frees itself and leaves the old map untouched.
int map_realloc(msl_sf *h, size_t cap, size_t keep);
int write_ctl(msl_sf *h);   // the device-side control block of the map stage, rewritten whenever one of the bases it holds is reallocated
int reserve_map(msl_sf *h, int n);   // room in the resident map for n more keyframes (run_batch, resident mode)
// The map was replaced from outside the keyframe chain and holds n surfels now: the host's bounds are exact again, the live-count snapshots still
// pending describe the old map, and the next keyframe takes the classic pair of launches.
void map_replaced(msl_sf *h, size_t n);
// The two ways through the AoS staging buffer d_aos (grown to fit), asynchronous on the map stream.
//   aos_in : n records of the host converted into the map, from slot 0 or (atEnd) behind the live count
//   aos_out: n records converted into d_aos -- the map's first n, or with sel the n surfels k_select_count has just counted -- and the stretches
//            runs[] of them copied to host (same indices)
struct AosRun { size_t i0, i1; };
struct MapSelect { int mode, arg; bool mark; };   // mode 0: surfels attached to pose `arg` (mark: deleted from the map), 1: seen at least `arg` times
int aos_in(msl_sf *h, const msl_surfel *host, size_t n, bool atEnd);
int aos_out(msl_sf *h, size_t n, const MapSelect *sel, msl_surfel *host, const AosRun *runs, size_t nRuns);

}  // namespace sf
}  // namespace msl
