// msl_surfel.hip -- surfel fusion for gfx950 (MI355X): the handle, streams and batching, and the C ABI.
//
// Replaces SurfelFusion (reference src/SurfelFusion.cpp) and the slot refill / tail compaction of
// SurfelMapping::fuseMap (src/SurfelMapping.cpp:353-392).  The kernels live in other translation units:
//   msl_sf_superpixel.hip   generateSuperPixels() of a keyframe depends only on that keyframe's images, never on the map, so it is
//                           FRAME-BATCHED on the "pre" stream (kb_* kernels, one launch sequence per batch of F keyframes);
//   msl_sf_fuse.hip, msl_sf_compact.hip, msl_sf_replay.hip, msl_sf_map.hip (maintenance)
//                           the map stage (fusion -> new surfels -> compaction) is sequential per keyframe, on the "map" stream:
//                           k_fuse + k_compact per keyframe (classic), or ONE k_fuse launch per keyframe with the compactions of a
//                           window of <= 32 keyframes replayed at its end (deferred); run_batch picks per batch: deferred for a handle on ONE
//                           caller-provided stream under low churn, classic otherwise (a handle with its own two streams: always classic);
// the two stages overlap across batches (double-buffered slot sets).

#include "msl_sf.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <new>
#include <vector>

using namespace msl;
using namespace msl::sf;

namespace {
const char *kSfNames[MSL_SF_NKERNELS] = {"kb_seed_init", "kb_assign", "kb_prop", "kb_commit_px", "kb_update_seeds", "kb_commit_seeds",
                                         "kb_seed_plane", "k_fuse", "k_empty", "k_compact", "k_convert", "copy"};
}  // namespace

struct msl_sf {
    int device = 0;
    SfDev dev{};
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
        DevBuf buf; size_t stride = 0;
        uint8_t *at(size_t slot) const { return (uint8_t *)buf.p + slot * stride; }
    };
    // The slot set, allocated to exactly 2 * maxBatch slots by alloc_slots: the per-slot arrays behind SfDev's bases, the pinned FrameDev staging,
    // and the images of host-image calls (allocated by the first such call; depth16: the raw 16-bit depth of msl_sf_fuse_resident_batch_d16)
    struct Slots {
        DevBuf frames, seeds, seedsTmp, cand, candOk, fused, tex, fuseRec, index, amap, tmin, arec, pxInv, wl, wlCount, chunkAbort, changed;
        PinBuf hFrames;
        ImageSlots gray, depth, member, depth16;
    } slot;
    DevBuf d_ctr; PinBuf h_ctr;
    DevBuf d_tickets, d_delU, d_dc, d_projTab;
    bool propLds = false;        // t(s) of one keyframe fits the LDS: single-launch relaxation
    bool classicNext = true;     // the map was replaced from outside the keyframe chain (upload / restore / append / detach): its first keyframe takes the classic
                                 // pair of launches, whose compaction handles any number of stale or deleted slots at full speed
    DevBuf d_new;
    // The resident map, replaced as a whole by map_realloc (layout: set_map_ptrs; its capacity in surfels: dev.cap).  rp: deferred compaction's
    // move lists, dense replay tables and staging
    struct MapBufs { DevBuf store, blockSums, blockUpd, delList, srcOf, rp; } map;
    size_t liveBound = 0;        // host-side upper bound of the live count: last known count + nseeds per keyframe enqueued since
    size_t liveKnown = 0;        // the most recent live count the host has seen (exact at that time; only a hint for k_fuse's speculative loads)
    unsigned long long liveKnownKf = 0;   // ... and the number of keyframes that had been enqueued when it was exact: an older snapshot never replaces a newer one
    // asynchronous refresh of that bound: after every batch the live count is copied to pinned memory behind an event; a later call picks
    // up whatever has arrived, so the bound follows the real count a couple of batches late instead of forcing a pipeline drain
    // every capacity / nseeds keyframes
    static constexpr int NSNAP = 4;
    static constexpr int SNAPW = 16;   // counters per snapshot: ctr[0 .. 15]
    PinBuf h_snap; hipEvent_t snapEv[NSNAP] = {}; unsigned long long snapKf[NSNAP] = {}; bool snapBusy[NSNAP] = {};
    bool snapLive[NSNAP] = {};   // the snapshot's live count still describes the resident map (no upload / restore since it was taken)
    unsigned long long kfEnq = 0; int snapNext = 0;
    // churn = surfels spawned + deleted per keyframe over the most recent batch the host has seen (from the running totals of two snapshots):
    // the deferred compaction is built for the steady state (a replay by ONE wave per window); under heavy churn the classic chain, whose
    // compaction works with all its workgroups, is faster
    long long churnNew = -1, churnDel = 0, churnKf = 0; unsigned long long churnAt = 0; double churn = 0.0;
    DevBuf d_aos;
    DevBuf d_snapStore; size_t snapN = 0; bool snapValid = false; long long snapWide = 0;   // msl_sf_map_snapshot / _restore (same layout as the map store)
    // host-vector mode (msl_sf_fuse_ex): the device map equals the caller's vector as the last call left it
    bool mirrorValid = false; size_t mirrorN = 0;
    PinBuf h_blk;    // per-sub-block deleted / updated counts of the call's k_fuse launch: two halves of h_blk.cap / 8 entries
    PinBuf h_list;   // {count | indices | records} of the sparse download
    KernelProfiler prof;
};

namespace {

// Map storage, in 4-byte words per surfel of capacity c (c is a multiple of 4096, so every array starts 32-byte aligned).  Each array's word
// offset is the one before it plus that one's record; array X of a store laid out for c surfels starts at word X * c.
//   map.store: hot | cold | rgbWide (3 ints) | utlWide (2 ints)
//   map.rp   : loc64 (first: 8-byte aligned) | stageCold | stageHot | moveDst | vposD | locKeys | vposKeys | dBig | stageRgb | stageUtl | bitmap c / 32 + 64
constexpr size_t HOT_W = sizeof(HotPk) / 4, COLD_W = sizeof(ColdRec) / 4;
constexpr size_t ST_HOT = 0, ST_COLD = ST_HOT + HOT_W, ST_RGB = ST_COLD + COLD_W, ST_UTL = ST_RGB + 3, MAP_WORDS = ST_UTL + 2;
constexpr size_t RP_LOC64 = 0, RP_STAGE_COLD = RP_LOC64 + 2, RP_STAGE_HOT = RP_STAGE_COLD + COLD_W, RP_MOVE_DST = RP_STAGE_HOT + HOT_W, RP_VPOS_D = RP_MOVE_DST + 1,
                 RP_LOC_KEYS = RP_VPOS_D + 1, RP_VPOS_KEYS = RP_LOC_KEYS + 1, RP_DBIG = RP_VPOS_KEYS + 1, RP_STAGE_RGB = RP_DBIG + 1, RP_STAGE_UTL = RP_STAGE_RGB + 3,
                 RP_BITMAP = RP_STAGE_UTL + 2, RP_WORDS = RP_BITMAP;   // (the bitmap is not per surfel: it follows the RP_WORDS * c words of the others)
constexpr size_t rp_bitmap_words(size_t c) { return c / 32 + 64; }
static_assert(ST_HOT == 0 && ST_COLD == 4 && ST_RGB == 12 && ST_UTL == 15 && MAP_WORDS == 17, "layout of map.store");
static_assert(RP_LOC64 == 0 && RP_STAGE_COLD == 2 && RP_STAGE_HOT == 10 && RP_MOVE_DST == 14 && RP_VPOS_D == 15 && RP_LOC_KEYS == 16 && RP_VPOS_KEYS == 17 &&
              RP_DBIG == 18 && RP_STAGE_RGB == 19 && RP_STAGE_UTL == 22 && RP_BITMAP == 24 && RP_WORDS == 24, "layout of map.rp");
void set_map_ptrs(msl_sf *h, size_t c) {
    MapSoA &M = h->dev.map;
    float *store = (float *)h->map.store.p;
    M.hot = reinterpret_cast<HotPk *>(store + ST_HOT * c);
    M.cold = reinterpret_cast<ColdRec *>(store + ST_COLD * c);
    M.rgbWide = reinterpret_cast<int *>(store + ST_RGB * c);    // exact ints of the COLD_WIDE records (untouched otherwise)
    M.utlWide = reinterpret_cast<int *>(store + ST_UTL * c);    // exact ints of the HOT_WIDE records
    M.wideFlag = h->dev.ctr + 13;
    SfDev &D = h->dev;
    D.cap = c;
    D.blockSums = (unsigned *)h->map.blockSums.p; D.blockUpd = (unsigned *)h->map.blockUpd.p; D.delList = (unsigned *)h->map.delList.p; D.srcOf = (unsigned *)h->map.srcOf.p;
    D.sbKeys = D.blockSums + h->blkStride; D.deal = D.blockSums + 2 * h->blkStride; D.dealG = 0;   // (three planes of one allocation: counts, screen keys, dealing table)
    unsigned *r = (unsigned *)h->map.rp.p;
    D.loc64 = reinterpret_cast<unsigned long long *>(r + RP_LOC64 * c);
    D.stageCold = reinterpret_cast<ColdRec *>(r + RP_STAGE_COLD * c);
    D.stageHot = reinterpret_cast<HotPk *>(r + RP_STAGE_HOT * c);
    D.moveDst = r + RP_MOVE_DST * c; D.vposD = r + RP_VPOS_D * c; D.locKeys = r + RP_LOC_KEYS * c; D.vposKeys = r + RP_VPOS_KEYS * c; D.dBig = r + RP_DBIG * c;
    D.stageRgb = reinterpret_cast<int *>(r + RP_STAGE_RGB * c); D.stageUtl = reinterpret_cast<int *>(r + RP_STAGE_UTL * c);
    D.bitmap = r + RP_BITMAP * c;
}

// The asynchronous live-count snapshots only ever LOWER liveBound; whenever the map is replaced from outside the keyframe chain
// (upload, restore) the ones still pending describe the old map and must be ignored.
void drop_live_snapshots(msl_sf *h) {
    for (int i = 0; i < msl_sf::NSNAP; i++) h->snapLive[i] = false;   // (their running totals -- the churn estimate -- stay valid)
}

int sync_all(msl_sf *h) {
    if (h->ownStreams && h->copyStream) MSL_HIP_TRY(hipStreamSynchronize(h->copyStream));
    MSL_HIP_TRY(hipStreamSynchronize(h->preStream));
    MSL_HIP_TRY(hipStreamSynchronize(h->mapStream));
    return MSL_OK;
}

// The device-side control block of the map stage: bases of the slot arrays and of the map's side arrays / lists (what only a few waves of a
// k_fuse launch read).  Rewritten whenever one of them is reallocated; the streams are idle then, and the window state it also holds
// (extents, deletion counts) is all zero between windows.
int write_ctl(msl_sf *h) {
    DeferCtl dc;
    memset(&dc, 0, sizeof(dc));
    const SfDev &D = h->dev;
    dc.flagStride = D.flagStride; dc.candOk = D.candOk; dc.fused = D.fused; dc.cand = D.cand;
    dc.aux.map = D.map; dc.aux.cap = D.cap; dc.aux.delU = D.delU; dc.aux.delUCount = D.delUCount; dc.aux.delList = D.delList;
    MSL_HIP_TRY(hipMemcpy(D.dc, &dc, sizeof(dc), hipMemcpyHostToDevice));
    return MSL_OK;
}

// (Re)allocate the resident map for `cap` surfels, preserving the first `keep` entries.  The new set is built beside the old one: a failed
// attempt frees itself and leaves the old map untouched.
int map_realloc(msl_sf *h, size_t cap, size_t keep) {
    cap = (cap + 4095) & ~(size_t)4095;
    const size_t bst = cap / SUB_ITEMS + 8200;   // per slice; >= 1024 / 8192 padding entries: the compaction reads its first tiles unconditionally
    const size_t rpWords = RP_WORDS * cap + rp_bitmap_words(cap);
    msl_sf::MapBufs m;
    MSL_HIP_TRY(grow_all(h->mapStream, {{m.store, sizeof(float) * MAP_WORDS * cap},
                                        {m.blockSums, sizeof(unsigned) * 3 * bst},           // deleted counts | screen keys | dealing table (SfDev::sbKeys, ::deal)
                                        {m.blockUpd, sizeof(unsigned) * DEFER_WIN * bst},    // one slice per keyframe of a deferred window (classic: the first)
                                        {m.delList, sizeof(unsigned) * cap}, {m.srcOf, sizeof(unsigned) * cap}, {m.rp, sizeof(unsigned) * rpWords}}));
    unsigned *nbs = (unsigned *)m.blockSums.p, *nrp = (unsigned *)m.rp.p;
    MSL_HIP_TRY(hipMemset(nbs, 0, sizeof(unsigned) * bst));
    MSL_HIP_TRY(hipMemset(nbs + bst, 0xFF, sizeof(unsigned) * bst));    // no key yet: "nothing in view"
    MSL_HIP_TRY(hipMemset(m.blockUpd.p, 0, sizeof(unsigned) * DEFER_WIN * bst));
    MSL_HIP_TRY(hipMemset(nrp + RP_LOC64 * cap, 0, sizeof(unsigned long long) * cap));         // loc64: empty (the replay leaves it clean)
    MSL_HIP_TRY(hipMemset(nrp + RP_VPOS_D * cap, 0, sizeof(unsigned) * cap));                  // vposD
    MSL_HIP_TRY(hipMemset(nrp + RP_BITMAP * cap, 0, sizeof(unsigned) * rp_bitmap_words(cap))); // bitmap
    if (keep && h->map.store.p) {
        const int rc = sync_all(h);
        if (rc != MSL_OK) return rc;
        const size_t oc = h->dev.cap;
        float *nstore = (float *)m.store.p;
        const float *ostore = (const float *)h->map.store.p;
        MSL_HIP_TRY(hipMemcpy(nstore + ST_HOT * cap, ostore + ST_HOT * oc, sizeof(HotPk) * keep, hipMemcpyDeviceToDevice));
        MSL_HIP_TRY(hipMemcpy(nstore + ST_COLD * cap, ostore + ST_COLD * oc, sizeof(ColdRec) * keep, hipMemcpyDeviceToDevice));
        MSL_HIP_TRY(hipMemcpy(nstore + ST_RGB * cap, ostore + ST_RGB * oc, sizeof(int) * 3 * keep, hipMemcpyDeviceToDevice));   // (rare path: no need to know whether any record is wide)
        MSL_HIP_TRY(hipMemcpy(nstore + ST_UTL * cap, ostore + ST_UTL * oc, sizeof(int) * 2 * keep, hipMemcpyDeviceToDevice));
    }
    h->map = std::move(m);
    h->blkStride = bst;
    h->dealG = 0;              // (the dealing table went with the old allocation)
    set_map_ptrs(h, cap);
    return write_ctl(h);
}

// The staged gray, depth and member images go together (a later host-image call allocates all three anew), and msl_sf_staged_gray has
// nothing to hand out until that call has run.  Every path that frees them comes through here.
void release_staged_images(msl_sf *h) {
    msl_sf::Slots &S = h->slot;
    S.gray = msl_sf::ImageSlots(); S.depth = msl_sf::ImageSlots(); S.member = msl_sf::ImageSlots();
    h->stagedSet = -1;
}

int alloc_slots(msl_sf *h, int maxBatch) {
    release_staged_images(h);
    h->slot = msl_sf::Slots();   // (the old set goes first)
    msl_sf::Slots &S = h->slot;
    SfDev &D = h->dev;
    const size_t slots = 2 * (size_t)maxBatch, ns = D.nseeds, npx = D.pxStride, fs = D.flagStride;
    MSL_HIP_TRY(grow_all(h->mapStream, {{S.frames, sizeof(FrameDev) * slots}, {S.seeds, sizeof(msl_seed) * ns * slots}, {S.seedsTmp, sizeof(msl_seed) * ns * slots},
                                        {S.cand, sizeof(msl_surfel) * ns * slots}, {S.candOk, fs * slots}, {S.fused, fs * slots},
                                        {S.tex, sizeof(uint2) * npx * slots}, {S.fuseRec, sizeof(float4) * 3 * ns * slots},
                                        {S.index, sizeof(unsigned short) * npx * slots}, {S.amap, sizeof(unsigned short) * npx * slots}, {S.tmin, sizeof(unsigned) * ns * slots},
                                        {S.arec, sizeof(AssignRec) * (ns * slots + 2)},   // + a record either side: kb_assign loads row pairs that may start one before / end one after
                                        {S.pxInv, sizeof(float) * npx * slots}, {S.wl, sizeof(unsigned) * npx * slots}, {S.wlCount, sizeof(unsigned) * slots},
                                        {S.chunkAbort, sizeof(int) * 32 * slots}, {S.changed, sizeof(int) * 8 * slots}}));
    MSL_HIP_TRY(S.hFrames.grow(sizeof(FrameDev) * slots, h->mapStream));
    MSL_HIP_TRY(hipMemset(S.tex.p, 0, S.tex.cap));
    MSL_HIP_TRY(hipMemset(S.fuseRec.p, 0, S.fuseRec.cap));
    MSL_HIP_TRY(hipMemset(S.wlCount.p, 0, S.wlCount.cap));
    MSL_HIP_TRY(hipMemset(S.arec.p, 0, S.arec.cap));
    MSL_HIP_TRY(hipMemset(S.seeds.p, 0, S.seeds.cap));
    MSL_HIP_TRY(hipMemset(S.index.p, 0, S.index.cap));
    MSL_HIP_TRY(hipMemset(S.fused.p, 1, S.fused.cap));     // (the bytes behind the lattice stay 1 = "spawns nothing": the map stage scans whole 16-byte words)
    MSL_HIP_TRY(hipMemset(S.candOk.p, 0, S.candOk.cap));
    D.frames = (FrameDev *)S.frames.p; D.seeds = (msl_seed *)S.seeds.p; D.seedsTmp = (msl_seed *)S.seedsTmp.p; D.cand = (msl_surfel *)S.cand.p;
    D.candOk = (uint8_t *)S.candOk.p; D.fused = (uint8_t *)S.fused.p; D.tex = (uint2 *)S.tex.p; D.fuseRec = (float4 *)S.fuseRec.p;
    D.index = (unsigned short *)S.index.p; D.amap = (unsigned short *)S.amap.p; D.tmin = (unsigned *)S.tmin.p; D.chunkAbort = (int *)S.chunkAbort.p; D.changed = (int *)S.changed.p;
    D.arec = (AssignRec *)S.arec.p + 1; D.pxInv = (float *)S.pxInv.p; D.wl = (unsigned *)S.wl.p; D.wlCount = (unsigned *)S.wlCount.p;
    { const int rc = write_ctl(h); if (rc != MSL_OK) return rc; }
    h->maxBatch = maxBatch;
    h->lastSlot = 0;            // the debug accessors must never index beyond the reallocated slot buffers
    for (msl_sf::SlotSet &t : h->sets) t.preValid = t.mapValid = t.copyValid = false;
    return MSL_OK;
}

// Counter snapshots that have arrived (their event has fired): a tighter bound / a fresher value of the live count, and the churn estimate -- spawned +
// deleted surfels per keyframe between two snapshots, from the running totals.
void consume_snapshots(msl_sf *h, size_t nseeds) {
    for (int i = 0; i < msl_sf::NSNAP; i++)
        if (h->snapBusy[i] && hipEventQuery(h->snapEv[i]) == hipSuccess) {
            h->snapBusy[i] = false;
            const long long *sn = (const long long *)h->h_snap.p + (size_t)i * msl_sf::SNAPW;
            if (h->snapLive[i]) {
                const size_t cand = (size_t)sn[0] + (size_t)(h->kfEnq - h->snapKf[i]) * nseeds;   // count then + what was enqueued since
                if (cand < h->liveBound) h->liveBound = cand;
                if (h->snapKf[i] >= h->liveKnownKf) { h->liveKnown = (size_t)sn[0]; h->liveKnownKf = h->snapKf[i]; }   // completed snapshots are visited in array order, not age order
            }
            if (h->snapKf[i] > h->churnAt) {   // running totals: new ctr[8], deleted ctr[9], keyframes ctr[11]
                if (h->churnNew >= 0 && sn[11] > h->churnKf) h->churn = (double)((sn[8] - h->churnNew) + (sn[9] - h->churnDel)) / (double)(sn[11] - h->churnKf);
                h->churnNew = sn[8]; h->churnDel = sn[9]; h->churnKf = sn[11]; h->churnAt = h->snapKf[i];
            }
        }
}

int read_ctr(msl_sf *h) {
    if (h->ownStreams && h->copyStream) MSL_HIP_TRY(hipStreamSynchronize(h->copyStream));
    MSL_HIP_TRY(hipStreamSynchronize(h->preStream));
    MSL_HIP_TRY(hipMemcpyAsync(h->h_ctr.p, h->dev.ctr, sizeof(long long) * 16, hipMemcpyDeviceToHost, h->mapStream));
    MSL_HIP_TRY(hipStreamSynchronize(h->mapStream));
    h->prof.drain();
    consume_snapshots(h, (size_t)h->dev.nseeds);   // (all pending snapshots have arrived: their churn information is kept, the live count below is newer)
    h->liveBound = (size_t)((const long long *)h->h_ctr.p)[0];   // both streams are idle: the count is exact
    h->liveKnown = h->liveBound; h->liveKnownKf = h->kfEnq;
    for (int i = 0; i < msl_sf::NSNAP; i++) h->snapBusy[i] = false;   // (their events have fired: the stream is idle)
    return MSL_OK;
}

int check_err(msl_sf *h) {
    const long long e = ((const long long *)h->h_ctr.p)[5];
    if (e) {
        (void)hipMemsetAsync(h->dev.ctr + 5, 0, sizeof(long long), h->mapStream);
        if (e == 20) set_error("resident surfel map capacity exceeded (reserve more with msl_sf_map_reserve)");
        else set_error("surfel pipeline device-side bound exceeded (code %lld)", e);
        return MSL_ERR_OVERFLOW;
    }
    return MSL_OK;
}
// The images of one batch as the caller handed them over.  Per kind: base pointer, row stride and frame stride in bytes, and (from check_images) the
// bytes actually present in one image -- the last row carries no stride padding.
struct ImageArg { const void *p = nullptr; size_t row = 0, frame = 0, bytes = 0; };
struct BatchImages {
    ImageArg gray, depth, depth16, member;   // (a frame stride left out is 0: one keyframe)
    msl_mem mem = MSL_MEM_HOST; float depthFactor = 1.0f;
    // the depth images are raw 16-bit values that become metres on the device, (float)raw * depthFactor (src/Frame.cc:96-97); `depth` is ignored then
    bool d16() const { return depth16.p != nullptr; }
};

int check_images(const msl_sf *h, int n, const int32_t *refs, const float *poses, BatchImages &I) {
    const size_t W = (size_t)h->dev.W, H = (size_t)h->dev.H;
    ImageArg &g = I.gray, &d = I.depth, &r = I.depth16, &m = I.member;
    if (n < 1 || n > h->maxBatch) { set_error("msl_sf: batch of %d keyframes exceeds the batch capacity %d", n, h->maxBatch); return MSL_ERR_INVALID; }
    if (I.d16()) {
        if (r.row < W * 2 || (r.row & 1) || (r.frame & 1) || ((uintptr_t)r.p & 1)) { set_error("msl_sf: bad 16-bit depth pointer or strides"); return MSL_ERR_INVALID; }
        d.row = W * 4; d.frame = d.row * H;   // the converted images are tightly packed
    }
    if (!g.p || (!d.p && !I.d16()) || !m.p || !poses || !refs || g.row < W || d.row < W * 4 || m.row < ((W + 1) / 2) * 4 || (d.row & 3) || (m.row & 3)) {
        set_error("msl_sf: bad image pointers or strides");
        return MSL_ERR_INVALID;
    }
    if (g.row * H >= (1ull << 32) || d.row * H >= (1ull << 32) || m.row * ((H + 1) / 2) >= (1ull << 32)) {   // (the kernels address an image with 32-bit byte offsets)
        set_error("msl_sf: image rows span 4 GB or more");
        return MSL_ERR_INVALID;
    }
    g.bytes = g.row * (H - 1) + W; d.bytes = d.row * (H - 1) + W * 4;
    m.bytes = m.row * ((H + 1) / 2 - 1) + ((W + 1) / 2) * 4;   // the membership image is ceil(H / 2) x ceil(W / 2) (PlaneDetection's cloud size)
    r.bytes = I.d16() ? r.row * (H - 1) + W * 2 : 0;
    return MSL_OK;
}

// Room in the resident map for n more keyframes.  The reference's mvLocalSurfels is an unbounded std::vector (include/Map.h:130): grow the resident
// map before a batch could overflow it.  Every keyframe adds at most nseeds surfels, so the host only needs an upper bound of the live count; the
// exact count is read back (one sync) only when that bound reaches the capacity.
int reserve_map(msl_sf *h, int n) {
    const SfDev &D = h->dev;
    h->mirrorValid = false;   // the resident map moves on without the host-vector caller
    const size_t need = (size_t)n * (size_t)D.nseeds;
    consume_snapshots(h, (size_t)D.nseeds);
    if (h->liveBound + need > D.cap) {
        int rc = read_ctr(h);
        if (rc != MSL_OK) return rc;
        rc = check_err(h);
        if (rc != MSL_OK) return rc;
        if (h->liveBound + need > D.cap) {
            rc = map_realloc(h, 2 * h->liveBound + 2 * need + 65536, h->liveBound);
            if (rc != MSL_OK) return rc;
        }
    }
    h->liveBound += need;
    h->kfEnq += (unsigned long long)n;
    return MSL_OK;
}

// n frames of one image kind into slots dstStride bytes apart: tightly packed frames of exactly the slot stride (the streaming case) travel as ONE
// copy, otherwise one copy per frame
int copy_frames(uint8_t *dst, size_t dstStride, int n, const void *src, size_t frameStride, size_t bytes, hipStream_t st) {
    if (frameStride == bytes && dstStride == bytes) {
        MSL_HIP_TRY(hipMemcpyAsync(dst, src, bytes * (size_t)n, hipMemcpyHostToDevice, st));
        return MSL_OK;
    }
    for (int f = 0; f < n; f++) MSL_HIP_TRY(hipMemcpyAsync(dst + f * dstStride, (const uint8_t *)src + f * frameStride, bytes, hipMemcpyHostToDevice, st));
    return MSL_OK;
}

// Where the images of a batch lie on the device: frame f of a kind at its base + f * its step (bytes)
struct FrameSrc { const uint8_t *gray, *depth, *member; size_t grayStep, depthStep, memberStep; };

// Host images are staged in the set's slots (copy stream), device-resident raw depth is converted into the handle's float slots (superpixel
// stream); every other device image is read where the caller has it.
int stage_images(msl_sf *h, int set, int n, const BatchImages &I, FrameSrc &src) {
    msl_sf::Slots &S = h->slot;
    msl_sf::SlotSet &T = h->sets[set];
    const ImageArg &g = I.gray, &d = I.depth, &r = I.depth16, &m = I.member;
    const int W = h->dev.W, H = h->dev.H;
    const size_t slot0 = (size_t)set * (size_t)h->maxBatch, slots = 2 * (size_t)h->maxBatch;
    const hipStream_t sp = h->preStream, sm = h->mapStream;
    if (I.mem != MSL_MEM_HOST) {
        h->stagedSet = -1;
        src = {(const uint8_t *)g.p, (const uint8_t *)d.p, (const uint8_t *)m.p, g.frame, d.frame, m.frame};
        if (!I.d16()) return MSL_OK;
        if (d.bytes > S.depth.stride) {
            const int rc = sync_all(h);
            if (rc != MSL_OK) return rc;
            release_staged_images(h);
            MSL_HIP_TRY(S.depth.buf.grow(d.bytes * slots, sm));
            S.depth.stride = d.bytes;
        }
        sp_launch_depth_u16(sp, r.p, r.row, r.frame, (float *)S.depth.at(slot0), S.depth.stride / 4, W, H, n, I.depthFactor);
        src.depth = S.depth.at(slot0); src.depthStep = S.depth.stride;
        return MSL_OK;
    }
    if (g.bytes > S.gray.stride || d.bytes > S.depth.stride || m.bytes > S.member.stride) {
        const int rc = sync_all(h);
        if (rc != MSL_OK) return rc;
        release_staged_images(h);
        MSL_HIP_TRY(grow_all(sm, {{S.gray.buf, g.bytes * slots}, {S.depth.buf, d.bytes * slots}, {S.member.buf, m.bytes * slots}}));
        S.gray.stride = g.bytes; S.depth.stride = d.bytes; S.member.stride = m.bytes;
    }
    if (r.bytes > S.depth16.stride) {
        const int rc = sync_all(h);
        if (rc != MSL_OK) return rc;
        S.depth16.stride = 0;
        MSL_HIP_TRY(S.depth16.buf.grow(r.bytes * slots, sm));
        S.depth16.stride = r.bytes;
    }
    // The images travel on their own stream so that they overlap the superpixel kernels of the previous call (the other slot set);
    // with caller-provided streams (msl_sf_set_stream) everything stays on that one stream.
    const hipStream_t sc = (h->ownStreams && h->copyStream) ? h->copyStream : sp;
    // The staged images of a set are read by the SUPERPIXEL stage only -- the map stage works on the slot arrays (texels, seed records, candidates) --
    // so the copies of call k wait for the superpixel stage of call k - 2 (pre), not for its map stage (map, which the superpixel stage of call k
    // still waits for): the link runs up to two calls ahead of the map chain (bench.py --io host: 17.6 k -> 19.0 k frames/s with f32 depth,
    // 18.8 k -> 20.1 k with raw 16-bit depth)
    if (sc != sp && T.preValid) MSL_HIP_TRY(hipStreamWaitEvent(sc, T.pre, 0));
    h->prof.begin(SK_COPY, sc);
    int rc = copy_frames(S.gray.at(slot0), S.gray.stride, n, g.p, g.frame, g.bytes, sc);
    if (rc == MSL_OK) rc = I.d16() ? copy_frames(S.depth16.at(slot0), S.depth16.stride, n, r.p, r.frame, r.bytes, sc)
                                   : copy_frames(S.depth.at(slot0), S.depth.stride, n, d.p, d.frame, d.bytes, sc);
    // a membership image shared by all keyframes of the call (member_frame_stride == 0) is staged once, in the set's first slot
    if (rc == MSL_OK) rc = copy_frames(S.member.at(slot0), S.member.stride, m.frame == 0 ? 1 : n, m.p, m.frame, m.bytes, sc);
    if (rc != MSL_OK) return rc;
    if (I.d16())   // raw -> metres behind the copies, on their stream (same rows of stride r.row in the staging slots)
        sp_launch_depth_u16(sc, S.depth16.at(slot0), r.row, S.depth16.stride, (float *)S.depth.at(slot0), S.depth.stride / 4, W, H, n, I.depthFactor);
    h->prof.end(sc);
    MSL_HIP_TRY(hipEventRecord(T.h2d, sc));   // (always: msl_sf_staged_gray hands it to other handles)
    if (sc != sp) MSL_HIP_TRY(hipStreamWaitEvent(sp, T.h2d, 0));
    h->stagedSet = set; h->stagedGs = g.row;
    src = {S.gray.at(slot0), S.depth.at(slot0), S.member.at(slot0), S.gray.stride, S.depth.stride, m.frame == 0 ? 0 : S.member.stride};
    return MSL_OK;
}

// The set's pinned FrameDev table (image addresses, pose and its inverse, reference index) and its one copy to the device
int fill_frames(msl_sf *h, int set, int n, const FrameSrc &src, const int32_t *refs, const float *poses) {
    msl_sf::SlotSet &T = h->sets[set];
    const size_t slot0 = (size_t)set * (size_t)h->maxBatch;
    if (T.copyValid) MSL_HIP_TRY(hipEventSynchronize(T.copy));   // pinned staging of this set is free again
    FrameDev *hf = (FrameDev *)h->slot.hFrames.p + slot0;
    for (int f = 0; f < n; f++) {
        FrameDev &F = hf[f];
        F.gray = src.gray + f * src.grayStep;
        F.depth = (const float *)(src.depth + f * src.depthStep);
        F.member = (const int32_t *)(src.member + f * src.memberStep);
        memcpy(F.pose, poses + 16 * f, sizeof(float) * 16);
        inverse4<float>(F.pose, F.invPose);   // pose.inverse() (:59), adjugate/determinant in float
        F.ref = refs[f]; F._pad = 0;
    }
    MSL_HIP_TRY(hipMemcpyAsync((FrameDev *)h->slot.frames.p + slot0, hf, sizeof(FrameDev) * n, hipMemcpyHostToDevice, h->preStream));
    MSL_HIP_TRY(hipEventRecord(T.copy, h->preStream));
    T.copyValid = true;
    return MSL_OK;
}

// D with every per-slot base shifted so that blockIdx.y/z == 0 addresses slot0
SfDev slot_view(const SfDev &D, int slot0) {
    SfDev P = D;
    P.frames = D.frames + slot0; P.seeds = D.seeds + (size_t)slot0 * D.nseeds; P.seedsTmp = D.seedsTmp + (size_t)slot0 * D.nseeds;
    P.cand = D.cand + (size_t)slot0 * D.nseeds; P.candOk = D.candOk + (size_t)slot0 * D.flagStride; P.fused = D.fused + (size_t)slot0 * D.flagStride;
    P.tex = D.tex + (size_t)slot0 * D.pxStride; P.fuseRec = D.fuseRec + (size_t)slot0 * D.nseeds * 3;
    P.index = D.index + (size_t)slot0 * D.pxStride; P.amap = D.amap + (size_t)slot0 * D.pxStride; P.tmin = D.tmin + (size_t)slot0 * D.nseeds;
    P.arec = D.arec + (size_t)slot0 * D.nseeds; P.pxInv = D.pxInv + (size_t)slot0 * D.pxStride; P.wl = D.wl + (size_t)slot0 * D.pxStride; P.wlCount = D.wlCount + slot0;
    P.chunkAbort = D.chunkAbort + slot0 * 32; P.changed = D.changed + slot0 * 8;
    return P;
}

// The switches of the map chain, read from the environment once per process (by the first batch)
struct SfPolicy {
    int dealEvery;               // MSL_SF_DEAL_EVERY (default 4, at least 1): the classic chain deals on every dealEvery-th keyframe of a call
    bool dealOff;                // MSL_SF_DEAL=0: sub-blocks in array order, for A/B measurements
    bool deferOff, deferForce;   // MSL_SF_DEFER=0: never a deferred window; =1: always (the parity tests); unset: the policy of launch_map_chain
};
const SfPolicy &sf_policy() {
    static const SfPolicy p = [] {
        const char *every = getenv("MSL_SF_DEAL_EVERY"), *deal = getenv("MSL_SF_DEAL"), *defer = getenv("MSL_SF_DEFER");
        return SfPolicy{every ? std::max(1, atoi(every)) : 4, deal && !strcmp(deal, "0"), defer && !strcmp(defer, "0"), defer && !strcmp(defer, "1")};
    }();
    return p;
}
constexpr double CHURN_MAX = 96.0;   // spawned + deleted surfels per keyframe up to which the one-wave replay beats k_compact (bench.py --map moving: 670)
// Dealing only while the map (48 bytes per surfel) fits the 256 MB Infinity Cache: a larger map is streamed from HBM, where waves that walk the array in
// order keep DRAM pages open -- 8 M surfels: k_fuse 76.9 us in array order, 80.5 us dealt (bench.py --surfels 8000000, A/B on one box)
constexpr int DEAL_MAX_GRID = (4 << 20) / SUB_ITEMS;

// The k_fuse launches of one batch: grid and load hint in sub-blocks, and whether the sub-blocks are dealt by screen position
struct FuseGrid { int nSubGrid, nSubHint; bool dealOn; };
FuseGrid fuse_grid(const msl_sf *h, bool compact) {
    const SfDev &D = h->dev;
    const size_t boundLive = compact ? h->liveBound : D.cap;
    // grid: the last known live count plus a margin (k_fuse is grid-stride, so a map that outgrew it is still covered), never beyond the upper
    // bound; hint: the sub-blocks that were full at the last known count load without waiting for the live count
    const size_t known = std::min(h->liveKnown, boundLive);
    // ... rounded up to a multiple of 64 sub-blocks inside the capacity (a multiple of 32 sub-blocks): the dealing table of the launch before is
    // a permutation for ONE grid size, so the grid should change rarely -- a wave beyond the live count costs one load
    const size_t subWant = (std::min(known + 2 * (size_t)D.nseeds, boundLive) + SUB_ITEMS - 1) / SUB_ITEMS;
    FuseGrid g;
    g.nSubGrid = (int)std::max<size_t>(8, std::min((subWant + 63) & ~(size_t)63, (size_t)D.cap / SUB_ITEMS));
    g.nSubHint = (int)(known / SUB_ITEMS);
    g.dealOn = !sf_policy().dealOff && (g.nSubGrid & 7) == 0 && (size_t)g.nSubGrid <= h->blkStride && g.nSubGrid <= DEAL_MAX_GRID;
    return g;
}

// Map stage of the n keyframes in `set`, on the map stream.  Deferred compaction (MSL_SF_DEFER=0 turns it off, =1 forces it; unset: the policy
// below): windows of <= DEFER_WIN keyframes, ONE launch per keyframe, the window's compactions replayed at its end (msl_sf_replay.hip).  Classic
// (k_fuse + k_compact per keyframe): single keyframes, the host-vector drop-in, the first keyframe after the map was replaced from outside, and
// batches enqueued while the recent churn (spawned + deleted surfels per keyframe, from the asynchronous counter snapshots) is high -- k_compact
// takes any number of stale or deleted slots with all its workgroups, the replay's single wave is built for the steady state.  Both leave
// identical maps.
int launch_map_chain(msl_sf *h, SfDev &P, int set, int n, bool compact) {
    const SfPolicy &pol = sf_policy();
    const hipStream_t sp = h->preStream, sm = h->mapStream;
    const int slot0 = set * h->maxBatch;
    const FrameDev *hf = (const FrameDev *)h->slot.hFrames.p + slot0;
    const FuseGrid g = fuse_grid(h, compact);
    // Policy.  The deferred chain is 8 us per keyframe shorter (22.6 against 31 us alone), which pays exactly when the map chain is the critical
    // path: a handle on ONE caller-provided stream (superpixel stage and map stage back to back: 20.8 k against 19.0 k keyframes/s).  With the
    // handle's own two streams the frame-batched superpixel stage is the longer one; k_fuse launches that follow each other without the idle
    // stretch of k_compact in between only take issue slots from it (front end 22 010 against 22 330 frames/s, k_fuse 18.8 against 16.3 us in the
    // timed region), so that shape keeps the classic pair.
    const bool churny = !pol.deferForce && (h->churn > CHURN_MAX || sp != sm);
    auto classic = [&](int f) {
        P.kf = 0;
        map_launch_fuse(h->prof, sm, P, f, hf[f], g.nSubGrid, g.nSubHint, false, g.dealOn && h->dealG == g.nSubGrid, (unsigned)h->blkStride);
        // k_compact's second workgroup deals the sub-blocks for the launches that follow (resident mode: 128 workgroups) -- on every dealEvery-th
        // keyframe of a call and whenever the table does not fit the grid: the pass takes one workgroup ~10 us against the compaction's ~6 beside it
        // (32 keys per thread through LDS atomics and scattered stores), and a table a few keyframes old still has nearly every sub-block in the
        // right band (the view moves a fraction of a band per keyframe; a misplaced sub-block only costs its XCD some extra lines)
        P.dealG = g.dealOn && compact && (f % pol.dealEvery == 0 || h->dealG != g.nSubGrid) ? g.nSubGrid : 0;
        map_launch_compact(h->prof, sm, P, f, compact);
        if (P.dealG) h->dealG = g.nSubGrid;
        h->kfClassic++;
    };
    int f = 0;
    const int fProbe = n / 2;   // only when its profiler slot is enabled: what an event pair reports for an EMPTY dispatch at this place of the chain
    if (!compact || pol.deferOff || churny || n < 2) {
        for (; f < n; f++) { classic(f); if (f == fProbe) map_launch_empty_pair(h->prof, sm); }
    } else {
        if (h->classicNext) { classic(0); f = 1; if (fProbe == 0) map_launch_empty_pair(h->prof, sm); }
        while (f < n) {
            const int w = std::min(DEFER_WIN, n - f);
            for (int q = 0; q < w; q++) {
                P.kf = q; P.prevSlotAbs = slot0 + f + q - 1;
                map_launch_fuse(h->prof, sm, P, f + q, hf[f + q], g.nSubGrid, g.nSubHint, true, g.dealOn && h->dealG == g.nSubGrid, (unsigned)h->blkStride);
                if (f + q == fProbe) map_launch_empty_pair(h->prof, sm);
            }
            P.kf = w; P.prevSlotAbs = slot0 + f + w - 1;
            map_launch_replay(h->prof, sm, P, w, (unsigned)h->blkStride);
            h->kfDeferred += (unsigned long long)w;
            if (g.dealOn) { P.dealG = g.nSubGrid; map_launch_deal(sm, P); h->dealG = g.nSubGrid; }   // one dealing per window, from the keys of its last keyframe
            f += w;
        }
    }
    if (compact) h->classicNext = false;
    if (sp != sm) { MSL_HIP_TRY(hipEventRecord(h->sets[set].map, sm)); h->sets[set].mapValid = true; }
    if (compact && h->h_snap.p) {   // snapshot of the live count after this batch (picked up by a later call, never waited for)
        const int i = h->snapNext;
        if (!h->snapBusy[i]) {
            MSL_HIP_TRY(hipMemcpyAsync((long long *)h->h_snap.p + (size_t)i * msl_sf::SNAPW, h->dev.ctr, sizeof(long long) * msl_sf::SNAPW, hipMemcpyDeviceToHost, sm));
            MSL_HIP_TRY(hipEventRecord(h->snapEv[i], sm));
            h->snapKf[i] = h->kfEnq; h->snapBusy[i] = true; h->snapLive[i] = true; h->snapNext = (i + 1) % msl_sf::NSNAP;
        }
    }
    MSL_HIP_TRY(hipGetLastError());
    h->lastSlot = slot0 + n - 1;
    h->batchNo++;
    return MSL_OK;
}

// One batch of n keyframes: their images staged in the slot set of this batch, the superpixel stage for all of them on the pre stream, then the
// map stage per keyframe on the map stream.  compact: the resident map (false: the host-vector drop-in, whose map is the caller's vector).
int run_batch(msl_sf *h, int n, const int32_t *refs, const float *poses, BatchImages I, bool compact) {
    int rc = check_images(h, n, refs, poses, I);
    if (rc != MSL_OK) return rc;
    if (compact) {
        rc = reserve_map(h, n);
        if (rc != MSL_OK) return rc;
    }
    SfDev &D = h->dev;
    const int set = (int)(h->batchNo & 1);
    msl_sf::SlotSet &T = h->sets[set];
    const hipStream_t sp = h->preStream, sm = h->mapStream;
    if (T.mapValid && sp != sm) MSL_HIP_TRY(hipStreamWaitEvent(sp, T.map, 0));   // the set's previous user is done
    D.gstride = I.gray.row; D.gbytes = I.gray.bytes; D.dstride = I.depth.row / 4; D.mstride = I.member.row / 4;
    D.gsB = (unsigned)I.gray.row; D.dsB = (unsigned)I.depth.row; D.msB = (unsigned)I.member.row;
    FrameSrc src;
    rc = stage_images(h, set, n, I, src);
    if (rc != MSL_OK) return rc;
    rc = fill_frames(h, set, n, src, refs, poses);
    if (rc != MSL_OK) return rc;
    SfDev P = slot_view(D, set * h->maxBatch);
    sp_launch_stage(h->prof, sp, P, n, h->propLds);
    if (sp != sm) {
        MSL_HIP_TRY(hipEventRecord(T.pre, sp));
        T.preValid = true;
        MSL_HIP_TRY(hipStreamWaitEvent(sm, T.pre, 0));
    }
    return launch_map_chain(h, P, set, n, compact);
}

}  // namespace

extern "C" {

msl_sf *msl_sf_create(int width, int height, float fx, float fy, float cx, float cy, float fuseFar, float fuseNear, int device) noexcept {
    try {
    if (width < 16 || height < 16 || fx == 0 || fy == 0 || (width / SP) * (height / SP) >= IDX_PLANE || (long long)width * height >= (1ll << 31)) {
        set_error("msl_sf_create: width/height must be >= 16 with fewer than 65534 superpixels, fx and fy non-zero");
        return nullptr;
    }
    if (bind_device(device) != MSL_OK) return nullptr;
    // (owned by a guard until the handle is complete: an exception below -- std::bad_alloc from the table vector -- lands in the catch barrier, and
    // the streams, events and device buffers created so far must go with it)
    std::unique_ptr<msl_sf, void (*)(msl_sf *)> guard(new msl_sf, [](msl_sf *p) { msl_sf_destroy(p); });
    msl_sf *h = guard.get();
    h->device = device;
    SfDev &D = h->dev;
    D.W = width; D.H = height; D.spW = width / SP; D.spH = height / SP; D.nseeds = D.spW * D.spH; D.npx = width * height;   // spWidth = width / SP_SIZE: truncation (:29-38)
    D.pxStride = (D.npx + 63) & ~63;
    D.flagStride = 64 * ((((D.nseeds + 63) / 64) + 15) & ~15);   // 64 lanes x a multiple of 16 seeds each
    D.fx = fx; D.fy = fy; D.cx = cx; D.cy = cy; D.fuseFar = fuseFar; D.fuseNear = fuseNear;
    bool ok = true;
    {   // the per-keyframe map stage is the latency-critical chain: highest priority for its stream, lowest for the
        // throughput-oriented frame-batched superpixel stage
        int lo = 0, hi = 0;
        ok = ok && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess;
        ok = ok && hipStreamCreateWithPriority(&h->preStream, hipStreamNonBlocking, lo) == hipSuccess;
        ok = ok && hipStreamCreateWithPriority(&h->mapStream, hipStreamNonBlocking, hi) == hipSuccess;
        ok = ok && hipStreamCreateWithFlags(&h->copyStream, hipStreamNonBlocking) == hipSuccess;
    }
    for (msl_sf::SlotSet &t : h->sets)
        for (hipEvent_t *e : {&t.pre, &t.map, &t.copy, &t.h2d}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    const hipStream_t sm = h->mapStream;
    ok = ok && h->d_ctr.grow(sizeof(long long) * 32, sm) == hipSuccess;   // 16 counters (read_ctr) + [16..18] the published live counts
    ok = ok && hipMemset(h->d_ctr.p, 0, sizeof(long long) * 32) == hipSuccess;
    ok = ok && h->h_ctr.grow(sizeof(long long) * 16, sm) == hipSuccess;
    ok = ok && h->h_snap.grow(sizeof(long long) * msl_sf::NSNAP * msl_sf::SNAPW, sm) == hipSuccess;
    for (int i = 0; i < msl_sf::NSNAP && ok; i++) ok = hipEventCreateWithFlags(&h->snapEv[i], hipEventDisableTiming) == hipSuccess;
    ok = ok && h->d_new.grow(sizeof(msl_surfel) * D.nseeds, sm) == hipSuccess;
    ok = ok && h->d_tickets.grow(sizeof(unsigned) * 8, sm) == hipSuccess && hipMemset(h->d_tickets.p, 0, sizeof(unsigned) * 8) == hipSuccess;   // [0..1] tickets, [3] change-list length, [4..6] the rotating hand-over counts
    ok = ok && h->d_delU.grow(sizeof(unsigned) * LIST_D, sm) == hipSuccess;
    ok = ok && h->d_dc.grow(sizeof(DeferCtl), sm) == hipSuccess && hipMemset(h->d_dc.p, 0, sizeof(DeferCtl)) == hipSuccess;
    {   // (u - cx) / fx and (v - cy) / fy of every integer pixel coordinate: the float expression of back_project
        // (src/SurfelFusion.cpp:80-85) evaluated once here instead of six divisions per pixel in kb_seed_plane
        std::vector<float> tab((size_t)width + 1 + height + 1);
        for (int u = 0; u <= width; u++) tab[u] = ((float)u - cx) / fx;
        for (int v = 0; v <= height; v++) tab[(size_t)width + 1 + v] = ((float)v - cy) / fy;
        ok = ok && h->d_projTab.grow(sizeof(float) * tab.size(), sm) == hipSuccess;
        ok = ok && hipMemcpy(h->d_projTab.p, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice) == hipSuccess;
        D.colX = (const float *)h->d_projTab.p; D.rowY = D.colX + width + 1;
    }
    if (ok) h->propLds = sp_init_attributes(D.nseeds);
    if (!ok) { set_error("msl_sf_create: HIP allocation failed"); return nullptr; }
    memset(h->h_ctr.p, 0, sizeof(long long) * 16);
    D.ctr = (long long *)h->d_ctr.p; D.newSurfels = (msl_surfel *)h->d_new.p; D.tickets = (unsigned *)h->d_tickets.p; D.delU = (unsigned *)h->d_delU.p;
    D.delUCount = D.tickets + 4; D.dc = (DeferCtl *)h->d_dc.p; D.kf = 0; D.prevSlotAbs = 0;
    h->prof.nk = MSL_SF_NKERNELS;
    if (alloc_slots(h, 1) != MSL_OK || map_realloc(h, 1 << 16, 0) != MSL_OK) return nullptr;
    return guard.release();
    } MSL_ABI_CATCH_PTR
}

void msl_sf_destroy(msl_sf *h) noexcept {
    try {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->copyStream) (void)hipStreamSynchronize(h->copyStream);
    if (h->preStream) (void)hipStreamSynchronize(h->preStream);
    if (h->mapStream) (void)hipStreamSynchronize(h->mapStream);
    h->prof.destroy();
    for (int i = 0; i < msl_sf::NSNAP; i++) if (h->snapEv[i]) (void)hipEventDestroy(h->snapEv[i]);
    for (const msl_sf::SlotSet &t : h->sets)
        for (hipEvent_t e : {t.pre, t.map, t.copy, t.h2d}) if (e) (void)hipEventDestroy(e);
    const hipStream_t streams[3] = {h->copyStream, h->ownStreams ? h->preStream : nullptr, h->ownStreams ? h->mapStream : nullptr};
    delete h;   // frees the buffers
    for (hipStream_t st : streams) if (st) (void)hipStreamDestroy(st);
    } MSL_ABI_CATCH_VOID
}

int msl_sf_staged_gray(msl_sf *h, const uint8_t **gray_dev, size_t *row_stride, size_t *frame_stride, void **uploaded_event) noexcept {
    try {
    if (!h || !gray_dev || !row_stride || !frame_stride || !uploaded_event) return MSL_ERR_INVALID;
    if (h->stagedSet < 0) { set_error("msl_sf_staged_gray: the last batch had no host images"); return MSL_ERR_INVALID; }   // (or release_staged_images freed them since)
    *gray_dev = h->slot.gray.at((size_t)h->stagedSet * (size_t)h->maxBatch);
    *row_stride = h->stagedGs; *frame_stride = h->slot.gray.stride; *uploaded_event = (void *)h->sets[h->stagedSet].h2d;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_set_stream(msl_sf *h, void *hip_stream) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    if (h->ownStreams) { (void)hipStreamDestroy(h->preStream); (void)hipStreamDestroy(h->mapStream); }
    h->preStream = h->mapStream = (hipStream_t)hip_stream; h->ownStreams = false;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_set_batch_capacity(msl_sf *h, int max_frames) noexcept {
    try {
    if (!h || max_frames < 1 || max_frames > 4096) { set_error("msl_sf_set_batch_capacity: invalid argument"); return MSL_ERR_INVALID; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    if (max_frames == h->maxBatch) return MSL_OK;
    return alloc_slots(h, max_frames);
    } MSL_ABI_CATCH_INT
}

int msl_sf_sync(msl_sf *h) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    return check_err(h);
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_reserve(msl_sf *h, size_t capacity) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    if (capacity <= h->dev.cap) return MSL_OK;
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    return map_realloc(h, capacity, (size_t)((const long long *)h->h_ctr.p)[0]);
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_upload(msl_sf *h, const msl_surfel *host, size_t n) noexcept {
    try {
    if (!h || (n && !host)) return MSL_ERR_INVALID;
    h->mirrorValid = false;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    if (n + (size_t)h->dev.nseeds > h->dev.cap) {
        rc = map_realloc(h, n + n / 4 + 4 * (size_t)h->dev.nseeds, 0);
        if (rc != MSL_OK) return rc;
    }
    hipStream_t s = h->mapStream;
    MSL_HIP_TRY(hipMemsetAsync(h->dev.ctr + 13, 0, sizeof(long long), s));   // a fresh map: no wide r, g, b records yet
    if (n) {
        MSL_HIP_TRY(h->d_aos.grow(sizeof(msl_surfel) * n, s));
        MSL_HIP_TRY(hipMemcpyAsync(h->d_aos.p, host, sizeof(msl_surfel) * n, hipMemcpyHostToDevice, s));
        map_launch_aos_to_soa(h->prof, s, h->dev, (const msl_surfel *)h->d_aos.p, (long long)n, false);
    }
    map_launch_set_ctr(s, h->dev, (long long)n, -1);
    MSL_HIP_TRY(hipStreamSynchronize(s));
    h->liveBound = n; h->liveKnown = n; h->liveKnownKf = h->kfEnq; h->classicNext = true;
    drop_live_snapshots(h);   // a count recorded before the upload would otherwise lower the bound below n
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_snapshot(msl_sf *h) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    rc = check_err(h);
    if (rc != MSL_OK) return rc;
    const long long *ctr = (const long long *)h->h_ctr.p;
    const size_t n = (size_t)ctr[0];
    h->snapValid = false;   // (until the copies below are complete)
    MSL_HIP_TRY(h->d_snapStore.grow(sizeof(float) * MAP_WORDS * ((n + 4095) & ~(size_t)4095), h->mapStream));
    if (n) {
        float *snap = (float *)h->d_snapStore.p;
        const size_t sc = h->d_snapStore.cap / (sizeof(float) * MAP_WORDS);   // surfels the store is laid out for
        MSL_HIP_TRY(hipMemcpy(snap + ST_HOT * sc, h->dev.map.hot, sizeof(HotPk) * n, hipMemcpyDeviceToDevice));
        MSL_HIP_TRY(hipMemcpy(snap + ST_COLD * sc, h->dev.map.cold, sizeof(ColdRec) * n, hipMemcpyDeviceToDevice));
        if (ctr[13] & 1) MSL_HIP_TRY(hipMemcpy(snap + ST_RGB * sc, h->dev.map.rgbWide, sizeof(int) * 3 * n, hipMemcpyDeviceToDevice));
        if (ctr[13] & 2) MSL_HIP_TRY(hipMemcpy(snap + ST_UTL * sc, h->dev.map.utlWide, sizeof(int) * 2 * n, hipMemcpyDeviceToDevice));
    }
    h->snapN = n; h->snapValid = true; h->snapWide = ctr[13];
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_restore(msl_sf *h) noexcept {
    try {
    if (!h || !h->snapValid) { set_error("msl_sf_map_restore: no snapshot"); return MSL_ERR_INVALID; }
    h->mirrorValid = false;
    MSL_HIP_TRY(hipSetDevice(h->device));
    const size_t n = h->snapN;
    if (n + (size_t)h->dev.nseeds > h->dev.cap) {   // the map was reallocated smaller than the snapshot (upload of a small map): grow again
        int rc = read_ctr(h);
        if (rc != MSL_OK) return rc;
        rc = map_realloc(h, n + n / 4 + 4 * (size_t)h->dev.nseeds, 0);
        if (rc != MSL_OK) return rc;
    }
    hipStream_t s = h->mapStream;   // ordered after every keyframe enqueued so far; the superpixel stream never touches the map
    if (n) {
        const float *snap = (const float *)h->d_snapStore.p;
        const size_t sc = h->d_snapStore.cap / (sizeof(float) * MAP_WORDS);
        MSL_HIP_TRY(hipMemcpyAsync(h->dev.map.hot, snap + ST_HOT * sc, sizeof(HotPk) * n, hipMemcpyDeviceToDevice, s));
        MSL_HIP_TRY(hipMemcpyAsync(h->dev.map.cold, snap + ST_COLD * sc, sizeof(ColdRec) * n, hipMemcpyDeviceToDevice, s));
        if (h->snapWide & 1) MSL_HIP_TRY(hipMemcpyAsync(h->dev.map.rgbWide, snap + ST_RGB * sc, sizeof(int) * 3 * n, hipMemcpyDeviceToDevice, s));
        if (h->snapWide & 2) MSL_HIP_TRY(hipMemcpyAsync(h->dev.map.utlWide, snap + ST_UTL * sc, sizeof(int) * 2 * n, hipMemcpyDeviceToDevice, s));
    }
    // the restored map has exactly the snapshot's wide-rgb state: without the flag a later snapshot would skip rgbWide and a restore of THAT
    // one would bring COLD_WIDE records back without their exact ints
    map_launch_set_ctr(s, h->dev, (long long)n, (int)h->snapWide);
    MSL_HIP_TRY(hipGetLastError());
    h->liveBound = n; h->liveKnown = n; h->liveKnownKf = h->kfEnq; h->classicNext = true;
    drop_live_snapshots(h);
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_size(msl_sf *h, size_t *n_out) noexcept {
    try {
    if (!h || !n_out) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    *n_out = (size_t)((const long long *)h->h_ctr.p)[0];
    return check_err(h);
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_download(msl_sf *h, msl_surfel *host, size_t cap, size_t *n_out) noexcept {
    try {
    if (!h || !n_out) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    const size_t n = (size_t)((const long long *)h->h_ctr.p)[0];
    *n_out = n;
    if (n > cap || (n && !host)) { set_error("msl_sf_map_download: capacity %zu < map size %zu", cap, n); return MSL_ERR_CAPACITY; }
    if (n) {
        hipStream_t s = h->mapStream;
        MSL_HIP_TRY(h->d_aos.grow(sizeof(msl_surfel) * n, s));
        map_launch_soa_to_aos(h->prof, s, h->dev, (msl_surfel *)h->d_aos.p, (long long)n);
        MSL_HIP_TRY(hipMemcpyAsync(host, h->d_aos.p, sizeof(msl_surfel) * n, hipMemcpyDeviceToHost, s));
        MSL_HIP_TRY(hipStreamSynchronize(s));
    }
    return check_err(h);
    } MSL_ABI_CATCH_INT
}

static int map_select(msl_sf *h, int mode, int arg, bool mark, msl_surfel *out, size_t cap, size_t *n_out, const char *what) {
    if (!h || !n_out) { set_error("%s: invalid argument", what); return MSL_ERR_INVALID; }
    if (mark) { h->mirrorValid = false; h->classicNext = true; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);                       // waits for both streams
    if (rc != MSL_OK) return rc;
    rc = check_err(h);
    if (rc != MSL_OK) return rc;
    const size_t n = (size_t)((const long long *)h->h_ctr.p)[0];
    *n_out = 0;
    if (n == 0) return MSL_OK;
    hipStream_t s = h->mapStream;
    const SfDev P = h->dev;
    map_launch_select_count(s, P, mode, arg);
    rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    const size_t m = (size_t)((const long long *)h->h_ctr.p)[7];
    *n_out = m;
    (void)hipMemsetAsync(h->dev.ctr + 7, 0, sizeof(long long), s);
    if (m > cap || (m && !out)) { set_error("%s: %zu surfels selected, capacity %zu", what, m, cap); return MSL_ERR_CAPACITY; }
    if (m == 0) return MSL_OK;
    MSL_HIP_TRY(h->d_aos.grow(sizeof(msl_surfel) * m, s));
    map_launch_select_write(s, P, mode, arg, (msl_surfel *)h->d_aos.p, mark ? 1 : 0);
    MSL_HIP_TRY(hipMemcpyAsync(out, h->d_aos.p, sizeof(msl_surfel) * m, hipMemcpyDeviceToHost, s));
    MSL_HIP_TRY(hipStreamSynchronize(s));
    return MSL_OK;
}

int msl_sf_map_detach(msl_sf *h, int pose_index, msl_surfel *out, size_t cap, size_t *n_out) noexcept { try {
    return map_select(h, 0, pose_index, true, out, cap, n_out, "msl_sf_map_detach"); } MSL_ABI_CATCH_INT }
int msl_sf_map_export(msl_sf *h, int min_update_times, msl_surfel *out, size_t cap, size_t *n_out) noexcept { try {
    return map_select(h, 1, min_update_times, false, out, cap, n_out, "msl_sf_map_export"); } MSL_ABI_CATCH_INT }
// System::saveSurfels (src/System.cc:296-382) for the cloud SurfelMapping::Stop builds (src/SurfelMapping.cpp:62-104): the local surfels
// seen at least min_update_times times (filtered on the device, map order), then the caller's inactive surfels.  ASCII PLY with the
// element / property layout the reference hands to tinyply; NaN positions are skipped (:311-312); alpha = 1, quality = weight,
// radius = size * 1000 (SurfelMapping.cpp:80).  Number formatting is that of a default std::ostream (tinyply itself is a third party).
int msl_sf_export_ply(msl_sf *h, int min_update_times, const msl_surfel *inactive, size_t n_inactive, const char *path) noexcept {
    try {
    if (!h || !path || (n_inactive && !inactive)) { set_error("msl_sf_export_ply: invalid argument"); return MSL_ERR_INVALID; }
    size_t n = 0;
    int rc = msl_sf_map_export(h, min_update_times, nullptr, 0, &n);
    if (rc != MSL_OK && rc != MSL_ERR_CAPACITY) return rc;
    std::vector<msl_surfel> pts(n + n_inactive);
    if (n) { rc = msl_sf_map_export(h, min_update_times, pts.data(), n, &n); if (rc != MSL_OK) return rc; }
    for (size_t i = 0; i < n_inactive; i++) pts[n + i] = inactive[i];
    size_t count = 0;
    for (const msl_surfel &e : pts) count += std::isnan(e.px) ? 0 : 1;
    std::ofstream os(path, std::ios::out);
    if (os.fail()) { set_error("msl_sf_export_ply: cannot open %s", path); return MSL_ERR_INVALID; }
    os << "ply\nformat ascii 1.0\nelement vertex " << count << "\n";
    for (const char *p : {"x", "y", "z", "nx", "ny", "nz"}) os << "property float " << p << "\n";
    for (const char *p : {"red", "green", "blue", "alpha"}) os << "property uchar " << p << "\n";
    for (const char *p : {"quality", "radius"}) os << "property float " << p << "\n";
    os << "element camera 1\n";
    for (const char *p : {"view_px", "view_py", "view_pz", "x_axisx", "x_axisy", "x_axisz", "y_axisx", "y_axisy", "y_axisz", "z_axisx", "z_axisy", "z_axisz",
                          "focal", "scalex", "scaley", "centerx", "centery"})
        os << "property float " << p << "\n";
    os << "property int viewportx\nproperty int viewporty\nproperty float k1\nproperty float k2\nend_header\n";
    for (const msl_surfel &e : pts) {
        if (std::isnan(e.px)) continue;
        os << e.px << " " << e.py << " " << e.pz << " " << e.nx << " " << e.ny << " " << e.nz << " " << (unsigned)(uint8_t)e.r << " " << (unsigned)(uint8_t)e.g << " "
           << (unsigned)(uint8_t)e.b << " 1 " << e.weight << " " << e.size * 1000 << "\n";
    }
    os << "0 0 0 1 0 0 0 1 0 0 0 1 0 0 0 0 0 " << (int)count << " 1 0 0\n";
    return os.fail() ? MSL_ERR_INVALID : MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_append(msl_sf *h, const msl_surfel *surfels, size_t n) noexcept {
    try {
    if (!h || (n && !surfels)) { set_error("msl_sf_map_append: invalid argument"); return MSL_ERR_INVALID; }
    h->mirrorValid = false;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    if (n == 0) return MSL_OK;
    const size_t cur = (size_t)((const long long *)h->h_ctr.p)[0];
    if (cur + n + (size_t)h->dev.nseeds > h->dev.cap) {
        rc = map_realloc(h, cur + n + (cur + n) / 4 + 4 * (size_t)h->dev.nseeds, cur);
        if (rc != MSL_OK) return rc;
    }
    hipStream_t s = h->mapStream;
    MSL_HIP_TRY(h->d_aos.grow(sizeof(msl_surfel) * n, s));
    MSL_HIP_TRY(hipMemcpyAsync(h->d_aos.p, surfels, sizeof(msl_surfel) * n, hipMemcpyHostToDevice, s));
    map_launch_aos_to_soa(h->prof, s, h->dev, (const msl_surfel *)h->d_aos.p, (long long)n, true);
    map_launch_add_ctr(s, h->dev, (long long)n);
    MSL_HIP_TRY(hipStreamSynchronize(s));
    h->liveBound = cur + n; h->liveKnown = cur + n; h->liveKnownKf = h->kfEnq; h->classicNext = true;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_fuse_resident_batch(msl_sf *h, int n_frames, const int32_t *refs, const uint8_t *gray, size_t gray_stride,
                               size_t gray_frame_stride, const float *depth, size_t depth_stride, size_t depth_frame_stride,
                               const int32_t *member, size_t member_stride, size_t member_frame_stride, msl_mem img_mem,
                               const float *poses_colmajor) noexcept {
    try {
    if (!h) { set_error("msl_sf_fuse_resident_batch: NULL handle"); return MSL_ERR_INVALID; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    return run_batch(h, n_frames, refs, poses_colmajor, {{gray, gray_stride, gray_frame_stride}, {depth, depth_stride, depth_frame_stride}, {},
                                                         {member, member_stride, member_frame_stride}, img_mem}, true);
    } MSL_ABI_CATCH_INT
}

int msl_sf_fuse_resident_batch_d16(msl_sf *h, int n_frames, const int32_t *refs, const uint8_t *gray, size_t gray_stride, size_t gray_frame_stride,
                                   const uint16_t *depth16, size_t depth16_stride, size_t depth16_frame_stride, float depth_factor,
                                   const int32_t *member, size_t member_stride, size_t member_frame_stride, msl_mem img_mem,
                                   const float *poses_colmajor) noexcept {
    try {
    if (!h) { set_error("msl_sf_fuse_resident_batch_d16: NULL handle"); return MSL_ERR_INVALID; }
    if (!depth16) { set_error("msl_sf_fuse_resident_batch_d16: NULL depth"); return MSL_ERR_INVALID; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    return run_batch(h, n_frames, refs, poses_colmajor, {{gray, gray_stride, gray_frame_stride}, {}, {depth16, depth16_stride, depth16_frame_stride},
                                                         {member, member_stride, member_frame_stride}, img_mem, depth_factor}, true);
    } MSL_ABI_CATCH_INT
}

int msl_sf_fuse_resident(msl_sf *h, int referenceFrameIndex, const uint8_t *gray, size_t gray_stride, const float *depth,
                         size_t depth_stride, const int32_t *member, size_t member_stride, msl_mem img_mem,
                         const float pose_colmajor[16]) noexcept {
    try {
    if (!h) { set_error("msl_sf_fuse_resident: NULL handle"); return MSL_ERR_INVALID; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    const int32_t ref = referenceFrameIndex;
    return run_batch(h, 1, &ref, pose_colmajor, {{gray, gray_stride}, {depth, depth_stride}, {}, {member, member_stride}, img_mem}, true);
    } MSL_ABI_CATCH_INT
}

int msl_sf_last_counters(msl_sf *h, int64_t counters[5]) noexcept {
    try {
    if (!h || !counters) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    const long long *ctr = (const long long *)h->h_ctr.p;
    counters[0] = ctr[4]; counters[1] = ctr[1]; counters[2] = ctr[2]; counters[3] = ctr[3]; counters[4] = ctr[0];
    return check_err(h);
    } MSL_ABI_CATCH_INT
}

// Host-vector mode.  The caller's vector is the map for this call; what travels is kept to what has to:
//   in : the whole vector (56 B per surfel) -- unless MSL_SF_LOCAL_UNCHANGED says it still is what the previous call on this handle left there, in
//        which case the device copy of that call is used as it stands (checked: same length, no other map operation on the handle in between);
//   out: only the stretches of the vector that hold surfels this keyframe touched.  k_fuse leaves a deleted and an updated count per SUB_ITEMS-surfel
//        sub-block; sub-blocks with neither are byte-identical to the caller's copy and are not sent back (runs of touched sub-blocks travel as
//        one copy each, small gaps bridged; more than 64 runs collapse into fewer by bridging larger gaps).
int msl_sf_fuse_ex(msl_sf *h, int referenceFrameIndex, const uint8_t *gray, size_t gray_stride, const float *depth, size_t depth_stride,
                   const int32_t *member, size_t member_stride, const float pose_colmajor[16], msl_surfel *local, size_t n_local,
                   msl_surfel *new_out, size_t new_cap, size_t *n_new, unsigned flags) noexcept {
    try {
    if (!h || !pose_colmajor || !n_new || (n_local && !local)) { set_error("msl_sf_fuse: invalid argument"); return MSL_ERR_INVALID; }
    if (new_cap < (size_t)h->dev.nseeds || !new_out) { set_error("msl_sf_fuse: new_cap must be >= (w/8)*(h/8) = %d", h->dev.nseeds); return MSL_ERR_CAPACITY; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc;
    const bool reuse = (flags & MSL_SF_LOCAL_UNCHANGED) && h->mirrorValid && h->mirrorN == n_local;
    if (reuse) {
        // the device map is the caller's vector already: only the per-call counters start over
        map_launch_set_ctr(h->mapStream, h->dev, (long long)n_local, -1);
        h->liveBound = n_local; h->liveKnown = n_local; h->liveKnownKf = h->kfEnq;
    } else {
        rc = msl_sf_map_upload(h, local, n_local);
        if (rc != MSL_OK) return rc;
    }
    h->mirrorValid = false;   // (until this call has completed)
    const int32_t ref = referenceFrameIndex;
    rc = run_batch(h, 1, &ref, pose_colmajor, {{gray, gray_stride}, {depth, depth_stride}, {}, {member, member_stride}, MSL_MEM_HOST}, false);
    if (rc != MSL_OK) return rc;
    hipStream_t s = h->mapStream;
    const size_t nblk = (n_local + SUB_ITEMS - 1) / SUB_ITEMS;
    if (nblk > h->h_blk.cap / (2 * sizeof(unsigned))) MSL_HIP_TRY(h->h_blk.grow(sizeof(unsigned) * 2 * (nblk + 1024), s));
    const size_t blkHalf = h->h_blk.cap / (2 * sizeof(unsigned));   // deleted counts | updated counts
    const unsigned *blk = (const unsigned *)h->h_blk.p;
    if (nblk) {
        MSL_HIP_TRY(hipMemcpyAsync(h->h_blk.p, h->dev.blockSums, sizeof(unsigned) * nblk, hipMemcpyDeviceToHost, s));
        MSL_HIP_TRY(hipMemcpyAsync((unsigned *)h->h_blk.p + blkHalf, h->dev.blockUpd, sizeof(unsigned) * nblk, hipMemcpyDeviceToHost, s));
    }
    rc = read_ctr(h);   // the call's first synchronisation: counters and the per-sub-block counts are on the host
    if (rc != MSL_OK) return rc;
    rc = check_err(h);
    if (rc != MSL_OK) return rc;
    const size_t K = (size_t)((const long long *)h->h_ctr.p)[1];
    *n_new = K;
    // what was touched, and where
    struct Run { size_t b0, b1; };
    std::vector<Run> runs;
    size_t touched = 0, runSurfels = 0;
    for (size_t b = 0; b < nblk; b++) touched += (size_t)blk[b] + blk[blkHalf + b];
    for (size_t gapMax = 4; ; gapMax *= 4) {
        runs.clear();
        for (size_t b = 0; b < nblk; b++) {
            if (!(blk[b] | blk[blkHalf + b])) continue;
            if (!runs.empty() && b - runs.back().b1 <= gapMax) runs.back().b1 = b + 1;
            else runs.push_back({b, b + 1});
        }
        if (runs.size() <= 64) break;
    }
    for (const Run &r : runs) runSurfels += std::min(r.b1 * SUB_ITEMS, n_local) - r.b0 * SUB_ITEMS;
    // Two ways back.  Runs of touched sub-blocks copied straight into the caller's vector (~45 GB/s), or -- when few surfels in many sub-blocks
    // changed (a map in no particular order) -- a compact {index, record} list scattered by the CPU (~6 ns per record on top of its 60 bytes).
    const size_t listLimit = n_local / 8;
    msl_surfel *aos = (msl_surfel *)h->d_aos.p;   // (>= n_local entries: msl_sf_map_upload, or the call before that one)
    const double costRuns = 56.0 * (double)runSurfels / 45e9, costList = (double)touched * (60.0 / 45e9 + 6e-9);
    if (touched && touched <= listLimit && costList < costRuns) {
        const size_t need = 256 + (sizeof(unsigned) + sizeof(msl_surfel)) * listLimit;
        MSL_HIP_TRY(h->h_list.grow(need, s));
        // device side: the count sits in tickets[3], indices in delList, records in the AoS buffer (both >= n_local entries)
        unsigned *d_count = h->dev.tickets + 3;
        MSL_HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned), s));
        map_launch_collect_changed(s, h->dev, (int)ref, (long long)n_local, d_count, h->dev.delList, aos, (unsigned)listLimit);
        uint8_t *list = (uint8_t *)h->h_list.p;
        unsigned *hc = reinterpret_cast<unsigned *>(list);
        unsigned *hi = reinterpret_cast<unsigned *>(list + 256);
        msl_surfel *hr = reinterpret_cast<msl_surfel *>(list + 256 + sizeof(unsigned) * listLimit);
        MSL_HIP_TRY(hipMemcpyAsync(hc, d_count, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        MSL_HIP_TRY(hipStreamSynchronize(s));
        // (the list may be longer than `touched`: a surfel that carried lastUpdate == ref before the call is listed as well -- harmless, its
        // record is unchanged -- so the length is read first; a list beyond the staging size falls back to the runs)
        const size_t cnt = *hc;
        if (cnt <= listLimit) {
            MSL_HIP_TRY(hipMemcpyAsync(hi, h->dev.delList, sizeof(unsigned) * cnt, hipMemcpyDeviceToHost, s));
            MSL_HIP_TRY(hipMemcpyAsync(hr, aos, sizeof(msl_surfel) * cnt, hipMemcpyDeviceToHost, s));
            if (K) MSL_HIP_TRY(hipMemcpyAsync(new_out, h->dev.newSurfels, sizeof(msl_surfel) * K, hipMemcpyDeviceToHost, s));
            MSL_HIP_TRY(hipStreamSynchronize(s));
            for (size_t j = 0; j < cnt; j++) local[hi[j]] = hr[j];
            h->mirrorValid = true; h->mirrorN = n_local;
            return MSL_OK;
        }
    }
    if (nblk && !runs.empty())
        map_launch_soa_to_aos(h->prof, s, h->dev, aos, (long long)n_local);
    for (const Run &r : runs) {
        const size_t i0 = r.b0 * SUB_ITEMS, i1 = std::min(r.b1 * SUB_ITEMS, n_local);
        MSL_HIP_TRY(hipMemcpyAsync(local + i0, aos + i0, sizeof(msl_surfel) * (i1 - i0), hipMemcpyDeviceToHost, s));
    }
    if (K) MSL_HIP_TRY(hipMemcpyAsync(new_out, h->dev.newSurfels, sizeof(msl_surfel) * K, hipMemcpyDeviceToHost, s));
    MSL_HIP_TRY(hipStreamSynchronize(s));
    h->mirrorValid = true; h->mirrorN = n_local;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_fuse(msl_sf *h, int referenceFrameIndex, const uint8_t *gray, size_t gray_stride, const float *depth, size_t depth_stride,
                const int32_t *member, size_t member_stride, const float pose_colmajor[16], msl_surfel *local, size_t n_local,
                msl_surfel *new_out, size_t new_cap, size_t *n_new) noexcept {
    try {
    return msl_sf_fuse_ex(h, referenceFrameIndex, gray, gray_stride, depth, depth_stride, member, member_stride, pose_colmajor, local, n_local, new_out,
                          new_cap, n_new, 0u);
    } MSL_ABI_CATCH_INT
}

int msl_sf_debug_seeds(msl_sf *h, msl_seed *out) noexcept {
    try {
    if (!h || !out) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    const size_t ns = h->dev.nseeds;
    MSL_HIP_TRY(hipMemcpy(out, h->dev.seeds + ns * h->lastSlot, sizeof(msl_seed) * ns, hipMemcpyDeviceToHost));
    std::vector<uint8_t> fused(ns);
    MSL_HIP_TRY(hipMemcpy(fused.data(), h->dev.fused + (size_t)h->dev.flagStride * h->lastSlot, ns, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ns; i++) out[i].fused = fused[i] & 1;   // (2 = invalid candidate, not a fusion)
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_sf_debug_ctr(msl_sf *h, int64_t out[16]) noexcept {
    try {
    if (!h || !out) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    for (int i = 0; i < 16; i++) out[i] = ((const long long *)h->h_ctr.p)[i];
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_sf_debug_scratch(msl_sf *h, int which, size_t offset_words, uint32_t *out, size_t n_words) noexcept {
    try {
    if (!h || !out || which < 0 || which > 5) return MSL_ERR_INVALID;
    if (which == 5) {   // keyframes this handle sent through the classic chain / through deferred windows (host state)
        if (n_words < 2) return MSL_ERR_INVALID;
        out[0] = (uint32_t)h->kfClassic; out[1] = (uint32_t)h->kfDeferred;
        return MSL_OK;
    }
    if (which == 4) {   // the grid the dealing table currently is a permutation for (host state; 0: none)
        if (n_words < 1) return MSL_ERR_INVALID;
        out[0] = (uint32_t)h->dealG;
        return MSL_OK;
    }
    if (offset_words + n_words > (which < 2 ? h->dev.cap : h->blkStride)) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    const uint32_t *src = which == 0 ? h->dev.srcOf : which == 1 ? h->dev.delList : which == 2 ? h->dev.sbKeys : h->dev.deal;
    MSL_HIP_TRY(hipMemcpy(out, src + offset_words, sizeof(uint32_t) * n_words, hipMemcpyDeviceToHost));
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
// What an event pair carried by a dispatch (hipExtLaunchKernelGGL) reports for a kernel that does nothing: n launches of an empty kernel with
// `grid` single-wave workgroups on the map stream.  bench.py quotes it next to the roofline kernel's event time: rocprofv3's kernel duration
// (first wave start to last wave end) is shorter than the event time by about this much.
int msl_sf_debug_event_overhead(msl_sf *h, int grid, int n, float *mean_us) noexcept {
    try {
    if (!h || !mean_us || n < 1 || grid < 1) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    std::vector<hipEvent_t> ev(2 * (size_t)n);
    for (auto &e : ev) MSL_HIP_TRY(hipEventCreate(&e));
    for (int i = 0; i < n; i++) map_launch_empty(h->mapStream, grid, ev[2 * i], ev[2 * i + 1]);
    MSL_HIP_TRY(hipStreamSynchronize(h->mapStream));
    double tot = 0;
    for (int i = 0; i < n; i++) { float ms = 0; MSL_HIP_TRY(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1])); tot += ms; }
    for (auto &e : ev) (void)hipEventDestroy(e);
    *mean_us = (float)(tot * 1e3 / n);
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_sf_debug_index(msl_sf *h, int32_t *out) noexcept {
    try {
    if (!h || !out) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    const size_t npx = h->dev.npx;
    std::vector<unsigned short> tmp(npx);
    MSL_HIP_TRY(hipMemcpy(tmp.data(), h->dev.index + (size_t)h->dev.pxStride * h->lastSlot, sizeof(unsigned short) * npx, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npx; i++) out[i] = tmp[i];
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_profile_enable(msl_sf *h, int on) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    h->prof.drain();
    h->prof.set_mode(on);
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_sf_profile_stride(msl_sf *h, int stride) noexcept {
    try {
    if (!h || stride < 1) return MSL_ERR_INVALID;
    h->prof.stride = stride;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_sf_profile_read(msl_sf *h, float *ms, int32_t *launches) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc != MSL_OK) return rc;
    h->prof.drain();
    for (int i = 0; i < MSL_SF_NKERNELS; i++) { if (ms) ms[i] = h->prof.ms[i]; if (launches) launches[i] = h->prof.launches[i]; }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}
int msl_debug_deal(const uint32_t *keys_host, int n_subblocks, uint32_t *deal_host) noexcept { try { return map_debug_deal(keys_host, n_subblocks, deal_host); } MSL_ABI_CATCH_INT }
int msl_debug_div100(const float *x_host, double *out_host, size_t n) noexcept { try { return sp_debug_div100(x_host, out_host, n); } MSL_ABI_CATCH_INT }
int msl_debug_chain_sum(const float *x_host, const int32_t *n_host, int lists, int huber, float *out_host) noexcept { try { return sp_debug_chain(x_host, n_host, lists, huber, out_host); } MSL_ABI_CATCH_INT }
const char *msl_sf_kernel_name(int k) noexcept { try { return (k >= 0 && k < MSL_SF_NKERNELS) ? kSfNames[k] : ""; } MSL_ABI_CATCH_PTR }

}  // extern "C"