// msl_surfel.hip -- surfel fusion for gfx950 (MI355X): the handle's lifecycle and streams, slot allocation and image staging, the batch driver,
// the resident entry points and the profiler calls (the other host units: msl_sf_handle.h).
//
// Replaces SurfelFusion (reference src/SurfelFusion.cpp) and the slot refill / tail compaction of
// SurfelMapping::fuseMap (src/SurfelMapping.cpp:353-392).  The kernels live in other translation units:
//   msl_sf_superpixel.hip   generateSuperPixels() of a keyframe depends only on that keyframe's images, never on the map, so it is FRAME-BATCHED on the
//                           "pre" stream (one launch sequence per batch of F keyframes; its kb_* kernels by role: msl_sf_sp_assign / _seeds / _plane.hip);
//   msl_sf_fuse.hip, msl_sf_compact.hip, msl_sf_replay.hip, msl_sf_map.hip (maintenance)
//                           the map stage (fusion -> new surfels -> compaction) is sequential per keyframe, on the "map" stream:
//                           k_fuse + k_compact per keyframe (classic), or ONE k_fuse launch per keyframe with the compactions of a
//                           window of <= 32 keyframes replayed at its end (deferred); run_batch picks per batch: deferred for a handle on ONE
//                           caller-provided stream under low churn, classic otherwise (a handle with its own two streams: always classic);
// the two stages overlap across batches (double-buffered slot sets).

#include "msl_sf_handle.h"

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

namespace msl {
namespace sf {

int sync_all(msl_sf *h) {
    if (h->ownStreams && h->copyStream) MSL_HIP_TRY(hipStreamSynchronize(h->copyStream));
    MSL_HIP_TRY(hipStreamSynchronize(h->preStream));
    MSL_HIP_TRY(hipStreamSynchronize(h->mapStream));
    return MSL_OK;
}

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

namespace {

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

}  // namespace

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

}  // namespace sf
}  // namespace msl

using namespace msl;
using namespace msl::sf;

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
    return settle(h);
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

}  // extern "C"
