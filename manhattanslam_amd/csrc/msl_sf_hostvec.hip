// msl_sf_hostvec.hip -- host-vector mode of the surfel handle: msl_sf_fuse / msl_sf_fuse_ex, the drop-in for SurfelFusion::fuseInitializeMap.  No
// kernel lives here.
//
// The caller's vector is the map for this call; what travels is kept to what has to:
//   in : the whole vector (56 B per surfel) -- unless MSL_SF_LOCAL_UNCHANGED says it still is what the previous call on this handle left there, in
//        which case the device copy of that call is used as it stands (checked: same length, no other map operation on the handle in between);
//   out: only the stretches of the vector that hold surfels this keyframe touched.  k_fuse leaves a deleted and an updated count per SUB_ITEMS-surfel
//        sub-block, and plan_download (msl_sf_plan.h) turns them into runs of sub-blocks -- or, when few surfels in many sub-blocks changed, into an
//        attempt at a compact {index, record} list.

#include "msl_sf_handle.h"
#include "msl_sf_plan.h"

#include <vector>

using namespace msl;
using namespace msl::sf;

namespace {

// The sparse way back: a compact {index, record} list of the surfels keyframe `ref` touched, on its way to pinned memory; the CPU scatters it into
// the caller's vector once the stream is idle.  fetched = false: the list outgrew its staging -- the runs take over.
struct ChangeList { const unsigned *idx = nullptr; const msl_surfel *rec = nullptr; size_t n = 0; bool fetched = false; };
int fetch_list(msl_sf *h, int ref, size_t n_local, size_t listLimit, ChangeList &out) {
    const hipStream_t s = h->mapStream;
    MSL_HIP_TRY(h->h_list.grow(256 + (sizeof(unsigned) + sizeof(msl_surfel)) * listLimit, s));
    // device side: the count sits in tickets[3], indices in delList, records in the AoS buffer (both >= n_local entries: d_aos from msl_sf_map_upload,
    // or the call before that one)
    unsigned *d_count = h->dev.tickets + 3;
    msl_surfel *aos = (msl_surfel *)h->d_aos.p;
    MSL_HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned), s));
    map_launch_collect_changed(s, h->dev, ref, (long long)n_local, d_count, h->dev.delList, aos, (unsigned)listLimit);
    uint8_t *list = (uint8_t *)h->h_list.p;
    unsigned *hc = reinterpret_cast<unsigned *>(list);
    unsigned *hi = reinterpret_cast<unsigned *>(list + 256);
    msl_surfel *hr = reinterpret_cast<msl_surfel *>(list + 256 + sizeof(unsigned) * listLimit);
    MSL_HIP_TRY(hipMemcpyAsync(hc, d_count, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    MSL_HIP_TRY(hipStreamSynchronize(s));
    // (the list may be longer than what k_fuse touched: a surfel that carried lastUpdate == ref before the call is listed as well -- harmless, its
    // record is unchanged -- so the length is read first)
    const size_t cnt = *hc;
    if (cnt > listLimit) return MSL_OK;
    MSL_HIP_TRY(hipMemcpyAsync(hi, h->dev.delList, sizeof(unsigned) * cnt, hipMemcpyDeviceToHost, s));
    MSL_HIP_TRY(hipMemcpyAsync(hr, aos, sizeof(msl_surfel) * cnt, hipMemcpyDeviceToHost, s));
    out.idx = hi; out.rec = hr; out.n = cnt; out.fetched = true;
    return MSL_OK;
}

// The dense way back: the map converted once, every run of touched sub-blocks copied straight into the caller's vector
int download_runs(msl_sf *h, const DownloadPlan &plan, msl_surfel *local, size_t n_local) {
    if (plan.runs.empty()) return MSL_OK;
    std::vector<AosRun> runs;
    for (const DownloadPlan::Run &r : plan.runs) runs.push_back({r.b0 * SUB_ITEMS, std::min(r.b1 * SUB_ITEMS, n_local)});
    return aos_out(h, n_local, nullptr, local, runs.data(), runs.size());
}

}  // namespace

extern "C" {

int msl_sf_fuse_ex(msl_sf *h, int referenceFrameIndex, const uint8_t *gray, size_t gray_stride, const float *depth, size_t depth_stride,
                   const int32_t *member, size_t member_stride, const float pose_colmajor[16], msl_surfel *local, size_t n_local,
                   msl_surfel *new_out, size_t new_cap, size_t *n_new, unsigned flags) noexcept {
    try {
    if (!h || !pose_colmajor || !n_new || (n_local && !local)) { set_error("msl_sf_fuse: invalid argument"); return MSL_ERR_INVALID; }
    if (new_cap < (size_t)h->dev.nseeds || !new_out) { set_error("msl_sf_fuse: new_cap must be >= (w/8)*(h/8) = %d", h->dev.nseeds); return MSL_ERR_CAPACITY; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc;
    if ((flags & MSL_SF_LOCAL_UNCHANGED) && h->mirrorValid && h->mirrorN == n_local) {
        // the device map is the caller's vector already: only the per-call counters start over
        map_launch_set_ctr(h->mapStream, h->dev, (long long)n_local, -1);
        map_replaced(h, n_local);
    } else {
        rc = msl_sf_map_upload(h, local, n_local);
        if (rc != MSL_OK) return rc;
    }
    h->mirrorValid = false;   // (until this call has completed)
    const int32_t ref = referenceFrameIndex;
    rc = run_batch(h, 1, &ref, pose_colmajor, {{gray, gray_stride}, {depth, depth_stride}, {}, {member, member_stride}, MSL_MEM_HOST}, false);
    if (rc != MSL_OK) return rc;
    const hipStream_t s = h->mapStream;
    const size_t nblk = (n_local + SUB_ITEMS - 1) / SUB_ITEMS;
    if (nblk > h->h_blk.cap / (2 * sizeof(unsigned))) MSL_HIP_TRY(h->h_blk.grow(sizeof(unsigned) * 2 * (nblk + 1024), s));
    const size_t blkHalf = h->h_blk.cap / (2 * sizeof(unsigned));   // deleted counts | updated counts
    unsigned *blk = (unsigned *)h->h_blk.p;
    if (nblk) {
        MSL_HIP_TRY(hipMemcpyAsync(blk, h->dev.blockSums, sizeof(unsigned) * nblk, hipMemcpyDeviceToHost, s));
        MSL_HIP_TRY(hipMemcpyAsync(blk + blkHalf, h->dev.blockUpd, sizeof(unsigned) * nblk, hipMemcpyDeviceToHost, s));
    }
    rc = settle(h);   // the call's first synchronisation: counters and the per-sub-block counts are on the host
    if (rc != MSL_OK) return rc;
    const size_t K = (size_t)host_ctr(h, CTR_NEW);
    *n_new = K;
    const DownloadPlan plan = plan_download(blk, blk + blkHalf, nblk, n_local, SUB_ITEMS);
    ChangeList list;
    if (plan.tryList) rc = fetch_list(h, (int)ref, n_local, plan.listLimit, list);
    if (rc == MSL_OK && !list.fetched) rc = download_runs(h, plan, local, n_local);
    if (rc != MSL_OK) return rc;
    if (K) MSL_HIP_TRY(hipMemcpyAsync(new_out, h->dev.newSurfels, sizeof(msl_surfel) * K, hipMemcpyDeviceToHost, s));
    MSL_HIP_TRY(hipStreamSynchronize(s));
    for (size_t j = 0; j < list.n; j++) local[list.idx[j]] = list.rec[j];
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

}  // extern "C"
