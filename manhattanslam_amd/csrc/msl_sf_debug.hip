// msl_sf_debug.hip -- debug accessors of the surfel handle (include/msl_debug.h), the stand-alone kernel probes, and the profiler's kernel names.
// No kernel lives here.

#include "msl_sf_handle.h"

#include <vector>

using namespace msl;
using namespace msl::sf;

namespace {
const char *kSfNames[MSL_SF_NKERNELS] = {"kb_seed_init", "kb_assign", "kb_prop", "kb_commit_px", "kb_update_seeds", "kb_commit_seeds",
                                         "kb_seed_plane", "k_fuse", "k_empty", "k_compact", "k_convert", "copy"};
}  // namespace

extern "C" {

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
    static_assert(CTR_COUNT == 16, "msl_sf_debug_ctr hands out every counter");
    for (int i = 0; i < CTR_COUNT; i++) out[i] = host_ctr(h, (SfCtr)i);
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

int msl_debug_deal(const uint32_t *keys_host, int n_subblocks, uint32_t *deal_host) noexcept { try { return map_debug_deal(keys_host, n_subblocks, deal_host); } MSL_ABI_CATCH_INT }
int msl_debug_div100(const float *x_host, double *out_host, size_t n) noexcept { try { return sp_debug_div100(x_host, out_host, n); } MSL_ABI_CATCH_INT }
int msl_debug_chain_sum(const float *x_host, const int32_t *n_host, int lists, int huber, float *out_host) noexcept { try { return sp_debug_chain(x_host, n_host, lists, huber, out_host); } MSL_ABI_CATCH_INT }
int msl_debug_newton_delta(const float *sumA_host, const int32_t *inr_host, size_t n, float *out_host, float *literal_host) noexcept { try { return sp_debug_newton(sumA_host, inr_host, n, out_host, literal_host); } MSL_ABI_CATCH_INT }
int msl_debug_group_sums(const double *x_host, int groups, int nvals, double *out_host, double *ref_host) noexcept { try { return sp_debug_group_sums(x_host, groups, nvals, out_host, ref_host); } MSL_ABI_CATCH_INT }
const char *msl_sf_kernel_name(int k) noexcept { try { return (k >= 0 && k < MSL_SF_NKERNELS) ? kSfNames[k] : ""; } MSL_ABI_CATCH_PTR }

}  // extern "C"
