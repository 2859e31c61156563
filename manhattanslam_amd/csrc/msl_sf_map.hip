// msl_sf_map.hip -- map maintenance of the surfel fusion on the device-resident map: ordered selection (moveAddSurfels / Stop of the reference's
// src/SurfelMapping.cpp), AoS <-> SoA conversion, counters, the change list of the host-vector mode, the profiler's empty kernel.  The map
// stage's overview and the record accessors: msl_sf_map_dev.h; fusion, compaction and replay: msl_sf_fuse.hip, msl_sf_compact.hip, msl_sf_replay.hip.

#include "msl_sf_map_dev.h"

namespace {
// ---- map maintenance: ordered selection of surfels by a predicate -------------------------------
// mode 0: updateTimes > 0 && lastUpdate == arg (moveAddSurfels, src/SurfelMapping.cpp:213)   mode 1: updateTimes >= arg (Stop, :68)
__device__ __forceinline__ bool select_pred(const HotRec &h, int mode, int arg) {
    return mode == 0 ? (h.updateTimes > 0 && h.lastUpdate == arg) : (h.updateTimes >= arg);
}
__global__ __launch_bounds__(256) void k_select_count(SfDev P, int mode, int arg) {
    __shared__ unsigned s_c;
    const long long n = P.ctr[CTR_LIVE];
    const long long nblk = (n + SCAN_ITEMS - 1) / SCAN_ITEMS;
    for (long long b = blockIdx.x; b < nblk; b += gridDim.x) {
        if (threadIdx.x == 0) s_c = 0;
        __syncthreads();
        unsigned c = 0;
        for (int k = 0; k < SCAN_ITEMS / 256; k++) {
            const long long i = b * SCAN_ITEMS + k * 256 + threadIdx.x;
            if (i < n && select_pred(hot_load(P.map, i), mode, arg)) c++;
        }
        if (c) atomicAdd(&s_c, c);
        __syncthreads();
        if (threadIdx.x == 0) P.blockSums[b] = s_c;
        __syncthreads();
    }
}
__global__ __launch_bounds__(1024) void k_select_scan(SfDev P) {   // one workgroup: exclusive scan of the chunk counts, total -> CTR_SELECTED
    __shared__ unsigned s_wave[17];
    const long long n = P.ctr[CTR_LIVE];
    const int nblk = (int)((n + SCAN_ITEMS - 1) / SCAN_ITEMS);
    unsigned carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += 1024) {
        const int b = b0 + threadIdx.x;
        const unsigned v = b < nblk ? P.blockSums[b] : 0;
        unsigned tot;
        const unsigned ex = carry + block_excl_scan(v, s_wave, &tot);
        if (b < nblk) P.blockSums[b] = ex;
        carry += tot;
    }
    if (threadIdx.x == 0) P.ctr[CTR_SELECTED] = carry;
}
__global__ __launch_bounds__(256) void k_select_write(SfDev P, int mode, int arg, msl_surfel *out, int markDeleted) {
    __shared__ unsigned s_wave[17];
    const long long n = P.ctr[CTR_LIVE];
    const long long nblk = (n + SCAN_ITEMS - 1) / SCAN_ITEMS;
    for (long long b = blockIdx.x; b < nblk; b += gridDim.x) {
        unsigned base = P.blockSums[b];
        for (int k = 0; k < SCAN_ITEMS / 256; k++) {           // 256 consecutive surfels per round keep the map order
            const long long i = b * SCAN_ITEMS + k * 256 + threadIdx.x;
            HotRec h{};
            unsigned tl = 0;
            if (i < n) { tl = P.map.hot[i].tl; h = hot_load(P.map, i); }
            const bool sel = i < n && select_pred(h, mode, arg);
            unsigned tot;
            const unsigned pos = base + block_excl_scan(sel ? 1u : 0u, s_wave, &tot);
            if (sel) {
                msl_surfel e;
                load_surfel(P.map, i, h, e);
                out[pos] = e;
                if (markDeleted) hot_mark_deleted(P.map, i, tl);   // "Delete the surfel from the local point" (:224)
            }
            base += tot;
        }
    }
}
__global__ void k_add_ctr(long long *ctr, long long add) {
    if (threadIdx.x == 0) { ctr[CTR_LIVE] += add; ctr[CTR_BEFORE] = ctr[CTR_LIVE]; ctr[CTR_AFTER] = ctr[CTR_LIVE]; }
}
__global__ __launch_bounds__(256) void k_aos_to_soa_at(MapSoA M, const msl_surfel *src, long long n, const long long *ctr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) store_surfel(M, ctr[CTR_LIVE] + i, src[i]);
}

// AoS <-> SoA conversion for upload / download / host-vector mode
__global__ __launch_bounds__(256) void k_aos_to_soa(MapSoA M, const msl_surfel *src, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) store_surfel(M, i, src[i]);
}
__global__ __launch_bounds__(256) void k_soa_to_aos(MapSoA M, msl_surfel *dst, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const HotRec h = hot_load(M, i);
    msl_surfel e;
    load_surfel(M, i, h, e);
    dst[i] = e;
}
// wide: -1 = leave the wide-record flags (CTR_WIDE) alone (upload: k_aos_to_soa has just set them if needed), otherwise the restored snapshot's flags
__global__ void k_set_ctr(long long *ctr, long long n, unsigned *delUCount, int wide) {
    if (threadIdx.x == 0) {
        delUCount[0] = 0;
        ctr[CTR_LIVE] = n; ctr[CTR_NEW] = 0; ctr[CTR_DELETED] = 0; ctr[CTR_UPDATED] = 0; ctr[CTR_BEFORE] = n; ctr[CTR_AFTER] = n; ctr[CTR_TAIL_FLAG] = 0;
        if (wide >= 0) ctr[CTR_WIDE] = wide;
    }
}

// Host-vector mode, sparse case: the records this keyframe touched (updated: lastUpdate == ref; deleted: updateTimes == 0) of the sub-blocks that
// report any, as a compact list {index, reference-layout record}.  One wave per sub-block; slots by one atomic per wave.
__global__ __launch_bounds__(64) void k_collect_changed(SfDev P, int ref, long long n, unsigned *count, unsigned *idxOut, msl_surfel *recOut, unsigned capOut) {
    const long long sb = blockIdx.x;
    if (!(P.blockSums[sb] | P.blockUpd[sb])) return;
    const unsigned lane = threadIdx.x;
    for (int k = 0; k < SUB_ITEMS / 64; k++) {
        const long long i = sb * SUB_ITEMS + k * 64 + lane;
        HotRec h; h.px = h.py = h.pz = 0; h.updateTimes = 1; h.lastUpdate = ref - 1;
        if (i < n) h = hot_load(P.map, i);
        const bool ch = i < n && (h.updateTimes == 0 || h.lastUpdate == ref);
        const unsigned long long m = __ballot(ch);
        if (!m) continue;
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(count, (unsigned)__popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (ch) {
            const unsigned j = base + lane_rank(m);
            if (j < capOut) { msl_surfel e; load_surfel(P.map, i, h, e); recOut[j] = e; idxOut[j] = (unsigned)i; }
        }
    }
}

__global__ void k_empty(int grid_dummy) { (void)grid_dummy; }
}  // namespace

namespace msl {
namespace sf {
void map_launch_empty_pair(KernelProfiler &prof, hipStream_t st) {   // what an event pair reports for an EMPTY dispatch at this place of the chain
    hipEvent_t ea, eb;   // (the pair's first event completes with the previous command, so every event time contains the dependent-launch gap)
    if (prof.kernel_pair(SK_NEW, &ea, &eb)) hipExtLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, st, ea, eb, 0, 0);
}
void map_launch_set_ctr(hipStream_t st, const SfDev &P, long long n, int wide) { hipLaunchKernelGGL(k_set_ctr, dim3(1), dim3(64), 0, st, P.ctr, n, P.delUCount, wide); }
void map_launch_add_ctr(hipStream_t st, const SfDev &P, long long add) { hipLaunchKernelGGL(k_add_ctr, dim3(1), dim3(64), 0, st, P.ctr, add); }
void map_launch_aos_to_soa(KernelProfiler &prof, hipStream_t st, const SfDev &P, const msl_surfel *src, long long n, bool atEnd) {
    if (atEnd) hipLaunchKernelGGL(k_aos_to_soa_at, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P.map, src, n, P.ctr);
    else MSL_SF_LAUNCH(prof, SK_CONVERT, st, k_aos_to_soa, dim3((unsigned)((n + 255) / 256)), dim3(256), P.map, src, n);
}
void map_launch_soa_to_aos(KernelProfiler &prof, hipStream_t st, const SfDev &P, msl_surfel *dst, long long n) {
    MSL_SF_LAUNCH(prof, SK_CONVERT, st, k_soa_to_aos, dim3((unsigned)((n + 255) / 256)), dim3(256), P.map, dst, n);
}
void map_launch_select_count(hipStream_t st, const SfDev &P, int mode, int arg) {
    hipLaunchKernelGGL(k_select_count, dim3(512), dim3(256), 0, st, P, mode, arg);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, st, P);
}
void map_launch_select_write(hipStream_t st, const SfDev &P, int mode, int arg, msl_surfel *out, int markDeleted) {
    hipLaunchKernelGGL(k_select_write, dim3(512), dim3(256), 0, st, P, mode, arg, out, markDeleted);
}
void map_launch_collect_changed(hipStream_t st, const SfDev &P, int ref, long long n, unsigned *count, unsigned *idxOut, msl_surfel *recOut, unsigned capOut) {
    const unsigned nblk = (unsigned)((n + SUB_ITEMS - 1) / SUB_ITEMS);
    hipLaunchKernelGGL(k_collect_changed, dim3(nblk), dim3(64), 0, st, P, ref, n, count, idxOut, recOut, capOut);
}
void map_launch_empty(hipStream_t st, int grid, hipEvent_t a, hipEvent_t b) { hipExtLaunchKernelGGL(k_empty, dim3((unsigned)grid), dim3(64), 0, st, a, b, 0, grid); }
}  // namespace sf
}  // namespace msl
