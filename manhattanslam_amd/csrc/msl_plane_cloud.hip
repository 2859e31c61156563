// msl_plane_cloud.hip -- the plane clouds for gfx950: the tail of Frame::ExtractPlanes and the map-plane merge.
//
// msl_plane_clouds      Frame::ExtractPlanes after runPlaneDetection (reference src/Frame.cc:611-653) with Frame::MaxPointDistanceFromPlane
//                       (:662-709): gather, pcl::VoxelGrid, the gate, pcl::SACSegmentation, the sign rule
// msl_map_plane_merge   the loop of src/Tracking.cc:429-436 over MapPlane::UpdateCoefficientsAndPoints(Frame&, id) (src/MapPlane.cc:201-218)
//
// tests/plane_cloud_model.py is the contract; every sum here is either an integer sum (no order) or runs in the layout
// that model states.  On the matcher handle's stream:
//   k_pc_voxel    resident workgroups walk the (frame, detector plane) items: voxel_filter of the gathered vertices -> the coarse cloud
//   k_pc_model    one workgroup per (frame, detector plane): the coarse cloud in LDS, gate, RANSAC iterations one after another (each a
//                 sample by thread 0 and an inlier count by all), the refit in 256 interleaved partials and a tree, Jacobi in thread 0
//   k_pc_compact  one workgroup per frame: the kept planes in detector order, offsets, the copy into the CSR
//   k_pm_merge    resident workgroups walk the (frame, frame plane) items; the first frame plane that names a row owns it and runs the
//                 row's merges in ascending k, the running cloud in the item's scratch
//   k_pm_scan     one workgroup per frame: the row counts, the prefix sum, merge_status
//   k_pm_copy     one wave per (frame, row): the row from the merge's scratch or, untouched, from the input
// voxel_filter: no point is sorted.  Pass 1 inserts the 64-bit voxel keys ((vz, vy, vx), 21 bits each) into an open-addressing hash of
// 8192 slots in LDS and tracks the bounding box; the at most 4096 unique keys are sorted in LDS (bitonic) and every slot learns its rank;
// pass 2 adds each point's quantised coordinates (int64), count and colour to the accumulators of its rank with atomics -- in LDS for a
// cloud of at most 1024 voxels, in the workgroup's global slab above that; the means are written in rank order.
#include "msl_index_check.h"
#include "msl_jacobi.h"
#include "msl_match_handle.h"
#include "msl_match_math.h"
#include "msl_plane_tables.h"

#include <algorithm>
#include <climits>
#include <cmath>

using namespace msl;

namespace {

constexpr int MAX_VOX = MSL_PLANE_CLOUD_MAX_VOXELS, HASH = 8192, VOX_NT = 1024, MODEL_NT = 256, MAX_BLOCKS = 256;
constexpr int MAX_ITER = 4096;
constexpr int LDS_VOX = 1024;                      // voxel_filter: clouds up to this many voxels accumulate in LDS
constexpr int VOX_BIAS = 1 << 20;                  // voxel indices lie in [-2^20, 2^20): |x| < 32768 and 1 / leaf <= 32
constexpr unsigned long long NO_KEY = ~0ull;       // keys hold 63 bits
static_assert(MAX_VOX == 4096 && HASH == 2 * MAX_VOX && MAX_VOX + VOX_NT < HASH, "the hash never fills: inserts stop above MAX_VOX");
static_assert(MAX_VOX == 16 * MODEL_NT, "k_pc_model: 16 coarse points per thread in the ordered compaction");

// The LDS of a voxel_filter workgroup (dynamic: above the static limit)
struct VoxLds {
    unsigned long long key[HASH];                  // the hash: voxel keys, NO_KEY = free
    unsigned long long sorted[MAX_VOX];            // the unique keys, ascending
    uint16_t rank[HASH];                           // slot -> position of its key in sorted
    unsigned long long sum[3][LDS_VOX];            // the accumulators of a cloud of at most LDS_VOX voxels (larger ones: the Slab)
    unsigned cnt[LDS_VOX];
    unsigned col[3][LDS_VOX];
    int lo[3], hi[3];                              // bounding box in voxels
    int count, fill;
};
static_assert(sizeof(VoxLds) <= 160 * 1024, "one workgroup per CU");

// The accumulators of one workgroup for a cloud of more than LDS_VOX voxels, by rank
struct Slab {
    unsigned long long sum[3][MAX_VOX];            // int64 sums of the quantised coordinates (two's complement: unsigned adds wrap alike)
    unsigned cnt[MAX_VOX];
    unsigned col[3][MAX_VOX];
};

// The per-item scratch: coarse cloud, count, status, coefficients
struct Work {
    float *pts; uint8_t *rgb; int32_t *cnt, *st; float *coef;
};
inline size_t work_bytes(size_t items) { return items * ((size_t)MAX_VOX * 15 + 24); }
inline Work work_of(void *base, size_t items) {
    Work W;
    W.pts = (float *)base;
    W.cnt = (int32_t *)(W.pts + items * MAX_VOX * 3);
    W.st = W.cnt + items;
    W.coef = (float *)(W.st + items);
    W.rgb = (uint8_t *)(W.coef + items * 4);
    return W;
}

__device__ __forceinline__ bool usable(float x, float y, float z) { return fabsf(x) < 32768.0f && fabsf(y) < 32768.0f && fabsf(z) < 32768.0f; }
__device__ __forceinline__ unsigned key_slot(unsigned long long k) { return (unsigned)((k * 0x9E3779B97F4A7C15ull) >> 51); }   // 13 bits
__device__ __forceinline__ unsigned long long voxel_key(int vx, int vy, int vz) {
    return ((unsigned long long)(unsigned)(vz + VOX_BIAS) << 42) | ((unsigned long long)(unsigned)(vy + VOX_BIAS) << 21) |
           (unsigned long long)(unsigned)(vx + VOX_BIAS);
}
__device__ __forceinline__ unsigned find_slot(const VoxLds &L, unsigned long long k) {
    unsigned s = key_slot(k);
    for (int probe = 0; probe < HASH && L.key[s] != k; probe++) s = (s + 1) & (HASH - 1);
    return s;
}

// pcl::VoxelGrid of the n points src(i, p, c) hands out (false: absent) by the whole workgroup.  Returns 0 with *out_n voxels written to
// out_pts (and out_rgb when colour), or MSL_PLANE_CLOUD_GRID / _VOXELS with nothing written.  out_pts may be memory src reads: every read
// is behind a barrier before the first write.  Uniform: every thread gets the same status and count.
template <class Src>
__device__ int voxel_filter(VoxLds &L, Slab *S, int n, float inv, bool colour, Src src, float *out_pts, uint8_t *out_rgb, int *out_n) {
    const int t = threadIdx.x, nt = blockDim.x;
    __syncthreads();                                                          // the previous use of L is over
    for (int s = t; s < HASH; s += nt) L.key[s] = NO_KEY;
    if (t < 3) { L.lo[t] = INT_MAX; L.hi[t] = INT_MIN; }
    if (t == 0) { L.count = 0; L.fill = 0; }
    __syncthreads();
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};   // this thread's bounding box: one LDS atomic per axis at the end
    for (int i = t; i < n; i += nt) {
        float p[3]; uint8_t c[3];
        if (!src(i, p, c) || !usable(p[0], p[1], p[2])) continue;
        const int vx = (int)floorf(p[0] * inv), vy = (int)floorf(p[1] * inv), vz = (int)floorf(p[2] * inv);
        lo[0] = min(lo[0], vx); hi[0] = max(hi[0], vx);
        lo[1] = min(lo[1], vy); hi[1] = max(hi[1], vy);
        lo[2] = min(lo[2], vz); hi[2] = max(hi[2], vz);
        if (__hip_atomic_load(&L.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > MAX_VOX) continue;   // already too many
        const unsigned long long k = voxel_key(vx, vy, vz);
        unsigned s = key_slot(k);
        for (int probe = 0; probe < HASH; probe++) {
            unsigned long long old = L.key[s];
            if (old == NO_KEY) old = atomicCAS(&L.key[s], NO_KEY, k);
            if (old == NO_KEY) { atomicAdd(&L.count, 1); break; }
            if (old == k) break;
            s = (s + 1) & (HASH - 1);
        }
    }
    if (lo[0] <= hi[0]) {
#pragma unroll
        for (int a = 0; a < 3; a++) { atomicMin(&L.lo[a], lo[a]); atomicMax(&L.hi[a], hi[a]); }
    }
    __syncthreads();
    const int count = L.count;
    if (count == 0) { *out_n = 0; return 0; }
    const long long span = (long long)((long long)L.hi[0] - L.lo[0] + 1) * ((long long)L.hi[1] - L.lo[1] + 1) * ((long long)L.hi[2] - L.lo[2] + 1);
    if (span > (long long)INT_MAX) return MSL_PLANE_CLOUD_GRID;
    if (count > MAX_VOX) return MSL_PLANE_CLOUD_VOXELS;
    const int n2 = pow2_at_least(count);
    for (int r = t; r < n2; r += nt) L.sorted[r] = NO_KEY;
    __syncthreads();
    for (int s = t; s < HASH; s += nt)
        if (L.key[s] != NO_KEY) L.sorted[atomicAdd(&L.fill, 1)] = L.key[s];
    bitonic_sort(L.sorted, n2);
    const bool small = count <= LDS_VOX;                                      // the accumulators fit in LDS: the atomics stay on the CU
    for (int r = t; r < count; r += nt) {
        L.rank[find_slot(L, L.sorted[r])] = (uint16_t)r;
        if (small) {
            L.sum[0][r] = 0; L.sum[1][r] = 0; L.sum[2][r] = 0; L.cnt[r] = 0;
            L.col[0][r] = 0; L.col[1][r] = 0; L.col[2][r] = 0;
        } else {
            S->sum[0][r] = 0; S->sum[1][r] = 0; S->sum[2][r] = 0; S->cnt[r] = 0;
            S->col[0][r] = 0; S->col[1][r] = 0; S->col[2][r] = 0;
        }
    }
    __threadfence();                                                          // the zeros are in place before the first atomic
    __syncthreads();
    for (int i = t; i < n; i += nt) {
        float p[3]; uint8_t c[3];
        if (!src(i, p, c) || !usable(p[0], p[1], p[2])) continue;
        const int vx = (int)floorf(p[0] * inv), vy = (int)floorf(p[1] * inv), vz = (int)floorf(p[2] * inv);
        const int r = L.rank[find_slot(L, voxel_key(vx, vy, vz))];
        unsigned long long q[3];
#pragma unroll
        for (int a = 0; a < 3; a++) q[a] = (unsigned long long)(long long)rint((double)p[a] * 16777216.0);
        if (small) {
#pragma unroll
            for (int a = 0; a < 3; a++) atomicAdd(&L.sum[a][r], q[a]);
            atomicAdd(&L.cnt[r], 1u);
            if (colour) {
#pragma unroll
                for (int a = 0; a < 3; a++) atomicAdd(&L.col[a][r], (unsigned)c[a]);
            }
        } else {
#pragma unroll
            for (int a = 0; a < 3; a++) atomicAdd(&S->sum[a][r], q[a]);
            atomicAdd(&S->cnt[r], 1u);
            if (colour) {
#pragma unroll
                for (int a = 0; a < 3; a++) atomicAdd(&S->col[a][r], (unsigned)c[a]);
            }
        }
    }
    __threadfence();
    __syncthreads();                                                          // every read of src is over: out_pts may alias it
    for (int r = t; r < count; r += nt) {
        const unsigned cnt = small ? L.cnt[r] : __hip_atomic_load(&S->cnt[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const long long sum = (long long)(small ? L.sum[a][r] : __hip_atomic_load(&S->sum[a][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            out_pts[3 * (size_t)r + a] = (float)((double)sum / 16777216.0 / (double)cnt);
        }
        if (colour) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const unsigned cs = small ? L.col[a][r] : __hip_atomic_load(&S->col[a][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                out_rgb[3 * (size_t)r + a] = (uint8_t)((float)cs / (float)cnt);
            }
        }
    }
    *out_n = count;
    __syncthreads();                                                          // the output is there for the whole workgroup
    return 0;
}

// ---- msl_plane_clouds -----------------------------------------------------------------------------------------------------------------------
struct CloudDev {
    int nFrames, nv, maxPlanes, pcap, ptcap;
    msl_plane_cloud_params prm;
    const double *cloud; const uint8_t *rgb; const int32_t *vOff, *vIdx; const msl_peac_plane *planes; const int32_t *nPlanes; const uint32_t *seed;
    int32_t *nOut; float *coef; int32_t *npts, *src, *ptOff; float *pts; uint8_t *rgbOut; int32_t *status;
    Slab *slab; Work W;
};

extern __shared__ unsigned long long dyn_lds[];

__global__ __launch_bounds__(VOX_NT) void k_pc_voxel(CloudDev D) {
    VoxLds &L = *reinterpret_cast<VoxLds *>(dyn_lds);
    Slab *S = D.slab + blockIdx.x;
    const float inv = 1.0f / D.prm.leaf;
    const bool colour = D.rgb != nullptr;
    const int items = D.nFrames * D.maxPlanes;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int f = it / D.maxPlanes, i = it - f * D.maxPlanes;
        if (i >= clampi(D.nPlanes[f], 0, D.maxPlanes)) continue;
        const int32_t *off = D.vOff + (size_t)f * (D.maxPlanes + 1);
        const int b = clampi(off[i], 0, D.nv), e = clampi(off[i + 1], b, D.nv), nv = D.nv;
        const int32_t *idx = D.vIdx + (size_t)f * nv + b;
        const double *cloud = D.cloud + (size_t)f * nv * 3;
        const uint8_t *rgb = colour ? D.rgb + (size_t)f * nv * 3 : nullptr;
        int cnt = 0;
        const int st = voxel_filter(L, S, e - b, inv, colour,
                                    [=](int q, float *p, uint8_t *c) {
                                        const int v = idx[q];
                                        if (v < 0 || v >= nv) return false;                   // outside the cloud: absent
                                        for (int a = 0; a < 3; a++) p[a] = (float)cloud[3 * (size_t)v + a];   // src/Frame.cc:616-618
                                        if (rgb) for (int a = 0; a < 3; a++) c[a] = rgb[3 * (size_t)v + a];
                                        return true;
                                    },
                                    D.W.pts + (size_t)it * MAX_VOX * 3, D.W.rgb + (size_t)it * MAX_VOX * 3, &cnt);
        if (threadIdx.x == 0) { D.W.cnt[it] = st ? 0 : cnt; D.W.st[it] = st; }
    }
}

// The LDS of k_pc_model
struct ModelLds {
    float p[3][MAX_VOX];
    uint16_t list[MAX_VOX];                        // the inliers, ascending
    double part[MODEL_NT][3];
    int scan[MODEL_NT];
    float hyp[4];
    int valid, cnt, any;
};

__device__ __forceinline__ float plane_dist(const float *h, float x, float y, float z) { return fabsf(h[0] * x + h[1] * y + h[2] * z + h[3]); }

// Three sums over the n listed points in the fixed layout (element e to partial e mod 256 in ascending order, then a pairwise tree); the
// values of element e are val(e, out[3]).  Every thread gets the sums.
template <class Val>
__device__ __forceinline__ void tree_sum3(ModelLds &M, int n, Val val, double out[3]) {
    const int t = threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int e = t; e < n; e += MODEL_NT) {
        double v[3];
        val(e, v);
        acc[0] = acc[0] + v[0]; acc[1] = acc[1] + v[1]; acc[2] = acc[2] + v[2];
    }
    __syncthreads();
    M.part[t][0] = acc[0]; M.part[t][1] = acc[1]; M.part[t][2] = acc[2];
    for (int h = MODEL_NT / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if (t < h) {
            M.part[t][0] = M.part[t][0] + M.part[t + h][0]; M.part[t][1] = M.part[t][1] + M.part[t + h][1];
            M.part[t][2] = M.part[t][2] + M.part[t + h][2];
        }
    }
    __syncthreads();
    out[0] = M.part[0][0]; out[1] = M.part[0][1]; out[2] = M.part[0][2];
}

__global__ __launch_bounds__(MODEL_NT) void k_pc_model(CloudDev D) {
    __shared__ ModelLds M;
    const int f = blockIdx.y, i = blockIdx.x, t = threadIdx.x;
    if (i >= clampi(D.nPlanes[f], 0, D.maxPlanes)) return;
    const int it = f * D.maxPlanes + i;
    if (D.W.st[it] != 0) return;                                              // the voxel grid's status stands
    const int N = clampi(D.W.cnt[it], 0, MAX_VOX);
    const float *src = D.W.pts + (size_t)it * MAX_VOX * 3;
    for (int q = t; q < N; q += MODEL_NT) { M.p[0][q] = src[3 * q]; M.p[1][q] = src[3 * q + 1]; M.p[2][q] = src[3 * q + 2]; }
    // the gate (src/Frame.cc:626-634, :668-682)
    const msl_peac_plane &P = D.planes[(size_t)f * D.maxPlanes + i];
    float g[4];
    g[0] = (float)P.normal[0]; g[1] = (float)P.normal[1]; g[2] = (float)P.normal[2];
    g[3] = (float)-(P.normal[0] * P.center[0] + P.normal[1] * P.center[1] + P.normal[2] * P.center[2]);
    const float th = D.prm.dis_th;
    if (t == 0) M.any = 0;
    __syncthreads();
    bool far = false;
    for (int q = t; q < N; q += MODEL_NT) far = far || plane_dist(g, M.p[0][q], M.p[1][q], M.p[2][q]) > th;
    if (far) atomicOr(&M.any, 1);
    __syncthreads();
    if (M.any) { if (t == 0) D.W.st[it] = MSL_PLANE_CLOUD_GATE; return; }
    if (N < 4) { if (t == 0) D.W.st[it] = MSL_PLANE_CLOUD_FEW; return; }
    // RANSAC: one iteration after another, as the stop test reads the best count so far
    const unsigned seed = D.seed[f] ^ fmix32((unsigned)i);
    const int maxIt = D.prm.max_iterations;
    const double pStop = 1.0 - D.prm.probability;
    float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int bestN = 0;
    bool have = false;
    for (int k = 0;; k++) {
        if (t == 0) {                                                         // the sample: swap-with-back removal without the list
            const unsigned h0 = sampler_iteration(seed, k);
            int pos[3], val[3], s[3];
            for (int j = 0; j < 3; j++) {
                const int r = sampler_draw(h0, j, (unsigned)(N - j));
                int v = r, back = N - 1 - j;
                for (int q = 0; q < 3; q++) {                                 // later replacements shadow earlier ones
                    if (q < j && pos[q] == r) v = val[q];
                    if (q < j && pos[q] == back) back = val[q];
                }
                pos[j] = r; val[j] = back; s[j] = v;
            }
            const float p0[3] = {M.p[0][s[0]], M.p[1][s[0]], M.p[2][s[0]]};
            const float a[3] = {M.p[0][s[1]] - p0[0], M.p[1][s[1]] - p0[1], M.p[2][s[1]] - p0[2]};
            const float b[3] = {M.p[0][s[2]] - p0[0], M.p[1][s[2]] - p0[1], M.p[2][s[2]] - p0[2]};
            const float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
            const float nn = (float)sqrt((double)(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]));
            M.valid = nn > 0 ? 1 : 0;
            const float nx = c[0] / nn, ny = c[1] / nn, nz = c[2] / nn;
            M.hyp[0] = nx; M.hyp[1] = ny; M.hyp[2] = nz; M.hyp[3] = -(nx * p0[0] + ny * p0[1] + nz * p0[2]);
            M.cnt = 0;
        }
        __syncthreads();
        const bool valid = M.valid != 0;
        const float h[4] = {M.hyp[0], M.hyp[1], M.hyp[2], M.hyp[3]};
        if (valid) {
            int c = 0;
            for (int q = t; q < N; q += MODEL_NT) c += plane_dist(h, M.p[0][q], M.p[1][q], M.p[2][q]) < th ? 1 : 0;
            if (c) atomicAdd(&M.cnt, c);
        }
        __syncthreads();
        const int cnt = M.cnt;
        if (valid && cnt > bestN) { bestN = cnt; have = true; best[0] = h[0]; best[1] = h[1]; best[2] = h[2]; best[3] = h[3]; }
        __syncthreads();                                                      // M.hyp and M.cnt are free for the next sample
        const int done = k + 1;
        if (done >= maxIt) break;
        const double w = (double)bestN / (double)N, q = 1.0 - w * w * w;
        double pw = 1.0;
        for (int e = 0; e < done; e++) pw = pw * q;
        if (pw <= pStop) break;
    }
    if (!have) { if (t == 0) D.W.st[it] = MSL_PLANE_CLOUD_NO_MODEL; return; }
    float out[4] = {best[0], best[1], best[2], best[3]};
    if (bestN > 3) {                                                          // the refit over the inliers in ascending order
        int mine = 0;
        for (int q = 16 * t; q < 16 * t + 16 && q < N; q++) mine += plane_dist(best, M.p[0][q], M.p[1][q], M.p[2][q]) < th ? 1 : 0;
        M.scan[t] = mine;
        __syncthreads();
        int at = 0;
        for (int q = 0; q < t; q++) at += M.scan[q];
        for (int q = 16 * t; q < 16 * t + 16 && q < N; q++)
            if (plane_dist(best, M.p[0][q], M.p[1][q], M.p[2][q]) < th) M.list[at++] = (uint16_t)q;
        __syncthreads();
        const int n = bestN;
        double s[3], cen[3], xx[3], yy[3];
        tree_sum3(M, n, [&](int e, double *v) { const int q = M.list[e]; v[0] = (double)M.p[0][q]; v[1] = (double)M.p[1][q]; v[2] = (double)M.p[2][q]; }, s);
        cen[0] = s[0] / (double)n; cen[1] = s[1] / (double)n; cen[2] = s[2] / (double)n;
        tree_sum3(M, n, [&](int e, double *v) {
            const int q = M.list[e];
            const double dx = (double)M.p[0][q] - cen[0], dy = (double)M.p[1][q] - cen[1], dz = (double)M.p[2][q] - cen[2];
            v[0] = dx * dx; v[1] = dx * dy; v[2] = dx * dz;
        }, xx);
        tree_sum3(M, n, [&](int e, double *v) {
            const int q = M.list[e];
            const double dy = (double)M.p[1][q] - cen[1], dz = (double)M.p[2][q] - cen[2];
            v[0] = dy * dy; v[1] = dy * dz; v[2] = dz * dz;
        }, yy);
        if (t == 0) {
            double A[9] = {xx[0], xx[1], xx[2], xx[1], yy[0], yy[1], xx[2], yy[1], yy[2]};
            double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll 1
            for (int sw = 0; sw < JACOBI_SWEEPS; sw++) jacobi_sweep<3>(A, V);
            // descending order with the lower index first on ties: the last is the smallest, the highest index among equals
            int m = 0; double dm = A[0];
            if (A[4] <= dm) { dm = A[4]; m = 1; }
            if (A[8] <= dm) { dm = A[8]; m = 2; }
            const double v0 = m == 0 ? V[0] : (m == 1 ? V[1] : V[2]), v1 = m == 0 ? V[3] : (m == 1 ? V[4] : V[5]),
                         v2 = m == 0 ? V[6] : (m == 1 ? V[7] : V[8]);
            const double nn = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
            const double nx = v0 / nn, ny = v1 / nn, nz = v2 / nn;
            out[0] = (float)nx; out[1] = (float)ny; out[2] = (float)nz; out[3] = (float)-(nx * cen[0] + ny * cen[1] + nz * cen[2]);
        }
    }
    if (t == 0) {
        const float oldVal = g[3], newVal = out[3];                           // src/Frame.cc:694-706
        if ((newVal < 0 && oldVal > 0) || (newVal > 0 && oldVal < 0)) { out[0] = -out[0]; out[1] = -out[1]; out[2] = -out[2]; out[3] = -out[3]; }
        for (int c = 0; c < 4; c++) D.W.coef[4 * (size_t)it + c] = out[c];
    }
}

__global__ __launch_bounds__(MODEL_NT) void k_pc_compact(CloudDev D) {
    __shared__ int keptSrc[MAX_PCAP], keptOff[MAX_PCAP + 1], nKept;
    const int f = blockIdx.x, t = threadIdx.x;
    const int np = clampi(D.nPlanes[f], 0, D.maxPlanes);
    if (t == 0) {                                                             // the push_backs of src/Frame.cc:651-652, in detector order
        int n = 0, run = 0;
        bool full = false;
        keptOff[0] = 0;
        for (int i = 0; i < np; i++) {
            const int it = f * D.maxPlanes + i;
            int st = D.W.st[it];
            if (st == MSL_PLANE_CLOUD_KEPT) {
                const int c = D.W.cnt[it];
                if (full || n == D.pcap || run + c > D.ptcap) { full = true; st = MSL_PLANE_CLOUD_NO_ROOM; }
                else { keptSrc[n] = i; run += c; keptOff[++n] = run; }
            }
            D.status[(size_t)f * D.maxPlanes + i] = st;
        }
        nKept = n;
        D.nOut[f] = n;
        D.ptOff[(size_t)f * (D.pcap + 1)] = 0;
    }
    __syncthreads();
    const int n = nKept;
    if (t < n) {
        const int it = f * D.maxPlanes + keptSrc[t];
        const size_t k = (size_t)f * D.pcap + t;
        for (int c = 0; c < 4; c++) D.coef[4 * k + c] = D.W.coef[4 * (size_t)it + c];
        D.npts[k] = keptOff[t + 1] - keptOff[t];
        D.src[k] = keptSrc[t];
        D.ptOff[(size_t)f * (D.pcap + 1) + t + 1] = keptOff[t + 1];
    }
    for (int k = 0; k < n; k++) {
        const int it = f * D.maxPlanes + keptSrc[k], c3 = 3 * (keptOff[k + 1] - keptOff[k]);
        const size_t o3 = ((size_t)f * D.ptcap + keptOff[k]) * 3;
        const float *sp = D.W.pts + (size_t)it * MAX_VOX * 3;
        const uint8_t *sc = D.W.rgb + (size_t)it * MAX_VOX * 3;
        for (int q = t; q < c3; q += MODEL_NT) {
            D.pts[o3 + q] = sp[q];
            if (D.rgbOut) D.rgbOut[o3 + q] = sc[q];
        }
    }
}

// ---- msl_map_plane_merge --------------------------------------------------------------------------------------------------------------------
struct MergeDev {
    int nFrames, pcap, fptcap, mcap, ptcap;
    msl_plane_cloud_params prm;
    const int32_t *nPlanes, *ptOff; const float *pts; const uint8_t *rgb; const int32_t *into; const double *Twc;
    const int32_t *mpOff; const float *mpPts; const uint8_t *mpRgb; const int32_t *nMap;
    int32_t *offOut; float *ptsOut; uint8_t *rgbOut; int32_t *status;
    Slab *slab; Work W;
};

// The row frame plane k merges into, or -1 (none, or outside the map)
__device__ __forceinline__ int row_of(const MergeDev &D, int f, int k, int nMap) {
    const int j = D.into[(size_t)f * D.pcap + k];
    return j >= 0 && j < nMap ? j : -1;
}
// The first frame plane that names row j, or -1
__device__ __forceinline__ int owner_of(const MergeDev &D, int f, int j, int np, int nMap) {
    for (int k = 0; k < np; k++)
        if (row_of(D, f, k, nMap) == j) return k;
    return -1;
}

__global__ __launch_bounds__(VOX_NT) void k_pm_merge(MergeDev D) {
    VoxLds &L = *reinterpret_cast<VoxLds *>(dyn_lds);
    Slab *S = D.slab + blockIdx.x;
    const float inv = 1.0f / D.prm.leaf;
    const bool colour = D.rgb != nullptr;
    const int items = D.nFrames * D.pcap;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int f = it / D.pcap, k0 = it - f * D.pcap;
        const int np = clampi(D.nPlanes[f], 0, D.pcap), nMap = clampi(D.nMap[f], 0, D.mcap);
        if (k0 >= np) continue;
        const int j = row_of(D, f, k0, nMap);
        if (j < 0 || owner_of(D, f, j, np, nMap) != k0) continue;
        const int32_t *mo = D.mpOff + (size_t)f * (D.mcap + 1);
        const int mb = clampi(mo[j], 0, D.ptcap), me = clampi(mo[j + 1], mb, D.ptcap);
        const float *cur = D.mpPts + ((size_t)f * D.ptcap + mb) * 3;          // the row's cloud so far
        const uint8_t *curRgb = colour ? D.mpRgb + ((size_t)f * D.ptcap + mb) * 3 : nullptr;
        int curN = me - mb, failed = 0;
        bool merged = false;
        float *tmp = D.W.pts + (size_t)it * MAX_VOX * 3;
        uint8_t *tmpRgb = D.W.rgb + (size_t)it * MAX_VOX * 3;
        const double *Tp = D.Twc + 12 * (size_t)f;
        double T[12];
        for (int q = 0; q < 12; q++) T[q] = Tp[q];
        const int32_t *fo = D.ptOff + (size_t)f * (D.pcap + 1);
        for (int k = k0; k < np; k++) {                                       // ascending k, each merge on the previous result
            if (row_of(D, f, k, nMap) != j) continue;
            const int fb = clampi(fo[k], 0, D.fptcap), fe = clampi(fo[k + 1], fb, D.fptcap), nF = fe - fb;
            const float *fp = D.pts + ((size_t)f * D.fptcap + fb) * 3;
            const uint8_t *fc = colour ? D.rgb + ((size_t)f * D.fptcap + fb) * 3 : nullptr;
            int cnt = 0;
            const int st = voxel_filter(L, S, nF + curN, inv, colour,
                                        [=](int q, float *p, uint8_t *c) {
                                            if (q < nF) {                      // pcl::transformPointCloud, then *combinedPoints += *mvPlanePoints
                                                const double x = fp[3 * (size_t)q], y = fp[3 * (size_t)q + 1], z = fp[3 * (size_t)q + 2];
                                                for (int r = 0; r < 3; r++) p[r] = (float)(T[4 * r] * x + T[4 * r + 1] * y + T[4 * r + 2] * z + T[4 * r + 3]);
                                                if (fc) for (int a = 0; a < 3; a++) c[a] = fc[3 * (size_t)q + a];
                                            } else {
                                                const size_t m = (size_t)(q - nF);
                                                for (int a = 0; a < 3; a++) p[a] = cur[3 * m + a];
                                                if (curRgb) for (int a = 0; a < 3; a++) c[a] = curRgb[3 * m + a];
                                            }
                                            return true;
                                        },
                                        tmp, tmpRgb, &cnt);
            if (st == 0) { cur = tmp; curRgb = colour ? tmpRgb : nullptr; curN = cnt; merged = true; }
            else if (!failed) failed = st;
        }
        if (threadIdx.x == 0) { D.W.cnt[it] = merged ? curN : -1; D.W.st[it] = failed ? failed : MSL_PLANE_MERGE_MERGED; }
    }
}

__global__ __launch_bounds__(MODEL_NT) void k_pm_scan(MergeDev D) {
    __shared__ int cnt[MAX_PLANE_MCAP + 1];
    __shared__ int16_t own[MAX_PLANE_MCAP];
    __shared__ uint8_t stat[MAX_PLANE_MCAP];
    const int f = blockIdx.x, t = threadIdx.x;
    const int np = clampi(D.nPlanes[f], 0, D.pcap), nMap = clampi(D.nMap[f], 0, D.mcap);
    for (int j = t; j < nMap; j += MODEL_NT) own[j] = -1;
    __syncthreads();
    if (t == 0)
        for (int k = np - 1; k >= 0; k--) {                                   // descending: the first frame plane of a row stays
            const int j = row_of(D, f, k, nMap);
            if (j >= 0) own[j] = (int16_t)k;
        }
    __syncthreads();
    const int32_t *mo = D.mpOff + (size_t)f * (D.mcap + 1);
    for (int j = t; j < nMap; j += MODEL_NT) {
        const int mb = clampi(mo[j], 0, D.ptcap), me = clampi(mo[j + 1], mb, D.ptcap);
        int c = me - mb, st = MSL_PLANE_MERGE_UNTOUCHED;
        if (own[j] >= 0) {
            const int it = f * D.pcap + own[j];
            st = D.W.st[it];
            if (D.W.cnt[it] >= 0) c = D.W.cnt[it];
        }
        cnt[j + 1] = c; stat[j] = (uint8_t)st;
    }
    __syncthreads();
    if (t == 0) {                                                             // the prefix sum; from the first row that does not fit on: empty
        int run = 0;
        bool full = false;
        cnt[0] = 0;
        for (int j = 0; j < nMap; j++) {
            const int c = cnt[j + 1];
            if (full || run + c > D.ptcap) { full = true; stat[j] = MSL_PLANE_MERGE_NO_ROOM; }
            else run += c;
            cnt[j + 1] = run;
        }
    }
    __syncthreads();
    for (int j = t; j <= nMap; j += MODEL_NT) D.offOut[(size_t)f * (D.mcap + 1) + j] = cnt[j];
    for (int j = t; j < nMap; j += MODEL_NT) D.status[(size_t)f * D.mcap + j] = stat[j];
}

__global__ __launch_bounds__(WAVE) void k_pm_copy(MergeDev D) {
    const int j = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    const int np = clampi(D.nPlanes[f], 0, D.pcap), nMap = clampi(D.nMap[f], 0, D.mcap);
    if (j >= nMap) return;
    const int32_t *oo = D.offOut + (size_t)f * (D.mcap + 1);
    const int ob = oo[j], n3 = 3 * (oo[j + 1] - ob);
    if (n3 <= 0) return;
    const int k = owner_of(D, f, j, np, nMap);
    const float *sp; const uint8_t *sc;
    if (k >= 0 && D.W.cnt[f * D.pcap + k] >= 0) {
        sp = D.W.pts + (size_t)(f * D.pcap + k) * MAX_VOX * 3; sc = D.W.rgb + (size_t)(f * D.pcap + k) * MAX_VOX * 3;
    } else {                                                                  // untouched, or every merge failed: the input row, bit for bit
        const int mb = clampi(D.mpOff[(size_t)f * (D.mcap + 1) + j], 0, D.ptcap);
        sp = D.mpPts + ((size_t)f * D.ptcap + mb) * 3; sc = D.mpRgb ? D.mpRgb + ((size_t)f * D.ptcap + mb) * 3 : nullptr;
    }
    const size_t o3 = ((size_t)f * D.ptcap + ob) * 3;
    for (int q = t; q < n3; q += WAVE) {
        D.ptsOut[o3 + q] = sp[q];
        if (D.rgbOut) D.rgbOut[o3 + q] = sc[q];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
bool params_ok(const char *who, const msl_plane_cloud_params *p) {
    if (!(p->leaf >= 1.0f / 32 && p->leaf <= 3.0e38f) || !(p->dis_th == p->dis_th) || p->max_iterations < 1 || p->max_iterations > MAX_ITER ||
        !(p->probability >= 0.0 && p->probability <= 1.0)) {
        set_error("%s: params outside their limits (leaf >= 1 / 32, 1 <= max_iterations <= %d, 0 <= probability <= 1)", who, MAX_ITER);
        return false;
    }
    return true;
}

int check_clouds(int n_frames, int n_vertices, int max_planes, int pcap, int ptcap, const msl_plane_cloud_params *params, const double *cloud,
                 const uint8_t *rgb, const int32_t *vertex_offsets, const int32_t *vertex_indices, const msl_peac_plane *planes,
                 const int32_t *n_planes, const uint32_t *seed, msl_mem mem, int32_t *n_out, float *plane_coef, int32_t *plane_npts,
                 int32_t *plane_src, int32_t *pt_off, float *pts, uint8_t *rgb_out, int32_t *status, msl_mem out_mem) {
    const char *who = "msl_plane_clouds";
    if (!in_range(who, "n_frames", n_frames, 1, MAX_PLANE_FRAMES) || !in_range(who, "n_vertices", n_vertices, 1, MSL_PLANE_CLOUD_MAX_VERTICES) ||
        !in_range(who, "max_planes", max_planes, 1, MAX_PCAP) || !in_range(who, "pcap", pcap, 1, MAX_PCAP) ||
        !in_range(who, "ptcap", ptcap, 1, MAX_PLANE_PTCAP)) return MSL_ERR_INVALID;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(cloud), MSL_NAMED(vertex_offsets), MSL_NAMED(vertex_indices), MSL_NAMED(planes),
                         MSL_NAMED(n_planes), MSL_NAMED(seed), MSL_NAMED(n_out), MSL_NAMED(plane_coef), MSL_NAMED(plane_npts),
                         MSL_NAMED(plane_src), MSL_NAMED(pt_off), MSL_NAMED(pts), MSL_NAMED(status)})) return MSL_ERR_INVALID;
    if ((rgb != nullptr) != (rgb_out != nullptr)) { set_error("%s: rgb and rgb_out go together (both, or both NULL)", who); return MSL_ERR_INVALID; }
    if (!params_ok(who, params)) return MSL_ERR_INVALID;
    if (mem == MSL_MEM_HOST) {
        char why[160];
        if (!check::offsets_ok("vertex_offsets", "n_planes", n_frames, max_planes, n_vertices, vertex_offsets, n_planes, why, sizeof why) ||
            !check::vertex_indices_ok(n_frames, max_planes, n_vertices, vertex_offsets, vertex_indices, n_planes, why, sizeof why))
            return refuse(who, why);
    }
    return MSL_OK;
}

int launch_clouds(msl_match *h, int n_frames, int n_vertices, int max_planes, int pcap, int ptcap, const msl_plane_cloud_params *params,
                  const double *cloud, const uint8_t *rgb, const int32_t *vertex_offsets, const int32_t *vertex_indices,
                  const msl_peac_plane *planes, const int32_t *n_planes, const uint32_t *seed, msl_mem mem, int32_t *n_out, float *plane_coef,
                  int32_t *plane_npts, int32_t *plane_src, int32_t *pt_off, float *pts, uint8_t *rgb_out, int32_t *status, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, V = F * n_vertices, p = F * pcap, items = F * max_planes;
    CloudDev D{};
    D.nFrames = n_frames; D.nv = n_vertices; D.maxPlanes = max_planes; D.pcap = pcap; D.ptcap = ptcap; D.prm = *params;
    Stage S(h, mem, out_mem);
    D.cloud = S.in(cloud, 3 * V); D.rgb = S.in(rgb, 3 * V); D.vOff = S.in(vertex_offsets, items + F); D.vIdx = S.in(vertex_indices, V);
    D.planes = S.in(planes, items); D.nPlanes = S.in(n_planes, F); D.seed = S.in(seed, F);
    // rows beyond the counts keep their bytes: the outputs are in/out
    D.nOut = S.out(n_out, F); D.coef = S.inout(plane_coef, 4 * p); D.npts = S.inout(plane_npts, p); D.src = S.inout(plane_src, p);
    D.ptOff = S.inout(pt_off, p + F); D.pts = S.inout(pts, 3 * F * ptcap); D.rgbOut = S.inout(rgb_out, 3 * F * ptcap);
    D.status = S.inout(status, items);
    MSL_HIP_TRY(S.error());
    const int blocks = (int)std::min<size_t>(items, MAX_BLOCKS);
    MSL_HIP_TRY(h->pcSlab.grow(sizeof(Slab) * MAX_BLOCKS, st));
    MSL_HIP_TRY(h->pcWork.grow(work_bytes(items), st));
    D.slab = (Slab *)h->pcSlab.p; D.W = work_of(h->pcWork.p, items);
    MSL_HIP_TRY(allow_lds(h, LDS_PC_VOXEL, k_pc_voxel, sizeof(VoxLds)));
    hipLaunchKernelGGL(k_pc_voxel, dim3((unsigned)blocks), dim3(VOX_NT), sizeof(VoxLds), st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pc_model, dim3((unsigned)max_planes, (unsigned)n_frames), dim3(MODEL_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pc_compact, dim3((unsigned)n_frames), dim3(MODEL_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_merge(int n_frames, int pcap, int fptcap, int mcap, int ptcap, const msl_plane_cloud_params *params, const int32_t *n_planes,
                const int32_t *pt_off, const float *pts, const uint8_t *rgb, const int32_t *merge_into, const double *Twc,
                const int32_t *mp_pt_off, const float *mp_pts, const uint8_t *mp_rgb, const int32_t *n_map, msl_mem mem, int32_t *mp_pt_off_out,
                float *mp_pts_out, uint8_t *mp_rgb_out, int32_t *merge_status, msl_mem out_mem) {
    const char *who = "msl_map_plane_merge";
    if (!in_range(who, "n_frames", n_frames, 1, MAX_PLANE_FRAMES) || !in_range(who, "pcap", pcap, 1, MAX_PCAP) ||
        !in_range(who, "fptcap", fptcap, 1, MAX_PLANE_PTCAP) || !in_range(who, "mcap", mcap, 1, MAX_PLANE_MCAP) ||
        !in_range(who, "ptcap", ptcap, 1, MAX_PLANE_PTCAP)) return MSL_ERR_INVALID;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(n_planes), MSL_NAMED(pt_off), MSL_NAMED(pts), MSL_NAMED(merge_into), MSL_NAMED(Twc),
                         MSL_NAMED(mp_pt_off), MSL_NAMED(mp_pts), MSL_NAMED(n_map), MSL_NAMED(mp_pt_off_out), MSL_NAMED(mp_pts_out),
                         MSL_NAMED(merge_status)})) return MSL_ERR_INVALID;
    if ((rgb != nullptr) != (mp_rgb != nullptr) || (rgb != nullptr) != (mp_rgb_out != nullptr)) {
        set_error("%s: rgb, mp_rgb and mp_rgb_out go together (all, or all NULL)", who);
        return MSL_ERR_INVALID;
    }
    if (!params_ok(who, params)) return MSL_ERR_INVALID;
    if (mem == MSL_MEM_HOST) {
        char why[160];
        if (!check::offsets_ok("pt_off", "n_planes", n_frames, pcap, fptcap, pt_off, n_planes, why, sizeof why) ||
            !check::offsets_ok("mp_pt_off", "n_map", n_frames, mcap, ptcap, mp_pt_off, n_map, why, sizeof why) ||
            !check::merge_into_ok(n_frames, pcap, mcap, merge_into, n_planes, n_map, why, sizeof why))
            return refuse(who, why);
    }
    return MSL_OK;
}

int launch_merge(msl_match *h, int n_frames, int pcap, int fptcap, int mcap, int ptcap, const msl_plane_cloud_params *params,
                 const int32_t *n_planes, const int32_t *pt_off, const float *pts, const uint8_t *rgb, const int32_t *merge_into, const double *Twc,
                 const int32_t *mp_pt_off, const float *mp_pts, const uint8_t *mp_rgb, const int32_t *n_map, msl_mem mem,
                 int32_t *mp_pt_off_out, float *mp_pts_out, uint8_t *mp_rgb_out, int32_t *merge_status, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, p = F * pcap, m = F * mcap, items = p;
    MergeDev D{};
    D.nFrames = n_frames; D.pcap = pcap; D.fptcap = fptcap; D.mcap = mcap; D.ptcap = ptcap; D.prm = *params;
    Stage S(h, mem, out_mem);
    D.nPlanes = S.in(n_planes, F); D.ptOff = S.in(pt_off, p + F); D.pts = S.in(pts, 3 * F * fptcap); D.rgb = S.in(rgb, 3 * F * fptcap);
    D.into = S.in(merge_into, p); D.Twc = S.in(Twc, 12 * F); D.mpOff = S.in(mp_pt_off, m + F); D.mpPts = S.in(mp_pts, 3 * F * ptcap);
    D.mpRgb = S.in(mp_rgb, 3 * F * ptcap); D.nMap = S.in(n_map, F);
    // rows beyond the counts keep their bytes: the outputs are in/out
    D.offOut = S.inout(mp_pt_off_out, m + F); D.ptsOut = S.inout(mp_pts_out, 3 * F * ptcap); D.rgbOut = S.inout(mp_rgb_out, 3 * F * ptcap);
    D.status = S.inout(merge_status, m);
    MSL_HIP_TRY(S.error());
    const int blocks = (int)std::min<size_t>(items, MAX_BLOCKS);
    MSL_HIP_TRY(h->pcSlab.grow(sizeof(Slab) * MAX_BLOCKS, st));
    MSL_HIP_TRY(h->pcWork.grow(work_bytes(items), st));
    D.slab = (Slab *)h->pcSlab.p; D.W = work_of(h->pcWork.p, items);
    MSL_HIP_TRY(allow_lds(h, LDS_PC_MERGE, k_pm_merge, sizeof(VoxLds)));
    hipLaunchKernelGGL(k_pm_merge, dim3((unsigned)blocks), dim3(VOX_NT), sizeof(VoxLds), st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pm_scan, dim3((unsigned)n_frames), dim3(MODEL_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pm_copy, dim3((unsigned)mcap, (unsigned)n_frames), dim3(WAVE), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_plane_clouds(msl_match *h, int n_frames, int n_vertices, int max_planes, int pcap, int ptcap, const msl_plane_cloud_params *params,
                     const double *cloud, const uint8_t *rgb, const int32_t *vertex_offsets, const int32_t *vertex_indices,
                     const msl_peac_plane *planes, const int32_t *n_planes, const uint32_t *seed, msl_mem mem, int32_t *n_out, float *plane_coef,
                     int32_t *plane_npts, int32_t *plane_src, int32_t *pt_off, float *pts, uint8_t *rgb_out, int32_t *status,
                     msl_mem out_mem) noexcept {
    try {
    return handle_form("msl_plane_clouds", check_clouds, launch_clouds, h, n_frames, n_vertices, max_planes, pcap, ptcap, params, cloud, rgb,
                       vertex_offsets, vertex_indices, planes, n_planes, seed, mem, n_out, plane_coef, plane_npts, plane_src, pt_off, pts, rgb_out,
                       status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_plane_clouds_batch(int device, int n_frames, int n_vertices, int max_planes, int pcap, int ptcap, const msl_plane_cloud_params *params,
                           const double *cloud, const uint8_t *rgb, const int32_t *vertex_offsets, const int32_t *vertex_indices,
                           const msl_peac_plane *planes, const int32_t *n_planes, const uint32_t *seed, msl_mem mem, int32_t *n_out,
                           float *plane_coef, int32_t *plane_npts, int32_t *plane_src, int32_t *pt_off, float *pts, uint8_t *rgb_out,
                           int32_t *status, msl_mem out_mem) noexcept {
    // the outputs keep their bytes beyond the counts: device-memory outputs are read as well
    try {
    return batch_form(check_clouds, launch_clouds, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, n_vertices, max_planes,
                      pcap, ptcap, params, cloud, rgb, vertex_offsets, vertex_indices, planes, n_planes, seed, mem, n_out, plane_coef, plane_npts,
                      plane_src, pt_off, pts, rgb_out, status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_map_plane_merge(msl_match *h, int n_frames, int pcap, int fptcap, int mcap, int ptcap, const msl_plane_cloud_params *params,
                        const int32_t *n_planes, const int32_t *pt_off, const float *pts, const uint8_t *rgb, const int32_t *merge_into,
                        const double *Twc, const int32_t *mp_pt_off, const float *mp_pts, const uint8_t *mp_rgb, const int32_t *n_map, msl_mem mem,
                        int32_t *mp_pt_off_out, float *mp_pts_out, uint8_t *mp_rgb_out, int32_t *merge_status, msl_mem out_mem) noexcept {
    try {
    return handle_form("msl_map_plane_merge", check_merge, launch_merge, h, n_frames, pcap, fptcap, mcap, ptcap, params, n_planes, pt_off, pts, rgb,
                       merge_into, Twc, mp_pt_off, mp_pts, mp_rgb, n_map, mem, mp_pt_off_out, mp_pts_out, mp_rgb_out, merge_status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_map_plane_merge_batch(int device, int n_frames, int pcap, int fptcap, int mcap, int ptcap, const msl_plane_cloud_params *params,
                              const int32_t *n_planes, const int32_t *pt_off, const float *pts, const uint8_t *rgb, const int32_t *merge_into,
                              const double *Twc, const int32_t *mp_pt_off, const float *mp_pts, const uint8_t *mp_rgb, const int32_t *n_map,
                              msl_mem mem, int32_t *mp_pt_off_out, float *mp_pts_out, uint8_t *mp_rgb_out, int32_t *merge_status,
                              msl_mem out_mem) noexcept {
    try {
    return batch_form(check_merge, launch_merge, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, pcap, fptcap, mcap, ptcap,
                      params, n_planes, pt_off, pts, rgb, merge_into, Twc, mp_pt_off, mp_pts, mp_rgb, n_map, mem, mp_pt_off_out, mp_pts_out,
                      mp_rgb_out, merge_status, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
