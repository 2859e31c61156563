// msl_keyframe_planes.hip -- a keyframe that is born with planes, for gfx950: the plane loop of Tracking::CreateNewKeyFrame (reference
// src/Tracking.cc:1620-1645) and of Tracking::StereoInitialization (:594-602) with what the KeyFrame constructor and SetPose do with planes
// (src/KeyFrame.cc:50-52, 74-86) as msl_keyframe_planes[_batch]; the plane part of LocalMapping::ProcessNewKeyFrame
// (src/LocalMapping.cc:160-218) with Map::Add[Partial]ManhattanObservation (src/Map.cc:247-275) as msl_manhattan_observe[_batch].
//
// Kernels (one workgroup per frame):
//   k_keyframe_planes    64 threads, lane k = frame plane k.  The new planes are ranked by a ballot, so the rows are handed out in ascending k
//                        and the first plane without a row is followed only by planes without one; "the first k that names a row" is a
//                        walk over the lanes below k in LDS.
//   k_manhattan_observe  1024 threads.  The at most 64 distinct held rows are ranked ascending into dense ids; the gate of every pair of frame
//                        planes is one bit of a 64 x 64 matrix; every passing triple sets bit (a << 12 | b << 6 | c), a < b < c dense ids,
//                        of a 64^3-bit map in LDS (32 KiB) and every passing pair bit (a << 6 | b) of a 64^2-bit map.  The dense id is
//                        monotone in the row, so the set bits in ascending order are the keyframe's keys sorted and without duplicates.
//                        Bits whose key the old table holds are cleared (binary search); the rest are ranked by a scan of per-word popcounts.
//                        Merge: a new key goes to its rank + its lower bound in the old table, an old entry to its index + the number of new
//                        keys whose lower bound is at or below it (a binary search over the lower bounds, which ascend).  The merged tail is
//                        built in scratch of the handle and copied back, so no thread overwrites an entry another still has to read.
// Pins (tests/kfplanes_model.py is the sequential model; contraction off): msl.h's list.
#include "msl_match_handle.h"
#include "msl_index_check.h"
#include "msl_match_math.h"
#include "msl_plane_tables.h"

namespace {

using namespace msl;

constexpr int OB_NT = 1024;                        // k_manhattan_observe: the binary searches are chains of dependent loads; 16 waves keep more in flight
const char *const WHO_KP = "msl_keyframe_planes", *const WHO_MO = "msl_manhattan_observe";

// ==== msl_keyframe_planes ====================================================================================================================
struct KfpDev {
    int pcap, mcap, kcap, mode;
    const msl_kfplanes_frame *frames;
    const float *coef; const int32_t *npts, *nPlanes; const float *Tcw; const uint8_t *outlier;
    int32_t *match; float *mpW; uint8_t *mpFlags; int32_t *mpFirst, *nMap; float *kfRwc, *kfCoef; int32_t *kfNpts;
    int32_t *kfMatch; uint8_t *planeNew, *obsAdd; int32_t *mergeInto; double *Twc; int32_t *nNew, *setNotErase, *status;
};

__global__ __launch_bounds__(64) void k_keyframe_planes(KfpDev D) {
    __shared__ int s_m[3][MAX_PCAP];
    __shared__ uint8_t s_o[MAX_PCAP];
    const size_t f = blockIdx.x;
    const int k = threadIdx.x;
    const msl_kfplanes_frame R = D.frames[f];
    const bool on = R.enable != 0 && R.kf_slot >= 0 && R.kf_slot < D.kcap, init = D.mode == MSL_KFPLANES_INIT;
    const int np = clampi(D.nPlanes[f], 0, D.pcap), nMap = clampi(D.nMap[f], 0, D.mcap);
    const size_t pk = f * D.pcap + k;
    const float *T = D.Tcw + 12 * f;
    int m[3] = {-1, -1, -1};
    bool o0 = false;
    if (k < np) {
        for (int s = 0; s < 3; s++) {
            const int v = D.match[3 * pk + s];
            m[s] = (v >= 0 && v < nMap) ? v : -1;
        }
        o0 = D.outlier[3 * pk] != 0;
    }
    for (int s = 0; s < 3; s++) s_m[s][k] = m[s];
    s_o[k] = o0 ? 1 : 0;
    __syncthreads();
    const bool held = !init && m[0] >= 0;
    const bool isNew = on && k < np && (init || (!held && !o0));                   // reaches :1637 (every plane of :594)
    const unsigned long long want = __ballot(isNew);
    const int row = nMap + __popcll(want & ((1ull << k) - 1ull));
    const bool made = isNew && row < D.mcap;
    const int nNew = __popcll(__ballot(made));
    if (k < np) {
        uint8_t add[3] = {0, 0, 0};
        int st = MSL_KFPLANES_SKIPPED, km0 = m[0];
        if (on) {
            if (made) { add[0] = 1; st = MSL_KFPLANES_NEW; km0 = row; }
            else if (isNew) st = MSL_KFPLANES_NO_ROOM;
            else if (held) {                                                       // AddObservation (:1629): the first k of the row
                st = MSL_KFPLANES_HELD;
                bool first = true;
                for (int q = 0; q < k; q++) first = first && s_m[0][q] != m[0];
                add[0] = first ? 1 : 0;
            }
            for (int s = 1; s < 3 && !init && !o0; s++) {                          // :1621-1626, against mvbPlaneOutlier[i]
                if (m[s] < 0) continue;
                bool first = true;
                for (int q = 0; q < k; q++) first = first && !(s_m[s][q] == m[s] && !s_o[q]);
                add[s] = first ? 1 : 0;
            }
        }
        D.kfMatch[3 * pk] = km0; D.kfMatch[3 * pk + 1] = m[1]; D.kfMatch[3 * pk + 2] = m[2];
        for (int s = 0; s < 3; s++) D.obsAdd[3 * pk + s] = add[s];
        D.planeNew[pk] = made ? 1 : 0;
        D.mergeInto[pk] = made ? row : -1;
        D.status[pk] = st;
        if (made) {
            const size_t mj = f * D.mcap + row;
            float pM[4];
            world_coef(T, D.coef + 4 * pk, pM);
            for (int c = 0; c < 4; c++) D.mpW[4 * mj + c] = pM[c];
            D.mpFlags[mj] = 1; D.mpFirst[mj] = R.kf_id;
            if (init) D.match[3 * pk] = row;                                       // :601
        }
    }
    if (on) {                                                                      // the KeyFrame's row: SetPose and the constructor's copies
        const size_t kr = f * D.kcap + R.kf_slot;
        if (k < 9) D.kfRwc[9 * kr + k] = T[4 * (k % 3) + k / 3];
        for (int q = k; q < D.pcap; q += 64) {
            for (int c = 0; c < 4; c++) D.kfCoef[4 * (kr * D.pcap + q) + c] = q < np ? D.coef[4 * (f * D.pcap + q) + c] : 0.0f;
            D.kfNpts[kr * D.pcap + q] = q < np ? D.npts[f * D.pcap + q] : 0;
        }
    }
    if (k == 0) {
        float Ow[3];
        camera_centre(T, Ow);
        double *W = D.Twc + 12 * f;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) W[4 * r + c] = (double)T[4 * c + r];
            W[4 * r + 3] = (double)Ow[r];
        }
        D.nNew[f] = nNew;
        D.setNotErase[f] = (!init && want != 0ull) ? 1 : 0;
        if (nNew > 0) D.nMap[f] = nMap + nNew;
    }
}

int check_kfplanes(int n_frames, int pcap, int mcap, int kcap, int mode, const msl_kfplanes_frame *frames, const float *plane_coef,
                   const int32_t *plane_npts, const int32_t *n_planes, const float *Tcw, const uint8_t *plane_outlier, msl_mem mem,
                   int32_t *plane_match, float *mp_w, uint8_t *mp_flags, int32_t *mp_first_kf, int32_t *n_map, float *kf_Rwc, float *kf_coef,
                   int32_t *kf_npts, int32_t *kf_plane_match, uint8_t *plane_new, uint8_t *obs_add, int32_t *merge_into, double *Twc,
                   int32_t *n_new, int32_t *set_not_erase, int32_t *status, msl_mem out_mem) {
    const char *who = WHO_KP;
    if (!none_null(who, {MSL_NAMED(frames), MSL_NAMED(plane_coef), MSL_NAMED(plane_npts), MSL_NAMED(n_planes), MSL_NAMED(Tcw),
                         MSL_NAMED(plane_outlier), MSL_NAMED(plane_match), MSL_NAMED(mp_w), MSL_NAMED(mp_flags), MSL_NAMED(mp_first_kf),
                         MSL_NAMED(n_map), MSL_NAMED(kf_Rwc), MSL_NAMED(kf_coef), MSL_NAMED(kf_npts), MSL_NAMED(kf_plane_match),
                         MSL_NAMED(plane_new), MSL_NAMED(obs_add), MSL_NAMED(merge_into), MSL_NAMED(Twc), MSL_NAMED(n_new),
                         MSL_NAMED(set_not_erase), MSL_NAMED(status)})) return MSL_ERR_INVALID;
    if (!in_range(who, "n_frames", n_frames, 1, MAX_PLANE_FRAMES) || !in_range(who, "pcap", pcap, 1, MAX_PCAP) ||
        !in_range(who, "mcap", mcap, 1, MAX_PLANE_MCAP) || !in_range(who, "kcap", kcap, 1, MAX_PLANE_KCAP)) return MSL_ERR_INVALID;
    if (mode < MSL_KFPLANES_KEYFRAME || mode > MSL_KFPLANES_INIT) { set_error("%s: mode %d is not an MSL_KFPLANES_* mode", who, mode); return MSL_ERR_INVALID; }
    char why[256];
    // plane_match and n_map are in/out: they live in out_mem memory
    if (mem == MSL_MEM_HOST && out_mem == MSL_MEM_HOST) {
        if (!check::counts_ok("n_planes", "pcap", n_frames, pcap, n_planes, why, sizeof(why)) ||
            !check::counts_ok("n_map", "mcap", n_frames, mcap, n_map, why, sizeof(why)) ||
            !check::plane_match_ok("plane_match", n_frames, pcap, 3, plane_match, n_planes, n_map, why, sizeof(why))) return refuse(who, why);
    }
    if (mem == MSL_MEM_HOST && !check::kf_slots_ok(n_frames, kcap, &frames->kf_slot, &frames->kf_id, 4, why, sizeof(why))) return refuse(who, why);
    return MSL_OK;
}

int launch_kfplanes(msl_match *h, int n_frames, int pcap, int mcap, int kcap, int mode, const msl_kfplanes_frame *frames, const float *plane_coef,
                    const int32_t *plane_npts, const int32_t *n_planes, const float *Tcw, const uint8_t *plane_outlier, msl_mem mem,
                    int32_t *plane_match, float *mp_w, uint8_t *mp_flags, int32_t *mp_first_kf, int32_t *n_map, float *kf_Rwc, float *kf_coef,
                    int32_t *kf_npts, int32_t *kf_plane_match, uint8_t *plane_new, uint8_t *obs_add, int32_t *merge_into, double *Twc,
                    int32_t *n_new, int32_t *set_not_erase, int32_t *status, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t F = (size_t)n_frames, p = F * pcap, m = F * mcap, kr = F * kcap;
    KfpDev D{};
    D.pcap = pcap; D.mcap = mcap; D.kcap = kcap; D.mode = mode;
    Stage S(h, mem, out_mem);
    D.frames = S.in(frames, F); D.coef = S.in(plane_coef, 4 * p); D.npts = S.in(plane_npts, p); D.nPlanes = S.in(n_planes, F);
    D.Tcw = S.in(Tcw, 12 * F); D.outlier = S.in(plane_outlier, 3 * p);
    D.match = S.inout(plane_match, 3 * p); D.mpW = S.inout(mp_w, 4 * m); D.mpFlags = S.inout(mp_flags, m); D.mpFirst = S.inout(mp_first_kf, m);
    D.nMap = S.inout(n_map, F); D.kfRwc = S.inout(kf_Rwc, 9 * kr); D.kfCoef = S.inout(kf_coef, 4 * kr * pcap); D.kfNpts = S.inout(kf_npts, kr * pcap);
    D.kfMatch = S.out(kf_plane_match, 3 * p); D.planeNew = S.out(plane_new, p); D.obsAdd = S.out(obs_add, 3 * p);
    D.mergeInto = S.out(merge_into, p); D.Twc = S.out(Twc, 12 * F); D.nNew = S.out(n_new, F); D.setNotErase = S.out(set_not_erase, F);
    D.status = S.out(status, p);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_keyframe_planes, dim3((unsigned)n_frames), dim3(64), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

// ==== msl_manhattan_observe ==================================================================================================================
struct ObsDev {
    int pcap, mcap, fcap, qcap, kcap;
    float th;
    const msl_kfplanes_frame *frames;
    const int32_t *kfMatch; const float *coef; const int32_t *nPlanes; const uint8_t *mpFlags; const int32_t *mpFirst, *nMap;
    int32_t *fullTab, *nFull, *partTab, *nPart, *addedFull, *addedPart, *setNotErase; uint8_t *recent; int32_t *status;
    int32_t *scratch;                               // per frame: [fcap] merged triples, [fcap] lower bounds, [qcap] merged pairs, [qcap]
};

// What a workgroup knows of its keyframe: per dense id the row and the first frame plane that holds it
struct ObsRows {
    int row[MAX_PCAP], first[MAX_PCAP];
};

// Bit `bit` of a key map as dense ids, ascending
template <int W>
__device__ __forceinline__ void ids_of(int bit, int *id) {
    if constexpr (W == 3) { id[0] = bit >> 12; id[1] = (bit >> 6) & 63; id[2] = bit & 63; }
    else { id[0] = bit >> 6; id[1] = bit & 63; }
}

// The keys of `bits` (nWords words; cnt: one count per word) that `tab` (nOld sorted entries of cap) does not hold, merged into it.
// Returns the number added, or 0 with *noRoom when the table cannot take them all (the table is left as it was).  Every thread of the
// workgroup calls it.  Thread t takes the words t, t + 1024, ...: the keys are dense where the first id is small, and a thread with a run of
// consecutive words there would hold several times the average.  The rank of a key is the scan of the per-word counts plus its place in
// its word.
template <int W>
__device__ int merge_keys(unsigned *bits, uint16_t *cnt, int nWords, int32_t *tab, int nOld, int cap, int32_t *scrTab, int32_t *scrLb, int kfSlot,
                          const ObsRows &S, unsigned *s_wave, bool *noRoom) {
    constexpr int ST = mf::stride(W);
    const int t = threadIdx.x;
    for (int w = t; w < nWords; w += OB_NT) {                                      // drop the keys the table holds
        unsigned word = bits[w];
        for (unsigned left = word; left; left &= left - 1) {
            const int b = __ffs(left) - 1;
            int id[W], key[W];
            ids_of<W>(32 * w + b, id);
            for (int q = 0; q < W; q++) key[q] = S.row[id[q]];
            bool found;
            lower_bound_key<W>(tab, nOld, key, &found);
            if (found) word &= ~(1u << b);
        }
        bits[w] = word;
        cnt[w] = (uint16_t)__popc(word);
    }
    __syncthreads();
    block_scan_array_incl(cnt, nWords, s_wave);                                    // at most C(64, 3) = 41 664 keys: the sums fit 16 bits
    const unsigned total = cnt[nWords - 1];
    *noRoom = (long long)nOld + (long long)total > (long long)cap;
    if (*noRoom || total == 0) return 0;                                           // uniform
    for (int w = t; w < nWords; w += OB_NT) {
        unsigned r = cnt[w] - (unsigned)__popc(bits[w]);
        for (unsigned left = bits[w]; left; left &= left - 1, r++) {
            int id[W], key[W];
            ids_of<W>(32 * w + __ffs(left) - 1, id);
            for (int q = 0; q < W; q++) key[q] = S.row[id[q]];
            bool found;
            const int lb = lower_bound_key<W>(tab, nOld, key, &found);
            scrLb[r] = lb;
            int32_t *e = scrTab + (size_t)(r + lb) * ST;
            for (int q = 0; q < W; q++) { e[q] = key[q]; e[mf::index_at(W, q)] = S.first[id[q]]; }
            e[mf::kf_at(W)] = kfSlot;
        }
    }
    __threadfence_block();
    __syncthreads();
    const int from = scrLb[0];                                                     // entries below the first new key stay where they are
    for (int e = from + t; e < nOld; e += OB_NT) {
        int lo = 0, hi = (int)total;                                               // the number of new keys with a lower bound <= e
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (scrLb[mid] <= e) lo = mid + 1; else hi = mid;
        }
        for (int q = 0; q < ST; q++) scrTab[(size_t)(e + lo) * ST + q] = tab[(size_t)e * ST + q];
    }
    __threadfence_block();
    __syncthreads();
    for (size_t i = (size_t)from * ST + t; i < (size_t)(nOld + (int)total) * ST; i += OB_NT) tab[i] = scrTab[i];
    __syncthreads();
    return (int)total;
}

__global__ __launch_bounds__(OB_NT) void k_manhattan_observe(ObsDev D) {
    __shared__ unsigned s_tri[MAX_PCAP * MAX_PCAP * MAX_PCAP / 32];
    __shared__ unsigned s_pair[MAX_PCAP * MAX_PCAP / 32];
    __shared__ uint16_t s_cnt[MAX_PCAP * MAX_PCAP * MAX_PCAP / 32];
    __shared__ unsigned long long s_ok[MAX_PCAP];
    __shared__ int s_h[MAX_PCAP], s_id[MAX_PCAP];
    __shared__ uint8_t s_isFirst[MAX_PCAP];
    __shared__ float s_coef[MAX_PCAP][3];
    __shared__ ObsRows S;
    __shared__ unsigned s_wave[17];
    const size_t f = blockIdx.x;
    const int t = threadIdx.x;
    const msl_kfplanes_frame R = D.frames[f];
    const bool on = R.enable != 0 && R.kf_slot >= 0 && R.kf_slot < D.kcap;
    const int np = clampi(D.nPlanes[f], 0, D.pcap), nMap = clampi(D.nMap[f], 0, D.mcap);
    for (int w = t; w < MAX_PCAP * MAX_PCAP * MAX_PCAP / 32; w += OB_NT) s_tri[w] = 0;
    if (t < MAX_PCAP * MAX_PCAP / 32) s_pair[t] = 0;
    if (t < MAX_PCAP) {
        // mvpMapPlanes[t] when not NULL and not bad, of an enabled frame: held_row() and, below, sort3() of msl_plane_tables.h written out,
        // because either call moves this kernel's instruction text (2004 -> 2006 and a reordering) and its rate was not measured again
        int hld = -1;
        if (t < np) {
            const int m = D.kfMatch[3 * (f * D.pcap + t)];
            if (on && m >= 0 && m < nMap && (D.mpFlags[f * D.mcap + m] & 1)) hld = m;
            D.recent[f * D.pcap + t] = (hld >= 0 && D.mpFirst[f * D.mcap + hld] == R.kf_id) ? 1 : 0;       // :167-169
            for (int c = 0; c < 3; c++) s_coef[t][c] = D.coef[4 * (f * D.pcap + t) + c];
        }
        s_h[t] = hld;
    }
    __syncthreads();
    if (t < MAX_PCAP) {
        bool first = s_h[t] >= 0;
        for (int q = 0; q < t; q++) first = first && s_h[q] != s_h[t];
        s_isFirst[t] = first ? 1 : 0;
        unsigned long long ok = 0ull;
        if (s_h[t] >= 0)
            for (int j = 0; j < np; j++) {
                if (s_h[j] < 0) continue;
                const float *a = s_coef[t < j ? t : j], *b = s_coef[t < j ? j : t];
                const float angle = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
                if (angle < D.th && angle > -D.th) ok |= 1ull << j;               // :192, :209
            }
        s_ok[t] = ok;
    }
    __syncthreads();
    if (t < MAX_PCAP && s_h[t] >= 0) {                                             // the dense id: the distinct held rows below this one
        int id = 0;
        for (int q = 0; q < np; q++) id += (s_isFirst[q] && s_h[q] < s_h[t]) ? 1 : 0;
        s_id[t] = id;
        if (s_isFirst[t]) { S.row[id] = s_h[t]; S.first[id] = t; }
    }
    __syncthreads();
    for (int q = t; q < np * np; q += OB_NT) {
        const int i = q / np, j = q - i * np;
        if (i >= j || s_h[i] < 0 || s_h[j] < 0 || s_h[i] == s_h[j] || !(s_ok[i] >> j & 1ull)) continue;
        const int a = s_id[i], b = s_id[j];
        for (int k = j + 1; k < np; k++) {
            if (s_h[k] < 0 || s_h[k] == s_h[i] || s_h[k] == s_h[j] || !(s_ok[i] >> k & 1ull) || !(s_ok[j] >> k & 1ull)) continue;
            int x = a, y = b, z = s_id[k];
            if (x > y) { const int u = x; x = y; y = u; }
            if (y > z) { const int u = y; y = z; z = u; }
            if (x > y) { const int u = x; x = y; y = u; }
            const int bit = x << 12 | y << 6 | z;
            atomicOr(&s_tri[bit >> 5], 1u << (bit & 31));
        }
        const int bit = min(a, b) << 6 | max(a, b);
        atomicOr(&s_pair[bit >> 5], 1u << (bit & 31));
    }
    __syncthreads();
    constexpr int FW = mf::FULL, PW = mf::PART;
    int32_t *scr = D.scratch + f * ((size_t)D.fcap * mf::scratch_ints(FW) + (size_t)D.qcap * mf::scratch_ints(PW));
    bool fullNoRoom, partNoRoom;
    const int nFull = clampi(D.nFull[f], 0, D.fcap), nPart = clampi(D.nPart[f], 0, D.qcap);
    const int addedFull = merge_keys<FW>(s_tri, s_cnt, MAX_PCAP * MAX_PCAP * MAX_PCAP / 32, D.fullTab + f * D.fcap * mf::stride(FW), nFull, D.fcap,
                                         scr, scr + (size_t)D.fcap * mf::stride(FW), R.kf_slot, S, s_wave, &fullNoRoom);
    scr += (size_t)D.fcap * mf::scratch_ints(FW);
    const int addedPart = merge_keys<PW>(s_pair, s_cnt, MAX_PCAP * MAX_PCAP / 32, D.partTab + f * D.qcap * mf::stride(PW), nPart, D.qcap, scr,
                                         scr + (size_t)D.qcap * mf::stride(PW), R.kf_slot, S, s_wave, &partNoRoom);
    if (t == 0) {
        D.addedFull[f] = addedFull; D.addedPart[f] = addedPart;
        D.setNotErase[f] = addedFull + addedPart > 0 ? 1 : 0;
        D.status[f] = (fullNoRoom ? MSL_MANHATTAN_FULL_NO_ROOM : 0) | (partNoRoom ? MSL_MANHATTAN_PART_NO_ROOM : 0);
        if (addedFull > 0) D.nFull[f] = nFull + addedFull;
        if (addedPart > 0) D.nPart[f] = nPart + addedPart;
    }
}

int check_observe(int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params, const msl_kfplanes_frame *frames,
                  const int32_t *kf_plane_match, const float *plane_coef, const int32_t *n_planes, const uint8_t *mp_flags,
                  const int32_t *mp_first_kf, const int32_t *n_map, msl_mem mem, int32_t *full_tab, int32_t *n_full, int32_t *part_tab,
                  int32_t *n_part, int32_t *added_full, int32_t *added_part, int32_t *set_not_erase, uint8_t *recent_plane, int32_t *status,
                  msl_mem out_mem) {
    const char *who = WHO_MO;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(frames), MSL_NAMED(kf_plane_match), MSL_NAMED(plane_coef), MSL_NAMED(n_planes),
                         MSL_NAMED(mp_flags), MSL_NAMED(mp_first_kf), MSL_NAMED(n_map), MSL_NAMED(full_tab), MSL_NAMED(n_full), MSL_NAMED(part_tab),
                         MSL_NAMED(n_part), MSL_NAMED(added_full), MSL_NAMED(added_part), MSL_NAMED(set_not_erase), MSL_NAMED(recent_plane),
                         MSL_NAMED(status)})) return MSL_ERR_INVALID;
    if (!in_range(who, "n_frames", n_frames, 1, MAX_PLANE_FRAMES) || !in_range(who, "pcap", pcap, 1, MAX_PCAP) ||
        !in_range(who, "mcap", mcap, 1, MAX_PLANE_MCAP) || !in_range(who, "fcap", fcap, 1, MAX_FCAP) ||
        !in_range(who, "qcap", qcap, 1, MAX_QCAP) || !in_range(who, "kcap", kcap, 1, MAX_PLANE_KCAP)) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST) {
        if (!check::counts_ok("n_planes", "pcap", n_frames, pcap, n_planes, why, sizeof(why)) ||
            !check::counts_ok("n_map", "mcap", n_frames, mcap, n_map, why, sizeof(why)) ||
            !check::plane_match_ok("kf_plane_match", n_frames, pcap, 1, kf_plane_match, n_planes, n_map, why, sizeof(why)) ||
            !check::kf_slots_ok(n_frames, kcap, &frames->kf_slot, &frames->kf_id, 4, why, sizeof(why))) return refuse(who, why);
    }
    if (out_mem == MSL_MEM_HOST) {
        if (!check::counts_ok("n_full", "fcap", n_frames, fcap, n_full, why, sizeof(why)) ||
            !check::counts_ok("n_part", "qcap", n_frames, qcap, n_part, why, sizeof(why)) ||
            !check::tables_sorted_ok("full_tab", n_frames, fcap, mf::stride(mf::FULL), mf::FULL, full_tab, n_full, why, sizeof(why)) ||
            !check::tables_sorted_ok("part_tab", n_frames, qcap, mf::stride(mf::PART), mf::PART, part_tab, n_part, why, sizeof(why)))
            return refuse(who, why);
    }
    return MSL_OK;
}

int launch_observe(msl_match *h, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params,
                   const msl_kfplanes_frame *frames, const int32_t *kf_plane_match, const float *plane_coef, const int32_t *n_planes,
                   const uint8_t *mp_flags, const int32_t *mp_first_kf, const int32_t *n_map, msl_mem mem, int32_t *full_tab, int32_t *n_full,
                   int32_t *part_tab, int32_t *n_part, int32_t *added_full, int32_t *added_part, int32_t *set_not_erase, uint8_t *recent_plane,
                   int32_t *status, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t F = (size_t)n_frames, p = F * pcap, m = F * mcap;
    ObsDev D{};
    D.pcap = pcap; D.mcap = mcap; D.fcap = fcap; D.qcap = qcap; D.kcap = kcap; D.th = params->mf_ver_th;
    Stage S(h, mem, out_mem);
    D.frames = S.in(frames, F); D.kfMatch = S.in(kf_plane_match, 3 * p); D.coef = S.in(plane_coef, 4 * p); D.nPlanes = S.in(n_planes, F);
    D.mpFlags = S.in(mp_flags, m); D.mpFirst = S.in(mp_first_kf, m); D.nMap = S.in(n_map, F);
    D.fullTab = S.inout(full_tab, mf::stride(mf::FULL) * F * fcap); D.nFull = S.inout(n_full, F);
    D.partTab = S.inout(part_tab, mf::stride(mf::PART) * F * qcap); D.nPart = S.inout(n_part, F);
    D.addedFull = S.out(added_full, F); D.addedPart = S.out(added_part, F); D.setNotErase = S.out(set_not_erase, F);
    D.recent = S.out(recent_plane, p); D.status = S.out(status, F);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(h->kfpScratch.grow(sizeof(int32_t) * F * ((size_t)fcap * mf::scratch_ints(mf::FULL) + (size_t)qcap * mf::scratch_ints(mf::PART)), h->stream));
    D.scratch = (int32_t *)h->kfpScratch.p;
    hipLaunchKernelGGL(k_manhattan_observe, dim3((unsigned)n_frames), dim3(OB_NT), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_keyframe_planes(msl_match *h, int n_frames, int pcap, int mcap, int kcap, int mode, const msl_kfplanes_frame *frames,
                        const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const float *Tcw,
                        const uint8_t *plane_outlier, msl_mem mem, int32_t *plane_match, float *mp_w, uint8_t *mp_flags, int32_t *mp_first_kf,
                        int32_t *n_map, float *kf_Rwc, float *kf_coef, int32_t *kf_npts, int32_t *kf_plane_match, uint8_t *plane_new,
                        uint8_t *obs_add, int32_t *merge_into, double *Twc, int32_t *n_new, int32_t *set_not_erase, int32_t *status,
                        msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_KP, check_kfplanes, launch_kfplanes, h, n_frames, pcap, mcap, kcap, mode, frames, plane_coef, plane_npts, n_planes, Tcw,
                       plane_outlier, mem, plane_match, mp_w, mp_flags, mp_first_kf, n_map, kf_Rwc, kf_coef, kf_npts, kf_plane_match, plane_new,
                       obs_add, merge_into, Twc, n_new, set_not_erase, status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_keyframe_planes_batch(int device, int n_frames, int pcap, int mcap, int kcap, int mode, const msl_kfplanes_frame *frames,
                              const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const float *Tcw,
                              const uint8_t *plane_outlier, msl_mem mem, int32_t *plane_match, float *mp_w, uint8_t *mp_flags,
                              int32_t *mp_first_kf, int32_t *n_map, float *kf_Rwc, float *kf_coef, int32_t *kf_npts, int32_t *kf_plane_match,
                              uint8_t *plane_new, uint8_t *obs_add, int32_t *merge_into, double *Twc, int32_t *n_new, int32_t *set_not_erase,
                              int32_t *status, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_kfplanes, launch_kfplanes, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, pcap, mcap, kcap, mode,
                      frames, plane_coef, plane_npts, n_planes, Tcw, plane_outlier, mem, plane_match, mp_w, mp_flags, mp_first_kf, n_map, kf_Rwc,
                      kf_coef, kf_npts, kf_plane_match, plane_new, obs_add, merge_into, Twc, n_new, set_not_erase, status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_manhattan_observe(msl_match *h, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params,
                          const msl_kfplanes_frame *frames, const int32_t *kf_plane_match, const float *plane_coef, const int32_t *n_planes,
                          const uint8_t *mp_flags, const int32_t *mp_first_kf, const int32_t *n_map, msl_mem mem, int32_t *full_tab,
                          int32_t *n_full, int32_t *part_tab, int32_t *n_part, int32_t *added_full, int32_t *added_part, int32_t *set_not_erase,
                          uint8_t *recent_plane, int32_t *status, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_MO, check_observe, launch_observe, h, n_frames, pcap, mcap, fcap, qcap, kcap, params, frames, kf_plane_match, plane_coef,
                       n_planes, mp_flags, mp_first_kf, n_map, mem, full_tab, n_full, part_tab, n_part, added_full, added_part, set_not_erase,
                       recent_plane, status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_manhattan_observe_batch(int device, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params,
                                const msl_kfplanes_frame *frames, const int32_t *kf_plane_match, const float *plane_coef,
                                const int32_t *n_planes, const uint8_t *mp_flags, const int32_t *mp_first_kf, const int32_t *n_map, msl_mem mem,
                                int32_t *full_tab, int32_t *n_full, int32_t *part_tab, int32_t *n_part, int32_t *added_full, int32_t *added_part,
                                int32_t *set_not_erase, uint8_t *recent_plane, int32_t *status, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_observe, launch_observe, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, pcap, mcap, fcap, qcap,
                      kcap, params, frames, kf_plane_match, plane_coef, n_planes, mp_flags, mp_first_kf, n_map, mem, full_tab, n_full, part_tab,
                      n_part, added_full, added_part, set_not_erase, recent_plane, status, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
