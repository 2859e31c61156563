// msl_sf_map_dev.h -- what the four translation units of the surfel map stage for gfx950 (MI355X) share (internal, device side):
//   msl_sf_fuse.hip      k_fuse: fuseSurfelsKernel (reference src/SurfelFusion.cpp:167-283); in a deferred window also the new surfels of the keyframe before
//   msl_sf_compact.hip   k_compact: initializeSurfels (:285-331) and the slot refill / tail compaction of SurfelMapping::fuseMap
//                        (src/SurfelMapping.cpp:366-391); the dealing of k_fuse's sub-blocks by screen position (k_deal)
//   msl_sf_replay.hip    the end of a deferred window: k_defer_tail, k_replay, k_gather, k_scatter
//   msl_sf_map.hip       map maintenance: ordered selection, AoS <-> SoA conversion, counters, change collection
// all on a device-resident map of 16-byte hot + 32-byte cold records.  Here: the record accessors, what k_fuse takes by value, and the spawn
// helpers that k_fuse and k_defer_tail both use.
//
// Two ways through a keyframe (msl_surfel.hip decides):
//   classic  : k_fuse<false> -> k_compact           two dependent launches per keyframe; the array is in the reference's order after
//                                                   every keyframe (single keyframes, the host-vector drop-in, the first keyframe after
//                                                   the map was replaced from outside)
//   deferred : k_fuse<true> x F -> k_defer_tail -> k_replay -> k_gather -> k_scatter      (round 5) ONE launch per keyframe.
//              fuseSurfelsKernel treats every surfel independently of its array position, so inside a window of F <= 32 keyframes nothing
//              is moved: a keyframe's new surfels are appended physically behind the array (by the "spawn wave" of the NEXT keyframe's fuse
//              launch, which fuses them right away), deleted slots stay as holes and are logged.  The window's placements and tail moves
//              (new surfel k -> k-th largest hole else appended; back-to-front refill, SurfelMapping.cpp:372-390) are then replayed
//              SYMBOLICALLY by one wave over the logs -- virtual position <-> element, only for the few positions that differ from the
//              identity -- and applied as one gather + scatter, which leaves the array exactly as F classic keyframes would have.
//
// HBM-bound integer/float streaming; no MFMA.  Every float expression keeps the reference's evaluation order and float/double
// promotions; compiled with -ffp-contract=off.
#pragma once

#include "msl_sf.h"

#ifdef __HIPCC__

using namespace msl;
using namespace msl::sf;

// Everything stays in an unnamed namespace, where it was while the stage was one file: a kernel's symbol carries the names of its parameter
// types (FuseArgs, FuseFrame), and with the same symbols every kernel's instruction stream stays what it was (profiles/README.md).
namespace {

// ---- record accessors ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ld_agent(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_agent64(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent64(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ void set_wide_flag_ptr(long long *flag, unsigned long long bit) { atomicOr(reinterpret_cast<unsigned long long *>(flag), bit); }
__device__ __forceinline__ void set_wide_flag(const MapSoA &M, unsigned long long bit) { set_wide_flag_ptr(M.wideFlag, bit); }
// updateTimes / lastUpdate of a record whose packed word is tl (the side array only for HOT_WIDE: rare)
__device__ __forceinline__ void tl_unpack(const MapSoA &M, long long i, unsigned tl, int &ut, int &lu) {
    ut = tl_ut(tl); lu = tl_lu(tl);
    if (tl & 0x80000000u) {
        if (tl == HOT_WIDE) { ut = M.utlWide[2 * i]; lu = M.utlWide[2 * i + 1]; }
        else { ut = 0; lu = 0; }   // HOT_HOLE
    }
}
__device__ __forceinline__ HotRec hot_load(const MapSoA &M, long long i) {
    const HotPk p = M.hot[i];
    HotRec h; h.px = p.px; h.py = p.py; h.pz = p.pz;
    tl_unpack(M, i, p.tl, h.updateTimes, h.lastUpdate);
    return h;
}
__device__ __forceinline__ unsigned tl_store_word(const MapSoA &M, long long i, int ut, int lu) {   // the packed word; writes the side array when it does not fit
    if (tl_fits(ut, lu)) return tl_pack(ut, lu);
    M.utlWide[2 * i] = ut; M.utlWide[2 * i + 1] = lu;
    set_wide_flag(M, 2ull);
    return HOT_WIDE;
}
__device__ __forceinline__ void hot_store(const MapSoA &M, long long i, const HotRec &h) {
    HotPk p; p.px = h.px; p.py = h.py; p.pz = h.pz; p.tl = tl_store_word(M, i, h.updateTimes, h.lastUpdate);
    M.hot[i] = p;
}
// updateTimes = 0 (:201, :229): lastUpdate stays what it was (the host-vector drop-in hands the record back)
__device__ __forceinline__ void hot_mark_deleted(const MapSoA &M, long long i, unsigned tl) {
    if (tl == HOT_WIDE) M.utlWide[2 * i] = 0;
    else M.hot[i].tl = tl & 0xFFFFFu;
}
__device__ __forceinline__ bool hot_is_deleted(const MapSoA &M, long long i) {
    const unsigned tl = M.hot[i].tl;
    return tl == HOT_WIDE ? M.utlWide[2 * i] == 0 : (tl == HOT_HOLE || (tl >> 20) == 0);
}

// Cold records travel as two 16-byte words: a plain struct copy of the 32-byte-aligned ColdRec goes through a private
// temporary that the compiler parks in LDS (12 KB per workgroup in k_compact before this).
struct ColdBits { uint4 a, b; };
__device__ __forceinline__ ColdRec cold_load(const ColdRec *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    ColdBits v; v.a = q[0]; v.b = q[1];
    ColdRec c;
    c.nx = __uint_as_float(v.a.x); c.ny = __uint_as_float(v.a.y); c.nz = __uint_as_float(v.a.z); c.size = __uint_as_float(v.a.w);
    c.color = __uint_as_float(v.b.x); c.weight = __uint_as_float(v.b.y); c.rgbf = v.b.z; c._spare = v.b.w;
    return c;
}
__device__ __forceinline__ void cold_store(ColdRec *p, const ColdRec &c) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(__float_as_uint(c.nx), __float_as_uint(c.ny), __float_as_uint(c.nz), __float_as_uint(c.size));
    q[1] = make_uint4(__float_as_uint(c.color), __float_as_uint(c.weight), c.rgbf, c._spare);
}

__device__ __forceinline__ void store_surfel(const MapSoA &M, long long i, const msl_surfel &e) {
    HotRec h; h.px = e.px; h.py = e.py; h.pz = e.pz; h.updateTimes = e.updateTimes; h.lastUpdate = e.lastUpdate;
    ColdRec c; c.nx = e.nx; c.ny = e.ny; c.nz = e.nz; c.size = e.size; c.color = e.color; c.weight = e.weight; c._spare = 0;
    if (rgb_fits(e.r, e.g, e.b)) c.rgbf = rgb_pack(e.r, e.g, e.b);
    else { c.rgbf = COLD_WIDE; set_wide_flag(M, 1ull); M.rgbWide[3 * i] = e.r; M.rgbWide[3 * i + 1] = e.g; M.rgbWide[3 * i + 2] = e.b; }
    hot_store(M, i, h); cold_store(M.cold + i, c);
}
__device__ __forceinline__ void load_surfel(const MapSoA &M, long long i, const HotRec &h, msl_surfel &e) {
    const ColdRec c = cold_load(M.cold + i);
    e.px = h.px; e.py = h.py; e.pz = h.pz; e.nx = c.nx; e.ny = c.ny; e.nz = c.nz; e.size = c.size; e.color = c.color;
    if (c.rgbf & COLD_WIDE) { e.r = M.rgbWide[3 * i]; e.g = M.rgbWide[3 * i + 1]; e.b = M.rgbWide[3 * i + 2]; }
    else { e.r = (int)(c.rgbf & 255u); e.g = (int)((c.rgbf >> 8) & 255u); e.b = (int)((c.rgbf >> 16) & 255u); }
    e.weight = c.weight; e.updateTimes = h.updateTimes; e.lastUpdate = h.lastUpdate;
}
__device__ __forceinline__ void move_surfel(const MapSoA &M, long long dst, long long src) {
    const ColdRec c = cold_load(M.cold + src);
    const HotPk p = M.hot[src];
    M.hot[dst] = p; cold_store(M.cold + dst, c);
    if (p.tl == HOT_WIDE) { M.utlWide[2 * dst] = M.utlWide[2 * src]; M.utlWide[2 * dst + 1] = M.utlWide[2 * src + 1]; }
    if (c.rgbf & COLD_WIDE) { M.rgbWide[3 * dst] = M.rgbWide[3 * src]; M.rgbWide[3 * dst + 1] = M.rgbWide[3 * src + 1]; M.rgbWide[3 * dst + 2] = M.rgbWide[3 * src + 2]; }
}

// "Last workgroup continues" hand-off (cdna_hip_programming.md G16): every workgroup publishes its global stores with an
// agent-scope release, then takes a ticket; the one that draws the last ticket acquires and carries on with the next
// stage inside the same launch, saving a dependent kernel boundary (~5 us each on this latency-critical chain).
__device__ __forceinline__ bool last_workgroup(unsigned *ticket, unsigned *s_flag) {
    // Everything the continuing workgroup reads from this launch is stored write-through (agent-scope atomic stores /
    // RMW atomics) and read back with agent-scope loads, so no L2 write-back fence is needed.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = atomicAdd(ticket, 1u);
        *s_flag = (t == gridDim.x - 1) ? 1u : 0u;
        if (*s_flag) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // reset for the next launch
    }
    __syncthreads();
    return *s_flag != 0;
}

// int(projectU + 0.5) of :204-205 (a double addition, truncation towards zero) without double arithmetic: for u >= 1/2 it equals
// floor(u) + (u - floor(u) >= 1/2) -- floor and the difference are exact in float --, and for smaller u (or NaN) both expressions are
// <= 0, which the image test (pUInt < 1) rejects whatever the exact value is; the clamp keeps the conversion defined for huge / infinite u.
__device__ __forceinline__ int round_half_up_pixel(float u) {
    const float c = fminf(fmaxf(u, -4.0f), 1.0e6f);   // NaN -> -4
    const float f = floorf(c);
    return (int)f + ((c - f) >= 0.5f ? 1 : 0);
}
__device__ __forceinline__ unsigned lane_rank(unsigned long long m) {   // number of set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// 16-byte stores of the records phase B rewrites: plain stores (the lines stay dirty in the XCD's L2 until the kernel ends).  Measured and dropped in
// round 5 (A/B on one box): sc1 = write-through (+2.5 us per launch), nt (+0.3 us).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st16(void *p, u32x4 v) { *reinterpret_cast<u32x4 *>(p) = v; }

// What k_fuse reads of the handle and of the keyframe: slim copies of SfDev / FrameDev with the slot offsets folded in on the host.  The
// whole structs are ~150 dwords of kernel arguments = scalar registers the compiler loads up front and then spills around the hot loop;
// what only the spawn wave of a deferred launch needs (the previous keyframe's candidate arrays) and the side arrays of wide records stay in
// memory (DeferCtl).
struct FuseFrame {
    float inv[12];   // rows 0..2 of pose.inverse(), inv[3 c + r] = invPose[4 c + r] (the fourth row is never used)
    int ref;
    const FrameDev *frame;   // the keyframe's device record: the pose itself (only the update path of phase B rotates a normal back into the world)
};
struct FuseArgs {
    int W, H, nseeds, kf;          // kf: keyframe number inside a deferred window (its launch materialises the new surfels of kf - 1 first)
    int prevSlot;                  // superpixel slot of keyframe kf - 1, counted from the first slot of the handle (DeferCtl holds the array bases)
    int rowScale;                  // (254 << 16) / H: image row -> screen key 0 .. 253 of the dealing (SfDev::sbKeys)
    float fx, fy, cx, cy, fuseFar, fuseNear;
    const uint2 *tex; const float4 *fuseRec; uint8_t *fused;   // this keyframe's slot
    HotPk *hot; ColdRec *cold;
    long long *ctr;
    unsigned *blockSums, *blockUpd;   // per-sub-block deleted (classic) / updated counts (deferred: the keyframe's slice)
    unsigned *sbKeys;              // per-sub-block screen key this launch leaves for the next dealing
    const unsigned *deal;          // wave -> sub-block table of THIS launch (XCD-major: [w & 7][w >> 3]); nullptr: array order in runs of FUSE_CHUNK per XCD
    unsigned *delOut;              // where deleted slots go: classic delU[LIST_D] (k_compact's hand-over list), deferred the window's deletion log
    unsigned *delCount;            // ... and their count: classic delUCount, deferred DeferCtl::delCnt[kf]
    DeferCtl *dc;                  // extents and deletion counts of a deferred window; and what only a few waves per launch need (DeferCtl::aux):
                                   // side arrays of wide records, deletion lists, capacity -- loaded where they are used instead of living in scalar
                                   // registers through the whole kernel
};
__host__ inline FuseArgs fuse_args(const SfDev &P, int slot, bool deferred, unsigned blkStride, bool dealt = false) {   // blkStride: entries per blockUpd slice
    FuseArgs A;
    A.W = P.W; A.H = P.H; A.nseeds = P.nseeds; A.kf = P.kf; A.prevSlot = P.prevSlotAbs; A.rowScale = (254 << 16) / P.H;
    A.sbKeys = P.sbKeys; A.deal = dealt ? P.deal : nullptr;
    A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy; A.fuseFar = P.fuseFar; A.fuseNear = P.fuseNear;
    A.tex = P.tex + (size_t)slot * P.pxStride; A.fuseRec = P.fuseRec + (size_t)slot * P.nseeds * 3; A.fused = P.fused + (size_t)slot * P.flagStride;
    A.hot = P.map.hot; A.cold = P.map.cold; A.ctr = P.ctr;
    A.dc = P.dc;
    A.blockSums = P.blockSums; A.blockUpd = P.blockUpd + (size_t)(deferred ? P.kf : 0) * blkStride;
    A.delOut = deferred ? P.delList : P.delU;
    A.delCount = deferred ? &P.dc->delCnt[P.kf < DEFER_WIN ? P.kf : 0] : P.delUCount;
    return A;
}
__host__ inline FuseFrame fuse_frame(const FrameDev &F, const FrameDev *dev) {
    FuseFrame f;
    for (int c = 0; c < 4; c++) for (int r = 0; r < 3; r++) f.inv[3 * c + r] = F.invPose[4 * c + r];
    f.ref = F.ref; f.frame = dev;
    return f;
}

// ---- new surfels of the previous keyframe, materialised by the fuse launch that follows it (deferred compaction) ----------------------
// initializeSurfels (:285-331): every seed whose candidate is valid and that no fusion consumed spawns a surfel, in seed order.  New surfel
// k of the keyframe before (slot P.prevSlot) goes to the physical slot E0 + k (E0 = the extent that keyframe's fuse launch worked on).  The
// spawn wave of the next launch (workgroup 0; k_defer_tail for a window's last keyframe) scans the `fused` bytes of the whole lattice (lane l
// owns the `per` consecutive seeds from l * per on).  A seed spawns iff its byte is 0: kb_seed_init clears it, kb_seed_plane sets 2 where the
// candidate is invalid (candOk = 0), a fusion sets 1; the padding behind the lattice holds 1.  It publishes the new extent, writes the records
// 128 at a time and fuses them like any others.  All 64 lanes must call these.
__device__ __forceinline__ unsigned spawn_word(unsigned fw) { return ~(fw | (fw >> 1)) & 0x01010101u; }   // one bit per byte that is 0
// Pass 1: this lane's number of spawning seeds; the wave-wide exclusive prefix and the total K come from one scan.
__device__ __forceinline__ unsigned spawn_count(const FuseArgs &P, unsigned lane, unsigned &excl) {
    const DeferCtl *dc = P.dc;
    const int fs = dc->flagStride;
    const uint8_t *fusedP = dc->fused + (size_t)P.prevSlot * fs;   // of keyframe kf - 1
    const int per = fs >> 6, nch = per >> 4;   // seeds per lane (a multiple of 16), 16-byte words per lane
    unsigned cnt = 0;
    const uint4 *fq = reinterpret_cast<const uint4 *>(fusedP + (size_t)lane * per);
    for (int c = 0; c < nch; c += 5) {   // five words per trip (640 x 480: the whole lattice in ONE round trip, beside the wave's hot records)
        uint4 b[5];
#pragma unroll
        for (int q = 0; q < 5; q++) b[q] = fq[min(c + q, nch - 1)];
#pragma unroll
        for (int q = 0; q < 5; q++)
            if (c + q < nch) cnt += (unsigned)(__popc(spawn_word(b[q].x)) + __popc(spawn_word(b[q].y)) + __popc(spawn_word(b[q].z)) + __popc(spawn_word(b[q].w)));
    }
    const unsigned incl = wave_incl_scan(cnt);
    excl = incl - cnt;
    return (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
}
// Pass 2 (only when the keyframe spawned something that lands in this sub-block): slot i of the sub-block takes new surfel k = i - E0; its seed is
// the (k - excl[owner])-th spawning seed of the lane whose range contains it.
__device__ __forceinline__ void emit_records(const FuseArgs &P, long long E0, long long c0, int nj, unsigned lane, unsigned K, unsigned excl) {
    const DeferCtl *dc = P.dc;
    const int fs = dc->flagStride;
    const uint8_t *fusedP = dc->fused + (size_t)P.prevSlot * fs;
    const int per = fs >> 6, nch = per >> 4;
    const msl_surfel *cand = dc->cand + (size_t)P.prevSlot * P.nseeds;
#pragma unroll 1
    for (int j = 0; j < nj; j++) {
        const long long i = c0 + 64 * j + lane, kS = i - E0;
        const bool on = kS >= 0 && kS < (long long)K;
        const unsigned k = on ? (unsigned)kS : 0u;
        // owner: the last lane whose exclusive prefix is <= k (its inclusive prefix then exceeds k)
        unsigned lo = 0, hi = 63, eLo = 0;
#pragma unroll
        for (int s = 0; s < 6; s++) {
            const unsigned mid = (lo + hi + 1) >> 1;
            const unsigned e = (unsigned)__builtin_amdgcn_ds_bpermute((int)(mid * 4u), (int)excl);
            if (e <= k) { lo = mid; eLo = e; } else hi = mid - 1;
        }
        unsigned r = k - eLo;   // the r-th spawning seed of lane `lo`'s range
        int seed = -1;
        const uint4 *of = reinterpret_cast<const uint4 *>(fusedP + (size_t)lo * per);
        for (int c = 0; c < nch; c++) {
            const uint4 b = of[c];
            const unsigned w[4] = {spawn_word(b.x), spawn_word(b.y), spawn_word(b.z), spawn_word(b.w)};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned pc = (unsigned)__popc(w[q]);
                if (seed < 0) {
                    if (r < pc) {
                        unsigned m = w[q];
                        for (unsigned t = 0; t < r; t++) m &= m - 1;
                        seed = (int)lo * per + 16 * c + 4 * q + (__builtin_ctz(m) >> 3);
                    } else r -= pc;
                }
            }
        }
        if (on && seed >= 0) {
            if ((unsigned long long)i < dc->aux.cap) store_surfel(dc->aux.map, i, cand[seed]);
            else { long long code = 20; asm volatile("" : "+v"(code)); P.ctr[CTR_ERR] = code; }   // capacity exceeded (the host reserves nseeds slots per keyframe: never
                                                                                          // happens; the constant is kept out of the loop-invariant registers)
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the wave reads these records back right away
}

static_assert(SUB_ITEMS == 256 || SUB_ITEMS == 128 || SUB_ITEMS == 64, "k_fuse: four or two records per lane; k_compact lists a sub-block with one thread per slot");

}  // namespace

#endif  // __HIPCC__
