// msl_sf_compact.hip -- map stage of the surfel fusion, the classic chain behind k_fuse<false>: k_compact (initializeSurfels, reference
// src/SurfelFusion.cpp:285-331, and the slot refill / tail compaction of src/SurfelMapping.cpp:366-391) and the dealing of the next fuse
// launch's sub-blocks by screen position (k_compact's second workgroup; k_deal).  The stage's overview: msl_sf_map_dev.h.

#include "msl_sf_map_dev.h"

namespace {
// ---- dealing the sub-blocks to the XCDs by screen position (round 6) ----------------------------------------------------------------------
// Workgroup g of a launch runs on XCD g % 8, and every XCD has its own L2.  With the sub-blocks handed out in ARRAY order every XCD's waves
// project all over the screen: each of the eight L2s fetched the whole texel map (2.46 MB) and all seed records of the keyframe -- about 17 of
// the 52 MB k_fuse read per launch (round 5 counters).  Array neighbours do project to neighbouring pixels (creation order = superpixel
// raster order of the source keyframe), so a sub-block's in-view surfels cover a narrow band of image rows; k_fuse leaves that band's mean row
// as the sub-block's screen key, and this pass -- one workgroup beside the compaction, one launch behind the fusion that measured the keys --
// sorts the sub-blocks by key and cuts the list into eight equal runs: XCD x gets the x-th run (adaptive bands: equal numbers of in-view
// sub-blocks whatever the distribution of the rows), in row order, followed by its share of the sub-blocks with nothing in view, so that
// every XCD runs exactly G / 8 waves and the heavy ones are dispatched first.  Counting sort on the 255 key values in the LDS.
// The table is a hint: whatever the keys are, deal[] is a permutation of 0 .. G - 1 (G a multiple of 8).
// Run x is walked by the waves with index w, w & 7 == x.  In a classic launch wave w is workgroup w and runs on XCD w & 7; in a deferred launch the
// spawn workgroup sits at blockIdx 0, so wave w is workgroup w + 1 and runs on XCD (w + 1) % 8: run x then lives on XCD (x + 1) % 8 -- still one
// XCD per run, which is all that matters here.
template <int NT>
__device__ __forceinline__ void deal_subblocks(const unsigned *keys, int G, unsigned *deal, unsigned *s_hist, unsigned *s_off, unsigned *s_wave, unsigned *s_aux) {
    static_assert(NT == 256, "one histogram bin per thread");
    // Thread t owns the 32 consecutive sub-blocks [base + 32 t, base + 32 t + 32) of a chunk of 8192 (a map of 1 M surfels is one chunk): their keys
    // arrive as eight 16-byte loads issued together and are packed to one byte each.  The two passes walk the eight registers in ROLLED loops (the
    // group is rotated by one register per step and is itself again after eight) -- four waves that run alone on their SIMDs pay every dependent LDS
    // round trip and every instruction (4 cycles each) in full, so: no returning atomic in pass 1, four in flight per step in pass 2 together with
    // the per-key table word that says where the key's ranks go, and the sub-blocks with nothing in view (a third to two thirds of the map, all
    // in bin 255) are ranked by prefix sums instead of atomics.  (Round 6 history: straight-line code for 32 keys per thread was 40 KB of
    // instructions executed once -- 15 us beside the compaction's 8; one key per loop trip with two dependent LDS round trips each -- 18 us; a
    // seven-compare search for the XCD of every rank -- 12 us.)
    const unsigned t = threadIdx.x;
    constexpr int CH = 32 * NT;
    auto load_pack = [&](int base, unsigned (&kp)[8]) {
        uint4 v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = *reinterpret_cast<const uint4 *>(keys + base + 32 * (int)t + 4 * q);   // (the key plane is padded by > 8192 entries)
#pragma unroll
        for (int q = 0; q < 8; q++) kp[q] = min(v[q].x, 255u) | (min(v[q].y, 255u) << 8) | (min(v[q].z, 255u) << 16) | (min(v[q].w, 255u) << 24);
    };
    auto next_word = [&](unsigned (&kp)[8]) -> unsigned {   // the group's first register; the group rotated by one
        const unsigned w = kp[0];
#pragma unroll
        for (int q = 0; q < 7; q++) kp[q] = kp[q + 1];
        kp[7] = w;
        return w;
    };
    // pass 1 over a chunk: histogram of the in-view keys; returns the thread's number of sub-blocks with nothing in view
    auto count_chunk = [&](int base, unsigned (&kp)[8], bool hist) -> unsigned {
        unsigned fc = 0;
#pragma unroll 1
        for (int d = 0; d < 8; d++) {
            const unsigned w = next_word(kp);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const unsigned key = (w >> (8 * b)) & 255u;
                const bool in = base + 32 * (int)t + 4 * d + b < G;
                if (hist && in && key != 255u) atomicAdd(&s_hist[key], 1u);
                fc += in && key == 255u ? 1u : 0u;
            }
        }
        return fc;
    };
    unsigned k0[8];
    load_pack(0, k0);
    s_hist[t] = 0;
    __syncthreads();
    const unsigned fc0 = count_chunk(0, k0, true);
    for (int base = CH; base < G; base += CH) { unsigned kc[8]; load_pack(base, kc); (void)count_chunk(base, kc, true); }
    __syncthreads();
    // in-view rank r -> XCD x = floor(8 r / NI): the ranks [inS(x), inS(x + 1)); the fillers take what is left of each XCD's G / 8 waves: XCD x the
    // filler ranks [outS(x), outS(x + 1)), outS(x) = x G / 8 - inS(x)
    unsigned NI, fTot0, ex, fb0;   // NI: sub-blocks with something in view
    block_excl_scan_pair(t < 255u ? s_hist[t] : 0u, fc0, s_wave, &NI, &fTot0, ex, fb0);
    const unsigned gs = (unsigned)G >> 3;
    auto inS = [&](unsigned x) { return (x * NI + 7u) >> 3; };
    auto outS = [&](unsigned x) { return x * gs - inS(x); };
    {   // per key: the XCD its first rank falls into and how many more ranks fit there (nearly always all of the bin's); the running rank of the
        // bin counts from that XCD's start, so an atomic's return value IS the place in the XCD's run
        unsigned x0 = 0;
#pragma unroll
        for (unsigned y = 1; y < 8; y++) x0 += ex >= inS(y) ? 1u : 0u;
        s_off[t] = ex - inS(x0);
        s_hist[t] = x0 | ((inS(x0 + 1) - inS(x0)) << 3);
        if (t < 9) s_aux[t] = inS(t);   // (a rank that crosses into the next XCD's run looks its bounds up here)
    }
    __syncthreads();
    unsigned fillBase = 0;
    auto place_chunk = [&](int base, unsigned (&kp)[8], unsigned fb, unsigned ftot) {   // fb: the rank of the thread's first filler inside the chunk (array order)
        fb += fillBase;
        fillBase += ftot;
        unsigned xf = 0;
#pragma unroll
        for (unsigned y = 1; y < 8; y++) xf += fb >= outS(y) ? 1u : 0u;
        unsigned jf = (inS(xf + 1) - inS(xf)) + (fb - outS(xf));
#pragma unroll 1
        for (int d = 0; d < 8; d++) {
            const unsigned w = next_word(kp);
            unsigned rr[4], tb[4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const unsigned key = (w >> (8 * b)) & 255u;
                rr[b] = 0; tb[b] = 0;
                if (base + 32 * (int)t + 4 * d + b < G && key != 255u) { rr[b] = atomicAdd(&s_off[key], 1u); tb[b] = s_hist[key]; }
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
                // branch-free: the place of an in-view sub-block (its rank inside the XCD the key's table word names) or of a filler (the thread's
                // running filler place) selected per lane; only a rank that crosses into the next XCD's run -- rare -- takes a (wave-level) slow path.
                // (With a divergent branch per kind every step ran both sides one after the other: 6 us for this pass.)
                const unsigned key = (w >> (8 * b)) & 255u;
                const int sb = base + 32 * (int)t + 4 * d + b;
                const bool in = sb < G, iv = in && key != 255u, fl = in && key == 255u;
                unsigned x = tb[b] & 7u, room = tb[b] >> 3, j = rr[b];
                if (__builtin_expect(__ballot((iv && j >= room) || (fl && jf >= gs)) != 0ull, 0)) {
                    if (iv) while (j >= room) { j -= room; x++; room = s_aux[x + 1] - s_aux[x]; }      // the bin straddles two XCDs' runs
                    if (fl) while (jf >= gs) { xf++; jf = s_aux[xf + 1] - s_aux[xf]; }                  // this XCD's run is full: on to the next one with room for fillers
                }
                const unsigned at = (iv ? x : xf) * gs + (iv ? j : jf);
                if (in) deal[at] = (unsigned)sb;
                jf += fl ? 1u : 0u;
            }
        }
    };
    place_chunk(0, k0, fb0, fTot0);
    for (int base = CH; base < G; base += CH) {
        unsigned kc[8];
        load_pack(base, kc);
        const unsigned fc = count_chunk(base, kc, false);
        unsigned ftot;
        const unsigned fb = block_excl_scan(fc, s_wave, &ftot);
        place_chunk(base, kc, fb, ftot);
    }
    __syncthreads();   // (the caller reuses the LDS arrays)
}
__global__ __launch_bounds__(256) void k_deal(const unsigned *keys, int G, unsigned *deal) {
    __shared__ unsigned s_hist[256], s_off[256], s_wave[33], s_aux[16];
    deal_subblocks<256>(keys, G, deal, s_hist, s_off, s_wave, s_aux);
}

constexpr int TAIL_MAX_HOPS = 64;   // relay hops resolved per hole before the literal loop takes over (k_compact)

// =============================================================================================
// Classic compaction (one launch per keyframe, behind k_fuse<false>)
// =============================================================================================
// Resident-map compaction (SurfelMapping.cpp:366-391) with prefix sums.  Deleted slots ascending d_0..d_{D-1};
// new surfel k -> d_{D-1-k} while any remain, else appended.  If D > K the literal `while` loop (:386-390) moves,
// at step i = 1..R (R = D-K), the element at position n-i into the i-th largest leftover hole; a hole inside the
// tail [nFinal, n) only relays what lands in it.  So the a-th smallest leftover hole (< nFinal) finally receives
// resolve(nFinal + a), resolve(p) = p if p is live, else resolve(n - rank_desc(p)): a short upward chain.

// k_compact: everything after k_fuse in ONE launch.
//   every workgroup : exclusive scan of the per-chunk deleted counts (each workgroup scans the <= cap/1024 partials itself,
//                     so there is no inter-workgroup dependency), then lists the deleted slots of its own chunks in
//                     ascending order (write-through stores);
//   last workgroup  : initializeSurfels (:285-331) = ordered emission of the seed candidates the fuse step did not consume,
//                     counters, new surfel k -> k-th largest deleted slot else appended, tail sources resolved and moved.
// mode 1 (host-vector drop-in, one workgroup): emission and counters only; the caller compacts (SurfelMapping.cpp:366-391).
constexpr int SMALL_D = 512, SMALL_CHUNKS = 48;   // single-workgroup path: few deletions in few chunks

// What k_compact reads of the handle: a slim copy of SfDev with the keyframe's slot folded in (round 6; 36 instead of ~150 dwords of kernel
// arguments).  Unlike k_fuse in round 5 the kernel's register count did not follow (182 VGPRs in the 8-word form: the prefetched counts, flag
// words and candidate records of the steady-state path are live together by design -- every load of the chain leaves before the first use; a
// 128-register cap spills 78 of them to scratch), so what the slim arguments buy is the shorter scalar prologue only.
struct CompactArgs {
    int nseeds, flagStride, dealG, _pad;
    unsigned long long cap;
    MapSoA map;
    long long *ctr;
    const uint8_t *candOk, *fused;     // this keyframe's slot
    const msl_surfel *cand;            // ...
    msl_surfel *newSurfels;
    unsigned *blockSums, *blockUpd, *delList, *srcOf, *tickets, *delU, *delUCount;
    const unsigned *sbKeys; unsigned *deal;
};
__host__ inline CompactArgs compact_args(const SfDev &P, int slot) {
    CompactArgs A;
    A.nseeds = P.nseeds; A.flagStride = P.flagStride; A.dealG = P.dealG; A._pad = 0; A.cap = P.cap; A.map = P.map; A.ctr = P.ctr;
    A.candOk = P.candOk + (size_t)slot * P.flagStride; A.fused = P.fused + (size_t)slot * P.flagStride; A.cand = P.cand + (size_t)slot * P.nseeds;
    A.newSurfels = P.newSurfels; A.blockSums = P.blockSums; A.blockUpd = P.blockUpd; A.delList = P.delList; A.srcOf = P.srcOf; A.tickets = P.tickets;
    A.delU = P.delU; A.delUCount = P.delUCount; A.sbKeys = P.sbKeys; A.deal = P.deal;
    return A;
}

// LDS is kept to ~3.5 KB: on a GPU saturated by the LDS-heavy batched kernels a larger workgroup waits for a CU to drain.
// NQW: the seed flags of a thread arrive in ONE round trip as NQW 32-bit words per array (8: <= 32 seeds per thread, 640 x 480 has 19; 24: <= 96,
// 1280 x 960 has 76); 0: the generic loop (any size or alignment).  Separate instantiations: the 24-word form costs 45 registers more (227
// against 182), which the common geometry need not carry.
template <int NQW>
__global__ __launch_bounds__(256) void k_compact(CompactArgs P, int mode) {
    constexpr int NT = 256, TILE = 4 * NT;
    __shared__ unsigned s_wave[33];
    __shared__ unsigned s_dl[SMALL_D];          // single-workgroup paths: the ascending deleted-slot list stays in LDS
    __shared__ unsigned s_raw[LIST_D];          // fastest path: k_fuse's unordered hand-over list
    __shared__ unsigned s_last, s_upd, s_nzChunks, s_base, s_cntChunk;
    __shared__ unsigned s_nzIdx[SMALL_CHUNKS], s_nzCnt[SMALL_CHUNKS], s_nzSortIdx[SMALL_CHUNKS], s_nzSortCnt[SMALL_CHUNKS];   // sub-blocks with deletions
    __shared__ int s_fallback;
    __builtin_amdgcn_s_setprio(3);   // latency-critical serial chain next to the throughput-oriented batched kernels
    // Steady state (k_fuse handed over <= LIST_D deleted slots): workgroup 0 does everything alone; the others leave after one load
    // instead of fetching the partials and flags as well.
    // (round 6) the second workgroup first deals the sub-blocks for the next fuse launch from the screen keys this keyframe's launch left
    // (deal_subblocks above) -- beside workgroup 0's compaction, not behind it
    if (mode == 0 && blockIdx.x == 1 && P.dealG > 0) deal_subblocks<NT>(P.sbKeys, P.dealG, P.deal, s_raw, s_dl, s_wave, s_nzIdx);
    if (mode == 0 && blockIdx.x != 0 && *P.delUCount <= LIST_D) return;
    // Loads that do not depend on anything are issued first; in particular every workgroup already fetches the seed flags
    // the continuation needs, so the continuing workgroup does not start its dependent chain with a cold memory round trip.
    const uint4 bs0 = *reinterpret_cast<const uint4 *>(P.blockSums + 4 * threadIdx.x);   // first tile of chunk partials
    constexpr int NBU = 8;
    uint4 bu[NBU];   // the first 8192 per-sub-block updated counts = a map of 1 M surfels in one trip (arrays are padded by >= 8192 zeroed entries)
#pragma unroll
    for (int q = 0; q < NBU; q++) bu[q] = *reinterpret_cast<const uint4 *>(P.blockUpd + TILE * q + 4 * threadIdx.x);
    static_assert(LIST_D == NT, "one hand-over entry per thread");
    const unsigned du = P.delU[threadIdx.x];
    const unsigned dHand = *P.delUCount;   // k_fuse's running total of deleted slots = D of this keyframe
    const long long n = P.ctr[CTR_LIVE];
    const bool bad = P.ctr[CTR_ERR] == 20;
    const uint8_t *candOk = P.candOk, *fused = P.fused;
    const int per = (((P.nseeds + NT - 1) / NT) + 3) & ~3;      // seeds per thread, multiple of 4: aligned 32-bit flag loads
    const int s0 = threadIdx.x * per, s1 = min(s0 + per, P.nseeds);
    unsigned cnt = 0;
    unsigned long long emit = 0, emitHi = 0;   // bit j: seed s0 + j spawns a surfel (emit: j < 64; emitHi: 64 <= j < 128)
    const msl_surfel *cand = P.cand;
    const bool aligned4 = (P.nseeds & 3) == 0 && ((reinterpret_cast<size_t>(candOk) | reinterpret_cast<size_t>(fused)) & 3) == 0;
    // all flag words of the thread in ONE round trip: 8 words each for <= 32 seeds per thread (640 x 480: 19), 24 words for <= 96 (1280 x 960: 76 --
    // round 3 walked the seeds beyond the 64th one by one, two dependent byte loads each, and the kernel took 30 us at that size)
    auto flags_in_one_trip = [&](auto nqTag) {
        constexpr int NQ = decltype(nqTag)::value;
        unsigned cw[NQ], fw[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const int i = s0 + 4 * q;
            const bool in = 4 * q < per && i < s1;
            cw[q] = in ? *reinterpret_cast<const unsigned *>(candOk + i) : 0u;
            fw[q] = in ? *reinterpret_cast<const unsigned *>(fused + i) : 0u;
        }
#pragma unroll
        for (int q = 0; q < NQ; q += 8)   // (a common use per group of loads keeps them from being sunk into their consumers)
            asm volatile("" ::"v"(cw[q]), "v"(cw[q + 1]), "v"(cw[q + 2]), "v"(cw[q + 3]), "v"(cw[q + 4]), "v"(cw[q + 5]), "v"(cw[q + 6]), "v"(cw[q + 7]),
                         "v"(fw[q]), "v"(fw[q + 1]), "v"(fw[q + 2]), "v"(fw[q + 3]), "v"(fw[q + 4]), "v"(fw[q + 5]), "v"(fw[q + 6]), "v"(fw[q + 7]));
#pragma unroll
        for (int q = 0; q < NQ; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned e = (s0 + 4 * q + j < s1 && ((cw[q] >> (8 * j)) & 0xFF) && !((fw[q] >> (8 * j)) & 0xFF)) ? 1u : 0u;
                cnt += e;
                if (4 * q + j < 64) emit |= (unsigned long long)e << ((4 * q + j) & 63);
                else emitHi |= (unsigned long long)e << ((4 * q + j - 64) & 63);
            }
    };
    if constexpr (NQW > 0) {
        (void)aligned4;   // (the host picked this instantiation: per <= 4 NQW and aligned flag arrays)
        flags_in_one_trip(std::integral_constant<int, NQW>{});
    } else {
        for (int i = s0; i < s1; i += 4) {
            unsigned c4, f4;
            if (i + 4 <= P.nseeds && ((reinterpret_cast<size_t>(candOk + i) | reinterpret_cast<size_t>(fused + i)) & 3) == 0) {
                c4 = *reinterpret_cast<const unsigned *>(candOk + i); f4 = *reinterpret_cast<const unsigned *>(fused + i);
            } else {
                c4 = f4 = 0;
                for (int j = 0; j < 4 && i + j < P.nseeds; j++) { c4 |= (unsigned)candOk[i + j] << (8 * j); f4 |= (unsigned)fused[i + j] << (8 * j); }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned e = (i + j < s1 && ((c4 >> (8 * j)) & 0xFF) && !((f4 >> (8 * j)) & 0xFF)) ? 1u : 0u;
                cnt += e;
                if (i + j - s0 < 64) emit |= (unsigned long long)e << (i + j - s0);
                else if (i + j - s0 < 128) emitHi |= (unsigned long long)e << (i + j - s0 - 64);
            }
        }
    }
    const long long nblk = (n + SUB_ITEMS - 1) / SUB_ITEMS;   // sub-block partials written by k_fuse
    const long long nWg = nblk;   // k_fuse waves (blockUpd entries): one per sub-block
    // The prefetched updated counts are folded into ONE register here, as soon as the flag words have been consumed (they were requested before
    // them, so they have arrived): 32 registers that stayed live down to the continuation otherwise -- the kernel's register count decides how soon a
    // workgroup of this latency-critical launch finds room on a CU that the frame-batched kernels fill.  Round 6: 182 -> 87 VGPRs with this and without
    // the prefetch of the thread's first two candidate surfels into registers (51 registers, for a round trip that only keyframes with new surfels
    // pay): k_compact 12.2 -> 9.1 us in the timed region (its time alone is unchanged), config 3 +2 %, moving camera 14.8 -> 16.1 k frames/s.
    unsigned updPart = 0;
#pragma unroll
    for (int q = 0; q < NBU; q++) {
        const long long c = TILE * q + 4 * threadIdx.x;
        updPart += (c < nWg ? bu[q].x : 0u) + (c + 1 < nWg ? bu[q].y : 0u) + (c + 2 < nWg ? bu[q].z : 0u) + (c + 3 < nWg ? bu[q].w : 0u);
    }
    s_raw[threadIdx.x] = du;
    if (threadIdx.x == 0) { s_upd = 0; s_fallback = 0; s_nzChunks = 0; }
    __syncthreads();
    // k_fuse already counted the deleted slots; when they all fit its hand-over list (the steady state) the per-sub-block
    // counts are not needed at all.  Otherwise one pass over them (4 consecutive per thread and tile) lists the sub-blocks
    // that contain deletions.
    const bool fastest = mode == 0 && dHand <= LIST_D;
    unsigned vsum = 0;
    if (!fastest)
        for (long long t0 = 0; t0 < nblk; t0 += TILE) {
            const long long c = t0 + 4 * threadIdx.x;
            const uint4 v4 = t0 == 0 ? bs0 : *reinterpret_cast<const uint4 *>(P.blockSums + c);
            const unsigned x[4] = {c < nblk ? v4.x : 0u, c + 1 < nblk ? v4.y : 0u, c + 2 < nblk ? v4.z : 0u, c + 3 < nblk ? v4.w : 0u};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x[j] > 0) {
                    vsum += x[j];
                    const unsigned q = atomicAdd(&s_nzChunks, 1u);
                    if (q < SMALL_CHUNKS) { s_nzIdx[q] = (unsigned)(c + j); s_nzCnt[q] = x[j]; }
                }
        }
    unsigned Dtot, Ku, exUnused, pos;
    block_excl_scan_pair(vsum, cnt, s_wave, &Dtot, &Ku, exUnused, pos);   // total deletions + emission scan
    const long long D = fastest ? (long long)dHand : (long long)Dtot;
    // single-workgroup paths: workgroup 0 does everything alone -- no ticket, no write-through list
    const bool small = mode == 0 && !fastest && D <= SMALL_D && s_nzChunks <= SMALL_CHUNKS;
    const bool single = fastest || small;
    if (single && blockIdx.x != 0) return;
    if (mode == 0 && !bad) {
        if (fastest) {
            if (threadIdx.x < D) {   // rank-sort in LDS
                unsigned r = 0;
                for (unsigned j = 0; j < (unsigned)D; j++) r += s_raw[j] < du ? 1u : 0u;
                s_dl[r] = du;
            }
        } else if (small) {
            // few sub-blocks hold all deletions: order them by index (rank sort); a sub-block's offset in the ascending
            // list is the sum of the counts before it -- no scan over the (thousands of) empty sub-blocks
            const unsigned nz = s_nzChunks;
            if (threadIdx.x < nz) {
                const unsigned me = s_nzIdx[threadIdx.x];
                unsigned r = 0;
                for (unsigned j = 0; j < nz; j++) r += s_nzIdx[j] < me ? 1u : 0u;
                s_nzSortIdx[r] = me; s_nzSortCnt[r] = s_nzCnt[threadIdx.x];
            }
            __syncthreads();
            unsigned base = 0;
            for (unsigned it = 0; it < nz; it++) {
                const long long i0 = (long long)s_nzSortIdx[it] * SUB_ITEMS + threadIdx.x;   // one slot per thread: ascending
                const unsigned f = (threadIdx.x < (unsigned)SUB_ITEMS && i0 < n && hot_is_deleted(P.map, i0)) ? 1u : 0u;
                unsigned tt;
                const unsigned w = base + block_excl_scan(f, s_wave, &tt);
                if (f) s_dl[w] = (unsigned)i0;
                base += s_nzSortCnt[it];
            }
        } else {
            // every workgroup lists the deleted slots of its own sub-blocks in ascending order; a sub-block's base offset
            // lives in the registers of the thread that scanned it and is broadcast through one LDS word
            unsigned carry = 0;
            for (long long t0 = 0; t0 < nblk; t0 += TILE) {
                const long long c = t0 + 4 * threadIdx.x;
                const uint4 v4 = t0 == 0 ? bs0 : *reinterpret_cast<const uint4 *>(P.blockSums + c);
                const unsigned v[4] = {c < nblk ? v4.x : 0u, c + 1 < nblk ? v4.y : 0u, c + 2 < nblk ? v4.z : 0u, c + 3 < nblk ? v4.w : 0u};
                unsigned tot;
                const unsigned ex = carry + block_excl_scan(v[0] + v[1] + v[2] + v[3], s_wave, &tot);
                const long long nIter = (min(t0 + TILE, nblk) - t0 - blockIdx.x + gridDim.x - 1) / gridDim.x;
                for (long long it = 0; it < nIter; it++) {
                    const long long b = t0 + blockIdx.x + it * gridDim.x;
                    const int q = (int)(b - t0);
                    if ((int)threadIdx.x == (q >> 2)) {
                        const int comp = q & 3;
                        s_base = ex + (comp > 0 ? v[0] : 0u) + (comp > 1 ? v[1] : 0u) + (comp > 2 ? v[2] : 0u);
                        s_cntChunk = v[comp];
                    }
                    __syncthreads();
                    const unsigned base = s_base, cntChunk = s_cntChunk;
                    if (cntChunk == 0) { __syncthreads(); continue; }   // nothing deleted in this sub-block
                    const long long i0 = b * SUB_ITEMS + threadIdx.x;       // one slot per thread keeps the list ascending
                    const unsigned f = (threadIdx.x < (unsigned)SUB_ITEMS && i0 < n && hot_is_deleted(P.map, i0)) ? 1u : 0u;
                    unsigned tt;
                    const unsigned w = base + block_excl_scan(f, s_wave, &tt);   // (its barriers also protect s_base)
                    if (f) st_agent(&P.delList[w], (unsigned)i0);
                }
                carry += tot;
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if (mode == 0 && !single && !last_workgroup(&P.tickets[1], &s_last)) return;
    // ================= continuation: one workgroup =================
    // updated count
    {
        unsigned u = updPart;
        for (long long c2 = (long long)NBU * TILE + threadIdx.x; c2 < nWg; c2 += blockDim.x) u += P.blockUpd[c2];
        u = wave_incl_scan(u);                                   // one LDS atomic per wave instead of 256 on one address
        if ((threadIdx.x & 63) == 63 && u) atomicAdd(&s_upd, u);
    }
    // initializeSurfels (:285-331): thread t owns the contiguous seeds [t*per, (t+1)*per); emission order = seed index order
    const long long K = Ku;
    const long long nAfter = mode == 1 ? n : (D >= K ? n - (D - K) : n + (K - D));
    const bool place = mode == 0 && !bad && (unsigned long long)nAfter <= P.cap;
    auto DL = [&](long long j) -> unsigned { return single ? s_dl[j] : ld_agent(&P.delList[j]); };
    if (cnt) {
        auto emit_one = [&](const msl_surfel &e) {
            const long long k = pos++;
            P.newSurfels[k] = e;                    // host-vector mode and debugging read this list
            if (place)                              // new surfel k -> k-th largest deleted slot while any remain, else appended
                store_surfel(P.map, k < D ? (long long)DL(D - 1 - k) : n + (k - D), e);   // (SurfelMapping.cpp:372-384)
        };
        for (unsigned long long m = emit; m; m &= m - 1) emit_one(cand[s0 + __builtin_ctzll(m)]);
        for (unsigned long long mh = emitHi; mh; mh &= mh - 1) emit_one(cand[s0 + 64 + __builtin_ctzll(mh)]);
        for (int i = s0 + 128; i < s1; i++)
            if (candOk[i] && !fused[i]) emit_one(cand[i]);
    }
    __syncthreads();   // s_upd complete; new-surfel stores ordered before the tail moves below (same workgroup)
    if (threadIdx.x == 0) {
        P.ctr[CTR_NEW] = K; P.ctr[CTR_DELETED] = D; P.ctr[CTR_UPDATED] = s_upd; P.ctr[CTR_BEFORE] = n; P.ctr[CTR_AFTER] = nAfter;
        // running totals over all keyframes of this handle (one writer per launch, launches are ordered): bench.py derives the
        // per-keyframe averages of a timed region from their differences
        P.ctr[CTR_TOT_NEW] += K; P.ctr[CTR_TOT_DELETED] += D; P.ctr[CTR_TOT_UPDATED] += s_upd; P.ctr[CTR_TOT_KF] += 1; P.ctr[CTR_TOT_BEFORE] += n;
        if ((unsigned long long)nAfter > P.cap) P.ctr[CTR_ERR] = 20;  // capacity exceeded
    }
    if (!place) { if (threadIdx.x == 0) *P.delUCount = 0; return; }   // (host-vector mode, or the deferred capacity error: the live count stays)
    const long long t0 = threadIdx.x, stride = blockDim.x;
    if (D > K) {
        const long long R = D - K, nFinal = n - R;
        auto lower = [&](long long x) -> long long {   // first index in delList[0..R) with value >= x
            long long lo = 0, hi = R;
            while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)DL(mid) < x) lo = mid + 1; else hi = mid; }
            return lo;
        };
        const long long cntLow = lower(nFinal);
        for (long long a = t0; a < cntLow; a += stride) {
            long long p = nFinal + a;
            int hop = 0;
            for (; hop < TAIL_MAX_HOPS; hop++) {
                const long long lb = lower(p);
                if (lb < R && (long long)DL(lb) == p) p = n - (R - lb);   // relay hole: follow to where its content came from
                else break;
            }
            if (hop == TAIL_MAX_HOPS) s_fallback = 1;   // pathological chain: fall back to the literal loop
            P.srcOf[a] = (unsigned)p;
        }
        __syncthreads();   // also orders the new-surfel stores above before the moves below (same workgroup)
        if (s_fallback) {
            if (threadIdx.x == 0)   // literal back-to-front loop (SurfelMapping.cpp:386-390), pathological delete patterns only
                for (long long i = 1; i <= R; i++) {
                    const long long hole = DL(R - i), src = n - i;
                    if (src != hole) move_surfel(P.map, hole, src);
                }
        } else {
            for (long long a = t0; a < cntLow; a += stride) move_surfel(P.map, (long long)DL(a), (long long)P.srcOf[a]);
        }
    }
    if (threadIdx.x == 0) { P.ctr[CTR_LIVE] = nAfter; *P.delUCount = 0; }   // publish the new live count, re-arm the hand-over list
}
}  // namespace

namespace msl {
namespace sf {
void map_launch_compact(KernelProfiler &prof, hipStream_t st, const SfDev &P, int slot, bool resident) {
    const CompactArgs A = compact_args(P, slot);
    const int per = (((P.nseeds + 255) / 256) + 3) & ~3;   // seeds per thread (k_compact)
    const bool aligned4 = (P.nseeds & 3) == 0 && ((reinterpret_cast<size_t>(A.candOk) | reinterpret_cast<size_t>(A.fused)) & 3) == 0;
    const dim3 grid(resident ? 128 : 1);
    if (per <= 32 && aligned4) MSL_SF_LAUNCH(prof, SK_COMPACT, st, k_compact<8>, grid, dim3(256), A, resident ? 0 : 1);
    else if (per <= 96 && aligned4) MSL_SF_LAUNCH(prof, SK_COMPACT, st, k_compact<24>, grid, dim3(256), A, resident ? 0 : 1);
    else MSL_SF_LAUNCH(prof, SK_COMPACT, st, k_compact<0>, grid, dim3(256), A, resident ? 0 : 1);   // scan + new surfels + refill + tail compaction
}
void map_launch_deal(hipStream_t st, const SfDev &P) { hipLaunchKernelGGL(k_deal, dim3(1), dim3(256), 0, st, P.sbKeys, P.dealG, P.deal); }
// Test hook: the dealing of G sub-blocks (a multiple of 8) with the given screen keys, host arrays, synchronous.
int map_debug_deal(const uint32_t *keys_host, int G, uint32_t *deal_host) {
    if (!keys_host || !deal_host || G < 8 || (G & 7)) return MSL_ERR_INVALID;
    const size_t pad = (size_t)G + 8192;   // the key plane of a handle is padded the same way (whole chunks are loaded)
    DevBuf keys, deal;
    MSL_HIP_TRY(grow_all(0, {{keys, sizeof(unsigned) * pad}, {deal, sizeof(unsigned) * (G + 64)}}));
    unsigned *dk = (unsigned *)keys.p, *dd = (unsigned *)deal.p;
    MSL_HIP_TRY(hipMemset(dk, 0xFF, sizeof(unsigned) * pad)); MSL_HIP_TRY(hipMemset(dd, 0xFF, sizeof(unsigned) * G));
    MSL_HIP_TRY(hipMemcpy(dk, keys_host, sizeof(unsigned) * G, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_deal, dim3(1), dim3(256), 0, 0, dk, G, dd);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(hipMemcpy(deal_host, dd, sizeof(unsigned) * G, hipMemcpyDeviceToHost));
    return MSL_OK;
}
}  // namespace sf
}  // namespace msl
