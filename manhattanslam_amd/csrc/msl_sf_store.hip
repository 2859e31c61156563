// msl_sf_store.hip -- the resident surfel map as the host sees it: the layout of its storage, the live-count bookkeeping, and the map-exchange
// part of the C ABI (reserve, upload, download, snapshot, restore, size, detach, export, append, counters).  No kernel lives here; nothing outside
// this file knows how the map's arrays lie in their allocations.

#include "msl_sf_handle.h"

#include <cmath>
#include <fstream>
#include <vector>

namespace msl {
namespace sf {

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
constexpr size_t round_cap(size_t n) { return (n + 4095) & ~(size_t)4095; }

void set_map_ptrs(msl_sf *h, size_t c) {
    MapSoA &M = h->dev.map;
    float *store = (float *)h->map.store.p;
    M.hot = reinterpret_cast<HotPk *>(store + ST_HOT * c);
    M.cold = reinterpret_cast<ColdRec *>(store + ST_COLD * c);
    M.rgbWide = reinterpret_cast<int *>(store + ST_RGB * c);    // exact ints of the COLD_WIDE records (untouched otherwise)
    M.utlWide = reinterpret_cast<int *>(store + ST_UTL * c);    // exact ints of the HOT_WIDE records
    M.wideFlag = h->dev.ctr + CTR_WIDE;
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

// The four planes of a map store: word offset per surfel of capacity, bytes per surfel, and the wide-record flag (CTR_WIDE) without which the
// plane holds nothing (0: always in use)
struct StorePlane { size_t word, bytes; long long wide; };
constexpr StorePlane kStorePlanes[4] = {{ST_HOT, sizeof(HotPk), 0}, {ST_COLD, sizeof(ColdRec), 0}, {ST_RGB, sizeof(int) * 3, 1}, {ST_UTL, sizeof(int) * 2, 2}};
constexpr long long ALL_PLANES = 3;
// The first n surfels of a store laid out for srcCap surfels into one laid out for dstCap, device to device: hot and cold, and the side arrays
// the flags `wide` name.  async: the stream the copies are ordered on; nullptr: synchronous copies.
int copy_store(void *dst, size_t dstCap, const void *src, size_t srcCap, size_t n, long long wide, const hipStream_t *async) {
    for (const StorePlane &pl : kStorePlanes) {
        if (pl.wide && !(wide & pl.wide)) continue;
        float *d = (float *)dst + pl.word * dstCap;
        const float *s = (const float *)src + pl.word * srcCap;
        if (async) MSL_HIP_TRY(hipMemcpyAsync(d, s, pl.bytes * n, hipMemcpyDeviceToDevice, *async));
        else MSL_HIP_TRY(hipMemcpy(d, s, pl.bytes * n, hipMemcpyDeviceToDevice));
    }
    return MSL_OK;
}
size_t snap_cap(const msl_sf *h) { return h->d_snapStore.cap / (sizeof(float) * MAP_WORDS); }   // surfels the snapshot store is laid out for

// The asynchronous live-count snapshots only ever LOWER liveBound; whenever the map is replaced from outside the keyframe chain the ones still
// pending describe the old map and must be ignored.
void drop_live_snapshots(msl_sf *h) {
    for (int i = 0; i < msl_sf::NSNAP; i++) h->snapLive[i] = false;   // (their running totals -- the churn estimate -- stay valid)
}

// Counter snapshots that have arrived (their event has fired): a tighter bound / a fresher value of the live count, and the churn estimate -- spawned +
// deleted surfels per keyframe between two snapshots, from the running totals.
void consume_snapshots(msl_sf *h, size_t nseeds) {
    for (int i = 0; i < msl_sf::NSNAP; i++)
        if (h->snapBusy[i] && hipEventQuery(h->snapEv[i]) == hipSuccess) {
            h->snapBusy[i] = false;
            const long long *sn = (const long long *)h->h_snap.p + (size_t)i * msl_sf::SNAPW;
            if (h->snapLive[i]) {
                const size_t cand = (size_t)sn[CTR_LIVE] + (size_t)(h->kfEnq - h->snapKf[i]) * nseeds;   // count then + what was enqueued since
                if (cand < h->liveBound) h->liveBound = cand;
                if (h->snapKf[i] >= h->liveKnownKf) { h->liveKnown = (size_t)sn[CTR_LIVE]; h->liveKnownKf = h->snapKf[i]; }   // completed snapshots are visited in array order, not age order
            }
            if (h->snapKf[i] > h->churnAt) {
                if (h->churnNew >= 0 && sn[CTR_TOT_KF] > h->churnKf)
                    h->churn = (double)((sn[CTR_TOT_NEW] - h->churnNew) + (sn[CTR_TOT_DELETED] - h->churnDel)) / (double)(sn[CTR_TOT_KF] - h->churnKf);
                h->churnNew = sn[CTR_TOT_NEW]; h->churnDel = sn[CTR_TOT_DELETED]; h->churnKf = sn[CTR_TOT_KF]; h->churnAt = h->snapKf[i];
            }
        }
}

}  // namespace

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

int map_realloc(msl_sf *h, size_t cap, size_t keep) {
    cap = round_cap(cap);
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
        int rc = sync_all(h);
        if (rc != MSL_OK) return rc;
        rc = copy_store(m.store.p, cap, h->map.store.p, h->dev.cap, keep, ALL_PLANES, nullptr);   // (rare path: no need to know whether any record is wide)
        if (rc != MSL_OK) return rc;
    }
    h->map = std::move(m);
    h->blkStride = bst;
    h->dealG = 0;              // (the dealing table went with the old allocation)
    set_map_ptrs(h, cap);
    return write_ctl(h);
}

int read_ctr(msl_sf *h) {
    if (h->ownStreams && h->copyStream) MSL_HIP_TRY(hipStreamSynchronize(h->copyStream));
    MSL_HIP_TRY(hipStreamSynchronize(h->preStream));
    MSL_HIP_TRY(hipMemcpyAsync(h->h_ctr.p, h->dev.ctr, sizeof(long long) * CTR_COUNT, hipMemcpyDeviceToHost, h->mapStream));
    MSL_HIP_TRY(hipStreamSynchronize(h->mapStream));
    h->prof.drain();
    consume_snapshots(h, (size_t)h->dev.nseeds);   // (all pending snapshots have arrived: their churn information is kept, the live count below is newer)
    h->liveBound = live_count(h);   // both streams are idle: the count is exact
    h->liveKnown = h->liveBound; h->liveKnownKf = h->kfEnq;
    for (int i = 0; i < msl_sf::NSNAP; i++) h->snapBusy[i] = false;   // (their events have fired: the stream is idle)
    return MSL_OK;
}

int check_err(msl_sf *h) {
    const long long e = host_ctr(h, CTR_ERR);
    if (e) {
        (void)hipMemsetAsync(h->dev.ctr + CTR_ERR, 0, sizeof(long long), h->mapStream);
        if (e == 20) set_error("resident surfel map capacity exceeded (reserve more with msl_sf_map_reserve)");
        else set_error("surfel pipeline device-side bound exceeded (code %lld)", e);
        return MSL_ERR_OVERFLOW;
    }
    return MSL_OK;
}

// The reference's mvLocalSurfels is an unbounded std::vector (include/Map.h:130): grow the resident map before a batch could overflow it.  Every
// keyframe adds at most nseeds surfels, so the host only needs an upper bound of the live count; the exact count is read back (one sync) only
// when that bound reaches the capacity.
int reserve_map(msl_sf *h, int n) {
    const SfDev &D = h->dev;
    h->mirrorValid = false;   // the resident map moves on without the host-vector caller
    const size_t need = (size_t)n * (size_t)D.nseeds;
    consume_snapshots(h, (size_t)D.nseeds);
    if (h->liveBound + need > D.cap) {
        int rc = settle(h);
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

void map_replaced(msl_sf *h, size_t n) {
    h->liveBound = n; h->liveKnown = n; h->liveKnownKf = h->kfEnq; h->classicNext = true;
    drop_live_snapshots(h);   // a count recorded before would otherwise lower the bound below n
}

int aos_in(msl_sf *h, const msl_surfel *host, size_t n, bool atEnd) {
    const hipStream_t s = h->mapStream;
    MSL_HIP_TRY(h->d_aos.grow(sizeof(msl_surfel) * n, s));
    MSL_HIP_TRY(hipMemcpyAsync(h->d_aos.p, host, sizeof(msl_surfel) * n, hipMemcpyHostToDevice, s));
    map_launch_aos_to_soa(h->prof, s, h->dev, (const msl_surfel *)h->d_aos.p, (long long)n, atEnd);
    return MSL_OK;
}

int aos_out(msl_sf *h, size_t n, const MapSelect *sel, msl_surfel *host, const AosRun *runs, size_t nRuns) {
    const hipStream_t s = h->mapStream;
    MSL_HIP_TRY(h->d_aos.grow(sizeof(msl_surfel) * n, s));
    msl_surfel *aos = (msl_surfel *)h->d_aos.p;
    if (sel) map_launch_select_write(s, h->dev, sel->mode, sel->arg, aos, sel->mark ? 1 : 0);
    else map_launch_soa_to_aos(h->prof, s, h->dev, aos, (long long)n);
    for (size_t r = 0; r < nRuns; r++)
        MSL_HIP_TRY(hipMemcpyAsync(host + runs[r].i0, aos + runs[r].i0, sizeof(msl_surfel) * (runs[r].i1 - runs[r].i0), hipMemcpyDeviceToHost, s));
    return MSL_OK;
}

namespace {

// detach (mark) / export: the selected surfels counted, then written out in map order
int map_select(msl_sf *h, const MapSelect &sel, msl_surfel *out, size_t cap, size_t *n_out, const char *what) {
    if (!h || !n_out) { set_error("%s: invalid argument", what); return MSL_ERR_INVALID; }
    if (sel.mark) { h->mirrorValid = false; h->classicNext = true; }
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = settle(h);                         // waits for both streams
    if (rc != MSL_OK) return rc;
    *n_out = 0;
    if (live_count(h) == 0) return MSL_OK;
    const hipStream_t s = h->mapStream;
    map_launch_select_count(s, h->dev, sel.mode, sel.arg);
    rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    const size_t m = (size_t)host_ctr(h, CTR_SELECTED);
    *n_out = m;
    (void)hipMemsetAsync(h->dev.ctr + CTR_SELECTED, 0, sizeof(long long), s);
    if (m > cap || (m && !out)) { set_error("%s: %zu surfels selected, capacity %zu", what, m, cap); return MSL_ERR_CAPACITY; }
    if (m == 0) return MSL_OK;
    const AosRun all{0, m};
    rc = aos_out(h, m, &sel, out, &all, 1);
    if (rc != MSL_OK) return rc;
    MSL_HIP_TRY(hipStreamSynchronize(s));
    return MSL_OK;
}

}  // namespace

}  // namespace sf
}  // namespace msl

using namespace msl;
using namespace msl::sf;

extern "C" {

int msl_sf_map_reserve(msl_sf *h, size_t capacity) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    if (capacity <= h->dev.cap) return MSL_OK;
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    return map_realloc(h, capacity, live_count(h));
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
    MSL_HIP_TRY(hipMemsetAsync(h->dev.ctr + CTR_WIDE, 0, sizeof(long long), s));   // a fresh map: no wide records yet
    if (n) {
        rc = aos_in(h, host, n, false);
        if (rc != MSL_OK) return rc;
    }
    map_launch_set_ctr(s, h->dev, (long long)n, -1);
    MSL_HIP_TRY(hipStreamSynchronize(s));
    map_replaced(h, n);
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_snapshot(msl_sf *h) noexcept {
    try {
    if (!h) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = settle(h);
    if (rc != MSL_OK) return rc;
    const size_t n = live_count(h);
    const long long wide = host_ctr(h, CTR_WIDE);
    h->snapValid = false;   // (until the copies below are complete)
    MSL_HIP_TRY(h->d_snapStore.grow(sizeof(float) * MAP_WORDS * round_cap(n), h->mapStream));
    if (n) {
        rc = copy_store(h->d_snapStore.p, snap_cap(h), h->map.store.p, h->dev.cap, n, wide, nullptr);
        if (rc != MSL_OK) return rc;
    }
    h->snapN = n; h->snapValid = true; h->snapWide = wide;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_restore(msl_sf *h) noexcept {
    try {
    if (!h || !h->snapValid) { set_error("msl_sf_map_restore: no snapshot"); return MSL_ERR_INVALID; }
    h->mirrorValid = false;
    MSL_HIP_TRY(hipSetDevice(h->device));
    const size_t n = h->snapN;
    int rc;
    if (n + (size_t)h->dev.nseeds > h->dev.cap) {   // the map was reallocated smaller than the snapshot (upload of a small map): grow again
        rc = read_ctr(h);
        if (rc != MSL_OK) return rc;
        rc = map_realloc(h, n + n / 4 + 4 * (size_t)h->dev.nseeds, 0);
        if (rc != MSL_OK) return rc;
    }
    const hipStream_t s = h->mapStream;   // ordered after every keyframe enqueued so far; the superpixel stream never touches the map
    if (n) {
        rc = copy_store(h->map.store.p, h->dev.cap, h->d_snapStore.p, snap_cap(h), n, h->snapWide, &s);
        if (rc != MSL_OK) return rc;
    }
    // the restored map has exactly the snapshot's wide-record state: without the flags a later snapshot would skip rgbWide and a restore of THAT
    // one would bring COLD_WIDE records back without their exact ints
    map_launch_set_ctr(s, h->dev, (long long)n, (int)h->snapWide);
    MSL_HIP_TRY(hipGetLastError());
    map_replaced(h, n);
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_size(msl_sf *h, size_t *n_out) noexcept {
    try {
    if (!h || !n_out) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    *n_out = live_count(h);   // (written before the error check: the caller sees it with the error code as well)
    return check_err(h);
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_download(msl_sf *h, msl_surfel *host, size_t cap, size_t *n_out) noexcept {
    try {
    if (!h || !n_out) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    const size_t n = live_count(h);
    *n_out = n;
    if (n > cap || (n && !host)) { set_error("msl_sf_map_download: capacity %zu < map size %zu", cap, n); return MSL_ERR_CAPACITY; }
    if (n) {
        const AosRun all{0, n};
        rc = aos_out(h, n, nullptr, host, &all, 1);
        if (rc != MSL_OK) return rc;
        MSL_HIP_TRY(hipStreamSynchronize(h->mapStream));
    }
    return check_err(h);
    } MSL_ABI_CATCH_INT
}

int msl_sf_map_detach(msl_sf *h, int pose_index, msl_surfel *out, size_t cap, size_t *n_out) noexcept { try {
    return map_select(h, {0, pose_index, true}, out, cap, n_out, "msl_sf_map_detach"); } MSL_ABI_CATCH_INT }
int msl_sf_map_export(msl_sf *h, int min_update_times, msl_surfel *out, size_t cap, size_t *n_out) noexcept { try {
    return map_select(h, {1, min_update_times, false}, out, cap, n_out, "msl_sf_map_export"); } MSL_ABI_CATCH_INT }
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
    const size_t cur = live_count(h);
    if (cur + n + (size_t)h->dev.nseeds > h->dev.cap) {
        rc = map_realloc(h, cur + n + (cur + n) / 4 + 4 * (size_t)h->dev.nseeds, cur);
        if (rc != MSL_OK) return rc;
    }
    rc = aos_in(h, surfels, n, true);
    if (rc != MSL_OK) return rc;
    map_launch_add_ctr(h->mapStream, h->dev, (long long)n);
    MSL_HIP_TRY(hipStreamSynchronize(h->mapStream));
    map_replaced(h, cur + n);
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_sf_last_counters(msl_sf *h, int64_t counters[5]) noexcept {
    try {
    if (!h || !counters) return MSL_ERR_INVALID;
    MSL_HIP_TRY(hipSetDevice(h->device));
    int rc = read_ctr(h);
    if (rc != MSL_OK) return rc;
    const SfCtr order[5] = {CTR_BEFORE, CTR_NEW, CTR_DELETED, CTR_UPDATED, CTR_LIVE};
    for (int i = 0; i < 5; i++) counters[i] = host_ctr(h, order[i]);
    return check_err(h);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
