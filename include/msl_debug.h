/*
 * msl_debug.h -- test / measurement accessors of libmsl.so (NOT part of the drop-in boundary, which is msl.h).
 *
 * Used by tests/ (intermediate stages against the CPU oracle), bench.py (device counters, HIP-event timing of single kernels) and the
 * experiment tools under tools/.  Same conventions as msl.h: extern "C", plain pointers, MSL_OK or a negative msl_status.
 */
#ifndef MSL_DEBUG_H
#define MSL_DEBUG_H

#include "msl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ORB extractor ---- */
/* Debug accessors for the parity tests (host output, synchronous, after an extract call):
 * pyramid level image of frame f (unpadded, tightly packed w*h), its blurred version, and the
 * FAST candidates handed to the quadtree (x,y in level pixel coords, response), in order. */
/* Experiment builds (-DMSL_OCT_STAMPS): n <= 200 64-bit words = (100 MHz device clock, shader clock) pairs the level-0 quadtree workgroup of frame 0
 * parked at its phase boundaries; zeros otherwise. */
MSL_API int msl_orb_debug_stamps(msl_orb *h, uint64_t *out, int n) MSL_NOEXCEPT;
MSL_API int msl_orb_debug_level_size(const msl_orb *h, int level, int *w, int *h_out) MSL_NOEXCEPT;
MSL_API int msl_orb_debug_level(msl_orb *h, int frame, int level, int blurred, uint8_t *out) MSL_NOEXCEPT;
MSL_API int msl_orb_debug_candidates(msl_orb *h, int frame, int level, int32_t *xys /*3 ints each*/,
                                     int cap, int *n_out) MSL_NOEXCEPT;
/* Per-kernel timing with HIP events on the handle's stream.  mode 0 = off, -1 = every kernel,
 * otherwise a bit mask of kernel ids (bit k = time kernel k only, so a timed region can carry a
 * single kernel's events).  msl_orb_profile_read returns accumulated milliseconds and launch
 * counts per kernel since the last enable call. */
#define MSL_ORB_NKERNELS 6
MSL_API int msl_orb_profile_enable(msl_orb *h, int mode) MSL_NOEXCEPT;
MSL_API int msl_orb_profile_read(msl_orb *h, float *ms /*[MSL_ORB_NKERNELS]*/,
                                 int32_t *launches /*[MSL_ORB_NKERNELS]*/) MSL_NOEXCEPT;
MSL_API const char *msl_orb_kernel_name(int k) MSL_NOEXCEPT;

/* ---- surfel fusion ---- */
/* Debug accessors (host output, synchronous): superpixel seeds and the pixel->seed index map
 * as left by the last fuse call. */
MSL_API int msl_sf_debug_seeds(msl_sf *h, msl_seed *out /*(w/8)*(h/8)*/) MSL_NOEXCEPT;
MSL_API int msl_sf_debug_index(msl_sf *h, int32_t *out /*w*h*/) MSL_NOEXCEPT;
/* The handle's 16 device counters after a sync (0: live surfels, 1-4/6: last keyframe's new / deleted / updated / before / after,
 * 5: deferred error code; 8-12: running totals over all keyframes since creation -- new, deleted, updated surfels, keyframes, live
 * surfels before each keyframe; 13: some record keeps wide r, g, b; 14-15: spare). */
MSL_API int msl_sf_debug_ctr(msl_sf *h, int64_t out[16]) MSL_NOEXCEPT;
/* n_words 32-bit words from offset_words of one of the map stage's scratch arrays (which = 0: tail-move sources, 1: deleted-slot list, 2: the screen
 * keys the last k_fuse launch left per sub-block, 3: the wave -> sub-block dealing table, XCD-major; 4: out[0] = the grid that table is a permutation
 * for, 0 if none; 5: out[0], out[1] = keyframes this handle has sent through the classic chain (k_fuse + k_compact) and through deferred windows; host
 * output, synchronous).  Instrumented experiment builds (-DMSL_FUSE_STAMPS=<keyframe>, tools/fuse_stamps.py) park device-clock stamps of
 * k_fuse / k_compact / kb_seed_plane there; otherwise the content is meaningless. */
/* Mean time (us) an event pair carried by a dispatch reports for an EMPTY kernel of `grid` single-wave workgroups on the map stream (n launches):
 * the measurement overhead contained in msl_sf_profile_read's per-kernel times (rocprofv3's kernel durations do not contain it). */
MSL_API int msl_sf_debug_event_overhead(msl_sf *h, int grid, int n, float *mean_us) MSL_NOEXCEPT;
MSL_API int msl_sf_debug_scratch(msl_sf *h, int which, size_t offset_words, uint32_t *out, size_t n_words) MSL_NOEXCEPT;

/* Test hook (host only): mse_out[i] = the MSE ahc::PlaneSeg::Stats::compute (AHCPlaneSeg.hpp:148-183) reports for stats[i], evaluated by the
 * scalar code (lanes = 0) or by the clustering's lock-step SIMD form with `lanes` (2, 4, 8, 16) candidates per group; MSL_ERR_INVALID if the CPU
 * lacks the instruction set that width is built for (4 and 8: AVX2, 16: AVX-512F). */
/* Test hook: 1 if msl_peac_membership_batch / msl_peac_extract_batch would cluster a call of n_frames keyframes on the device, 0 if on the host workers
 * (the automatic rule: more than eight frames per worker this process may use, the worker count being divided by LOCAL_WORLD_SIZE; MSL_PEAC_CLUSTER
 * = host / device overrides).  Frames whose node data does not fit the LDS take the host path regardless. */
MSL_API int msl_debug_peac_cluster_on_device(int n_frames) MSL_NOEXCEPT;
/* Worker threads of the plane extractor's host pool that could NOT be started since the process began (std::system_error from thread creation: the
 * calls went on with fewer workers; the first occurrence also leaves a line in msl_last_error() and on stderr).  0 in a healthy process. */
MSL_API long long msl_debug_peac_thread_shortfall(void) MSL_NOEXCEPT;
MSL_API int msl_debug_peac_mse(const msl_peac_stats *stats, size_t n, int lanes, double *mse_out) MSL_NOEXCEPT;
/* Test hook: the dealing of n_subblocks (a multiple of 8) k_fuse sub-blocks to the eight XCDs by screen key (0 .. 254: mean image row of the
 * sub-block's in-view surfels, >= 255: nothing in view), as k_compact / k_deal build it (msl_sf_compact.hip, deal_subblocks): deal[x * n / 8 + j] = the
 * sub-block wave 8 j + x takes.  Host arrays; synchronous. */
MSL_API int msl_debug_deal(const uint32_t *keys_host, int n_subblocks, uint32_t *deal_host) MSL_NOEXCEPT;
/* Test hook: out[i] = the kernels' division-free evaluation of (double)(x[i]*x[i]) / 100.0 (host arrays). */
MSL_API int msl_debug_div100(const float *x_host, double *out_host, size_t n) MSL_NOEXCEPT;
/* Test hook: out[q] = the strictly sequential (left-to-right) float sum of the first n[q] <= 256 entries of list q (256 floats each) as the superpixel
 * kernels evaluate it -- a rotating chain over 16 lanes (msl_sf_sp_dev.h); huber != 0: entries +-inf stand for the Huber tail's DOUBLE constant
 * +-0.4 (src/SurfelFusion.cpp:494-503).  Host arrays; synchronous. */
MSL_API int msl_debug_chain_sum(const float *x_host, const int32_t *n_host, int lists, int huber, float *out_host) MSL_NOEXCEPT;
/* Test hook: out[i] = the Newton step of the seed update (src/SurfelFusion.cpp:505) for the numerator sumA[i] and inr[i] (0 .. 256) in-band depths as
 * kb_update_seeds evaluates it -- one float division; literal[i] = the reference's expression (float)((double)(-sumA) / ((double)sumB + 10.0)), sumB =
 * (float)(2 inr), evaluated on the device as well.  Host arrays; synchronous. */
MSL_API int msl_debug_newton_delta(const float *sumA_host, const int32_t *inr_host, size_t n, float *out_host, float *literal_host) MSL_NOEXCEPT;
/* Test hook: the FP64 sums over the 16 lanes of a seed group as kb_seed_plane forms them.  Group q holds nvals (4: the Jacobian, 10: the Hessian) values
 * per lane, x[(q nvals + k) 16 + l].  nvals = 4: out[16 q + l] = what lane l holds after the joint reduction (the total of value l >> 2); nvals = 10:
 * out[16 q ..] = the column-major 4x4 matrix (Hessian + 5 I, both triangles) the group's lanes store.  ref[(q nvals + k) 16 + l] = the plain butterfly
 * (row_ror:8, row_ror:4, two quad permutes) of value k as lane l receives it.  Host arrays; synchronous. */
MSL_API int msl_debug_group_sums(const double *x_host, int groups, int nvals, double *out_host, double *ref_host) MSL_NOEXCEPT;

/* The per-hypothesis stage of the last msl_pnp_ransac call on h (host output, synchronous): *n_out = the iterations pair `pair` ran
 * (max(mRansacMaxIts, n_iterations), 0 when N < mRansacMinInliers); for the first min(*n_out, k_cap) of them the double pose compute_pose
 * returned (R [k][9] row-major, t [k][3]), the branch whose reprojection error won (1 / 2 / 3) and CheckInliers' count. */
MSL_API int msl_pnp_debug_hypotheses(msl_match *h, int pair, int k_cap, double *R, double *t, int32_t *branch, int32_t *count,
                                     int32_t *n_out) MSL_NOEXCEPT;

/* One keyline of the last msl_lines_3d call on h (host output, synchronous): counts[5] = the samples kept, the RANSAC iterations run, the
 * rounds of the refit loop, the sample indices of the end points A and B; iterations[64][4] = per iteration the two drawn sample indices,
 * the inlier count (-1 where |B - A| < EPS used the iteration up) and whether it became the record (zeros beyond the iterations run);
 * md[6] = the final m and d of extract3dline_mahdist. */
MSL_API int msl_lines_3d_debug(msl_match *h, int frame, int line, int32_t *counts, int32_t *iterations, double *md) MSL_NOEXCEPT;

/* One (item, neighbour) pair of the last msl_triangulate_new_points call on h (host output, synchronous): pair[12] = the device's F12 (9,
 * row-major), the epipole ex, ey and the baseline (zeros for a pair that was not formed); per idx1 < cap of that call the candidate match
 * BEFORE the rotation cull and the chain -- cand[2 idx1..] = idx2 (-1: none) and its rotation bin, cosines[3 idx1..] = cosParallaxRays,
 * cosParallaxStereo1, cosParallaxStereo2, x3d[4 idx1..] = the homogeneous x3D before the division (zeros unless triangulated). */
MSL_API int msl_debug_triangulate(msl_match *h, int item, int neigh, float *pair, int32_t *cand, float *cosines, float *x3d) MSL_NOEXCEPT;

/* One item of the last msl_fuse_map_points call on h (host output, synchronous), per candidate j < lcap of that call: uvr[3 j..] = u, v
 * (set once the point is not behind the camera) and ur (set once the projection is inside the image); level_n[2 j..] = nPredictedLevel
 * and vIndices.size() (set once the view-angle test passed).  Zeros where the candidate left earlier. */
MSL_API int msl_debug_fuse(msl_match *h, int item, float *uvr, int32_t *level_n) MSL_NOEXCEPT;

/* One item of the last msl_fuse_map_lines call on h (host output, synchronous), per candidate j < lcap of that call: uvr[5 j..] = u1, v1,
 * u2, v2 (set once both end points are inside the image) and radius (set once the view-angle test passed); level_n[2 j..] =
 * nPredictedLevel (not clamped) and vIndices.size() (set with the radius).  Zeros where the candidate left earlier. */
MSL_API int msl_debug_line_fuse(msl_match *h, int item, float *uvr, int32_t *level_n) MSL_NOEXCEPT;

/* The scratch budget of msl_local_points / msl_local_lines on h, in bytes (default 256 MiB): the frames of a call run in groups of
 * max(1, bytes / (4 * n_pts)) (n_lines for the line entry), one 32-bit stamp per (frame of the group, table row).  A test sets it low to cross a group
 * boundary with a small table; the results do not depend on it.  At least 4. */
MSL_API int msl_debug_local_map_budget(msl_match *h, size_t bytes) MSL_NOEXCEPT;

#define MSL_SF_NKERNELS 12
MSL_API int msl_sf_profile_enable(msl_sf *h, int mode) MSL_NOEXCEPT;
/* Sampling for the per-dispatch event pairs: only every stride-th launch of a timed kernel carries events (default 1 = every launch).  A
 * dispatch that carries events costs the stream ~0.3 us; bench.py times every 5th k_fuse launch of its timed region (a stride coprime with the
 * 32 keyframes of a call, so that every position of the chain is sampled equally). */
MSL_API int msl_sf_profile_stride(msl_sf *h, int stride) MSL_NOEXCEPT;
MSL_API int msl_sf_profile_read(msl_sf *h, float *ms, int32_t *launches) MSL_NOEXCEPT;
MSL_API const char *msl_sf_kernel_name(int k) MSL_NOEXCEPT;

/* Test hook of the C ABI's exception barrier: raises a failure inside the library (0: std::bad_alloc, 1: std::runtime_error, 2: a non-standard
 * exception, 3: std::bad_alloc in a worker thread of the plane extractor's pool) and returns what the boundary makes of it: MSL_ERR_NOMEM /
 * MSL_ERR_INTERNAL with msl_last_error() set; never an abort.  No device needed. */
MSL_API int msl_debug_throw(int kind) MSL_NOEXCEPT;

#ifdef __cplusplus
}
#endif
#endif /* MSL_DEBUG_H */
