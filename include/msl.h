/*
 * msl.h -- C ABI of the MI355X-native RGB-D front end (ORB extractor + surfel fusion).
 *
 * This is the drop-in boundary for ManhattanSLAM's two hot-path classes.  The reference has no
 * FFI layer; the interfaces replaced are C++ class members, cited per entry point below
 * (paths relative to the reference repository):
 *
 *   ORB_SLAM2::ORBextractor::ORBextractor(...)        include/ORBextractor.h:46-47, src/ORBextractor.cc:412-468
 *   ORB_SLAM2::ORBextractor::operator()(...)          include/ORBextractor.h:54-56, src/ORBextractor.cc:813-870
 *   ORB_SLAM2::ORBextractor::Get*Scale*()             include/ORBextractor.h:58-80
 *   SurfelFusion::SurfelFusion(...)                   include/SurfelFusion.h:127-129, src/SurfelFusion.cpp:29-38
 *   SurfelFusion::fuseInitializeMap(...)              include/SurfelFusion.h:131-138, src/SurfelFusion.cpp:40-73
 *   ORB_SLAM2::SurfelMapping::fuseMap(...)            src/SurfelMapping.cpp:353-392   (slot refill / tail compaction)
 *
 * All entry points are extern "C", take plain pointers and sizes, never throw, and return
 * MSL_OK (0) or a negative msl_status; msl_last_error() gives a thread-local message.
 * Every handle owns its HIP stream and scratch; a handle is used by one thread at a time
 * (same rule as the reference objects) but the calling thread may change between calls
 * (src/Frame.cc:100 spawns a fresh std::thread per frame) -- the device is re-bound on entry.
 *
 * There is NO CPU fallback: creation fails with MSL_ERR_NO_DEVICE when no gfx950 device is
 * usable.  The CPU oracle under oracle/ is test infrastructure and is not linked here.
 *
 * This header is the drop-in surface only.  The accessors the parity tests and bench.py use to look inside a handle (intermediate
 * stages, device counters, per-kernel HIP-event timing) are declared in msl_debug.h: exported by the same library, not part of the
 * boundary a maintainer of the reference binds.
 */
#ifndef MSL_H
#define MSL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSL_API __attribute__((visibility("default")))
/* No exception ever crosses this boundary: every entry point is noexcept and turns a failure inside the library (std::bad_alloc, a failed
 * thread spawn, ...) into a status code ("all noexcept, int return"). */
#ifdef __cplusplus
#define MSL_NOEXCEPT noexcept
#else
#define MSL_NOEXCEPT
#endif

typedef enum msl_status {
    MSL_OK = 0,
    MSL_ERR_INVALID = -1,      /* bad argument / unsupported geometry            */
    MSL_ERR_NO_DEVICE = -2,    /* no usable HIP device (no CPU fallback exists)  */
    MSL_ERR_HIP = -3,          /* a HIP runtime call failed                      */
    MSL_ERR_CAPACITY = -4,     /* caller-provided output capacity too small      */
    MSL_ERR_OVERFLOW = -5,     /* an internal device-side bound was exceeded     */
    MSL_ERR_NOMEM = -6,        /* host memory exhausted inside the library       */
    MSL_ERR_INTERNAL = -7      /* any other exception caught at the boundary     */
} msl_status;

typedef enum msl_mem {
    MSL_MEM_HOST = 0,          /* pointer is ordinary host memory                */
    MSL_MEM_DEVICE = 1         /* pointer is device memory on the handle's GPU   */
} msl_mem;

/* Same layout as cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id. */
typedef struct msl_keypoint {
    float x, y;
    float size;
    float angle;      /* degrees, [0,360) */
    float response;   /* FAST-9/16 corner score */
    int32_t octave;
    int32_t class_id; /* always -1 */
} msl_keypoint;

/* Same layout as the reference `struct Surfel` (include/Surfel.h:28-37), 56 bytes. */
typedef struct msl_surfel {
    float px, py, pz;
    float nx, ny, nz;
    float size;
    float color;
    int32_t r, g, b;
    float weight;
    int32_t updateTimes;
    int32_t lastUpdate;
} msl_surfel;

/* Same layout as SurfelFusion::SuperpixelSeed (include/SurfelFusion.h:46-58), 64 bytes.
 * Only used by the debug accessors of msl_debug.h that let the parity tests look at intermediate stages. */
typedef struct msl_seed {
    float x, y;
    float size;
    float normX, normY, normZ;
    float posX, posY, posZ;
    float viewCos;
    float meanDepth;
    float meanIntensity;
    int32_t r, g, b;
    uint8_t fused, stable, use, _pad;
} msl_seed;

MSL_API const char *msl_last_error(void) MSL_NOEXCEPT;
MSL_API const char *msl_version(void) MSL_NOEXCEPT;
/* Number of usable gfx950 devices (0 if none / HIP unavailable). */
MSL_API int msl_device_count(void) MSL_NOEXCEPT;

/* ------------------------------------------------------------------------------------------
 * ORB extractor
 * ---------------------------------------------------------------------------------------- */
typedef struct msl_orb msl_orb;

/* Replaces ORBextractor::ORBextractor (src/ORBextractor.cc:412-468).  max_width/max_height bound
 * the frame size, max_batch the number of frames one msl_orb_extract_batch call may carry. */
MSL_API msl_orb *msl_orb_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
                                int minThFAST, int max_width, int max_height, int max_batch,
                                int device) MSL_NOEXCEPT;
MSL_API void msl_orb_destroy(msl_orb *h) MSL_NOEXCEPT;

/* Scale tables of include/ORBextractor.h:58-80; each out array holds nlevels floats (NULL = skip). */
MSL_API int msl_orb_scale_tables(const msl_orb *h, float *scaleFactors, float *invScaleFactors,
                                 float *levelSigma2, float *invLevelSigma2) MSL_NOEXCEPT;
/* mnFeaturesPerLevel (src/ORBextractor.cc:433-445). */
MSL_API int msl_orb_features_per_level(const msl_orb *h, int32_t *out) MSL_NOEXCEPT;
/* Upper bound on keypoints per frame: nfeatures + 2*nlevels (the one-by-one phase of DistributeOctTree overshoots a level's quota by at most 2,
 * src/ORBextractor.cc:691-696); for frames at least ~4 times as wide as high with a small budget the first quadtree round alone returns up to
 * 4 * round(width / height) nodes per level (:536-552, 575-640), and the capacity of an extractor created for such a frame size includes them. */
MSL_API int msl_orb_capacity(const msl_orb *h) MSL_NOEXCEPT;
MSL_API int msl_orb_levels(const msl_orb *h) MSL_NOEXCEPT;

/* Replaces ORBextractor::operator() (src/ORBextractor.cc:813-870) for one CV_8UC1 frame held in
 * host memory.  stride is in bytes.  On return *n_out keypoints (level order 0..L-1, in-level
 * order = quadtree list order) and n_out*32 descriptor bytes are in the caller's host buffers.
 * An empty image (width==0||height==0||gray==NULL) returns MSL_OK with *n_out = 0 (:815-816). */
MSL_API int msl_orb_extract(msl_orb *h, const uint8_t *gray, int width, int height, size_t stride,
                            msl_keypoint *kps, uint8_t *desc32, int cap, int *n_out) MSL_NOEXCEPT;

/* Frame-batched variant (throughput path).  Frame f starts at gray + f*frame_stride.  Outputs for
 * frame f are written at kps + f*cap, desc32 + f*cap*32, n_out[f].  in_mem/out_mem say whether
 * the input / the three output pointers are host or device memory.  With device outputs the
 * call is asynchronous on the handle's stream: use msl_orb_sync() before reading. */
/* The extractor's stream waits for a hipEvent_t (e.g. the one msl_sf_staged_gray returns) before anything enqueued after this call. */
MSL_API int msl_orb_wait_event(msl_orb *h, void *hip_event) MSL_NOEXCEPT;
MSL_API int msl_orb_extract_batch(msl_orb *h, const uint8_t *gray, int n_frames, int width,
                                  int height, size_t row_stride, size_t frame_stride,
                                  msl_mem in_mem, msl_keypoint *kps, uint8_t *desc32, int cap,
                                  int32_t *n_out, msl_mem out_mem) MSL_NOEXCEPT;
/* ---- widening, SURVEY.md 8(f) rank 1: the Frame steps that consume the ORB output right after the join
 * (src/Frame.cc:107-153): UndistortKeyPoints (:437-463), ComputeStereoFromRGBD (:495-513), AssignFeaturesToGrid
 * (:155-168, PosInGrid :418-427), fused behind the extraction so the keypoints never leave HBM in between. ---- */
typedef struct msl_frame_params {
    float fx, fy, cx, cy;          /* mK (CV_32F) */
    float k1, k2, p1, p2, k3;      /* mDistCoef; k1 == 0 => mvKeysUn = mvKeys (src/Frame.cc:438-441) */
    float bf;                      /* mbf */
    float minX, maxX, minY, maxY;  /* mnMinX.. (ComputeImageBounds, src/Frame.cc:465-494): see msl_frame_image_bounds */
} msl_frame_params;
#define MSL_FRAME_GRID_ROWS 48     /* include/Frame.h:53-54 */
#define MSL_FRAME_GRID_COLS 64
/* ComputeImageBounds: fills minX..maxY from fx..k3 and the image size (host arithmetic only). */
MSL_API int msl_frame_image_bounds(msl_frame_params *p, int width, int height) MSL_NOEXCEPT;
/* msl_orb_extract_batch plus, per keypoint i of frame f (outputs at index f*cap + i, same memory space as kps):
 *   kps_un_xy[2i..2i+1] = mvKeysUn[i].pt      depth_out[i] = mvDepth[i] (-1 if the depth pixel is <= 0)
 *   uright_out[i] = mvuRight[i]               grid_cell[i] = posX * 48 + posY of mGrid[posX][posY], or -1 (PosInGrid false)
 * depth: CV_32FC1 metres (imDepthScaled), strides in bytes. */
MSL_API int msl_orb_extract_frame_batch(msl_orb *h, const uint8_t *gray, const float *depth, int n_frames, int width, int height,
                                        size_t gray_row_stride, size_t gray_frame_stride, size_t depth_row_stride,
                                        size_t depth_frame_stride, msl_mem in_mem, const msl_frame_params *params,
                                        msl_keypoint *kps, uint8_t *desc32, float *kps_un_xy, float *depth_out, float *uright_out,
                                        int32_t *grid_cell, int cap, int32_t *n_out, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_orb_sync(msl_orb *h) MSL_NOEXCEPT;
/* Use an externally owned hipStream_t (e.g. torch's current stream) instead of the handle's own. */
MSL_API int msl_orb_set_stream(msl_orb *h, void *hip_stream) MSL_NOEXCEPT;


/* ------------------------------------------------------------------------------------------
 * Surfel fusion
 * ---------------------------------------------------------------------------------------- */
typedef struct msl_sf msl_sf;

/* Replaces SurfelFusion::SurfelFusion (src/SurfelFusion.cpp:29-38).  Any width, height >= 16: like the reference, the superpixel lattice is
 * (width / 8) x (height / 8), truncated; the pixels right of / below the last whole cell still take part in every per-pixel step. */
MSL_API msl_sf *msl_sf_create(int width, int height, float fx, float fy, float cx, float cy,
                              float fuseFar, float fuseNear, int device) MSL_NOEXCEPT;
MSL_API void msl_sf_destroy(msl_sf *h) MSL_NOEXCEPT;

/* Host-vector mode == SurfelFusion::fuseInitializeMap (src/SurfelFusion.cpp:40-73).
 * gray: CV_8UC1 w*h; depth: CV_32FC1 metres; member: CV_32SC1 ceil(w/2)*ceil(h/2), -1 = no plane; strides
 * in bytes; pose = Twc as column-major 4x4 (Eigen::Matrix4f storage).  `local` (n_local surfels)
 * is updated in place; new surfels are written to new_out (<= (w/8)*(h/8)), count in *n_new. */
MSL_API int msl_sf_fuse(msl_sf *h, int referenceFrameIndex, const uint8_t *gray, size_t gray_stride,
                        const float *depth, size_t depth_stride, const int32_t *member,
                        size_t member_stride, const float pose_colmajor[16], msl_surfel *local,
                        size_t n_local, msl_surfel *new_out, size_t new_cap, size_t *n_new) MSL_NOEXCEPT;

/* The same with hints.  MSL_SF_LOCAL_UNCHANGED: local[0 .. n_local) is byte for byte what the previous msl_sf_fuse / msl_sf_fuse_ex call on this
 * handle left there (a caller that keeps the new surfels in a list of their own, or that has not run SurfelMapping::fuseMap's refill yet); the
 * library then fuses into the device copy of that call instead of uploading 56 bytes per surfel again.  The hint is ignored -- a full upload
 * happens -- when the length differs or any other map operation touched the handle in between.  Both forms send back only the stretches of
 * `local` that hold surfels this keyframe updated or deleted (per 256-surfel sub-block), not the whole vector. */
#define MSL_SF_LOCAL_UNCHANGED 1u
MSL_API int msl_sf_fuse_ex(msl_sf *h, int referenceFrameIndex, const uint8_t *gray, size_t gray_stride,
                           const float *depth, size_t depth_stride, const int32_t *member,
                           size_t member_stride, const float pose_colmajor[16], msl_surfel *local,
                           size_t n_local, msl_surfel *new_out, size_t new_cap, size_t *n_new, unsigned flags) MSL_NOEXCEPT;

/* Device-resident map mode: the live surfel map stays in HBM between keyframes. */
MSL_API int msl_sf_map_reserve(msl_sf *h, size_t capacity) MSL_NOEXCEPT;
MSL_API int msl_sf_map_upload(msl_sf *h, const msl_surfel *host, size_t n) MSL_NOEXCEPT;
MSL_API int msl_sf_map_download(msl_sf *h, msl_surfel *host, size_t cap, size_t *n_out) MSL_NOEXCEPT;
MSL_API int msl_sf_map_size(msl_sf *h, size_t *n_out) MSL_NOEXCEPT;
/* Replay support (bench.py's stationary sequence, tests): msl_sf_map_snapshot keeps a device-side copy of the resident map and its
 * live count (synchronous); msl_sf_map_restore puts that copy back, asynchronously on the map stream, ordered after every keyframe
 * enqueued so far -- a device-to-device copy of the records, no host traffic.  (No reference counterpart: Tracking::Reset does not
 * touch the surfel vectors, SURVEY.md App. D.) */
MSL_API int msl_sf_map_snapshot(msl_sf *h) MSL_NOEXCEPT;
MSL_API int msl_sf_map_restore(msl_sf *h) MSL_NOEXCEPT;

/* fuseInitializeMap + the SurfelMapping::fuseMap slot refill / tail compaction
 * (src/SurfelMapping.cpp:353-392) on the resident map.  Image pointers may be host or device
 * (img_mem).  Asynchronous on the handle's streams: only argument errors are reported by the call itself;
 * device-side errors are DEFERRED to the next msl_sf_sync / map_size / download / detach / append / export
 * / last_counters, which return MSL_ERR_OVERFLOW once.  The resident map grows on demand (like the
 * reference's std::vector): when the host-side upper bound of the live count reaches the capacity the call
 * syncs once and reallocates; msl_sf_map_reserve avoids that pause.  msl_sf_last_counters gives
 * {n_live_before, n_new, n_deleted, n_updated, n_live_after} of the last keyframe. */
MSL_API int msl_sf_fuse_resident(msl_sf *h, int referenceFrameIndex, const uint8_t *gray,
                                 size_t gray_stride, const float *depth, size_t depth_stride,
                                 const int32_t *member, size_t member_stride, msl_mem img_mem,
                                 const float pose_colmajor[16]) MSL_NOEXCEPT;
/* ---- widening, SURVEY.md 8(f) rank 4: map maintenance on the resident map (so SurfelMapping::moveAddSurfels and Stop() need
 * no full download/upload).  All three are synchronous and keep the reference's element order. ----
 * msl_sf_map_detach: the inner loop of moveAddSurfels (src/SurfelMapping.cpp:207-224) for one leaving pose: every live surfel
 *   (updateTimes > 0) whose lastUpdate == pose_index is copied, in map order, to `out` (host) and marked deleted in the map
 *   (updateTimes = 0).  *n_out = number found; MSL_ERR_CAPACITY (nothing modified) if it exceeds cap.
 * msl_sf_map_append: mvLocalSurfels.insert(end, ...) of re-entering poses (src/SurfelMapping.cpp:291-296).
 * msl_sf_map_export: the local-surfel filter of SurfelMapping::Stop (src/SurfelMapping.cpp:67-84): surfels with
 *   updateTimes >= min_update_times, in map order. */
MSL_API int msl_sf_map_detach(msl_sf *h, int pose_index, msl_surfel *out, size_t cap, size_t *n_out) MSL_NOEXCEPT;
MSL_API int msl_sf_map_append(msl_sf *h, const msl_surfel *surfels, size_t n) MSL_NOEXCEPT;
MSL_API int msl_sf_map_export(msl_sf *h, int min_update_times, msl_surfel *out, size_t cap, size_t *n_out) MSL_NOEXCEPT;
/* System::saveSurfels (src/System.cc:296-382) on the cloud of SurfelMapping::Stop (src/SurfelMapping.cpp:62-104): msl_sf_map_export(min_update_times)
 * followed by the caller's inactive surfels, written as the reference's ASCII PLY (vertex: x y z nx ny nz red green blue alpha quality radius; one
 * camera element).  (The map-plane points Stop() appends are Map data outside this library; pass them through `inactive` if wanted.) */
MSL_API int msl_sf_export_ply(msl_sf *h, int min_update_times, const msl_surfel *inactive, size_t n_inactive, const char *path) MSL_NOEXCEPT;

/* ---- widening, SURVEY.md 8(f) rank 2: the data-parallel front of the PEAC plane extractor (producer of membershipImg) ----
 * msl_peac_block_stats: for n_frames raw 16-bit depth images
 *   (a) the organised half-resolution point cloud of PlaneDetection::readDepthImage (src/PlaneExtractor.cpp:44-76):
 *       vertex (i/2, j/2) = (((double)j - cx) * z / fx, ((double)i - cy) * z / fy, z), z = (double)depth(i, j) * depthMapFactor,
 *       for even i, j; cloud_out[frame][(h/2... ceil) * (w/2 ... ceil)][3] doubles (may be NULL);
 *   (b) the initial node of every window_w x window_h block, i.e. the body of ahc::PlaneSeg::PlaneSeg
 *       (include/peac/AHCPlaneSeg.hpp:237-285) as ahc::PlaneFitter::initGraph calls it (include/peac/AHCPlaneFitter.hpp:756-776):
 *       points with z == 0 are missing data (include/PlaneExtractor.h:47-55), a block with missing data (INIT_STRICT; more
 *       than half missing for init_loose != 0) or a depth discontinuity |z - z_nb| > depth_alpha * |z| + depth_change_tol
 *       towards the right / lower neighbour (AHCPlaneSeg.hpp:41-43, AHCParamSet.hpp:140-142) is rejected (nouse = 1, N = 0,
 *       sums 0); otherwise the nine FP64 sums of ahc::PlaneSeg::Stats::push (AHCPlaneSeg.hpp:81-92) in window raster order.
 *       stats_out[frame][(H / window_h) * (W / window_w)], H = ceil(height / 2), W = ceil(width / 2), block (i, j) at i * Nw + j.
 * The PCA plane fit of each block (a 3x3 symmetric eigen-solve through Eigen), the graph and the agglomerative clustering stay
 * host code.  Synchronous; depth / outputs in host or device memory as `mem` / `out_mem` say. */
typedef struct msl_peac_stats {
    double sx, sy, sz, sxx, syy, szz, sxy, syz, sxz;   /* ahc::PlaneSeg::Stats (AHCPlaneSeg.hpp:59-63) */
    int32_t N;
    int32_t nouse;
} msl_peac_stats;
MSL_API int msl_peac_block_stats(int device, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width, int height,
                                 int n_frames, msl_mem mem, float fx, float fy, float cx, float cy, float depth_map_factor, int window_w,
                                 int window_h, double depth_alpha, double depth_change_tol, int init_loose, double *cloud_out,
                                 msl_peac_stats *stats_out, msl_mem out_mem) MSL_NOEXCEPT;

/* The rest of the plane extractor: the producer of SurfelFusion's inputPlaneMembershipImg (BASELINE config 4).
 * msl_peac_params = the members of ahc::PlaneFitter (include/peac/AHCPlaneFitter.hpp:122-131, 157-161) and ahc::ParamSet
 * (include/peac/AHCParamSet.hpp:36-76); msl_peac_default_params fills the reference's defaults (PlaneDetection overrides none).
 * msl_peac_block = the initial graph node of one window: its Stats plus the PCA plane fit of ahc::PlaneSeg::Stats::compute
 * (AHCPlaneSeg.hpp:148-183: centre of mass, unit normal towards the camera, MSE, curvature; NaN MSE / curvature for N < 4), the
 * 3x3 symmetric eigen-solve being LA::eig33sym = Eigen::SelfAdjointEigenSolver<Matrix3d> (include/peac/eig33sym.hpp:71-75).
 * msl_peac_block_fit: cloud + block statistics + PCA on the GPU (one wave per window, FP64, the reference's summation order).
 * msl_peac_membership_batch: PlaneDetection::readDepthImage + runPlaneDetection (src/PlaneExtractor.cpp:44-81) for n_frames
 *   depth images: block fit on the GPU; graph initialisation (AHCPlaneFitter.hpp:756-928) on the host; agglomerative clustering (:939-1143)
 *   on the GPU, one wave per frame, for calls of more than about three frames per usable CPU (on the host workers for smaller calls -- a lone
 *   frame is clustered faster by one core --, if a frame's node data does not fit the LDS, or as MSL_PEAC_CLUSTER=host / device says); block
 *   erosion (:490-596), region growing (:422-471) and the final merge / relabelling (:296-372) on the host (order-dependent pixel work: a
 *   FIFO flood fill), one frame per worker thread at a time (as many workers as the process may use CPUs: affinity mask and cgroup quota,
 *   at most 64).  Device-resident input must be complete, or enqueued on the legacy default stream, when the call is made.
 *   membership_out (HOST, [n_frames][ceil(h/2)][ceil(w/2)]) = plane_filter.membershipImg as SurfelMapping receives it
 *   (src/Tracking.cc:228): plane id >= 0, -1 = no plane, and -- exactly like the reference -- the region-growing visit counters
 *   -2..-6 on pixels that were tried and rejected.  n_planes_out (HOST, may be NULL) = extractedPlanes.size() per frame. */
typedef struct msl_peac_block {
    msl_peac_stats stats;
    double center[3], normal[3], mse, curvature;
} msl_peac_block;
typedef struct msl_peac_params {
    int32_t window_w, window_h;       /* windowWidth, windowHeight (10, 10) */
    int32_t min_support;              /* minSupport (3000) */
    int32_t max_step;                 /* maxStep (100000) */
    int32_t do_refine;                /* doRefine (true) */
    int32_t erode_type;               /* ErodeType: 0 none, 1 segment borders, 2 all borders (ERODE_ALL_BORDER) */
    int32_t init_loose;               /* initType == INIT_LOOSE (INIT_STRICT) */
    int32_t _pad;
    double depth_sigma, std_tol_init, std_tol_merge;              /* depthSigma, stdTol_init, stdTol_merge */
    double z_near, z_far, angle_near, angle_far;                  /* T_ang(P_INIT) */
    double similarity_th_merge, similarity_th_refine;             /* cos 60 deg, cos 30 deg */
    double depth_alpha, depth_change_tol;                         /* T_dz */
} msl_peac_params;
MSL_API void msl_peac_default_params(msl_peac_params *p) MSL_NOEXCEPT;
MSL_API int msl_peac_block_fit(int device, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width, int height,
                               int n_frames, msl_mem mem, float fx, float fy, float cx, float cy, float depth_map_factor,
                               const msl_peac_params *params, msl_peac_block *blocks_out, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_peac_membership_batch(int device, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width,
                                      int height, int n_frames, msl_mem mem, float fx, float fy, float cx, float cy, float depth_map_factor,
                                      const msl_peac_params *params, int32_t *membership_out, int32_t *n_planes_out) MSL_NOEXCEPT;
/* The host stage of msl_peac_membership_batch alone (graph initialisation, clustering, erosion, region growing; persistent worker threads, one
 * frame per thread at a time), on block fits the caller already has (blocks: HOST, [n_frames][Nh * Nw] as msl_peac_block_fit returns them) and the
 * HOST depth images they came from.  No device is touched: this is the part of the extractor that is sequential by construction. */
MSL_API int msl_peac_membership_from_blocks(const msl_peac_block *blocks, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes,
                                            int width, int height, int n_frames, float fx, float fy, float cx, float cy, float depth_map_factor,
                                            const msl_peac_params *params, int32_t *membership_out, int32_t *n_planes_out) MSL_NOEXCEPT;
/* Everything the reference's PlaneDetection hands on after runPlaneDetection (include/PlaneExtractor.h:57-62, src/PlaneExtractor.cpp:77-80):
 * msl_peac_membership_batch's outputs plus, per frame,
 *   planes_out         HOST [n_frames][max_planes]      plane_filter.extractedPlanes[i]: normal, centre, MSE, N (src/Frame.cc:626-632 reads them);
 *                                                       the call fails with MSL_ERR_CAPACITY if a frame has more than max_planes planes
 *   vertex_offsets_out HOST [n_frames][max_planes + 1]  plane_vertices_[i] = vertex_indices_out[f][offsets[i] .. offsets[i + 1])
 *   vertex_indices_out HOST [n_frames][ceil(h/2) * ceil(w/2)]  cloud vertex indices of every plane, raster order inside a plane (the pMembership
 *                                                       argument of PlaneFitter::run, AHCPlaneFitter.hpp:341-361); needs params->do_refine
 *   cloud_out          HOST [n_frames][ceil(h/2) * ceil(w/2)][3] doubles or NULL: PlaneDetection::cloud.vertices, the organised cloud of
 *                                                       readDepthImage (src/PlaneExtractor.cpp:60-74) as the device computed it for the block fit
 * Host worker threads: as many as the process may use CPUs (affinity mask, cgroup quota), divided by LOCAL_WORLD_SIZE when one process per GPU
 * shares the node (torch.distributed.run sets it); MSL_PEAC_THREADS overrides.
 * msl_peac_extract_from_blocks: the same from block fits the caller already has (host stage only, no device). */
typedef struct msl_peac_plane { double normal[3], center[3], mse; int32_t N, _pad; } msl_peac_plane;
MSL_API int msl_peac_extract_batch(int device, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes, int width, int height,
                                   int n_frames, msl_mem mem, float fx, float fy, float cx, float cy, float depth_map_factor,
                                   const msl_peac_params *params, int32_t *membership_out, int32_t *n_planes_out, int max_planes,
                                   msl_peac_plane *planes_out, int32_t *vertex_offsets_out, int32_t *vertex_indices_out, double *cloud_out) MSL_NOEXCEPT;
MSL_API int msl_peac_extract_from_blocks(const msl_peac_block *blocks, const uint16_t *depth, size_t depth_stride_bytes, size_t frame_stride_bytes,
                                         int width, int height, int n_frames, float fx, float fy, float cx, float cy, float depth_map_factor,
                                         const msl_peac_params *params, int32_t *membership_out, int32_t *n_planes_out, int max_planes,
                                         msl_peac_plane *planes_out, int32_t *vertex_offsets_out, int32_t *vertex_indices_out) MSL_NOEXCEPT;

/* ---- widening, SURVEY.md 8(f) rank 3: Hamming matching by projection, the next consumer of the ORB descriptors ----
 * msl_match_by_projection_batch: n_pairs independent calls of
 *     int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th)   (src/ORBmatcher.cc:547-678)
 * with Frame::GetFeaturesInArea (src/Frame.cc:332-381), ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:835-849) and the rotation
 * histogram / ComputeThreeMaxima (:799-830), for an ORBmatcher with mbCheckOrientation = check_orientation.
 * All per-keypoint arrays hold `cap` entries per pair (pair f at index f * cap); the current-frame arrays are exactly the
 * outputs of msl_orb_extract_frame_batch (mvKeys for octave / angle, mvKeysUn.pt, mvuRight, grid cell, descriptors), so in a
 * batched pipeline they never leave HBM.  Last frame, per keypoint i < n_last[f]:
 *   last_xyz[3 i..]  LastFrame.mvpMapPoints[i]->GetWorldPos()          last_desc[32 i..]  ->GetDescriptor()
 *   last_flags[i]    bit 0: mvpMapPoints[i] != NULL && !mvbOutlier[i]; bit 1: ->Observations() > 0
 *   last_octave[i]   LastFrame.mvKeys[i].octave                        last_angle[i]      LastFrame.mvKeysUn[i].angle
 *                    (a last_octave outside [0, nlevels) finds no candidates: that point matches nothing)
 * Tcw_cur / Tcw_last: rows 0-2 of the CV_32F 4x4 mTcw of the two frames, row-major (12 floats per pair).
 * CurrentFrame.mvpMapPoints is all NULL on entry (src/Tracking.cc:1252); on return match_out[f * cap + i2] is the index i of the
 * last-frame keypoint whose MapPoint current keypoint i2 holds, or -1 (NULL); nmatches[f] is the function's return value.
 * The greedy, order-dependent assignment of the reference (a candidate already held by a point with Observations() > 0 is
 * skipped, later points overwrite earlier ones) is reproduced exactly.  Limits: cap <= 8192, nlevels <= MSL_MATCH_MAX_LEVELS.
 * `mem` / `out_mem` say where the input / the two output arrays live. */
#define MSL_MATCH_MAX_LEVELS 16
typedef struct msl_match_params {
    float fx, fy, cx, cy;             /* CurrentFrame.fx .. cy */
    float bf;                         /* mbf; mb = mbf / fx (src/Frame.cc:150) */
    float minX, maxX, minY, maxY;     /* mnMinX .. (msl_frame_image_bounds) */
    float th;                         /* search window: radius = th * mvScaleFactors[octave] */
    int32_t check_orientation;        /* ORBmatcher::mbCheckOrientation */
    int32_t nlevels;
    float scale_factors[MSL_MATCH_MAX_LEVELS];   /* CurrentFrame.mvScaleFactors (msl_orb_scale_tables) */
} msl_match_params;
/* One matcher handle = one ORBmatcher object of the reference (src/ORBmatcher.cc:41): its own HIP stream and its own grow-only scratch and staging
 * buffers, used by one thread at a time, device re-bound at every entry.  msl_match_by_projection is asynchronous on the handle's stream when inputs
 * AND outputs are device memory (msl_match_sync / msl_match_set_stream as for the other handles); with host memory on either side it returns when the
 * caller's buffers are its own again.
 * Every entry point on the handle checks its arguments before it touches a device: an int argument outside its limits, a required array
 * that is NULL or a params field outside its range is refused with MSL_ERR_INVALID, msl_last_error() names it ("msl_match_local_points:
 * mcap 32769 outside 1 .. 32768", "msl_pose_optimize: Tcw is NULL", "msl_match_by_projection: fx is 0"), nothing is launched and no output
 * byte is written.  The _batch forms refuse before the device's shared handle is created, so also on a machine without a device.  (The
 * Tracking entries -- the searches, the pose optimisers, the bag-of-words calls, the relocalisation calls, msl_pnp_ransac, msl_lines_3d --
 * used to answer one "invalid argument (cap <= 8192, ...)" for all of these; the calls they accept are the same as then.) */
typedef struct msl_match msl_match;
MSL_API msl_match *msl_match_create(int device) MSL_NOEXCEPT;
MSL_API void msl_match_destroy(msl_match *h) MSL_NOEXCEPT;
MSL_API int msl_match_sync(msl_match *h) MSL_NOEXCEPT;
MSL_API int msl_match_set_stream(msl_match *h, void *hip_stream) MSL_NOEXCEPT;
MSL_API int msl_match_by_projection(msl_match *h, int n_pairs, int cap, const msl_match_params *params,
                                    const msl_keypoint *cur_kps, const float *cur_un_xy, const float *cur_uright,
                                    const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur,
                                    const float *last_xyz, const uint8_t *last_desc, const uint8_t *last_flags,
                                    const int32_t *last_octave, const float *last_angle, const int32_t *n_last,
                                    const float *Tcw_cur, const float *Tcw_last, msl_mem mem, int32_t *match_out,
                                    int32_t *nmatches, msl_mem out_mem) MSL_NOEXCEPT;
/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:835-849) for n descriptor pairs (host arrays, synchronous; parity hook for the popcount path). */
MSL_API int msl_match_descriptor_distances(msl_match *h, const uint8_t *a32, const uint8_t *b32, int n, int32_t *dist_out) MSL_NOEXCEPT;
/* Device-indexed convenience forms of the two calls above: a lazily created handle per device shared by all callers (serialised), always
 * synchronous; device-resident inputs must be complete, or enqueued on the legacy default stream, when the call is made. */
MSL_API int msl_match_by_projection_batch(int device, int n_pairs, int cap, const msl_match_params *params,
                                          const msl_keypoint *cur_kps, const float *cur_un_xy, const float *cur_uright,
                                          const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur,
                                          const float *last_xyz, const uint8_t *last_desc, const uint8_t *last_flags,
                                          const int32_t *last_octave, const float *last_angle, const int32_t *n_last,
                                          const float *Tcw_cur, const float *Tcw_last, msl_mem mem, int32_t *match_out,
                                          int32_t *nmatches, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_match_descriptor_distance(int device, const uint8_t *a32, const uint8_t *b32, int n, int32_t *dist_out) MSL_NOEXCEPT;

/* ---- Matching the local map: Tracking::SearchLocalPoints (src/Tracking.cc:1654-1695) after its first loop ----
 * n_frames independent calls of the visibility loop -- Frame::isInFrustum(pMP, view_cos_limit) (src/Frame.cc:204-259) with
 * MapPoint::PredictScale (src/MapPoint.cc:350-364) for every candidate local map point -- followed by
 *     int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th)   (src/ORBmatcher.cc:40-117)
 * for an ORBmatcher(nn_ratio), with RadiusByViewingCos (:119-124) and Frame::GetFeaturesInArea (src/Frame.cc:332-381).
 * Current frame: exactly the msl_match_by_projection current-frame arrays (`cap` entries per frame), plus
 *   cur_flags[i]     state of F.mvpMapPoints[i] after SearchLocalPoints' first loop (bad points NULLed):
 *                    bit 0: != NULL, bit 1: its Observations() > 0.  A keypoint with both bits is never handed out; one held by a
 *                    point without observations may be overwritten.
 * Local map points (mvpLocalMapPoints in order, `mcap` entries per frame), per point j < n_local[f]:
 *   mp_xyz[3 j..]    GetWorldPos()                      mp_normal[3 j..]  GetNormal()
 *   mp_dist[2 j..]   mfMinDistance, mfMaxDistance (raw: the 0.8f / 1.2f invariance factors are applied inside)
 *   mp_desc[32 j..]  GetDescriptor()
 *   mp_flags[j]      bit 0: candidate (!isBad() && mnLastFrameSeen != F.mnId), bit 1: Observations() > 0
 * Tcw: rows 0-2 of the CV_32F mTcw of each frame (12 floats); mOw is derived from it as Frame::UpdatePoseMatrices does.
 * On return match_out[f * cap + i2] is the local index j this call wrote into F.mvpMapPoints[i2] (the last writer), or -1 (unchanged);
 * n_to_match[f] is SearchLocalPoints' nToMatch (the in-view count: each such point gets IncreaseVisible()) and nmatches[f] the return
 * value of SearchByProjection (0 when nToMatch is 0, as when the call is skipped).  Optional outputs (NULL = not wanted), per point:
 * in_view[f * mcap + j] = mbTrackInView and track[f * mcap + j] = the tracking fields isInFrustum sets (all zero for points not in view).
 * The greedy, order-dependent hand-out of the reference (a keypoint held by a point with observations is skipped, later points
 * overwrite earlier ones, the best / second-best ratio test applies only when both are at the same octave) is reproduced exactly.
 * Limits: cap <= 8192, mcap <= 32768, nlevels <= MSL_MATCH_MAX_LEVELS; larger values are refused with MSL_ERR_INVALID before any launch.
 * Asynchronous on the handle's stream when inputs and outputs are device memory; with host memory on either side it returns when the
 * caller's buffers are its own again (as msl_match_by_projection). */
typedef struct msl_local_match_params {
    msl_match_params base;            /* fx..cy, bf, image bounds, th (3, or 5 after a relocalisation), nlevels, scale_factors; check_orientation unused */
    float log_scale_factor;           /* Frame::mfLogScaleFactor as the caller's Frame holds it */
    float view_cos_limit;             /* isInFrustum's viewingCosLimit (0.5 at the call site) */
    float nn_ratio;                   /* ORBmatcher::mfNNratio (0.8 at the call site) */
} msl_local_match_params;
typedef struct msl_local_track {
    float proj_x, proj_y, proj_xr;    /* mTrackProjX, mTrackProjY, mTrackProjXR */
    int32_t scale_level;              /* mnTrackScaleLevel */
    float view_cos;                   /* mTrackViewCos */
} msl_local_track;
MSL_API int msl_match_local_points(msl_match *h, int n_frames, int cap, int mcap, const msl_local_match_params *params,
                                   const msl_keypoint *cur_kps, const float *cur_un_xy, const float *cur_uright,
                                   const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_flags,
                                   const float *mp_xyz, const float *mp_normal, const float *mp_dist, const uint8_t *mp_desc,
                                   const uint8_t *mp_flags, const int32_t *n_local, const float *Tcw, msl_mem mem,
                                   int32_t *match_out, int32_t *n_to_match, int32_t *nmatches, uint8_t *in_view,
                                   msl_local_track *track, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_match_local_points_batch(int device, int n_frames, int cap, int mcap, const msl_local_match_params *params,
                                         const msl_keypoint *cur_kps, const float *cur_un_xy, const float *cur_uright,
                                         const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_flags,
                                         const float *mp_xyz, const float *mp_normal, const float *mp_dist, const uint8_t *mp_desc,
                                         const uint8_t *mp_flags, const int32_t *n_local, const float *Tcw, msl_mem mem,
                                         int32_t *match_out, int32_t *n_to_match, int32_t *nmatches, uint8_t *in_view,
                                         msl_local_track *track, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Matching map lines: LSDmatcher::SearchByProjection, both overloads (src/LSDmatcher.cpp:21-198) ----
 * Keylines come from the caller (LSD / LBD extraction is not part of this library).  Current frame, `lcap` entries per frame, keyline
 * j < n_cur_lines[f]:  cur_kl[j] = mvKeylinesUn[j] (pt.x, pt.y, angle, octave), cur_ldesc[32 j..] = mLdesc.row(j).
 * Both calls return match_out[f * lcap + j] = the index of the line this call wrote last into CurrentFrame.mvpMapLines[j], or -1, and
 * nmatches[f] = the function's return value (every accepted line counts, overwritten ones included).  The greedy, order-dependent hand-out
 * (a keyline held by a line with Observations() > 0 is skipped, later lines overwrite earlier ones) is reproduced exactly.
 * Optional pose-layout outputs (NULL = not wanted, out_mem like match_out): line_xyz[6 j..] (double) and line_has[j] exactly as
 * msl_pose_optimize reads them.  A slot the call writes gets the writer's world position, copied bit for bit, and line_has = 1.
 * msl_match_lines_by_projection also sets line_has = 0 for every other j < n_cur_lines[f] (its entry state is all NULL);
 * msl_match_local_lines leaves every other slot as it was.  Other bytes are not touched.
 * Asynchronous on the handle's stream when inputs and outputs are device memory; with host memory on either side it returns when the
 * caller's buffers are its own again (as msl_match_by_projection).  Limits: lcap <= 256, llcap <= 256, mlcap <= 32768,
 * nlevels <= MSL_MATCH_MAX_LEVELS; larger values are refused with MSL_ERR_INVALID before any launch. */
typedef struct msl_keyline {
    float x, y;                       /* KeyLine::pt */
    float angle;                      /* KeyLine::angle */
    int32_t octave;                   /* KeyLine::octave */
} msl_keyline;
typedef struct msl_line_match_params {
    msl_match_params base;            /* fx..cy, bf, image bounds, th (15 last frame; 1, or 5 after a relocalisation, local map), nlevels,
                                         scale_factors; check_orientation unused */
    float log_scale_factor;           /* Frame::mfLogScaleFactor (local map only) */
    float view_cos_limit;             /* isInFrustum's viewingCosLimit (0.6 at the call site; local map only) */
    float nn_ratio;                   /* LSDmatcher::mfNNratio (0.6, the constructor's default) */
} msl_line_match_params;
typedef struct msl_line_track {
    float proj_x1, proj_y1, proj_x2, proj_y2;   /* mTrackProjX1, mTrackProjY1, mTrackProjX2, mTrackProjY2 */
    int32_t scale_level;              /* mnTrackScaleLevel (MapLine::PredictScale is not clamped) */
    float view_cos;                   /* mTrackViewCos */
} msl_line_track;
/* msl_match_lines_by_projection: n_frames independent calls of
 *     int LSDmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th)   (src/LSDmatcher.cpp:21-134)
 * with Frame::GetLinesInArea (src/Frame.cc:384-415).  CurrentFrame.mvpMapLines is all NULL on entry (src/Tracking.cc:1255).
 * Last frame, `llcap` entries per frame, line i < n_last_lines[f]:
 *   last_line_xyz[6 i..]  mvpMapLines[i]->GetWorldPos() (Vector6d)        last_ldesc[32 i..]  ->GetDescriptor()
 *   last_line_flags[i]    bit 0: mvpMapLines[i] && !isBad() && !mvbLineOutlier[i]; bit 1: ->Observations() > 0
 *   last_line_octave[i]   LastFrame.mvKeylinesUn[i].octave (clamped to [0, nlevels) for the mvScaleFactors lookup)
 * Tcw_cur / Tcw_last as for msl_match_by_projection. */
MSL_API int msl_match_lines_by_projection(msl_match *h, int n_frames, int lcap, int llcap, const msl_line_match_params *params,
                                          const msl_keyline *cur_kl, const uint8_t *cur_ldesc, const int32_t *n_cur_lines,
                                          const double *last_line_xyz, const uint8_t *last_ldesc, const uint8_t *last_line_flags,
                                          const int32_t *last_line_octave, const int32_t *n_last_lines, const float *Tcw_cur,
                                          const float *Tcw_last, msl_mem mem, int32_t *match_out, int32_t *nmatches, double *line_xyz,
                                          uint8_t *line_has, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_match_lines_by_projection_batch(int device, int n_frames, int lcap, int llcap, const msl_line_match_params *params,
                                                const msl_keyline *cur_kl, const uint8_t *cur_ldesc, const int32_t *n_cur_lines,
                                                const double *last_line_xyz, const uint8_t *last_ldesc, const uint8_t *last_line_flags,
                                                const int32_t *last_line_octave, const int32_t *n_last_lines, const float *Tcw_cur,
                                                const float *Tcw_last, msl_mem mem, int32_t *match_out, int32_t *nmatches, double *line_xyz,
                                                uint8_t *line_has, msl_mem out_mem) MSL_NOEXCEPT;
/* msl_match_local_lines: Tracking::SearchLocalLines (src/Tracking.cc:1697-1737) after its first loop -- Frame::isInFrustum(pML,
 * view_cos_limit) (src/Frame.cc:261-327) with MapLine::PredictScale (src/MapLine.cpp:320-328) for every candidate local map line, then
 *     int LSDmatcher::SearchByProjection(Frame &F, const vector<MapLine*> &vpMapLines, th)   (src/LSDmatcher.cpp:137-198)
 * with RadiusByViewingCos (:252-257) when nToMatch > 0.  Current frame: the arrays above plus
 *   cur_line_flags[j]  state of F.mvpMapLines[j] after the first loop: bit 0: held, bit 1: the holder has Observations() > 0
 * Local map lines (mvpLocalMapLines in order, `mlcap` entries per frame), line i < n_local_lines[f]:
 *   ml_xyz[6 i..]  GetWorldPos() (double)            ml_normal[3 i..]  GetNormal() (double)
 *   ml_dist[2 i..] mfMinDistance, mfMaxDistance (raw: the 0.8f / 1.2f invariance factors are applied inside)
 *   ml_desc[32 i..] GetDescriptor()                   ml_flags[i]  bit 0: candidate (!isBad() && mnLastFrameSeen != F.mnId),
 *                                                                  bit 1: Observations() > 0
 * Tcw: rows 0-2 of the CV_32F mTcw (12 floats); mOw is derived from it.  Out: n_to_match[f] = nToMatch, and optionally in_view[f * mlcap + i]
 * = mbTrackInView and track[f * mlcap + i] = the tracking fields isInFrustum sets (all zero for lines not in view). */
MSL_API int msl_match_local_lines(msl_match *h, int n_frames, int lcap, int mlcap, const msl_line_match_params *params,
                                  const msl_keyline *cur_kl, const uint8_t *cur_ldesc, const int32_t *n_cur_lines, const uint8_t *cur_line_flags,
                                  const double *ml_xyz, const double *ml_normal, const float *ml_dist, const uint8_t *ml_desc,
                                  const uint8_t *ml_flags, const int32_t *n_local_lines, const float *Tcw, msl_mem mem, int32_t *match_out,
                                  int32_t *n_to_match, int32_t *nmatches, uint8_t *in_view, msl_line_track *track, double *line_xyz,
                                  uint8_t *line_has, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_match_local_lines_batch(int device, int n_frames, int lcap, int mlcap, const msl_line_match_params *params,
                                        const msl_keyline *cur_kl, const uint8_t *cur_ldesc, const int32_t *n_cur_lines,
                                        const uint8_t *cur_line_flags, const double *ml_xyz, const double *ml_normal, const float *ml_dist,
                                        const uint8_t *ml_desc, const uint8_t *ml_flags, const int32_t *n_local_lines, const float *Tcw,
                                        msl_mem mem, int32_t *match_out, int32_t *n_to_match, int32_t *nmatches, uint8_t *in_view,
                                        msl_line_track *track, double *line_xyz, uint8_t *line_has, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Pose-only optimisation: Optimizer::PoseOptimization (src/Optimizer.cc:53-590) ----
 * n_frames independent calls of  int Optimizer::PoseOptimization(Frame *pFrame)  for an Optimizer(angleInfo, disInfo, parInfo, verInfo,
 * planeChi, planeChiVP, aTh, parTh), with every edge type it creates: mono / stereo point edges, the two endpoint edges of a line, and
 * plane, parallel-plane and vertical-plane edges; g2o's Levenberg-Marquardt (4 rounds x 10 iterations, outlier classification after
 * each round) restated on the device in double.  Per frame f (arrays hold cap / xcap / lcap / pcap entries per frame):
 *   kps[i]             mvKeysUn[i] (only .octave is read)      un_xy[2 i..]   mvKeysUn[i].pt      uright[i]  mvuRight[i]
 *   pt_ref[i]          index into this frame's xyz of mvpMapPoints[i]->GetWorldPos(), or -1 for NULL (i < n_kps[f]; values outside
 *                      [0, xcap) count as NULL).  match_out of msl_match_by_projection (with last_xyz) or of msl_match_local_points
 *                      (with mp_xyz, after merging the points held before the call) feeds it directly.
 *   line_fn[3 j..]     mvKeyLineFunctions[j]                   line_xyz[6 j..]  mvpMapLines[j]->mWorldPos (start, end)
 *   line_has[j]        mvpMapLines[j] != NULL                  (j < n_lines[f])
 *   plane_coef[4 k..]  mvPlaneCoefficients[k]                  plane_w[12 k + 4 s..]  GetWorldPos() of mvpMapPlanes[k] (s = 0),
 *   plane_has[k]       bit s set: that plane is not NULL       mvpParallelPlanes[k] (s = 1), mvpVerticalPlanes[k] (s = 2)  (k < n_planes[f])
 *   Tcw[12]            rows 0-2 of the CV_32F mTcw
 * In/out (out_mem): outlier[i] = mvbOutlier, line_outlier[j] = mvbLineOutlier, plane_outlier[3 k + s] = mvbPlaneOutlier /
 * mvbParPlaneOutlier / mvbVerPlaneOutlier: entries with an edge get the final classification, the others keep their value.
 * Out: Tcw_out[12] the optimised pose (float, as Frame::SetPose stores it; the input pose when fewer than 3 correspondences),
 * n_good[f] the return value (nInitialCorrespondences - nBad, or 0).  Octaves outside [0, nlevels) are clamped.
 * Limits: cap <= 8192, xcap <= 32768, lcap <= 256, pcap <= 64, nlevels <= MSL_MATCH_MAX_LEVELS; larger values are refused with
 * MSL_ERR_INVALID before any launch.  msl_pose_optimize is asynchronous on the matcher handle's stream when inputs and outputs are
 * device memory; with host memory on either side it returns when the caller's buffers are its own again. */
typedef struct msl_pose_params {
    float fx, fy, cx, cy, bf;         /* Frame::fx .. cy, mbf */
    int32_t nlevels;
    float inv_level_sigma2[MSL_MATCH_MAX_LEVELS];   /* Frame::mvInvLevelSigma2 */
    double angle_info, dis_info, par_info, ver_info, plane_chi, plane_chi_vp, a_th, par_th;   /* the Optimizer constructor arguments */
} msl_pose_params;
MSL_API int msl_pose_optimize(msl_match *h, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                              const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps,
                              const float *xyz, const double *line_fn, const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines,
                              const float *plane_coef, const float *plane_w, const uint8_t *plane_has, const int32_t *n_planes,
                              const float *Tcw, msl_mem mem, uint8_t *outlier, uint8_t *line_outlier, uint8_t *plane_outlier,
                              float *Tcw_out, int32_t *n_good, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_pose_optimize_batch(int device, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                                    const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref,
                                    const int32_t *n_kps, const float *xyz, const double *line_fn, const double *line_xyz,
                                    const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w,
                                    const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw, msl_mem mem, uint8_t *outlier,
                                    uint8_t *line_outlier, uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Translation-only optimisation (Manhattan mode): Optimizer::TranslationOptimization (src/Optimizer.cc:592-1009) ----
 * n_frames independent calls of  int Optimizer::TranslationOptimization(Frame *pFrame), the optimiser of
 * Tracking::TranslationWithMotionModel (src/Tracking.cc:946-1050), on the same solver as msl_pose_optimize.  Every input has the
 * layout, meaning and limits of msl_pose_optimize, so the matchers' outputs and manhattanslam_amd.pose.pack feed it unchanged, except:
 *   Rcw[9 f..]  optional (NULL = absent): the CV_32F manhattanRcw of frame f, row-major.  It replaces rows 0-2 / columns 0-2 of that
 *               frame's Tcw before anything else, as mTcw's rotation block is overwritten at src/Tracking.cc:974.
 *   Planes      only plane_has bit 0 and plane_w[12 k + 0..3] (mvpMapPlanes) are read; only plane_outlier[3 k + 0] is written.  The
 *               bytes s = 1, 2 are left untouched (no parallel or vertical plane edges are created here).
 * Edges: EdgeSE3ProjectXYZOnlyTranslation / EdgeStereoSE3ProjectXYZOnlyTranslation / EdgeLineProjectXYZOnlyTranslation with
 * Xc = R_cw * Xw as a float product (line endpoints rounded to float first, :755-756 / :781-782), EdgePlaneOnlyTranslation with the
 * world plane flipped against the initial pose and rotated by R_cw (:836-853).  Only points count in nInitialCorrespondences; below 3 the
 * call returns 0 (:796) after clearing the point and line flags and before any plane edge exists, so the plane flags are untouched.  The
 * classification (:880-1000) recomputes line errors only for flagged lines and does not count bad lines; bad planes count in nBad.
 * Out: n_good[f] = nInitialCorrespondences - nBad (it can be negative), or 0; Tcw_out[12] the optimised pose as Frame::SetPose stores
 * it (the rotation has been through the quaternion round trip), or on the early return the input pose with Rcw written in.
 * Asynchronous on the matcher handle's stream when inputs and outputs are device memory; with host memory on either side it returns
 * when the caller's buffers are its own again.  Rcw is in `mem` memory like the other inputs. */
MSL_API int msl_pose_optimize_translation(msl_match *h, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                                          const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref,
                                          const int32_t *n_kps, const float *xyz, const double *line_fn, const double *line_xyz,
                                          const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w,
                                          const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw, const float *Rcw, msl_mem mem,
                                          uint8_t *outlier, uint8_t *line_outlier, uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good,
                                          msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_pose_optimize_translation_batch(int device, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                                                const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref,
                                                const int32_t *n_kps, const float *xyz, const double *line_fn, const double *line_xyz,
                                                const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w,
                                                const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw, const float *Rcw,
                                                msl_mem mem, uint8_t *outlier, uint8_t *line_outlier, uint8_t *plane_outlier, float *Tcw_out,
                                                int32_t *n_good, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Plane association: PlaneMatcher::SearchMapByCoefficients (src/PlaneMatcher.cpp:31-106) ----
 * n_frames independent calls of  int PlaneMatcher::SearchMapByCoefficients(Frame &pF, const vector<MapPlane*> &vpMapPlanes)  for a
 * PlaneMatcher(d_th, a_th, ver_th, par_th), with Frame::ComputePlaneWorldCoeff (src/Frame.cc:656-660).  Per frame f:
 *   plane_coef[4 k..]  mvPlaneCoefficients[k] (k < n_planes[f], `pcap` per frame)    Tcw[12]  rows 0-2 of the CV_32F mTcw
 * Map planes in GetAllMapPlanes() order (`mcap` per frame), j < n_map[f]:
 *   mp_w[4 j..]        GetWorldPos()                 mp_flags[j]  bit 0: !isBad()
 *   mp_pt_off[j], mp_pt_off[j + 1]  (mcap + 1 per frame): mvPlanePoints of plane j are points [off[j], off[j + 1]) of mp_pts[3 n..]
 *                      (x, y, z; `ptcap` points per frame; offsets are clamped to [0, ptcap])
 * In/out (out_mem): plane_match[3 k + s] = the index j of mvpMapPlanes[k] (s = 0), mvpParallelPlanes[k] (s = 1), mvpVerticalPlanes[k]
 * (s = 2), or -1 for NULL.  The reference never clears these pointers: a slot the call does not write keeps its value.
 * Out: nmatches[f] the return value; plane_w[12 k + 4 s..] / plane_has[k] for every k < n_planes[f] in exactly the layout
 * msl_pose_optimize[_translation] reads: bit s set and the world position of the plane copied bit for bit when slot s holds an index in
 * [0, n_map[f]), bit s clear and zeros otherwise.  Optional pM_out[4 k..] (NULL = not wanted): the world coefficients mTcw^T * coef.
 * Exactly reproduced: pM as a cv::Mat CV_32F product (double accumulation, one rounding per element); angle a float dot product, left to
 * right; PointDistanceFromPlane a float |a x + b y + c z + d| whose minimum starts at 100 and skips NaN points (an empty cloud gives 100);
 * the walk over the map planes with its tightening thresholds -- bad planes skipped, `angle > a_th && dis < ldTh` matches and continues,
 * a plane failing only the distance test falls through to the vertical (|angle| < lverTh) and then the parallel (|angle| > lparTh) test;
 * strict comparisons, so the first of equal candidates wins.  Two launches (distances, then the walk).
 * Counts: n_planes[f] is clamped to [0, pcap] and n_map[f] to [0, mcap]; entries beyond the clamped counts and points outside every
 * clamped offset range are never read, and no kernel writes rows k >= n_planes[f] of plane_match, plane_w, plane_has and pM_out:
 * device-memory arrays keep their bytes there (host-memory outputs other than plane_match are copied back whole: unspecified there).
 * Limits: pcap <= 64, mcap <= 4096, ptcap <= 2^22; larger values, a value below 1 (n_frames too) and a NULL array other than pM_out are
 * refused with MSL_ERR_INVALID before any launch, with msl_last_error() naming the argument, and nothing is written (the _batch form
 * refuses before it touches a device).  Asynchronous on the matcher handle's stream when inputs and outputs are device memory; with host
 * memory on either side it returns when the caller's buffers are its own again. */
typedef struct msl_plane_params {
    float d_th, a_th, ver_th, par_th;   /* Plane.AssociationDisRef, AssociationAngRef, VerticalThreshold, ParallelThreshold (src/Tracking.cc:144-154) */
    float mf_ver_th;                    /* Plane.MFVerticalThreshold: msl_manhattan_detect only */
} msl_plane_params;
MSL_API int msl_plane_associate(msl_match *h, int n_frames, int pcap, int mcap, int ptcap, const msl_plane_params *params,
                                const float *plane_coef, const int32_t *n_planes, const float *Tcw, const float *mp_w, const uint8_t *mp_flags,
                                const int32_t *mp_pt_off, const float *mp_pts, const int32_t *n_map, msl_mem mem, int32_t *plane_match,
                                int32_t *nmatches, float *plane_w, uint8_t *plane_has, float *pM_out, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_plane_associate_batch(int device, int n_frames, int pcap, int mcap, int ptcap, const msl_plane_params *params,
                                      const float *plane_coef, const int32_t *n_planes, const float *Tcw, const float *mp_w,
                                      const uint8_t *mp_flags, const int32_t *mp_pt_off, const float *mp_pts, const int32_t *n_map,
                                      msl_mem mem, int32_t *plane_match, int32_t *nmatches, float *plane_w, uint8_t *plane_has,
                                      float *pM_out, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Manhattan-frame detection: Tracking::DetectManhattan (src/Tracking.cc:651-844) ----
 * n_frames independent calls.  Per frame f: plane_coef and n_planes as for msl_plane_associate, plane_npts[k] = mvPlanePoints[k].size(),
 * plane_match in msl_plane_associate's layout (only slot s = 0, mvpMapPlanes, is read; indices outside [0, n_map[f]) count as NULL),
 * mp_flags / n_map as for msl_plane_associate (`mcap` per frame; bit 0 = !isBad()).
 * The Manhattan observation tables of Map, flattened by the caller (`fcap` / `qcap` entries per frame):
 *   full_tab[7 e..]  {a, b, c, kf, ia, ib, ic}  e < n_full[f]   map-plane indices a <= b <= c, the keyframe slot kf, and
 *                                                               GetIndexInKeyFrame(pKF) of planes a, b, c (-1 allowed)
 *   part_tab[5 e..]  {a, b, kf, ia, ib}         e < n_part[f]   the same for GetPartialManhattanObservation
 *   Both sorted ascending by their keys ((a, b, c) resp. (a, b), lexicographic).  Map hashes and compares its keys as unordered sets
 *   (src/Map.cc:32-123), so a sorted index tuple is an exact stand-in.  Host-memory tables are checked and refused (MSL_ERR_INVALID) when
 *   unsorted; sorting device-memory tables is the caller's contract.  An entry with an index -1 (or outside [0, pcap), or a slot outside
 *   [0, kcap)) is no candidate, as at :713 / :752.
 * Per keyframe slot r (`kcap` per frame): kf_Rwc[9 r..] = GetPoseInverse() rows / columns 0-2 (row-major), kf_coef[4 (r pcap + q)..] =
 *   mvPlaneCoefficients[q], kf_npts[r pcap + q] = mvPlanePoints[q].size().
 * Out: found[f] the return value, full[f] = fullManhattanFound, Rcw[9 f..] = manhattanRcw (row-major, the layout
 * msl_pose_optimize_translation reads) -- written only where found, the member is left unchanged otherwise (Rcw is in/out) -- and
 * optionally (NULL = not wanted) choice[6 f..] = {i, j, k (-1 for a partial pair), table entry, score, kf}, {-1, -1, -1, -1, 0, -1} when
 * nothing is found.
 * Exactly reproduced: the candidate order (for i, for j > i: the triples k > j, then the pair (i, j)), the gates (held, not bad,
 * the float dot products against +-mf_ver_th) and the choice -- the first candidate in that order reaching the largest score, if > 0, a
 * later pair replacing a triple.  The rotation: the partial case's third columns as float cross products, the column flipped only in the
 * partial case when |det + 1| < 0.5 (det in double), MFc and MFm replaced by their polar factors, Rwc = (kf_Rwc * MFm) * MFc^T as two
 * float products with double accumulation, Rcw = Rwc^T.  The polar factor U * Vt is not OpenCV's float Jacobi SVD: it is computed in
 * double by Newton's iteration X <- (X + X^-T) / 2 and rounded to float, so Rcw agrees with the reference within about 2e-6 per entry;
 * every integer output is exact.  One launch (one workgroup per frame).
 * Counts: n_planes[f], n_map[f], n_full[f] and n_part[f] are clamped to [0, pcap], [0, mcap], [0, fcap] and [0, qcap]; entries beyond
 * the clamped counts are never read (host-memory tables are sort-checked over the clamped counts).
 * Limits: pcap <= 64, mcap <= 4096, fcap <= 65536, qcap <= 65536, kcap <= 4096; larger values, a value below 1 (n_frames too), a NULL array
 * other than choice and an unsorted host-memory table are refused with MSL_ERR_INVALID before any launch, with msl_last_error() naming
 * the argument (the table and its frame), and nothing is written (the _batch form refuses before it touches a device).  Asynchronous on
 * the matcher handle's stream when inputs and outputs are device memory; with host memory on either side it returns when the caller's
 * buffers are its own again. */
MSL_API int msl_manhattan_detect(msl_match *h, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params,
                                 const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const int32_t *plane_match,
                                 const uint8_t *mp_flags, const int32_t *n_map, const int32_t *full_tab, const int32_t *n_full,
                                 const int32_t *part_tab, const int32_t *n_part, const float *kf_Rwc, const float *kf_coef,
                                 const int32_t *kf_npts, msl_mem mem, int32_t *found, int32_t *full, float *Rcw, int32_t *choice,
                                 msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_manhattan_detect_batch(int device, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap,
                                       const msl_plane_params *params, const float *plane_coef, const int32_t *plane_npts,
                                       const int32_t *n_planes, const int32_t *plane_match, const uint8_t *mp_flags, const int32_t *n_map,
                                       const int32_t *full_tab, const int32_t *n_full, const int32_t *part_tab, const int32_t *n_part,
                                       const float *kf_Rwc, const float *kf_coef, const int32_t *kf_npts, msl_mem mem, int32_t *found,
                                       int32_t *full, float *Rcw, int32_t *choice, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Plane clouds: the tail of Frame::ExtractPlanes and MapPlane::UpdateCoefficientsAndPoints ----
 * The step between msl_peac_extract_batch and msl_plane_associate / msl_manhattan_detect, and the map-plane clouds the next frame's
 * association reads.  PCL's results are implementation-defined (pcl::VoxelGrid sorts with an unstable std::sort and sums in float in that
 * order), so the contract is the sequential model tests/plane_cloud_model.py, which the kernels follow bit for bit.
 *
 * Voxel grid (pcl::VoxelGrid, leaf = params->leaf on every axis): voxel = (int)floorf(x * (1.0f / leaf)) per axis; output voxels in
 * ascending (vz, vy, vx), PCL's linear-index order; a point that is not finite or has a |coordinate| >= 32768 m is skipped; the centroid
 * is order-independent: every coordinate is (int64)rint((double)x * 2^24), summed as int64, mean = (float)((double)sum / (double)count)
 * scaled back by 2^-24 (exact); colour: integer sums of r, g, b, (float)sum / (float)count truncated to u8.  A bounding box of more than
 * INT32_MAX cells (PCL returns its input unfiltered) and a cloud of more than MSL_PLANE_CLOUD_MAX_VOXELS voxels are statuses.
 *
 * msl_plane_clouds: n_frames independent tails of Frame::ExtractPlanes (src/Frame.cc:611-653, MaxPointDistanceFromPlane :662-709).
 * In (mem), per frame f: cloud[f][n_vertices][3] doubles (msl_peac_extract_batch's cloud_out, cast to float as :616-618), rgb[f][n_vertices][3]
 * u8 or NULL (colour not carried; then rgb_out must be NULL too), vertex_offsets[f][max_planes + 1] / vertex_indices[f][n_vertices],
 * planes[f][max_planes], n_planes[f] (msl_peac_extract_batch's outputs of these names), seed[f].  Per detector plane i < n_planes[f]:
 * gather its vertices, voxel grid, then the gate: (a, b, c) = (float)normal, d = (float)-(nx cx + ny cy + nz cz) in double, the plane is
 * rejected if the float |a x + b y + c z + d|, left to right, is > dis_th at any coarse point, then if fewer than 4 coarse points remain;
 * then pcl::SACSegmentation pinned as: iteration k draws three distinct points with the sampler of msl_pnp_ransac (seed[f] ^ fmix32(i),
 * swap-with-back over a fresh identity permutation); float plane = normalised cross product, d = -n.p0; a zero cross product uses up the
 * iteration (PCL redraws); inliers float |n.p + d| < dis_th; a hypothesis replaces the best on a strictly larger count; stop after
 * iteration `it` when q^it <= 1 - probability (q = 1 - w^3, w = count / N, double, the power by repeated multiplication) or
 * it == max_iterations; no hypothesis at all drops the plane.  With more than 3 inliers the coefficients are refitted: centroid and centred
 * scatter matrix in double (element i of the ascending inliers to partial i mod 256, a pairwise tree over the partials), the eigenvector of
 * its smallest eigenvalue from the pinned Jacobi solver, normalised in double, d = -n.centroid, all four rounded to float.  Then the sign
 * rule of :704-706 against the gate's d.
 * Out (out_mem), per frame: n_out[f] (mnPlaneNum); plane_coef[f][pcap][4] and plane_npts[f][pcap] in exactly the layout msl_plane_associate
 * and msl_manhattan_detect read; plane_src[f][pcap] the detector plane of each kept plane; the coarse clouds as CSR pt_off[f][pcap + 1],
 * pts[f][ptcap][3] (and rgb_out[f][ptcap][3]); status[f][max_planes] per detector plane (MSL_PLANE_CLOUD_*).  Kept planes are compacted
 * in detector order (the push_backs of :651-652).  When pcap or ptcap is exhausted, that plane and every later kept one is dropped with
 * MSL_PLANE_CLOUD_NO_ROOM.
 *
 * msl_map_plane_merge: n_frames independent runs of the loop of src/Tracking.cc:429-436 (MapPlane::UpdateCoefficientsAndPoints(Frame&, id),
 * src/MapPlane.cc:201-218; the no-argument form of :178-199 on a new plane is a merge into a row with an empty cloud).
 * In (mem), per frame: the frame's plane clouds (n_planes[f], pt_off[f][pcap + 1], pts[f][fptcap][3], rgb[f][fptcap][3] or NULL: the
 * outputs above), merge_into[f][pcap] (a map row, or -1), Twc[f][12] doubles (rows 0-2, row-major; the caller inverts its pose), the map
 * clouds in msl_plane_associate's layout (mp_pt_off[f][mcap + 1], mp_pts[f][ptcap][3], n_map[f]; mp_rgb[f][ptcap][3] or NULL).  Colour is
 * carried when rgb, mp_rgb and mp_rgb_out are all given, and not when all are NULL (anything else is refused).
 * A frame point goes through (float)(T[4r] * x + T[4r + 1] * y + T[4r + 2] * z + T[4r + 3]) in double, left to right; the row's cloud is
 * appended and the sum voxel-filtered.  Several frame planes that name one row are merged one after another in ascending k, each seeing the
 * previous result.  A merge that fails (voxel limit, grid overflow) leaves the row's cloud as it was; the row's status is its first failure.
 * Out (out_mem): a new CSR of the whole map, mp_pt_off_out[f][mcap + 1] / mp_pts_out[f][ptcap][3] (/ mp_rgb_out), offsets an exact prefix
 * sum from 0, rows in map order, untouched rows copied bit for bit: the next msl_plane_associate takes it as it stands.
 * merge_status[f][mcap] (MSL_PLANE_MERGE_*).  When ptcap is exhausted that row and every later one is empty with MSL_PLANE_MERGE_NO_ROOM.
 *
 * Counts: n_planes[f] is clamped to [0, max_planes] / [0, pcap], n_map[f] to [0, mcap], offsets to their array.  Host-memory calls check
 * vertex_offsets, vertex_indices, pt_off, mp_pt_off and merge_into and refuse with the field named; with device memory an index outside
 * its table is absent (a vertex index is skipped, a merge_into outside [0, n_map) is -1), and nothing is read or written outside an array.
 * No kernel writes rows beyond the counts (plane_coef, plane_npts, plane_src and pt_off beyond n_out, points beyond the last offset, status
 * beyond n_planes, mp_pt_off_out / merge_status beyond n_map): device-memory arrays keep their bytes there.
 * Limits: n_frames <= 65535, n_vertices <= MSL_PLANE_CLOUD_MAX_VERTICES, max_planes <= 64, pcap <= 64, mcap <= 4096, ptcap and fptcap <= 2^22,
 * 1 / 32 <= leaf, max_iterations in [1, 4096], probability in [0, 1] (every count and capacity at least 1); anything else, or a NULL
 * array other than the colour arrays, is refused with MSL_ERR_INVALID before any launch, with msl_last_error() naming the argument, and
 * nothing is written (the _batch forms refuse before they touch a device).  Asynchronous on the matcher handle's stream when inputs and
 * outputs are device memory. */
#define MSL_PLANE_CLOUD_MAX_VOXELS 4096
#define MSL_PLANE_CLOUD_MAX_VERTICES 131072
#define MSL_PLANE_CLOUD_KEPT      0   /* in the output */
#define MSL_PLANE_CLOUD_GATE      1   /* a coarse point farther than dis_th from the detector's plane */
#define MSL_PLANE_CLOUD_FEW       2   /* fewer than 4 coarse points */
#define MSL_PLANE_CLOUD_NO_MODEL  3   /* every sample degenerate */
#define MSL_PLANE_CLOUD_VOXELS    4   /* more than MSL_PLANE_CLOUD_MAX_VOXELS voxels */
#define MSL_PLANE_CLOUD_GRID      5   /* the bounding box spans more than INT32_MAX cells */
#define MSL_PLANE_CLOUD_NO_ROOM   6   /* pcap or ptcap exhausted */
#define MSL_PLANE_MERGE_UNTOUCHED 0   /* no frame plane names the row: copied */
#define MSL_PLANE_MERGE_MERGED    1   /* every merge into the row succeeded */
#define MSL_PLANE_MERGE_VOXELS    4   /* the first failed merge: voxel limit (the row keeps its cloud for that merge) */
#define MSL_PLANE_MERGE_GRID      5   /* the first failed merge: grid overflow */
#define MSL_PLANE_MERGE_NO_ROOM   6   /* ptcap exhausted: the row is empty */
typedef struct msl_plane_cloud_params {
    float leaf;                 /* 0.2 (src/Frame.cc:637, src/MapPlane.cc:211) */
    float dis_th;               /* Plane.DistanceThreshold: mfDisTh (src/Tracking.cc:148) */
    int32_t max_iterations;     /* 50: pcl::SACSegmentation's default */
    int32_t _pad;
    double probability;         /* 0.99 */
} msl_plane_cloud_params;
MSL_API int msl_plane_clouds(msl_match *h, int n_frames, int n_vertices, int max_planes, int pcap, int ptcap,
                             const msl_plane_cloud_params *params, const double *cloud, const uint8_t *rgb, const int32_t *vertex_offsets,
                             const int32_t *vertex_indices, const msl_peac_plane *planes, const int32_t *n_planes, const uint32_t *seed,
                             msl_mem mem, int32_t *n_out, float *plane_coef, int32_t *plane_npts, int32_t *plane_src, int32_t *pt_off,
                             float *pts, uint8_t *rgb_out, int32_t *status, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_plane_clouds_batch(int device, int n_frames, int n_vertices, int max_planes, int pcap, int ptcap,
                                   const msl_plane_cloud_params *params, const double *cloud, const uint8_t *rgb,
                                   const int32_t *vertex_offsets, const int32_t *vertex_indices, const msl_peac_plane *planes,
                                   const int32_t *n_planes, const uint32_t *seed, msl_mem mem, int32_t *n_out, float *plane_coef,
                                   int32_t *plane_npts, int32_t *plane_src, int32_t *pt_off, float *pts, uint8_t *rgb_out, int32_t *status,
                                   msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_map_plane_merge(msl_match *h, int n_frames, int pcap, int fptcap, int mcap, int ptcap, const msl_plane_cloud_params *params,
                                const int32_t *n_planes, const int32_t *pt_off, const float *pts, const uint8_t *rgb, const int32_t *merge_into,
                                const double *Twc, const int32_t *mp_pt_off, const float *mp_pts, const uint8_t *mp_rgb, const int32_t *n_map,
                                msl_mem mem, int32_t *mp_pt_off_out, float *mp_pts_out, uint8_t *mp_rgb_out, int32_t *merge_status,
                                msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_map_plane_merge_batch(int device, int n_frames, int pcap, int fptcap, int mcap, int ptcap,
                                      const msl_plane_cloud_params *params, const int32_t *n_planes, const int32_t *pt_off, const float *pts,
                                      const uint8_t *rgb, const int32_t *merge_into, const double *Twc, const int32_t *mp_pt_off,
                                      const float *mp_pts, const uint8_t *mp_rgb, const int32_t *n_map, msl_mem mem, int32_t *mp_pt_off_out,
                                      float *mp_pts_out, uint8_t *mp_rgb_out, int32_t *merge_status, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Bag of words: the vocabulary, Frame::ComputeBoW / KeyFrame::ComputeBoW, and the reference-keyframe searches ----
 * The searches that open Tracking::TrackReferenceKeyFrame (src/Tracking.cc:1146-1175) and Tracking::TranslationEstimation (:846-877).
 *
 * msl_vocab: a DBoW2 TemplatedVocabulary<FORB::TDescriptor, FORB> on one device, as loadFromTextFile builds it
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1420).  Node table of n_nodes entries, entry 0 the root (its values are not read),
 * nodes 1 .. n_nodes - 1 in file order: parent[i] (in [0, i), else refused), is_leaf_flag[i] (the file's isLeaf > 0), desc32[32 i..],
 * weight[i].  Children belong to their parent in file order; word ids go to the flagged nodes in file order; every other node has word
 * id 0.  The children of each node are packed contiguously on the device as 32-byte records.  Limits: 2 <= k <= 20, 1 <= L <= 10,
 * scoring 0..5 (L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT), weighting 0..3 (TF_IDF, TF, IDF, BINARY), 1 <= n_nodes < 2^31;
 * NULL with msl_last_error() otherwise, and with no usable device (no CPU fallback).
 * msl_vocab_load_text parses DBoW2's text format: a header line "k L scoring weighting", then one line per node
 * "parent isLeaf d0 .. d31 weight".  Refused as the reference refuses a header (k, L, scoring, weighting outside the limits above; the reference
 * accepts k = 0 and 1, where its node-count arithmetic divides by zero), and a malformed node line.  Blank lines are skipped: the reference
 * loops on !eof(), so a file ending in a newline gives its root one more childless child (parent 0 from a failed parse, an uninitialised
 * descriptor, weight 0) -- undefined behaviour this loader does not reproduce.
 * msl_vocab_info: info[7] = {k, L, scoring, weighting, n_nodes, n_words, device}. */
typedef struct msl_vocab msl_vocab;
MSL_API msl_vocab *msl_vocab_create(int device, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent,
                                    const uint8_t *is_leaf_flag, const uint8_t *desc32, const double *weight) MSL_NOEXCEPT;
MSL_API msl_vocab *msl_vocab_load_text(int device, const char *path) MSL_NOEXCEPT;
MSL_API void msl_vocab_destroy(msl_vocab *v) MSL_NOEXCEPT;
MSL_API int msl_vocab_info(const msl_vocab *v, int32_t info[7]) MSL_NOEXCEPT;

/* msl_bow_transform: n_frames independent calls of
 *     void TemplatedVocabulary::transform(const vector<TDescriptor>&, BowVector&, FeatureVector&, int levelsup)   (TemplatedVocabulary.h:1126-1192)
 * with the per-feature descent (:1217-1255): Frame::ComputeBoW / KeyFrame::ComputeBoW call it with levelsup = 4.  desc[32 (f cap + i)..] and
 * n_desc[f] are msl_orb_extract_frame_batch's desc32 / n_out (`cap` keypoints per frame).  Per feature (all cap entries written):
 * word_out the word id, node_out the FeatureVector node at level L - levelsup (0, the root, when L - levelsup <= 0); both -1 when the
 * feature is stopped (word weight not > 0), when i >= n_desc[f], and for every feature of a vocabulary without words (DBoW2's empty()).
 * Feature i is in fv[node_out[i]]; each list is in ascending feature order by construction.  Optional (all three or none; NULL skips the
 * per-frame sort): the BowVector as ascending word ids bow_word[f cap + j] with bow_value (double), j < n_words[f]; -1 / 0 beyond.
 * Exactly reproduced: the descent -- the first child holds the initial best, a later child replaces it only at a strictly smaller Hamming
 * distance (ties to the earliest child in file order) -- stops at a node without children (a childless node that is not flagged keeps word
 * id 0 and its file weight); TF / TF_IDF accumulate v[id] += w in feature order, IDF / BINARY keep the first weight; every scoring but
 * DOT_PRODUCT normalises (L1: sum of fabs, L2_NORM: sqrt of the sum of squares, both in ascending word order, only when the norm is > 0),
 * otherwise TF / TF_IDF divide by v.size().  When the descent stops above level L - levelsup the reference leaves nid uninitialised;
 * node_out is then the node where the descent stopped.  The vocabulary must live on the handle's device (MSL_ERR_INVALID otherwise).
 * Limits: cap <= 8192.  Asynchronous on the matcher handle's stream when inputs and outputs are device memory; with host memory on either
 * side it returns when the caller's buffers are its own again. */
MSL_API int msl_bow_transform(msl_match *h, const msl_vocab *v, int n_frames, int cap, int levelsup, const uint8_t *desc, const int32_t *n_desc,
                              msl_mem mem, int32_t *word_out, int32_t *node_out, int32_t *bow_word, double *bow_value, int32_t *n_words,
                              msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_bow_transform_batch(int device, const msl_vocab *v, int n_frames, int cap, int levelsup, const uint8_t *desc,
                                    const int32_t *n_desc, msl_mem mem, int32_t *word_out, int32_t *node_out, int32_t *bow_word,
                                    double *bow_value, int32_t *n_words, msl_mem out_mem) MSL_NOEXCEPT;

/* msl_match_by_bow: n_pairs independent calls of
 *     int ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches)   (src/ORBmatcher.cc:146-247)
 * for an ORBmatcher(nn_ratio, check_orientation): 0.7 at both tracking sites, 0.75 in Tracking::Relocalization.  Per pair f, `cap`
 * entries per side:
 *   keyframe  kf_desc[32 i..] mDescriptors, kf_angle[i] mvKeysUn[i].angle, kf_node[i] its node_out (an earlier msl_bow_transform),
 *             kf_flags[i] bit 0: GetMapPointMatches()[i] && !isBad(), i < n_kf[f]
 *   frame     cur_kps[i] mvKeys (the angle is read), cur_desc, cur_node (its node_out), i < n_cur[f]
 * Out: match_out[f cap + iF] = the keyframe keypoint index whose map point vpMapPointMatches[iF] holds, or -1; nmatches[f] the return value.
 * match_out feeds msl_pose_optimize[_translation] as pt_ref directly, with the keyframe's map-point positions per keyframe keypoint as xyz.
 * Exactly reproduced: only nodes present on both sides are visited; in a node the keyframe features run in ascending order and a frame
 * feature matched earlier is skipped; bestDist1 is the first minimum over ascending frame indices, bestDist2 the second smallest distance
 * (equal to bestDist1 on a tie), both starting at 256; accepted when bestDist1 <= TH_LOW (50) and (float)bestDist1 < nn_ratio *
 * (float)bestDist2; the rotation histogram (HISTO_LENGTH 30, bin round(rot / 30), bin 30 -> 0) with ComputeThreeMaxima, every match outside
 * the kept bins NULLed.  Limits: cap <= 8192.  Memory and synchronisation as msl_bow_transform. */
typedef struct msl_bow_match_params {
    float nn_ratio;                   /* ORBmatcher::mfNNratio */
    int32_t check_orientation;        /* ORBmatcher::mbCheckOrientation */
} msl_bow_match_params;
MSL_API int msl_match_by_bow(msl_match *h, int n_pairs, int cap, const msl_bow_match_params *params, const uint8_t *kf_desc,
                             const float *kf_angle, const int32_t *kf_node, const uint8_t *kf_flags, const int32_t *n_kf,
                             const msl_keypoint *cur_kps, const uint8_t *cur_desc, const int32_t *cur_node, const int32_t *n_cur, msl_mem mem,
                             int32_t *match_out, int32_t *nmatches, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_match_by_bow_batch(int device, int n_pairs, int cap, const msl_bow_match_params *params, const uint8_t *kf_desc,
                                   const float *kf_angle, const int32_t *kf_node, const uint8_t *kf_flags, const int32_t *n_kf,
                                   const msl_keypoint *cur_kps, const uint8_t *cur_desc, const int32_t *cur_node, const int32_t *n_cur,
                                   msl_mem mem, int32_t *match_out, int32_t *nmatches, msl_mem out_mem) MSL_NOEXCEPT;

/* msl_match_lines_by_descriptor: n_pairs independent calls of
 *     int LSDmatcher::SearchByDescriptor(KeyFrame *pKF, Frame &currentF, vector<MapLine*> &vpMapLineMatches)   (src/LSDmatcher.cpp:201-234)
 * Keyframe lines (`klcap` per pair), q < n_kf_lines[f]: kf_ldesc[32 q..] mLineDescriptors, kf_line_flags[q] bit 0:
 * GetMapLineMatches()[q] != NULL (the reference does not test isBad() here), optional kf_line_xyz[6 q..] GetWorldPos() (double).
 * Current lines (`lcap` per pair), t < n_cur_lines[f]: cur_ldesc[32 t..] mLdesc.
 * Out: match_out[f lcap + t] = the last query q written into slot t, or -1; nmatches[f] the return value (every accepted write counts,
 * overwritten ones included).  Optional (both or neither, with kf_line_xyz): line_xyz[6 t..] / line_has[t] in the layout
 * msl_match_lines_by_projection writes for msl_pose_optimize -- a written slot gets the keyframe line's position bit for bit and
 * line_has = 1, every other t < n_cur_lines[f] line_has = 0; other bytes are not touched.
 * BFMatcher(NORM_HAMMING).knnMatch(kf, cur, 2) is restated, not linked: best = the lowest distance, the lowest train index on ties; second =
 * the next in (distance, train index) order, so an equal distance at a later index is the second (OpenCV's insertion order; parity with
 * OpenCV is unpinned).  Queries in ascending order; accepted when (float)d0 / (float)d1 < (float)(1.0f / 1.5f)
 * (0 / 0 is NaN and rejected) and bit 0 is set.  lineDescriptorMAD's results are dead in the reference and not computed.  With
 * n_kf_lines == 0 or n_cur_lines < 2 the reference reads past a vector's end (undefined); here the result is 0 matches, everything NULL.
 * Limits: lcap <= 256, klcap <= 256.  Memory and synchronisation as msl_bow_transform; line_xyz is in/out. */
MSL_API int msl_match_lines_by_descriptor(msl_match *h, int n_pairs, int lcap, int klcap, const uint8_t *kf_ldesc, const uint8_t *kf_line_flags,
                                          const double *kf_line_xyz, const int32_t *n_kf_lines, const uint8_t *cur_ldesc,
                                          const int32_t *n_cur_lines, msl_mem mem, int32_t *match_out, int32_t *nmatches, double *line_xyz,
                                          uint8_t *line_has, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_match_lines_by_descriptor_batch(int device, int n_pairs, int lcap, int klcap, const uint8_t *kf_ldesc,
                                                const uint8_t *kf_line_flags, const double *kf_line_xyz, const int32_t *n_kf_lines,
                                                const uint8_t *cur_ldesc, const int32_t *n_cur_lines, msl_mem mem, int32_t *match_out,
                                                int32_t *nmatches, double *line_xyz, uint8_t *line_has, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Relocalisation: the keyframe search of Tracking::Relocalization (src/Tracking.cc:1909-2055) ----
 * msl_match_keyframe_points: n_pairs independent calls of
 *     int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:680-797): th 10 / ORBdist 100 after the first pose optimisation, th 3 / ORBdist 64 after the second.
 * Current frame: the msl_match_by_projection current-frame arrays without mvuRight (`cap` entries per pair), plus
 *   cur_held[i]      CurrentFrame.mvpMapPoints[i] != NULL on entry (any non-zero byte).  A held keypoint is never handed out.
 * Keyframe (`kcap` entries per pair), per keypoint i < n_kf[f]:
 *   kf_xyz[3 i..]    GetMapPointMatches()[i]->GetWorldPos()
 *   kf_dist[2 i..]   its mfMinDistance, mfMaxDistance (raw: the 0.8f / 1.2f invariance factors are applied inside)
 *   kf_desc[32 i..]  its GetDescriptor()               kf_angle[i]  pKF->mvKeysUn[i].angle
 *   kf_flags[i]      bit 0: pMP && !pMP->isBad() && !sAlreadyFound.count(pMP)
 * Tcw: rows 0-2 of CurrentFrame.mTcw (12 floats per pair); Ow is derived from it as Frame::UpdatePoseMatrices does.
 * Out: match_out[f cap + i2] = the keyframe keypoint index this call wrote into CurrentFrame.mvpMapPoints[i2], or -1 (untouched, or
 * NULLed again by the rotation check); nmatches[f] the return value.  Keyframe-indexed like msl_match_by_bow's match_out, so one `where`
 * merges it into the pt_ref of the next msl_pose_optimize.
 * Exactly reproduced: there is no positive-depth test (a point behind the camera that projects into the image bounds is searched);
 * invzc is divided in double and rounded to float; dist3D is cv::norm (double accumulation and sqrt); PredictScale is clamped to
 * [0, nlevels - 1]; window radius th * scale_factors[level] over levels [level - 1, level + 1] with GetFeaturesInArea's level rule; the
 * best is the first minimum in walk order among the keypoints not held at that moment (dist < bestDist from 256), accepted when
 * bestDist <= orb_dist; keyframe keypoints run in ascending order, nothing is ever overwritten; the rotation histogram as in
 * msl_match_by_projection.  One divergence: with zc == 0 the projection is NaN or infinite; a NaN passes the reference's bounds test and
 * is then converted to int (undefined) -- here a non-finite u or v matches nothing.
 * Limits: cap <= 8192, kcap <= 8192, nlevels <= MSL_MATCH_MAX_LEVELS, 0 <= orb_dist <= 255 (from 256 up the reference would write
 * mvpMapPoints[-1]); anything else is refused with MSL_ERR_INVALID before any launch.  Memory and synchronisation as
 * msl_match_local_points.  Parity is relative to a sequential CPU model. */
typedef struct msl_keyframe_match_params {
    msl_match_params base;            /* fx..cy, image bounds, th (10, then 3), check_orientation, nlevels, scale_factors; bf unused */
    float log_scale_factor;           /* Frame::mfLogScaleFactor as the caller's Frame holds it */
    int32_t orb_dist;                 /* ORBdist (100, then 64) */
} msl_keyframe_match_params;
MSL_API int msl_match_keyframe_points(msl_match *h, int n_pairs, int cap, int kcap, const msl_keyframe_match_params *params,
                                      const msl_keypoint *cur_kps, const float *cur_un_xy, const int32_t *cur_grid_cell,
                                      const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_held, const float *kf_xyz,
                                      const float *kf_dist, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_flags,
                                      const int32_t *n_kf, const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *nmatches,
                                      msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_match_keyframe_points_batch(int device, int n_pairs, int cap, int kcap, const msl_keyframe_match_params *params,
                                            const msl_keypoint *cur_kps, const float *cur_un_xy, const int32_t *cur_grid_cell,
                                            const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_held, const float *kf_xyz,
                                            const float *kf_dist, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_flags,
                                            const int32_t *n_kf, const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *nmatches,
                                            msl_mem out_mem) MSL_NOEXCEPT;

/* msl_pnp_ransac: PnPsolver (src/PnPsolver.cc) as Tracking::Relocalization uses it (src/Tracking.cc:1960-2000) for n_pairs independent
 * (frame, candidate keyframe) pairs: each pair is one PnPsolver built from the pair's matches, SetRansacParameters(probability, min_inliers,
 * max_iterations, min_set, epsilon, th2) and ONE call iterate(n_iterations) on that fresh solver.  Because of the || in the loop condition
 * (:174) that call runs max(mRansacMaxIts, n_iterations) iterations unless Refine() succeeds earlier, and always ends with bNoMore.
 *
 * Correspondences (:76-96): for a current-frame keypoint i < n_kps[f], match[f][i] indexes the pair's xyz[f][kcap]; a value outside
 * [0, kcap) is NULL (the rule of msl_pose_optimize's pt_ref, so msl_match_by_bow's match_out feeds this call directly).  The valid entries
 * are taken in ascending i: mvP2D = un_xy[i], mvSigma2 = level_sigma2[octave] (octave clamped to [0, nlevels)), mvMaxError = sigma2 * th2.
 * mRansacMinInliers and mRansacMaxIts follow from their count N as in :128-147, evaluated on the host with its libm for every N <= cap and
 * uploaded as a table (rebuilt only when the RANSAC parameters or cap change).  N < mRansacMinInliers: no pose.
 *
 * Outputs per pair: status (0 none, 1 the first Refine() that succeeded -- refined count > mRansacMinInliers, :271 --, 2 the best unrefined
 * hypothesis), Tcw_out (rows 0-2 of the pose, converted to float as :205-211 / :272-278 do; the identity rows when status is 0), inlier[i]
 * per current keypoint (vbInliers), n_inliers, and pt_ref_out[i] = inlier[i] ? match[i] : -1, the `where` of Tracking.cc:1985-1994, so that
 * msl_pose_optimize follows with no element-wise step.  compute_pose runs in double and CheckInliers keeps its float / double mix (:286-312).
 *
 * Pinned where the reference is undefined or not restated (tests/pnp_model.py is the sequential model):
 *   - DUtils::Random (unseeded rand()): draw j of iteration k is fmix32(fmix32(seed[f] ^ k * 0x9E3779B1) ^ (j + 1) * 0x85EBCA77) with
 *     murmur3's 32-bit finaliser, randi = mulhi32(hash, available); the swap-with-back removal of :185-190 is kept.  seed is per pair.
 *   - cvSVD / cvSolve(CV_SVD) / cvInvert(CV_SVD): a cyclic Jacobi eigen-solver on the symmetric matrix (A^T A for the solves, the inverse
 *     and the 3x3 SVD) with a fixed round-robin pair order, 16 sweeps, no convergence branch, eigenpairs sorted by descending eigenvalue
 *     (lower index first on ties), no sign normalisation; eigenvalues at or below 1e-12 of the largest are dropped by the pseudo-inverse.
 *   - every sum over correspondences runs left to right; gauss_newton's X starts as zeros.
 * Limits: cap <= 8192, kcap <= 32768, 1 <= max_iterations <= 1024, 0 <= n_iterations <= 1024, nlevels <= MSL_MATCH_MAX_LEVELS, min_set == 4
 * (the reference's only use); anything else is refused with MSL_ERR_INVALID and msl_last_error() naming the field, before any launch.
 * Synchronisation: as msl_match_by_projection (asynchronous on the handle's stream with device memory on both sides; the first call with
 * new RANSAC parameters drains the stream once to upload the table). */
typedef struct msl_pnp_params {
    float fx, fy, cx, cy;
    int32_t nlevels;
    float level_sigma2[MSL_MATCH_MAX_LEVELS];    /* Frame::mvLevelSigma2 */
    double probability;                          /* SetRansacParameters: Tracking passes (0.99, 10, 300, 4, 0.5, 5.991) */
    int32_t min_inliers, max_iterations, min_set;
    float epsilon, th2;
    int32_t n_iterations;                        /* the argument of iterate(): Tracking passes 5 */
} msl_pnp_params;
MSL_API int msl_pnp_ransac(msl_match *h, int n_pairs, int cap, int kcap, const msl_pnp_params *params, const msl_keypoint *kps,
                           const float *un_xy, const int32_t *match, const int32_t *n_kps, const float *xyz, const uint32_t *seed, msl_mem mem,
                           float *Tcw_out, uint8_t *inlier, int32_t *pt_ref_out, int32_t *n_inliers, int32_t *status,
                           msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_pnp_ransac_batch(int device, int n_pairs, int cap, int kcap, const msl_pnp_params *params, const msl_keypoint *kps,
                                 const float *un_xy, const int32_t *match, const int32_t *n_kps, const float *xyz, const uint32_t *seed,
                                 msl_mem mem, float *Tcw_out, uint8_t *inlier, int32_t *pt_ref_out, int32_t *n_inliers, int32_t *status,
                                 msl_mem out_mem) MSL_NOEXCEPT;

/* ---- 3-D line reconstruction: Frame::GetLineDepth + Frame::Obtain3DLine (src/Frame.cc:179-186, :528-603, src/3DLineExtractor.cpp) ----
 * msl_lines_3d: for n_frames independent frames, the end-point depths of every keyline and, for every candidate keyline, one call of
 * Frame::Obtain3DLine(i, imDepth) -- the <= max_samples + 1 depth samples along the keyline, their covariances (compPt3dCov), the
 * Mahalanobis RANSAC with verify3dLine, the refit loop and the end points (extract3dline_mahdist), the acceptance test and the transform to
 * the world -- in double where the reference is in double; then the line half of the call site named by `order`, which decides where a
 * MapLine is constructed.  Per frame f (`lcap` entries per frame, keyline j < n_lines[f]):
 *   line_ends[4 j..]   mvKeylinesUn[j].startPointX, startPointY, endPointX, endPointY
 *   depth              mImDepth of the frame (CV_32F, already scaled): row r of frame f starts depth_frame_stride * f + depth_row_stride * r
 *                      BYTES after `depth`; width x height pixels
 *   line_flags[j]      bit 0: mvpMapLines[j] != NULL, bit 1: its Observations() > 0 (NULL = all 0; not read with MSL_LINE3D_ALL)
 *   Tcw[12]            rows 0-2 of the CV_32F mTcw; mRwc and mOw are derived from it (Frame::UpdatePoseMatrices)
 *   seed[j]            the sampler's seed of the keyline
 * Out, for every j < lcap (entries at or beyond n_lines[f] get -1 depths and zeros):
 *   line_depth[2 j..]  mvDepthLine[j]
 *   line_ok[j]         1 where the keyline is a candidate and Obtain3DLine returned a line; line_xyz[6 j..] its world end points A, B
 *                      (float values widened to double, as the reference stores them), six zeros otherwise
 *   n_support[j]       the supporting samples extract3dline_mahdist returned (0 when it was not reached)
 *   line_new[j]        1 where the call site constructs a MapLine from that line;  n_new[f] their number
 * Candidates have both end depths > 0 and, in the two ordered modes, are not held by a line with Observations() > 0.  A keyline's result
 * never depends on the others, so all candidates are computed and the walk is applied afterwards: in index order or in ascending
 * (min end depth, index) order, a keyline held with observations and a new line both count, a failed keyline does not, and the walk stops
 * once the count exceeds max_new_lines.  line_ok / line_xyz do not depend on the walk.
 * line_xyz and line_ok have the layout msl_match_lines_by_projection reads as last_line_xyz / bit 0 of last_line_flags, and
 * msl_pose_optimize as line_xyz / line_has.
 *
 * Pinned where the reference is undefined or not restated (tests/line3d_model.py is the sequential model):
 *   - cv::SVD: the cyclic Jacobi eigen-solver of msl_pnp_ransac (16 sweeps, round-robin pair order, descending eigenvalues, no sign
 *     normalisation) on the symmetric 3x3 matrix -- cov0 itself (its upper triangle) for a sample, P^T P of the centred inliers (sums left
 *     to right in ascending sample order) for the refit.  The Mahalanobis distance does not depend on the order or signs of DU's rows;
 *     the sign of the refit direction only swaps A and B, so the order of the end points is defined by this solver.
 *   - rand() % left: draw j of iteration k of a keyline is fmix32(fmix32(seed ^ k * 0x9E3779B1) ^ (j + 1) * 0x85EBCA77), the index
 *     mulhi32(hash, left), as in msl_pnp_ransac.
 *   - the comparison with static_cast<Vector6d>(NULL) is line_ok; numSmp == 0 and fewer than min_points samples are "no line".
 *   - GetLineDepth: an end point whose truncated coordinates fall outside the image has depth -1.0f.
 *   - non-finite values propagate by IEEE rules (a sample depth near 0.345 m makes sigma(z) zero); a NaN distance is not an inlier.
 * Limits: lcap <= 256, 1 <= max_samples <= 127, 0 <= max_iterations <= 64, min_points >= 2, order one of MSL_LINE3D_*, strides that are
 * multiples of 4 with depth_row_stride >= 4 * width; anything else is refused with MSL_ERR_INVALID and msl_last_error() naming the field,
 * before any launch.  Synchronisation: as msl_match_by_projection. */
typedef struct msl_line3d_params {
    float fx, fy, cx, cy;          /* Frame::fx .. cy; invfx = 1.0f / fx, invfy = 1.0f / fy are formed by the library in float */
    int32_t max_samples;           /* 100 */
    int32_t min_points;            /* 10  */
    int32_t max_iterations;        /* 10  */
    int32_t max_new_lines;         /* 30: the walk stops once the count exceeds it */
    double dist_thresh;            /* 1.5 (Mahalanobis) */
    double min_support;            /* 0.4: supporting samples / 2-D length */
    double min_length;             /* 0.02 m */
} msl_line3d_params;
#define MSL_LINE3D_ALL          0  /* StereoInitialization: every keyline with both end depths > 0 */
#define MSL_LINE3D_INDEX_ORDER  1  /* UpdateLastFrame: index order, the nLines > max_new_lines stop */
#define MSL_LINE3D_DEPTH_ORDER  2  /* CreateNewKeyFrame: ascending (min end depth, index), the same stop */
MSL_API int msl_lines_3d(msl_match *h, int n_frames, int lcap, int order, const msl_line3d_params *params, const float *line_ends,
                         const int32_t *n_lines, const float *depth, size_t depth_row_stride, size_t depth_frame_stride, int width,
                         int height, const uint8_t *line_flags, const float *Tcw, const uint32_t *seed, msl_mem mem, float *line_depth,
                         double *line_xyz, uint8_t *line_ok, uint8_t *line_new, int32_t *n_support, int32_t *n_new,
                         msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_lines_3d_batch(int device, int n_frames, int lcap, int order, const msl_line3d_params *params, const float *line_ends,
                               const int32_t *n_lines, const float *depth, size_t depth_row_stride, size_t depth_frame_stride, int width,
                               int height, const uint8_t *line_flags, const float *Tcw, const uint32_t *seed, msl_mem mem,
                               float *line_depth, double *line_xyz, uint8_t *line_ok, uint8_t *line_new, int32_t *n_support, int32_t *n_new,
                               msl_mem out_mem) MSL_NOEXCEPT;

/* ---- New map points: LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:303-522) ----
 * msl_triangulate_new_points: for n_items independent current keyframes KF1, each with up to ncap neighbour keyframes KF2 in covisibility
 * order: the baseline test, LocalMapping::ComputeF12 (:624-640), ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:257-406, with
 * CheckDistEpipolarLine, :127-144) and the triangulation loop with all its tests; for every created point what the MapPoint constructor,
 * ComputeDistinctiveDescriptors and UpdateNormalAndDepth (src/MapPoint.cc:282-322) give it.  The point half of SearchInNeighbors is
 * msl_fuse_candidates / msl_fuse_map_points below; the cullings and all MapPoint / KeyFrame bookkeeping stay with the caller
 * (INTEGRATION.md sections 3l, 3m).
 * Keyframes are passed once, as a table of n_tab keyframes with `cap` keypoints each; per keypoint i < n_kps[k] of keyframe k:
 *   kps_un[i]        mvKeysUn[i] (pt, angle, octave are read)         raw_xy[2 i..]  mvKeys[i].pt (UnprojectStereo reads the distorted point)
 *   uright[i]        mvuRight[i] (>= 0: a stereo keypoint)            depth[i]       mvDepth[i]
 *   desc[32 i..]     mDescriptors.row(i)                              node[i]        node_out of msl_bow_transform (-1: in no list)
 *   held[i]          any non-zero byte: GetMapPoint(i) != NULL (no isBad() test, as in the reference)
 *   Tcw[12 k..]      rows 0-2 of the CV_32F Tcw; Rwc, Ow and Twc are derived as KeyFrame::SetPose does
 * Items: cur[f] is the table index of KF1, neigh[f * ncap + r] those of its neighbours, r < n_neigh[f].  An item's neighbours are distinct
 * keyframes and none is cur[f]; items are independent and every item reads `held` as it was on entry.  A host-memory call checks all of
 * this (and the index ranges) and refuses a violation; with device memory it is the caller's contract -- an index outside the table, or
 * a neighbour equal to cur[f], is then treated as a neighbour skipped for its baseline (an invalid cur[f] as a keyframe without keypoints),
 * a repeated neighbour goes unnoticed.
 * Out, per (item f, neighbour r, idx1) at [(f * ncap + r) * cap + idx1]:
 *   match12          vMatches12[idx1] of SearchForTriangulation after the rotation cull, -1 = none
 *   status           one MSL_TRI_* code: what became of the pair (idx1, match12)
 *   nmatches[f * ncap + r]  the return value of SearchForTriangulation
 * per (item f, idx1) at [f * cap + idx1] -- every idx1 gets a point at most once per item, because the created point occupies it:
 *   new_neigh        the r whose pair created the point, -1 = none     new_idx2       its idx2 in that neighbour (-1)
 *   new_xyz[3 ..]    GetWorldPos()     new_normal[3 ..]  GetNormal()    new_dist[2 ..]  mfMinDistance, mfMaxDistance (raw)
 *   new_desc[32 ..]  GetDescriptor(): with two observations the first in creation order, the neighbour's row idx2
 *   (the layouts msl_match_local_points reads as mp_xyz, mp_normal, mp_dist, mp_desc; zeros where no point was created)
 * per item: new_order[f * cap + j], j < n_new[f] = the idx1 of the created points in creation order (neighbour order, then ascending
 * idx1), -1 beyond.  Slots beyond n_kps / n_neigh are -1 (indices) and 0 (everything else).
 * As in this reference (not upstream ORB-SLAM2) vbMatched2 is never set: every idx1 is searched on its own, two idx1 may take the same
 * idx2 and both be created; among equal distances the later idx2 wins.  The chain across neighbours is reproduced: an idx1 that got a
 * point is not searched against the later neighbours, which changes their rotation histograms.
 * Pinned where the reference is undefined or not restated (tests/triangulate_model.py is the sequential model):
 *   - cv::Mat products as cv::gemm's float kernel (double accumulation, one rounding); Mat::dot and cv::norm accumulate in double
 *   - K.inv(), K.t().inv(): the closed 3x3 form in double, each element rounded; F12 = ((K1^-T t12x) R12) K2^-1 left to right
 *   - cos(2 atan2(b / 2, depth)) = (d^2 - a^2) / (d^2 + a^2), a = b / 2, evaluated in double
 *   - cv::SVD: the cyclic Jacobi eigen-solver of msl_pnp_ransac on A^T A (double, n = 4); vt.row(3) = the eigenvector of the smallest
 *     eigenvalue, cast to float, then a float division by its fourth component
 *   - UnprojectStereo of a stereo keypoint with depth <= 0 (an empty Mat in the reference): MSL_TRI_LOW_PARALLAX
 *   - a keypoint whose octave is outside [0, nlevels) is never searched, on either side
 * Limits: cap <= 8192, ncap <= 16, n_tab <= 4096, nlevels <= MSL_MATCH_MAX_LEVELS, 1 <= n_items <= 65535; anything else, or a NULL
 * argument, is refused with MSL_ERR_INVALID before any launch, with msl_last_error() naming the field, and nothing is written (the _batch
 * form refuses before it touches a device).  Memory and synchronisation as msl_bow_transform: device pointers run asynchronously on the
 * handle's stream, with host memory on either side the call returns when the caller's buffers are its own again. */
typedef struct msl_triangulate_params {
    float fx, fy, cx, cy, invfx, invfy;          /* KeyFrame::fx .. invfy (one camera for every keyframe) */
    float bf, b;                                 /* mbf, mb */
    int32_t nlevels;                             /* mnScaleLevels */
    float scale_factors[MSL_MATCH_MAX_LEVELS];   /* mvScaleFactors */
    float level_sigma2[MSL_MATCH_MAX_LEVELS];    /* mvLevelSigma2 */
    float scale_factor;                          /* mfScaleFactor: ratioFactor = 1.5f * scale_factor */
    int32_t check_orientation;                   /* ORBmatcher::mbCheckOrientation (false at the call site) */
    int32_t only_stereo;                         /* bOnlyStereo (false at the call site) */
} msl_triangulate_params;
#define MSL_TRI_NO_MATCH           0   /* no match12 (also: idx1 taken by an earlier neighbour, or culled by the rotation histogram) */
#define MSL_TRI_TRIANGULATED       1   /* created by linear triangulation */
#define MSL_TRI_STEREO1            2   /* created by UnprojectStereo of KF1's keypoint */
#define MSL_TRI_STEREO2            3   /* created by UnprojectStereo of KF2's keypoint */
#define MSL_TRI_NEIGHBOUR_SKIPPED  4   /* baseline < b: the whole neighbour */
#define MSL_TRI_LOW_PARALLAX       5   /* no stereo and very low parallax */
#define MSL_TRI_W_ZERO             6   /* x3D(3) == 0 */
#define MSL_TRI_Z1                 7   /* z1 <= 0 */
#define MSL_TRI_Z2                 8   /* z2 <= 0 */
#define MSL_TRI_REPROJ1            9   /* reprojection error in KF1 */
#define MSL_TRI_REPROJ2           10   /* reprojection error in KF2 */
#define MSL_TRI_ZERO_DIST         11   /* dist1 == 0 || dist2 == 0 */
#define MSL_TRI_SCALE             12   /* scale consistency */
MSL_API int msl_triangulate_new_points(msl_match *h, int n_tab, int cap, int n_items, int ncap, const msl_triangulate_params *params,
                                       const msl_keypoint *kps_un, const float *raw_xy, const float *uright, const float *depth,
                                       const uint8_t *desc, const int32_t *node, const uint8_t *held, const int32_t *n_kps, const float *Tcw,
                                       const int32_t *cur, const int32_t *neigh, const int32_t *n_neigh, msl_mem mem, int32_t *match12,
                                       uint8_t *status, int32_t *nmatches, int32_t *new_neigh, int32_t *new_idx2, float *new_xyz,
                                       float *new_normal, float *new_dist, uint8_t *new_desc, int32_t *new_order, int32_t *n_new,
                                       msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_triangulate_new_points_batch(int device, int n_tab, int cap, int n_items, int ncap, const msl_triangulate_params *params,
                                             const msl_keypoint *kps_un, const float *raw_xy, const float *uright, const float *depth,
                                             const uint8_t *desc, const int32_t *node, const uint8_t *held, const int32_t *n_kps,
                                             const float *Tcw, const int32_t *cur, const int32_t *neigh, const int32_t *n_neigh, msl_mem mem,
                                             int32_t *match12, uint8_t *status, int32_t *nmatches, int32_t *new_neigh, int32_t *new_idx2,
                                             float *new_xyz, float *new_normal, float *new_dist, uint8_t *new_desc, int32_t *new_order,
                                             int32_t *n_new, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Fusing map points into neighbouring keyframes: LocalMapping::SearchInNeighbors, point half (src/LocalMapping.cc:545-569) ----
 * msl_fuse_map_points: n_items independent calls of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:408-546), each from the
 * state on entry.  msl_fuse_candidates: the de-duplicated vpFuseCandidates of :553-567.
 * Keyframes are a table of n_tab keyframes with `cap` keypoints each, as for msl_triangulate_new_points; per keypoint i < n_kps[k]:
 *   kps_un[i]        mvKeysUn[i] (pt and octave are read)              uright[i]      mvuRight[i] (>= 0: the stereo chi-square form)
 *   grid_cell[i]     the `cell` output of msl_orb_extract_frame_batch (KeyFrame::mGrid is the frame's)
 *   desc[32 i..]     mDescriptors.row(i)                                Tcw[12 k..]    rows 0-2 of the CV_32F Tcw; Ow as KeyFrame::SetPose
 *   held_id[i]       the id of GetMapPoint(i), -1 for NULL; a bad point that is still in the slot keeps its id
 * Map points are a table of n_pts points indexed by id (the layouts msl_match_local_points reads and msl_triangulate_new_points writes:
 * one item's slice of its output is a point table with id = idx1, its new_order a candidate list):
 *   pt_xyz[3 id..]   GetWorldPos()    pt_normal[3 id..]  GetNormal()    pt_dist[2 id..]  mfMinDistance, mfMaxDistance (raw; 0.8f / 1.2f inside)
 *   pt_desc[32 id..] GetDescriptor()  pt_flags[id]       bit 0: !isBad()    pt_nobs[id]   Observations()
 * msl_fuse_candidates: item f names n_targets[f] <= tcap target keyframes targets[f * tcap + t] in order.  cand[f * lcap + j] = the ids
 * held by the targets, targets in order and slots ascending, NULL and bad points left out, every id at its first occurrence only (the
 * mnFuseCandidateForKF rule).  n_cand[f] is the full count: entries beyond lcap are dropped, so the caller compares n_cand with lcap; slots
 * beyond the count are -1.
 * msl_fuse_map_points: item f fuses list[f] (a row of cand[n_lists][lcap] with n_cand[n_lists] entries; items may share a row) into the
 * keyframe tgt[f].  A list entry is a point id or -1 (NULL); the ids of one list are distinct (a second occurrence never does anything in
 * the reference -- by then the point is in the keyframe, bad, or unmatched exactly as before -- so a caller passes -1 for later duplicates
 * of GetMapPointMatches(), and that is exact).  Out, per (item f, candidate j) at [f * lcap + j]:
 *   best_idx, best_dist   bestIdx / bestDist of the search (-1 / 256 when nothing passed the filters, or the candidate left before the
 *                         search); written for every candidate that reaches the search, one that lands above th_low included
 *   status                one MSL_FUSE_* code: the exit of the loop body the candidate took
 *   other                 the id that held slot best_idx at that moment, -1 for none (and for every status below MSL_FUSE_ADDED)
 * per item: n_fused[f] = the return value.  Slots j >= n_cand[list[f]] are -1 (best_idx, other) and 0 (best_dist, status).
 * What is resolved: the search of every candidate depends only on the keyframe and the point, so it is exact whatever the order.  The
 * add / replace choice is resolved from the state on entry, candidates in ascending j, one state per slot s (holder, bad, nobs, stale):
 *   empty                   MSL_FUSE_ADDED, the holder becomes p with nobs = pt_nobs[p] + (uright[s] >= 0 ? 2 : 1) (src/MapPoint.cc:83-93)
 *   holder bad              MSL_FUSE_HELD_BAD, unchanged
 *   holder stale            MSL_FUSE_UNRESOLVED, unchanged
 *   nobs(h) > pt_nobs[p]    MSL_FUSE_REPLACED_BY_HELD, the holder is stale
 *   otherwise               MSL_FUSE_REPLACES_HELD, the holder becomes p, stale
 * Stale: the survivor's Observations() is the union of two observation sets, which the library does not know; from the third hit on one
 * slot the direction is the caller's to take from its live objects (rare).  The caller replays the results in order against its objects
 * and searches again only a survivor whose descriptor a Replace changed (tests/fuse_model.py proves the replay
 * equal to the sequential function).
 * Reproduced exactly (tests/fuse_model.py is the sequential model): p3Dc as cv::gemm's float kernel (double accumulation, one rounding);
 * invz = 1 / z a float division; x = X * invz, u = fx * x + cx, ur = u - bf * invz in float, no contraction; IsInImage with half-open
 * bounds (a non-finite projection fails it); dist3D = cv::norm and PO.dot(Pn) accumulated in double, dot < 0.5 * dist3D in double;
 * PredictScale with the raw mfMaxDistance (as msl_match_local_points); KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:469-504) without a
 * level filter, walked ix, then iy, then ascending index inside a cell; octave in [level - 1, level]; the chi-square tests compare the
 * float product e2 * inv_level_sigma2 with the doubles 7.8 (uright >= 0) and 5.99; dist < bestDist from 256, the first minimum in walk
 * order wins.
 * Pins: IsInKeyFrame(pKF) is read from the table, id in held_id[tgt][:n_kps] -- the caller keeps mObservations and mvpMapPoints
 * consistent or NULLs the candidate; a keypoint whose octave is outside [0, nlevels) is never a candidate; a held_id outside [0, n_pts)
 * is an empty slot.
 * Limits: cap <= 8192, n_tab <= 4096, n_pts <= 1048576, lcap <= 65536, tcap <= 64, n_items <= 4096, nlevels <= MSL_MATCH_MAX_LEVELS,
 * 0 <= th_low <= 255; anything else, or a NULL argument, is refused with MSL_ERR_INVALID before any launch, with msl_last_error() naming
 * the field, and nothing is written (the _batch forms refuse before they touch a device).  A host-memory call also checks the index
 * ranges (tgt, list, targets, n_targets, n_cand, every list entry) and the distinctness of each list, and refuses a violation; with device
 * memory these are the caller's contract: an index outside its table is treated as NULL, a bad tgt or list as a
 * keyframe without keypoints / an empty list, a repeated id goes unnoticed.  Memory and synchronisation as msl_bow_transform. */
typedef struct msl_fuse_params {
    float fx, fy, cx, cy, bf;                        /* KeyFrame::fx .. cy, mbf */
    float minX, maxX, minY, maxY;                    /* mnMinX .. mnMaxY (msl_frame_image_bounds) */
    float th;                                        /* 3.0 at both call sites */
    int32_t nlevels;                                 /* mnScaleLevels */
    float scale_factors[MSL_MATCH_MAX_LEVELS];       /* mvScaleFactors */
    float inv_level_sigma2[MSL_MATCH_MAX_LEVELS];    /* mvInvLevelSigma2 */
    float log_scale_factor;                          /* mfLogScaleFactor */
    int32_t th_low;                                  /* ORBmatcher::TH_LOW (50) */
} msl_fuse_params;
#define MSL_FUSE_NULL               0   /* NULL candidate (also: a slot beyond the list) */
#define MSL_FUSE_BAD                1   /* isBad() */
#define MSL_FUSE_IN_KEYFRAME        2   /* IsInKeyFrame(pKF) */
#define MSL_FUSE_BEHIND             3   /* p3Dc.z < 0 */
#define MSL_FUSE_OUT_OF_IMAGE       4   /* !IsInImage(u, v) */
#define MSL_FUSE_DISTANCE           5   /* dist3D outside [minDistance, maxDistance] */
#define MSL_FUSE_VIEW_ANGLE         6   /* PO.dot(Pn) < 0.5 * dist3D */
#define MSL_FUSE_NO_FEATURE         7   /* vIndices.empty() */
#define MSL_FUSE_NO_CANDIDATE       8   /* every index filtered out, bestDist still 256 */
#define MSL_FUSE_ABOVE_TH_LOW       9   /* bestDist > th_low */
#define MSL_FUSE_ADDED             10   /* the slot was empty: AddObservation + AddMapPoint */
#define MSL_FUSE_REPLACED_BY_HELD  11   /* pMP->Replace(pMPinKF) */
#define MSL_FUSE_REPLACES_HELD     12   /* pMPinKF->Replace(pMP) */
#define MSL_FUSE_HELD_BAD          13   /* the slot holds a bad point: counted, nothing done */
#define MSL_FUSE_UNRESOLVED        14   /* counted; the direction is the caller's (a stale holder) */
MSL_API int msl_fuse_candidates(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int tcap, int lcap, const int32_t *held_id,
                                const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *targets, const int32_t *n_targets, msl_mem mem,
                                int32_t *cand, int32_t *n_cand, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_fuse_candidates_batch(int device, int n_tab, int cap, int n_pts, int n_items, int tcap, int lcap, const int32_t *held_id,
                                      const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *targets, const int32_t *n_targets,
                                      msl_mem mem, int32_t *cand, int32_t *n_cand, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_fuse_map_points(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_lists, int lcap, const msl_fuse_params *params,
                                const msl_keypoint *kps_un, const float *uright, const int32_t *grid_cell, const uint8_t *desc,
                                const int32_t *n_kps, const float *Tcw, const int32_t *held_id, const float *pt_xyz, const float *pt_normal,
                                const float *pt_dist, const uint8_t *pt_desc, const uint8_t *pt_flags, const int32_t *pt_nobs,
                                const int32_t *tgt, const int32_t *list, const int32_t *cand, const int32_t *n_cand, msl_mem mem,
                                int32_t *best_idx, int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused,
                                msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_fuse_map_points_batch(int device, int n_tab, int cap, int n_pts, int n_items, int n_lists, int lcap,
                                      const msl_fuse_params *params, const msl_keypoint *kps_un, const float *uright, const int32_t *grid_cell,
                                      const uint8_t *desc, const int32_t *n_kps, const float *Tcw, const int32_t *held_id, const float *pt_xyz,
                                      const float *pt_normal, const float *pt_dist, const uint8_t *pt_desc, const uint8_t *pt_flags,
                                      const int32_t *pt_nobs, const int32_t *tgt, const int32_t *list, const int32_t *cand,
                                      const int32_t *n_cand, msl_mem mem, int32_t *best_idx, int32_t *best_dist, uint8_t *status,
                                      int32_t *other, int32_t *n_fused, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Refreshing map points and the covisibility of a keyframe: what LocalMapping runs right after the fusion ----
 * msl_refresh_map_points: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:210-270) and MapPoint::UpdateNormalAndDepth (:282-322)
 * for n_items distinct point ids ids[f] -- the loops of src/LocalMapping.cc:127-141 and :573-581, and as a one-item call the
 * ComputeDistinctiveDescriptors inside MapPoint::Replace.  It is the producer of pt_desc, pt_normal and pt_dist, which
 * msl_match_local_points and msl_fuse_map_points read, so the point table can stay in device memory from one keyframe to the next.
 * msl_covisibility: the counting and ordering of KeyFrame::UpdateConnections (src/KeyFrame.cc:230-299) for n_items keyframes kf[f] (table
 * indices) with threshold th (15 at the call site, :621 and :221 of src/LocalMapping.cc).
 * The observations of all points are one table in CSR form over the point table (n_pts points indexed by id, as for msl_fuse_map_points):
 *   obs_off[n_pts + 1]   the range of point id is [obs_off[id], obs_off[id + 1]); obs_off[n_pts] == n_obs_total
 *   obs_kf[o]            the keyframe table index of observation o         obs_idx[o]   its keypoint index in that keyframe
 * The order inside a range is the iteration order of mObservations (pointer order in the reference; a caller pins it, e.g. to keyframe
 * creation order).  The library never sorts it: the caller's order decides ties and the order of the float sum.
 * The keyframe table is the one of msl_fuse_map_points (kps_un: the octave is read; desc; n_kps; Tcw; held_id) with cap keypoints per
 * keyframe, plus kf_flags[k], bit 0: !isBad().  Point table: pt_xyz, pt_flags (bit 0: !isBad()) and pt_ref[id], the table index of mpRefKF.
 * msl_refresh_map_points.  what: MSL_REFRESH_DESC | MSL_REFRESH_NORMAL, at least one.  With MSL_REFRESH_DESC alone kps_un, Tcw, pt_xyz and
 * pt_ref may be NULL and desc may be any [n_tab][cap][32] descriptor table: with mLineDescriptors it is MapLine::
 * ComputeDistinctiveDescriptors (src/MapLine.cpp:195-255), the same selection over 32-byte rows (ids are then line ids, n_kps line counts).
 * Out, per item f:
 *   out_desc[32 f..], out_normal[3 f..], out_dist[2 f..]   mDescriptor; mNormalVector; mfMinDistance, mfMaxDistance -- zeros for a field
 *                                                          the reference leaves unchanged
 *   best_obs[f]      the position, in the point's own observation range, of the observation whose descriptor was chosen; -1 for none
 *   best_median[f]   its median distance (0 for none)        status[f]   MSL_REFRESH_* bits
 * pt_desc, pt_normal, pt_dist (each may be NULL; in out_mem memory): the point table.  A field that is written (status) is also written at
 * row ids[f], and only there: every other row, and the row of a field the reference leaves unchanged, keeps its bytes (a host-memory
 * table is staged whole and copied back whole; the device-memory form touches the rows alone).
 * Reproduced exactly (tests/mappoint_model.py is the sequential model):
 *   descriptor   the descriptors of the observations whose keyframe is not bad, in list order, N of them; the median of row i is the
 *                element (int)(0.5 * (N - 1)) of its sorted distances, the 0 on the diagonal included; the first i with a strictly
 *                smaller median wins (N = 1, 2: the first).  More than MSL_OBS_MAX live observations: MSL_REFRESH_TOO_MANY, the
 *                descriptor is unchanged and the caller does this point itself (the limit is the LDS budget of the selection).
 *   normal       every observation counts, bad keyframes included (UpdateNormalAndDepth has no isBad test): Ow from Tcw as KeyFrame::
 *                SetPose (cv::gemm's float kernel); normali = xyz - Ow in float; its norm the square root of a double sum; acc = acc +
 *                (float)((double)normali[a] * (1.0 / norm)) in list order from 0.0f; normal[a] = (float)((double)acc * (1.0 / n)) -- the
 *                two-observation form of msl_triangulate_new_points extended to n terms
 *   distances    max = (float)norm(xyz - Ow_ref) * scale_factors[level], min = max / scale_factors[nlevels - 1]; level = the octave of
 *                keypoint observations[pRefKF] of the reference keyframe
 * Pins: a pt_ref that is not among the point's observations has keypoint index 0 (map::operator[]); an octave outside [0, nlevels) is
 * MSL_REFRESH_BAD_OCTAVE and leaves normal and distances unchanged; non-finite values propagate by IEEE rules (a point at a camera
 * centre has a NaN normal).
 * msl_covisibility.  For every slot i < n_kps[k] of keyframe k = kf[f] whose held_id is a point of the table that is not bad, every
 * observation of that point in a keyframe other than k adds one to that keyframe's counter (a bad observer counts, the reference has no
 * test; a point held in two slots counts twice, as in the reference's slot loop).  obs_idx is not read.  Out:
 *   weight[f * n_tab + j]          KFcounter, 0 = absent
 *   conn, conn_w [f * ccap + r]    mvpOrderedConnectedKeyFrames / mvOrderedWeights: the keyframes with weight >= th by descending weight,
 *                                  equal weights by descending table index (sort of pair<int, KeyFrame*> + push_front, pointer order
 *                                  pinned to table order); if none reaches th, the single keyframe of maximum weight, the lowest index
 *                                  among equal maxima (strict > in ascending order)
 *   n_conn[f]                      the full count: entries beyond ccap are dropped, so the caller compares n_conn with ccap; slots beyond
 *                                  the count are -1 (conn) and 0 (conn_w)
 * An empty counter gives n_conn = 0 and an all-zero weight row: the reference's early return, the caller leaves its connections alone.
 * AddConnection on the other keyframes, the parent / child link and the assignment of the maps are msl_connections_apply's
 * MSL_CONN_UPDATE, which reads them from weight.
 * Limits: n_tab <= 4096, cap <= 8192, n_pts <= 1048576, n_items <= n_pts (refresh) / <= n_tab (covisibility), ccap <= n_tab, nlevels <=
 * MSL_MATCH_MAX_LEVELS, what non-zero and inside the mask; anything else, or a NULL array other than pt_desc / pt_normal / pt_dist and
 * those MSL_REFRESH_DESC alone does without (what is tested first), is refused with MSL_ERR_INVALID before any launch, with
 * msl_last_error() naming the field, and nothing is written (the _batch forms refuse before they touch a device).  A host-memory call
 * (mem) also checks the index arrays and refuses a
 * violation: obs_off ascending with obs_off[n_pts] == n_obs_total, obs_kf inside the table, obs_idx < n_kps[obs_kf], ids / kf in range,
 * ids distinct, pt_ref of every item in range.  With device memory these are the caller's contract: an observation whose obs_kf is outside
 * the table is skipped by both entries as if absent, one whose obs_idx is outside [0, cap) has no descriptor, an id outside the point table
 * is a bad point, a kf outside the table has an empty counter, a pt_ref outside the table is MSL_REFRESH_BAD_OCTAVE, a repeated id goes
 * unnoticed (its table row is written twice).  Memory and synchronisation as msl_bow_transform. */
typedef struct msl_refresh_params {
    int32_t nlevels;                                 /* mnScaleLevels */
    float scale_factors[MSL_MATCH_MAX_LEVELS];       /* mvScaleFactors */
} msl_refresh_params;
#define MSL_OBS_MAX                 256   /* the most live observations msl_refresh_map_points selects a descriptor from */
#define MSL_REFRESH_DESC              1   /* what: ComputeDistinctiveDescriptors */
#define MSL_REFRESH_NORMAL            2   /* what: UpdateNormalAndDepth */
#define MSL_REFRESH_DESC_WRITTEN      1   /* status: descriptor written */
#define MSL_REFRESH_NORMAL_WRITTEN    2   /* normal and distances written */
#define MSL_REFRESH_BAD               4   /* the point is bad: nothing */
#define MSL_REFRESH_NO_OBS            8   /* no observations: nothing */
#define MSL_REFRESH_NO_LIVE_KF       16   /* every observing keyframe is bad: descriptor unchanged (normal and distances still written) */
#define MSL_REFRESH_TOO_MANY         32   /* more than MSL_OBS_MAX observations in live keyframes: descriptor unchanged */
#define MSL_REFRESH_BAD_OCTAVE       64   /* the reference keypoint's octave is outside [0, nlevels): normal and distances unchanged */
MSL_API int msl_refresh_map_points(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int what,
                                   const msl_refresh_params *params, const msl_keypoint *kps_un, const uint8_t *desc, const int32_t *n_kps,
                                   const float *Tcw, const uint8_t *kf_flags, const int32_t *obs_off, const int32_t *obs_kf,
                                   const int32_t *obs_idx, const float *pt_xyz, const uint8_t *pt_flags, const int32_t *pt_ref,
                                   const int32_t *ids, msl_mem mem, uint8_t *out_desc, float *out_normal, float *out_dist, int32_t *best_obs,
                                   int32_t *best_median, uint8_t *status, uint8_t *pt_desc, float *pt_normal, float *pt_dist,
                                   msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_refresh_map_points_batch(int device, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int what,
                                         const msl_refresh_params *params, const msl_keypoint *kps_un, const uint8_t *desc,
                                         const int32_t *n_kps, const float *Tcw, const uint8_t *kf_flags, const int32_t *obs_off,
                                         const int32_t *obs_kf, const int32_t *obs_idx, const float *pt_xyz, const uint8_t *pt_flags,
                                         const int32_t *pt_ref, const int32_t *ids, msl_mem mem, uint8_t *out_desc, float *out_normal,
                                         float *out_dist, int32_t *best_obs, int32_t *best_median, uint8_t *status, uint8_t *pt_desc,
                                         float *pt_normal, float *pt_dist, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_covisibility(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int th,
                             const int32_t *held_id, const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *obs_off,
                             const int32_t *obs_kf, const int32_t *kf, msl_mem mem, int32_t *weight, int32_t *conn, int32_t *conn_w,
                             int32_t *n_conn, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_covisibility_batch(int device, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int th,
                                   const int32_t *held_id, const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *obs_off,
                                   const int32_t *obs_kf, const int32_t *kf, msl_mem mem, int32_t *weight, int32_t *conn, int32_t *conn_w,
                                   int32_t *n_conn, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Fusing map lines into neighbouring keyframes and refreshing them: LocalMapping::SearchInNeighbors, line half (src/LocalMapping.cc:583-618) ----
 * msl_fuse_map_lines: n_items independent calls of LSDmatcher::Fuse(pKF, vpMapLines, th) (src/LSDmatcher.cpp:259-382), each from the state
 * on entry.  msl_refresh_map_lines: MapLine::UpdateAverageDir (src/MapLine.cpp:262-308) for a batch of line ids, the only producer of the
 * ln_normal / ln_dist that msl_match_local_lines and msl_fuse_map_lines read, so the line table can stay in device memory from one keyframe
 * to the next.  The other two pieces of :583-618 are existing entries: vpLineFuseCandidates (:589-605) is msl_fuse_candidates over the line
 * held_id and ln_flags with cap = klcap; MapLine::ComputeDistinctiveDescriptors is msl_refresh_map_points with MSL_REFRESH_DESC alone.
 * Keyframes are a table of n_tab keyframes with klcap keylines each, as for msl_match_local_lines; per keyline i < n_kl[k]:
 *   kl[i]            mvKeyLines[i]: pt, angle, octave (KeyFrame::GetLinesInArea reads mvKeyLines, not the undistorted ones)
 *   ldesc[32 i..]    mLineDescriptors.row(i)                            Tcw[12 k..]    rows 0-2 of the CV_32F Tcw; Ow as KeyFrame::SetPose
 *   held_id[i]       the id of GetMapLine(i), -1 for NULL; a bad line that is still in the slot keeps its id
 * Map lines are a table of n_lines lines indexed by id, in the layouts msl_match_local_lines reads:
 *   ln_xyz[6 id..]   GetWorldPos() (double)   ln_normal[3 id..]  GetNormal() (double)   ln_dist[2 id..]  mfMinDistance, mfMaxDistance (raw;
 *   ln_desc[32 id..] GetDescriptor()          ln_flags[id]       bit 0: !isBad()        0.8f / 1.2f inside)   ln_nobs[id]   Observations()
 * msl_fuse_map_lines: tgt, list, cand[n_lists][lcap] and n_cand as for msl_fuse_map_points (items may share a row; an entry is a line id
 * or -1).  The ids of one list are distinct and the caller passes -1 for later duplicates.  What that costs: unlike a point, a repeated
 * line is searched again by the reference, can hit the slot it has just taken and add 1 to the return value (the self-hit below), which
 * SearchInNeighbors ignores; no object state differs.  Out, per (item f, candidate j) at [f * lcap + j]:
 *   best_idx, best_dist   bestIdx / bestDist of the search: -1 / INT_MAX when no keyline passed the level window, or the candidate left
 *                         before the search; bestDist starts at INT_MAX because 256 is a distance two 256-bit rows can have
 *   status                one MSL_LFUSE_* code: the exit of the loop body the candidate took
 *   other                 the id that held slot best_idx at that moment, -1 for none (and for every status below MSL_LFUSE_ADDED)
 * per item: n_fused[f] = the return value.  Slots j >= n_cand[list[f]] are -1 (best_idx, other) and 0 (best_dist, status).
 * This is not ORBmatcher::Fuse with other names:
 *   no IsInKeyFrame skip      only NULL and bad candidates leave early (:280); a line the keyframe already holds is searched again.  Best
 *                             keyline = the slot that holds it: Replace returns at src/MapLine.cpp:140, nothing changes, nFused++
 *                             (MSL_LFUSE_SELF).  Best keyline = an empty slot: AddObservation returns early (:77, nObs unchanged) but
 *                             AddMapLine writes the slot, and the line sits in two slots (MSL_LFUSE_ADDED)
 *   the projection            both depths are tested before anything is projected, with < 0.0f (Z == 0 passes, the projection is then
 *                             infinite or NaN); closed bounds tests that a NaN passes (msl_match_local_lines' projection)
 *   OM                        0.5 * (SP + EP) - Ow as the float addWeighted(SP, .5, EP, .5, 0) - Ow; dist = cv::norm, a double sum rounded
 *                             to float; a NaN passes the distance test; OM.dot(pn) with pn = the double normal converted to float,
 *                             accumulated in double, compared with 0.5 * dist in double
 *   MapLine::PredictScale     not clamped; mvScaleFactors[nPredictedLevel] clamps the index for the lookup only (the reference reads out
 *                             of bounds), the level window klLevel < L - 1 || klLevel > L uses the unclamped L with x86-64's int wrap
 *   KeyFrame::GetLinesInArea  (src/KeyFrame.cc:506-538) without a level filter, every keyline in ascending index, Frame::GetLinesInArea's
 *                             arithmetic: the double midpoint distance stored to float, slope > r * 0.01 in double without fabs, x1 == x2
 *                             gives +-inf or NaN, which passes
 *   the best keyline          strict <, so the first minimum in ascending keyline index; accepted when bestDist <= th_low
 * The add / replace choice is resolved from the state on entry, candidates in ascending j, one state per slot s (holder, bad, nobs, stale):
 *   empty                   MSL_LFUSE_ADDED, the holder becomes p with nobs = ln_nobs[p] + (p in held_id[tgt][:n_kl] ? 0 : 1); no stereo + 2
 *   holder bad              MSL_LFUSE_HELD_BAD, unchanged
 *   holder stale            MSL_LFUSE_UNRESOLVED, unchanged
 *   holder == p             MSL_LFUSE_SELF, unchanged
 *   nobs(h) > ln_nobs[p]    MSL_LFUSE_REPLACED_BY_HELD, the holder is stale
 *   otherwise               MSL_LFUSE_REPLACES_HELD, the holder becomes p, stale
 * Stale as for points.  Because nothing skips a line the keyframe holds, one line can be a candidate and a holder in the same item; its
 * ln_nobs is then the entry value although an earlier Replace of the item changed it.  The codes from MSL_LFUSE_ADDED on are therefore
 * the choice from the entry state: exact whenever neither the candidate nor the holder took part in an earlier Replace of the item, and
 * the caller's replay takes the choice from its live objects in every case (tests/linefuse_model.py proves the
 * replay equal to the sequential function).  The search (best_idx, best_dist and the codes below MSL_LFUSE_ADDED) is exact whatever the order.
 * Pins: membership of a line in the keyframe is read from the table, id in held_id[tgt][:n_kl]; a held_id outside [0, n_lines) is an empty
 * slot.
 * Limits: klcap <= 256, n_tab <= 4096, n_lines <= 1048576, lcap <= 65536, n_items <= 4096, nlevels <= MSL_MATCH_MAX_LEVELS, 0 <= th_low <=
 * 256; anything else, or a NULL argument, is refused with MSL_ERR_INVALID before any launch, with msl_last_error() naming the field, and
 * nothing is written (the _batch forms refuse before they touch a device).  A host-memory call also checks the index ranges (tgt, list,
 * n_cand, every list entry) and the distinctness of each list, and refuses a violation; with device memory these are
 * the caller's contract: an index outside its table is treated as NULL, a bad tgt as a keyframe without keylines, a bad list as an empty
 * list, a repeated id goes unnoticed; no index reads or writes outside its table.  Memory and synchronisation as msl_bow_transform.
 * msl_refresh_map_lines: n_items distinct line ids ids[f].  The observations are the CSR table of msl_refresh_map_points over the line
 * table (obs_off[n_lines + 1], obs_kf, obs_idx = the keyline index), in the caller's order inside a range (keyframe creation order pins the
 * reference's pointer order); the library never sorts it.  ln_ref[id] = the table index of mpRefKF.  Out, per item f: out_normal[3 f..]
 * (double), out_dist[2 f..] (mfMinDistance, mfMaxDistance) -- zeros where nothing was written -- and status[f], MSL_REFRESH_* bits:
 * MSL_REFRESH_NORMAL_WRITTEN, or MSL_REFRESH_BAD (a bad line), MSL_REFRESH_NO_OBS, MSL_REFRESH_BAD_OCTAVE with nothing written.  ln_normal,
 * ln_dist (each may be NULL; in out_mem memory): the line table; where the status says written, row ids[f] is written too, and only there.
 * Reproduced exactly (tests/linefuse_model.py is the sequential model):
 *   normal      OWi = the float camera centre (KeyFrame::SetPose, cv::gemm's float kernel) widened to double; middlePos = 0.5 * (head +
 *               tail) in double; normali = middlePos - OWi; normali.norm() = sqrt(x0 * x0 + (x1 * x1 + x2 * x2)), Eigen 3's unrolled
 *               reduction of a fixed 3-vector (a stated pin: parity with an Eigen build is unpinned); normal = normal + normali / norm in
 *               observation order from (0, 0, 0), n counting every observation, bad keyframes included; the result is normal / n
 *   distances   dist = the float cv::norm of (float addWeighted(SP, .5, EP, .5, 0)) - Ow(ref); mfMaxDistance = dist * scale_factors[level],
 *               level = the octave of the reference keyframe's keyline observations[pRefKF] (index 0 when the reference keyframe is not
 *               among the observations, as map::operator[] gives); mfMinDistance = mfMaxDistance / scale_factors[nlevels - 1]
 * An octave outside [0, nlevels), a ln_ref outside the table or a reference keyline outside [0, klcap) is MSL_REFRESH_BAD_OCTAVE.
 * Refresh limits: n_tab <= 4096, klcap <= 256, n_lines <= 1048576, n_items <= n_lines, nlevels <= MSL_MATCH_MAX_LEVELS; refused as above,
 * as is a NULL array other than ln_normal / ln_dist.  A host-memory call checks the CSR table and ids (in range, distinct); with device memory an observation whose obs_kf is outside the
 * table is skipped as if absent and an id outside the line table is a bad line. */
typedef struct msl_line_fuse_params {
    float fx, fy, cx, cy;                            /* KeyFrame::fx .. cy */
    float minX, maxX, minY, maxY;                    /* mnMinX .. mnMaxY (msl_frame_image_bounds) */
    float th;                                        /* 3.0 (include/LSDmatcher.h:50) */
    int32_t nlevels;                                 /* mnScaleLevels */
    float scale_factors[MSL_MATCH_MAX_LEVELS];       /* mvScaleFactors */
    float log_scale_factor;                          /* mfLogScaleFactor */
    int32_t th_low;                                  /* LSDmatcher::TH_LOW (50, src/LSDmatcher.cpp:16) */
} msl_line_fuse_params;
#define MSL_LFUSE_NULL               0   /* NULL candidate (also: a slot beyond the list) */
#define MSL_LFUSE_BAD                1   /* isBad() */
#define MSL_LFUSE_BEHIND             2   /* SPcZ < 0 || EPcZ < 0 */
#define MSL_LFUSE_OUT_OF_IMAGE       3   /* an end point outside [mnMin, mnMax] */
#define MSL_LFUSE_DISTANCE           4   /* dist outside [minDistance, maxDistance] */
#define MSL_LFUSE_VIEW_ANGLE         5   /* OM.dot(pn) < 0.5 * dist */
#define MSL_LFUSE_NO_FEATURE         6   /* vIndices.empty() */
#define MSL_LFUSE_NO_CANDIDATE       7   /* no index inside the level window, bestDist still INT_MAX */
#define MSL_LFUSE_ABOVE_TH_LOW       8   /* bestDist > th_low */
#define MSL_LFUSE_ADDED              9   /* the slot was empty: AddObservation + AddMapLine */
#define MSL_LFUSE_REPLACED_BY_HELD  10   /* pML->Replace(pMLinKF) */
#define MSL_LFUSE_REPLACES_HELD     11   /* pMLinKF->Replace(pML) */
#define MSL_LFUSE_HELD_BAD          12   /* the slot holds a bad line: counted, nothing done */
#define MSL_LFUSE_UNRESOLVED        13   /* counted; the direction is the caller's (a stale holder) */
#define MSL_LFUSE_SELF              14   /* the slot holds the candidate itself: counted, nothing done */
MSL_API int msl_fuse_map_lines(msl_match *h, int n_tab, int klcap, int n_lines, int n_items, int n_lists, int lcap,
                               const msl_line_fuse_params *params, const msl_keyline *kl, const uint8_t *ldesc, const int32_t *n_kl,
                               const float *Tcw, const int32_t *held_id, const double *ln_xyz, const double *ln_normal, const float *ln_dist,
                               const uint8_t *ln_desc, const uint8_t *ln_flags, const int32_t *ln_nobs, const int32_t *tgt,
                               const int32_t *list, const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *best_idx,
                               int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_fuse_map_lines_batch(int device, int n_tab, int klcap, int n_lines, int n_items, int n_lists, int lcap,
                                     const msl_line_fuse_params *params, const msl_keyline *kl, const uint8_t *ldesc, const int32_t *n_kl,
                                     const float *Tcw, const int32_t *held_id, const double *ln_xyz, const double *ln_normal,
                                     const float *ln_dist, const uint8_t *ln_desc, const uint8_t *ln_flags, const int32_t *ln_nobs,
                                     const int32_t *tgt, const int32_t *list, const int32_t *cand, const int32_t *n_cand, msl_mem mem,
                                     int32_t *best_idx, int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused,
                                     msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_refresh_map_lines(msl_match *h, int n_tab, int klcap, int n_lines, int n_items, int n_obs_total,
                                  const msl_refresh_params *params, const msl_keyline *kl, const int32_t *n_kl, const float *Tcw,
                                  const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const double *ln_xyz,
                                  const uint8_t *ln_flags, const int32_t *ln_ref, const int32_t *ids, msl_mem mem, double *out_normal,
                                  float *out_dist, uint8_t *status, double *ln_normal, float *ln_dist, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_refresh_map_lines_batch(int device, int n_tab, int klcap, int n_lines, int n_items, int n_obs_total,
                                        const msl_refresh_params *params, const msl_keyline *kl, const int32_t *n_kl, const float *Tcw,
                                        const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const double *ln_xyz,
                                        const uint8_t *ln_flags, const int32_t *ln_ref, const int32_t *ids, msl_mem mem,
                                        double *out_normal, float *out_dist, uint8_t *status, double *ln_normal, float *ln_dist,
                                        msl_mem out_mem) MSL_NOEXCEPT;

/* ---- The local map of a frame: Tracking::UpdateLocalMap (src/Tracking.cc:1754-1764) ----
 * The first step of Tracking::TrackLocalMap (:1350), for n_frames independent frames over one map: msl_local_keyframes is
 * UpdateLocalKeyFrames (:1813-1907); msl_local_points is UpdateLocalPoints (:1789-1810) fused with the first loop of SearchLocalPoints
 * (:1656-1668) and the gather of the rows out of the point table; msl_local_lines is UpdateLocalLines (:1766-1787) with the first loop of
 * SearchLocalLines (:1698-1710) over the line table.  The outputs of the last two are the arrays msl_match_local_points /
 * msl_match_local_lines take, so on device memory UpdateLocalMap -> SearchLocalPoints / SearchLocalLines is one chain on the handle's
 * stream with nothing in between.  tests/localmap_model.py is the sequential model.
 * The map is the tables of the LocalMapping entries: n_tab keyframes (kf_flags[k] bit 0: !isBad(); held_id[k][cap] / lheld_id[k][klcap] the
 * ids their slots hold, -1 for NULL, a bad element keeps its id; n_kps / n_kl), the point table of n_pts and the line table of n_lines rows
 * in the layouts of msl_fuse_map_points / msl_fuse_map_lines (pt_flags / ln_flags bit 0: !isBad(); pt_nobs / ln_nobs: Observations()), the
 * CSR observation table obs_off[n_pts + 1] / obs_kf of msl_refresh_map_points (obs_idx is not read).  Per keyframe k also conn[k * ccap ..]
 * and n_conn[k], exactly the rows msl_covisibility writes for kf = 0 .. n_tab - 1 (mvpOrderedConnectedKeyFrames; a ccap below 10 is the
 * caller's choice of seeing fewer than GetBestCovisibilityKeyFrames(10) would, like msl_covisibility's dropped entries), and parent[k], the
 * table index of mpParent, -1 for none.  The children of k are read as {c : parent[c] == k}.
 * Per frame f: cur_held[f * cap + i] = the id of mvpMapPoints[i], -1 for NULL (i < n_cur[f]); cur_lheld[f * lcap + j], n_cur_lines the same
 * for mvpMapLines.
 * msl_local_keyframes.  prev_kf[f * n_tab ..] / n_prev[f] (both may be NULL: empty) are the caller's mvpLocalKeyFrames on entry.  Out:
 *   votes[f * n_tab + k]     keyframeCounter, 0 = absent          ref_kf[f]     pKFmax, -1 = leave mpReferenceKF alone
 *   local_kf[f * n_tab + r]  mvpLocalKeyFrames in push order, -1 beyond n_local_kf[f]; a keyframe enters at most once, so n_tab suffices
 *   cur_cleared[f * cap + i] 1 where the slot holds a bad point: the caller NULLs it (:1825); 0 elsewhere, slots beyond n_cur included
 *   status[f]                0, or MSL_LOCALMAP_NO_VOTES
 * Reproduced exactly:
 *   votes        for every slot i < n_cur[f] whose id is a live point, every observation adds one to its keyframe's counter: a point held
 *                in two slots votes twice, a bad keyframe is counted here and filtered later
 *   empty        no counter above 0 is the early return of :1830: local_kf is a copy of prev_kf (as it stands, unchecked with device
 *                memory), ref_kf -1, MSL_LOCALMAP_NO_VOTES; UpdateLocalPoints then runs over the old list, as in the reference
 *   first loop   map<KeyFrame*, int> order is pinned to ascending table index, as msl_covisibility pins it; bad keyframes are skipped; max
 *                by strict >, so ref_kf is the lowest index among equal maxima of the live keyframes (-1 when every voted keyframe is
 *                bad: the list is then empty with status 0); every live voted keyframe is pushed
 *   second loop  walks the entries of the first loop only (the end iterator is taken before it) and stops at the top of an iteration once
 *                the list holds more than 80, so a first loop that pushes 81 or more adds nothing and a list can end at 83.  Per keyframe
 *                k: the first of conn[k][: min(10, n_conn[k], ccap)] that is live and not in the list; then the first live child not in
 *                the list, set<KeyFrame*> order pinned to ascending table index; then the parent if it is not in the list, with no isBad
 *                test -- and adding the parent leaves the whole walk (the break of :1897 is the outer loop's)
 * msl_local_points.  local_kf / n_local_kf: the outputs above (n_tab slots per frame).  Out, mcap entries per frame:
 *   local_id[f * mcap + j]   the ids of mvpLocalMapPoints in order: keyframes in list order, slots ascending below n_kps, first occurrence
 *                            only, NULL and bad points skipped; -1 beyond the count
 *   n_local[f]               the full count: entries beyond mcap are dropped and the caller compares, as with n_conn
 *   mp_xyz, mp_normal, mp_dist, mp_desc   row local_id of pt_xyz .. pt_desc, copied bit for bit; rows beyond the count keep their bytes
 *                            (a host-memory array is staged whole and copied back whole)
 *   mp_flags[f * mcap + j]   bit 0: the id is not among the live ids the frame holds (mnLastFrameSeen != F.mnId after :1664; every entry is
 *                            !isBad()), bit 1: pt_nobs > 0; 0 beyond the count
 *   cur_flags[f * cap + i]   bit 0: the slot holds a point that is not bad, bit 1: its pt_nobs > 0; 0 beyond n_cur
 * msl_local_lines: the same over lheld_id[k * klcap ..], n_kl, cur_lheld[f * lcap ..], n_cur_lines and the line table (ln_xyz double[6],
 * ln_normal double[3]); it writes local_line_id, n_local_lines, ml_xyz .. ml_flags (mlcap per frame) and cur_line_flags.
 * What stays with the caller: SetReferenceMapPoints / SetReferenceMapLines; mpReferenceKF = ref_kf; NULLing the slots cur_cleared names
 * (and those cur_flags / cur_line_flags bit 0 leaves clear); IncreaseVisible() and mnLastFrameSeen of the held elements (cur_flags) and of
 * the elements in view (in_view of the matchers); mnTrackReferenceForFrame is the call's own.
 * Local-map limits: n_frames >= 1, n_tab <= 4096, cap <= 8192, klcap <= 256, lcap <= 256, n_pts <= 1048576, n_lines <= 1048576, mcap <= 32768,
 * mlcap <= 32768, 1 <= ccap <= n_tab, n_obs_total >= 0; anything else, or a NULL array other than prev_kf / n_prev, is refused with
 * MSL_ERR_INVALID before any launch, with msl_last_error() naming the field, and nothing is written (the _batch forms refuse before they
 * touch a device).  A host-memory call (mem) also checks its index arrays and refuses a violation: the CSR table as msl_covisibility;
 * n_cur / n_cur_lines inside 0 .. cap and the ids below them -1 or inside their table; n_conn inside 0 .. ccap and its entries inside the
 * table; parent -1 or another keyframe of the table; n_prev / n_local_kf inside 0 .. n_tab and the lists' entries inside the table and
 * distinct.  With device memory these are the caller's contract: an index outside its table is absent -- an id is NULL (not cleared), an
 * obs_kf is skipped, a conn entry is no neighbour, a parent is none, a local_kf entry is a keyframe without slots; counts are clamped into
 * 0 .. their capacity; a repeated local_kf entry adds nothing (first occurrence); nothing reads or writes outside its array.
 * Scratch: a 32-bit stamp per (frame in flight, table row); frames run in groups whose stamps stay under 256 MiB.
 * Memory and synchronisation as msl_bow_transform. */
#define MSL_LOCALMAP_NO_VOTES 1   /* status: the counter was empty, local_kf is the list on entry */
MSL_API int msl_local_keyframes(msl_match *h, int n_frames, int cap, int n_tab, int n_pts, int n_obs_total, int ccap, const int32_t *cur_held,
                                const int32_t *n_cur, const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf,
                                const uint8_t *kf_flags, const int32_t *conn, const int32_t *n_conn, const int32_t *parent,
                                const int32_t *prev_kf, const int32_t *n_prev, msl_mem mem, int32_t *votes, int32_t *local_kf,
                                int32_t *n_local_kf, int32_t *ref_kf, uint8_t *cur_cleared, uint8_t *status, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_local_keyframes_batch(int device, int n_frames, int cap, int n_tab, int n_pts, int n_obs_total, int ccap,
                                      const int32_t *cur_held, const int32_t *n_cur, const uint8_t *pt_flags, const int32_t *obs_off,
                                      const int32_t *obs_kf, const uint8_t *kf_flags, const int32_t *conn, const int32_t *n_conn,
                                      const int32_t *parent, const int32_t *prev_kf, const int32_t *n_prev, msl_mem mem, int32_t *votes,
                                      int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, uint8_t *cur_cleared, uint8_t *status,
                                      msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_local_points(msl_match *h, int n_frames, int n_tab, int cap, int n_pts, int mcap, const int32_t *local_kf,
                             const int32_t *n_local_kf, const int32_t *held_id, const int32_t *n_kps, const int32_t *cur_held,
                             const int32_t *n_cur, const float *pt_xyz, const float *pt_normal, const float *pt_dist, const uint8_t *pt_desc,
                             const uint8_t *pt_flags, const int32_t *pt_nobs, msl_mem mem, int32_t *local_id, int32_t *n_local, float *mp_xyz,
                             float *mp_normal, float *mp_dist, uint8_t *mp_desc, uint8_t *mp_flags, uint8_t *cur_flags,
                             msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_local_points_batch(int device, int n_frames, int n_tab, int cap, int n_pts, int mcap, const int32_t *local_kf,
                                   const int32_t *n_local_kf, const int32_t *held_id, const int32_t *n_kps, const int32_t *cur_held,
                                   const int32_t *n_cur, const float *pt_xyz, const float *pt_normal, const float *pt_dist,
                                   const uint8_t *pt_desc, const uint8_t *pt_flags, const int32_t *pt_nobs, msl_mem mem, int32_t *local_id,
                                   int32_t *n_local, float *mp_xyz, float *mp_normal, float *mp_dist, uint8_t *mp_desc, uint8_t *mp_flags,
                                   uint8_t *cur_flags, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_local_lines(msl_match *h, int n_frames, int n_tab, int klcap, int lcap, int n_lines, int mlcap, const int32_t *local_kf,
                            const int32_t *n_local_kf, const int32_t *lheld_id, const int32_t *n_kl, const int32_t *cur_lheld,
                            const int32_t *n_cur_lines, const double *ln_xyz, const double *ln_normal, const float *ln_dist,
                            const uint8_t *ln_desc, const uint8_t *ln_flags, const int32_t *ln_nobs, msl_mem mem, int32_t *local_line_id,
                            int32_t *n_local_lines, double *ml_xyz, double *ml_normal, float *ml_dist, uint8_t *ml_desc, uint8_t *ml_flags,
                            uint8_t *cur_line_flags, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_local_lines_batch(int device, int n_frames, int n_tab, int klcap, int lcap, int n_lines, int mlcap, const int32_t *local_kf,
                                  const int32_t *n_local_kf, const int32_t *lheld_id, const int32_t *n_kl, const int32_t *cur_lheld,
                                  const int32_t *n_cur_lines, const double *ln_xyz, const double *ln_normal, const float *ln_dist,
                                  const uint8_t *ln_desc, const uint8_t *ln_flags, const int32_t *ln_nobs, msl_mem mem,
                                  int32_t *local_line_id, int32_t *n_local_lines, double *ml_xyz, double *ml_normal, float *ml_dist,
                                  uint8_t *ml_desc, uint8_t *ml_flags, uint8_t *cur_line_flags, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- The cullings of LocalMapping::Run: KeyFrameCulling (src/LocalMapping.cc:704-759) and the recent-element cullings (:227-301) ----
 * msl_cull_keyframes: n_items independent calls of LocalMapping::KeyFrameCulling over one map, each from the state on entry.  The map is
 * the tables of the other LocalMapping entries: the keyframe table of n_tab keyframes with cap keypoints each (kps_un: the octave is read;
 * uright; depth = mvDepth; held_id; n_kps) with kf_flags[k], bit 0: !isBad() (not read: the reference has no isBad test on a candidate),
 * bit 1: mbNotErase (set at src/Tracking.cc:1637 for a keyframe that created a map plane); the point table (pt_flags bit 0: !isBad(),
 * pt_nobs: Observations()); the CSR observation table obs_off / obs_kf / obs_idx of msl_refresh_map_points (obs_idx is read).
 * Item f: cand[f * ccap + r], r < n_cand[f] = GetVectorCovisibleKeyFrames() of the item's current keyframe in order -- exactly the conn /
 * n_conn rows msl_covisibility writes (an n_cand above ccap is clamped, as n_conn is the full count).  origin: the table index of the
 * keyframe with mnId == 0, or -1.  params->th_depth: mThDepth.  Out, per (item f, candidate r) at [f * ccap + r]:
 *   n_mps, n_redundant   nMPs and nRedundantObservations of the candidate's turn
 *   n_gone               the candidate's slots below n_kps whose point was live on entry and is bad at the candidate's turn
 *   status               one MSL_CULL_* code
 * Entries beyond n_cand are -1 (the counters) and 0 (status).
 * Reproduced exactly (tests/cull_model.py is the sequential model, and its literal twin):
 *   slot loop    slots i < n_kps[k]; a NULL or bad point is skipped; depth > th_depth || depth < 0 skips by the literal float tests, so a
 *                NaN depth counts; then nMPs++; a point held in two slots counts twice
 *   redundancy   only when the point's current Observations() > 3: its current observations in keyframes other than k whose keypoint
 *                octave is <= octave(i) + 1 are counted, and 3 make it redundant (the break does not change the result)
 *   verdict      (double)n_redundant > 0.9 * (double)n_mps, evaluated as 10 * n_redundant > 9 * n_mps in int, which is equal for every
 *                n_mps <= 8192; n_mps == 0 keeps the keyframe
 *   candidates   no isBad test: a bad candidate is counted and, if redundant, culled like any other; only origin is skipped without counting
 *   the chain    culling c is EraseObservation(c) on every point c holds in a slot, bad or not, once per point: the point's observation by
 *                c, if it has one, disappears and nObs drops by 2 when uright[c][obs_idx] >= 0, else by 1 (the observation's keypoint, not
 *                the slot's); a point whose nObs is then <= 2 turns bad, leaves every later candidate's n_mps, and later erasures on it do
 *                nothing.  A candidate with MSL_CULL_NOT_ERASE changes nothing for its successors
 *   inconsistent tables (msl_triangulate_new_points produces them)   an observation (c, idx) of p is erased only if c holds p in some
 *                slot below n_kps[c]; a held point that does not observe c is untouched; a point that is bad on entry has no observations,
 *                whatever the table says
 * Pin: MapPoint::SetBadFlag also NULLs slot obs_idx of every keyframe that still observes the point (EraseMapPointMatch).  Where that
 * slot holds the point itself, is empty or holds a bad point this changes nothing here.  Where it holds another live point q, the reference
 * takes q out of that keyframe's later walk; the entry does not follow that, and a caller whose tables can hold such a pair replays
 * the culled keyframes against its objects.
 * KeyFrame::SetBadFlag on the keyframes with MSL_CULL_CULLED, in order, is two logs: MSL_OBS_KF_ERASE of msl_observations_apply for the point
 * and line observations, MSL_CONN_KF_BAD of msl_connections_apply for the connections and the spanning tree.  What stays with the caller:
 * sending those logs, the database and map erasure, mTcp and the plane observations; this entry does not update the device tables.
 * msl_cull_recent: the verdict of MapPointCulling (:227-250), MapLineCulling (:252-275) and MapPlaneCulling (:277-301) for a list of n
 * recent elements: found / visible = mnFound / mnVisible, first_kf_id = mnFirstKFid, nobs = Observations(), flags bit 0: !isBad();
 * cur_kf_id = mpCurrentKeyFrame->mnId; th_obs = cnThObs (3 for points and lines, 2 for planes).  verdict[i] is the branch taken, tested in
 * the reference's order: bad; ratio < 0.25f; cur_kf_id - first_kf_id >= 2 && nobs <= th_obs; cur_kf_id - first_kf_id >= 3; none.  ratio_form
 * pins a real difference: MSL_RATIO_FLOAT is (float)found / visible (src/MapPoint.cc:205, src/MapPlane.cc:173), a float division whose
 * IEEE results for visible == 0 (inf, NaN) compare as on the CPU; MSL_RATIO_INT is (float)(found / visible), the integer division of
 * src/MapLine.cpp:190-193, which the reference divides by zero in when visible == 0 for an element that is not bad: a host-memory call
 * refuses that, with device memory the element gets MSL_RECENT_INVALID.  Ids are non-negative and their difference is taken in int.  List
 * surgery and SetBadFlag stay with the caller.
 * Cull limits: n_tab <= 4096, cap <= 8192, n_pts <= 1048576, 1 <= n_items <= 4096, n_obs_total >= 0, 1 <= ccap <= n_tab; 1 <= n <= 1048576,
 * cur_kf_id >= 0, th_obs >= 0, ratio_form one of the two; anything else, or a NULL argument, is refused with MSL_ERR_INVALID before any
 * launch, with msl_last_error() naming the field, and nothing is written (the _batch forms refuse before they touch a device).  A
 * host-memory call (mem) also checks its index arrays and refuses a violation: the CSR table as msl_covisibility, with obs_idx < n_kps;
 * n_cand inside 0 .. ccap and the entries below it inside the table and distinct; origin -1 or inside the table; found, visible and
 * first_kf_id not negative.  With device memory these are the caller's contract: an index outside its table is absent -- a cand entry gets
 * MSL_CULL_ABSENT and zero counters, an observation whose obs_kf is outside the table or whose obs_idx is outside [0, cap) is skipped, a
 * held_id outside the point table is NULL, an origin outside the table is none; a repeated candidate is walked again (its erasures are
 * already done); nothing reads or writes outside its array.  Memory and synchronisation as msl_bow_transform. */
typedef struct msl_cull_params {
    float th_depth;                                  /* KeyFrame::mThDepth */
} msl_cull_params;
#define MSL_CULL_KEPT        1   /* not redundant */
#define MSL_CULL_CULLED      2   /* redundant, SetBadFlag takes effect */
#define MSL_CULL_ORIGIN      3   /* skipped by :715, counters 0 */
#define MSL_CULL_NOT_ERASE   4   /* redundant, but SetBadFlag returned at src/KeyFrame.cc:354: no effect on later candidates */
#define MSL_CULL_ABSENT      5   /* index outside the table (device memory only), counters 0 */
#define MSL_RATIO_FLOAT      0   /* ratio_form: (float)found / visible -- points and planes */
#define MSL_RATIO_INT        1   /* ratio_form: (float)(found / visible) -- lines */
#define MSL_RECENT_KEEP        0   /* stays in the list */
#define MSL_RECENT_ERASE_BAD   1   /* already bad: drop from the list */
#define MSL_RECENT_CULL_RATIO  2   /* SetBadFlag, then drop */
#define MSL_RECENT_CULL_OBS    3   /* SetBadFlag, then drop */
#define MSL_RECENT_RETIRE      4   /* old enough: drop */
#define MSL_RECENT_INVALID     5   /* the integer ratio form with visible == 0 (device memory only) */
MSL_API int msl_cull_keyframes(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int origin,
                               const msl_cull_params *params, const msl_keypoint *kps_un, const float *uright, const float *depth,
                               const int32_t *held_id, const int32_t *n_kps, const uint8_t *kf_flags, const uint8_t *pt_flags,
                               const int32_t *pt_nobs, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx,
                               const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *n_mps, int32_t *n_redundant, int32_t *n_gone,
                               uint8_t *status, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_cull_keyframes_batch(int device, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int origin,
                                     const msl_cull_params *params, const msl_keypoint *kps_un, const float *uright, const float *depth,
                                     const int32_t *held_id, const int32_t *n_kps, const uint8_t *kf_flags, const uint8_t *pt_flags,
                                     const int32_t *pt_nobs, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx,
                                     const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *n_mps, int32_t *n_redundant,
                                     int32_t *n_gone, uint8_t *status, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_cull_recent(msl_match *h, int n, int cur_kf_id, int th_obs, int ratio_form, const int32_t *found, const int32_t *visible,
                            const int32_t *first_kf_id, const int32_t *nobs, const uint8_t *flags, msl_mem mem, uint8_t *verdict,
                            msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_cull_recent_batch(int device, int n, int cur_kf_id, int th_obs, int ratio_form, const int32_t *found, const int32_t *visible,
                                  const int32_t *first_kf_id, const int32_t *nobs, const uint8_t *flags, msl_mem mem, uint8_t *verdict,
                                  msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Editing the observation table: AddObservation, EraseObservation, SetBadFlag, Replace and the point loop of KeyFrame::SetBadFlag ----
 * msl_observations_apply executes a log of edits on the tables the other LocalMapping entries read -- the CSR observation table obs_off /
 * obs_kf / obs_idx of msl_refresh_map_points, the slots held_id of the keyframe table and the per-point arrays -- and writes the new CSR
 * table.  It is the producer of the observation table, so that table too can stay in device memory from one keyframe to the next: the
 * results of msl_triangulate_new_points, the statements of the fusion replay and the verdicts of the cullings reach it as a log of a few
 * thousand records.  It is MapPoint::AddObservation, EraseObservation, SetBadFlag and Replace
 * (src/MapPoint.cc:83-187), the MapLine forms of the same four (src/MapLine.cpp:75-172, with uright NULL and the line tables),
 * KeyFrame::AddMapPoint, EraseMapPointMatch and ReplaceMapPointMatch (src/KeyFrame.cc:185-197) and the point and line loops of
 * KeyFrame::SetBadFlag (:362-368).  tests/observations_model.py is the sequential model, and its literal twin.
 * The table: within a point's range the order is ascending obs_kf and a keyframe appears at most once (std::map's order with pointer order
 * pinned to table order); an insertion goes to its sorted place.  A new point or line is a row with an empty range on entry: the caller
 * sizes n_pts to include it.  The weight of observation (k, i) is 2 if uright[k][i] >= 0, else 1; with uright NULL every weight is 1.
 * In (mem): n_kps[n_tab]; uright[n_tab][cap] or NULL; obs_off[n_pts + 1], obs_kf, obs_idx; ops[n_ops].
 * In and out, in place (mem): held_id[n_tab][cap]; pt_flags[n_pts] (bit 0: !isBad(), the other bits keep their value); pt_nobs; pt_ref;
 * pt_found and pt_visible (mnFound / mnVisible: both given or both NULL); pt_replaced (mpReplaced, -1 = none; may be NULL).
 * Out (out_mem): obs_off_out[n_pts + 1] (from 0), obs_kf_out[ocap], obs_idx_out[ocap]: the table on exit, in arrays of its own (not the
 * entry's); op_status[n_ops]; touched[tcap]; counts[4].
 * The log is executed in order.  Op o is ops[o] = { op, a, b, c }:
 *   MSL_OBS_ADD (a = id, b = keyframe, c = keypoint)   pMP->AddObservation(pKF, c); pKF->AddMapPoint(pMP, c).  If b is not among the point's
 *                observations, (b, c) is inserted and its weight added to pt_nobs; in either case held_id[b][c] = a.  No bad test.
 *   MSL_OBS_ERASE (a = id, b = keyframe)   EraseObservation.  If b is not observed, nothing; else the weight is subtracted and the entry
 *                removed; if pt_ref[a] == b, pt_ref[a] becomes the first remaining keyframe (pin: -1 if none remains, where the reference
 *                dereferences end()); if pt_nobs[a] <= 2, MSL_OBS_SET_BAD runs on the point.
 *   MSL_OBS_SET_BAD (a = id)   SetBadFlag: bit 0 cleared, held_id[k][i] = -1 for every observation (k, i), the range emptied; pt_nobs stays.
 *   MSL_OBS_REPLACE (a = id, b = survivor)   Replace without its ComputeDistinctiveDescriptors (msl_refresh_map_points on the survivor).
 *                a == b: nothing.  Else a turns bad, pt_replaced[a] = b, its observations are taken and cleared; for each taken (k, i): if b
 *                does not observe k, held_id[k][i] = b and (k, i) joins b with its weight, else held_id[k][i] = -1; then pt_found[b] +=
 *                pt_found[a], pt_visible[b] += pt_visible[a].
 *   MSL_OBS_KF_ERASE (b = keyframe)   the point (or line) loop of KeyFrame::SetBadFlag: for i < n_kps[b] in order, MSL_OBS_ERASE(held_id[b][i],
 *                b) where the slot holds a row of the table.  Every MSL_OBS_KF_ERASE precedes every other op of the log.  The slots are
 *                those on entry: a slot an earlier cascade set to -1 belongs to a point whose range is already empty.  Pin: this is the
 *                live loop unless an observation (k, i) of a point that turns bad lies on a slot that holds another point which observes k
 *                too (tables only an inconsistent producer leaves, see msl_cull_keyframes' pin); a caller with such tables replays those
 *                keyframes itself.  SetBadFlag's two early returns, the connections and the spanning tree are MSL_CONN_KF_BAD of
 *                msl_connections_apply; the caller sends this op for MSL_CULL_CULLED alone.
 * held_id on exit is what the execution in order leaves: where several ops write one slot, the last in log order wins.
 * op_status[o]: MSL_OBS_CHANGED -- an observation list, a counter or a flag differs because of this op; MSL_OBS_TURNED_BAD -- a point went
 * from live to bad inside it (MSL_OBS_KF_ERASE: any of its points).
 * touched: ascending and distinct, the ids whose range or any per-point array differs between entry and exit; entries beyond the count are
 * -1.  msl_refresh_map_points takes an id of -1 as a bad point (its device-memory contract), so a device-memory caller passes ids = touched
 * and n_items = tcap on without reading the count.
 * counts: [0] the new n_obs_total; [1] the number of touched points, the full count even beyond tcap (as n_conn); [2] the number of
 * points that were too long; [3] the number of points live on entry and bad on exit.
 * Too long: no point may hold more than MSL_OBS_MAX observations while an op touches it.  A point an op names with more than that on
 * entry, or that an insertion (MSL_OBS_ADD, or the entries an MSL_OBS_REPLACE moves) would take beyond it, is counted in counts[2] once; the
 * op, and every later op that names a counted point, does nothing.  If counts[2] != 0 nothing else is written and the caller applies the
 * log itself: every in-place array and obs_*_out keep their bytes, counts is { n_obs_total, 0, counts[2], 0 }, op_status and touched are
 * unspecified.  Points no op names may have any length: they are copied.  (The work is done in the handle's scratch; the kernels that
 * write the caller's arrays read the count from device memory.)
 * n_obs_total of the next call: the consumers (msl_refresh_map_points, msl_covisibility, msl_local_keyframes, msl_cull_keyframes and this
 * entry) use it only to clamp obs_off into the arrays, so a device-memory caller that has not read counts[0] back passes ocap, the
 * size of the arrays: the table's own offsets end at counts[0] <= ocap.
 * Limits: n_tab <= 4096, cap <= 8192, n_pts <= 1048576, n_obs_total >= 0, 1 <= n_ops <= 65536 of which at most 256 MSL_OBS_KF_ERASE,
 * ocap >= n_obs_total + the number of MSL_OBS_ADD ops (an MSL_OBS_REPLACE moves entries, it never adds), 1 <= tcap <= n_pts; anything
 * else, a NULL array other than uright / pt_found / pt_visible / pt_replaced, or one of pt_found / pt_visible without the other, is refused
 * with MSL_ERR_INVALID before any launch, with msl_last_error() naming the field, and nothing is written (the _batch form refuses before
 * it touches a device).  A host-memory call (mem) also checks its index arrays and refuses a violation: the CSR table as
 * msl_cull_keyframes; a range that is not strictly ascending in obs_kf; an unknown op code; an op whose id, keyframe or keypoint is outside
 * n_pts, n_tab or n_kps[b]; an MSL_OBS_KF_ERASE behind another op, or more than 256 of them; an ocap below n_obs_total + the MSL_OBS_ADD ops.
 * With device memory these are the caller's contract: an op with an unknown code or a field outside its table, and an MSL_OBS_KF_ERASE
 * beyond the 256th, gets status 0 and does nothing; a held_id outside the table is skipped by MSL_OBS_KF_ERASE; an unsorted range comes out
 * sorted if an op names its point; offsets that do not ascend give ranges that overlap, and a point whose list no longer fits the scratch
 * sized for disjoint ranges is counted as too long; nothing reads or writes outside its array.
 * The result does not depend on scheduling: the log is walked in order by one wave, and every other kernel writes each byte once.
 * Memory and synchronisation as msl_bow_transform. */
typedef struct msl_obs_op {
    int32_t op;                                      /* MSL_OBS_* */
    int32_t a, b, c;                                 /* see the list above; a field an op does not read is ignored */
} msl_obs_op;
#define MSL_OBS_ADD          1
#define MSL_OBS_ERASE        2
#define MSL_OBS_SET_BAD      3
#define MSL_OBS_REPLACE      4
#define MSL_OBS_KF_ERASE     5
#define MSL_OBS_MAX_OPS      65536   /* the most ops of one log */
#define MSL_OBS_MAX_KF_ERASE 256     /* of which MSL_OBS_KF_ERASE */
#define MSL_OBS_CHANGED      1   /* op_status: a list, a counter or a flag changed because of this op */
#define MSL_OBS_TURNED_BAD   2   /* a point went from live to bad inside this op */
MSL_API int msl_observations_apply(msl_match *h, int n_tab, int cap, int n_pts, int n_obs_total, int n_ops, int ocap, int tcap,
                                   const int32_t *n_kps, const float *uright, const int32_t *obs_off, const int32_t *obs_kf,
                                   const int32_t *obs_idx, const msl_obs_op *ops, int32_t *held_id, uint8_t *pt_flags, int32_t *pt_nobs,
                                   int32_t *pt_ref, int32_t *pt_found, int32_t *pt_visible, int32_t *pt_replaced, msl_mem mem,
                                   int32_t *obs_off_out, int32_t *obs_kf_out, int32_t *obs_idx_out, uint8_t *op_status, int32_t *touched,
                                   int32_t *counts, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_observations_apply_batch(int device, int n_tab, int cap, int n_pts, int n_obs_total, int n_ops, int ocap, int tcap,
                                         const int32_t *n_kps, const float *uright, const int32_t *obs_off, const int32_t *obs_kf,
                                         const int32_t *obs_idx, const msl_obs_op *ops, int32_t *held_id, uint8_t *pt_flags,
                                         int32_t *pt_nobs, int32_t *pt_ref, int32_t *pt_found, int32_t *pt_visible, int32_t *pt_replaced,
                                         msl_mem mem, int32_t *obs_off_out, int32_t *obs_kf_out, int32_t *obs_idx_out, uint8_t *op_status,
                                         int32_t *touched, int32_t *counts, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Editing the covisibility graph and the spanning tree: AddConnection, UpdateConnections, KeyFrame::SetBadFlag ----
 * msl_connections_apply executes a log of graph edits, in order, on the tables msl_local_keyframes, msl_cull_keyframes, msl_fuse_candidates
 * and msl_reloc_candidates read: it is the producer of conn, conn_w, n_conn, parent and kf_flags bit 0, so the graph too can stay in device
 * memory from one keyframe to the next.  It is the writes of KeyFrame::UpdateConnections (src/KeyFrame.cc:
 * 266-316) behind the counting msl_covisibility does, AddConnection and UpdateBestCovisibles (:113-145), EraseConnection (:455-467) and the
 * connection and spanning-tree half of KeyFrame::SetBadFlag (:349-360 and :382-442).  tests/connections_model.py is the sequential model,
 * and its literal twin on objects.
 * In and out, in place (mem):
 *   cw[n_tab][n_tab]       row k is mConnectedKeyFrameWeights of keyframe k, 0 = absent (every weight the reference stores is >= 1)
 *   conn, conn_w [n_tab][ccap], n_conn[n_tab]   mvpOrderedConnectedKeyFrames / mvOrderedWeights in msl_covisibility's layout: n_conn is the
 *                          full count, slots beyond it are -1 (conn) and 0 (conn_w)
 *   parent[n_tab]          mpParent, -1 for none
 *   kf_flags[n_tab]        bit 0: !isBad(); bit 1: mbNotErase; bit 2: !mbFirstConnection (a new keyframe enters with flags == 1); the
 *                          other bits keep their value.  No entry of the library compares kf_flags as a whole byte
 * In (mem): weight[n_rows][n_tab], the rows msl_covisibility wrote (NULL exactly when n_rows == 0); ops[n_ops]; origin, the table index of
 * the keyframe with mnId == 0, or -1; th, 15 at both call sites.
 * Out (out_mem): op_status[n_ops]; touched[tcap]; counts[4].
 * A rebuilt row is UpdateBestCovisibles: every non-zero entry of the cw row by descending weight, equal weights by descending table index
 * (sort of pair<int, KeyFrame*> + push_front, pointer order pinned to table order as in msl_covisibility).
 * The log is executed in order.  Op o is ops[o] = { op, a, b, c }:
 *   MSL_CONN_UPDATE (a = keyframe k, b = weight row f)   the writes of UpdateConnections with KFcounter = W = weight[f], entry k read as 0.
 *                k bad: MSL_CONN_ALREADY_BAD, nothing (pin).  W all zero: MSL_CONN_EMPTY, nothing (the early return of :266).  Else, in
 *                ascending j, nmax and pKFmax by strict >; every j with W[j] >= th gets AddConnection(k, W[j]); if none reaches th, pKFmax
 *                alone.  AddConnection on j: cw[j][k] == W[j]: nothing, and row j is NOT rebuilt (the return of :121); else cw[j][k] = W[j]
 *                and row j is rebuilt from its whole map.  Then cw[k][:] = W, entries below th included, and row k of conn becomes the
 *                selected keyframes alone, ordered like a rebuilt row.  If bit 2 of kf_flags[k] is clear and k != origin: parent[k] =
 *                conn[k][0], bit 2 is set, and the status carries MSL_CONN_PARENT_SET.  Status MSL_CONN_DONE.
 *   MSL_CONN_KF_BAD (a = keyframe)   the connection and tree half of SetBadFlag.  a == origin or bit 1 set: MSL_CONN_KEPT (the two early
 *                returns).  Already bad: MSL_CONN_ALREADY_BAD, nothing (pin).  Else for every j with cw[a][j] != 0: if cw[j][a] != 0 it is
 *                cleared and row j is rebuilt from its whole map (EraseConnection); row a of cw, conn, conn_w and n_conn[a] are cleared;
 *                then the spanning-tree loop of :390-438 as written: the candidates start as { parent[a] }, the children are the live c
 *                with parent[c] == a in ascending index; per child its stored conn row (after this op's erasures) is walked in order,
 *                the weight of a link to a candidate is cw[c][.], raised by strict > from -1; the winner is re-parented to that
 *                candidate and becomes a candidate; repeated until no child has a link; the children left get parent[a].  parent[a]
 *                stays, bit 0 of kf_flags[a] is cleared.  Status MSL_CONN_DONE.  mTcp, Map::EraseKeyFrame, the database erase
 *                (msl_kfdb_erase) and the observation loops (MSL_OBS_KF_ERASE of msl_observations_apply) stay with the caller.
 * Two quirks of the reference follow and are reproduced: a row that was cut at th by its own MSL_CONN_UPDATE gains its entries below th the
 * first time a neighbour's edit rebuilds it; and a keyframe keeps a bad neighbour in its map when the neighbour's map never held it.
 * Pins: a second SetBadFlag on a bad keyframe would re-parent the children left in mspChildrens again, and an UpdateConnections on a bad
 * keyframe would put a bad child into a children set; the reference's call sites do neither, and both ops do nothing here.  A parent[a] of
 * -1 gives a candidate set without it and the children left get -1 (the reference dereferences NULL).  A ccap below a list's length is the
 * caller's choice of seeing fewer, as in msl_local_keyframes: the tree loop reads the stored row; with ccap == n_tab nothing is ever cut.
 * Weights up to INT32_MAX order correctly.
 * op_status[o]: MSL_CONN_DONE with or without MSL_CONN_PARENT_SET, or one of MSL_CONN_EMPTY, MSL_CONN_ALREADY_BAD, MSL_CONN_KEPT.
 * touched: ascending and distinct, the keyframes an executed op wrote: the updated keyframe, every keyframe whose map an AddConnection or
 * EraseConnection changed, the keyframe that turned bad, every re-parented child; entries beyond the count are -1.
 * counts: [0] the touched count, the full count even beyond tcap; [1] the keyframes turned bad; [2] the ChangeParent calls; [3] the touched
 * rows whose n_conn exceeds ccap on exit.
 * msl_fuse_targets: vpTargetKFs of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:527-543) for n_items current keyframes cur[f], the
 * producer of the targets / n_targets msl_fuse_candidates takes.  In: conn, n_conn (rows of ccap), kf_flags, nn (10) and nn2 (5).  Out:
 * targets[f * tcap ..] in push order, -1 beyond the count; n_targets[f], the full count (entries beyond tcap are dropped).  As written: of
 * the first nn neighbours of cur[f] one that is bad or already stamped is skipped; a kept one is pushed and stamped, and of its first nn2
 * neighbours those are pushed that are not bad, not stamped and not cur[f].  Second neighbours are NOT stamped, so one can appear twice, or
 * again later as a first neighbour.  Stamps start clear in every item.
 * Limits: n_tab <= 4096, 1 <= ccap <= n_tab, 0 <= n_rows <= n_tab, 1 <= n_ops <= 4096, 1 <= tcap <= n_tab (msl_connections_apply),
 * origin -1 or inside the table, th >= 1; msl_fuse_targets: 1 <= n_items <= n_tab, 1 <= nn, nn2 <= n_tab, 1 <= tcap <= 4096.  Anything else, or a NULL array
 * (weight with n_rows == 0 excepted: it is NULL exactly then), is refused with MSL_ERR_INVALID before any launch, with msl_last_error()
 * naming the field, and nothing is written (the _batch forms refuse before they touch a device).  A host-memory call (mem) also checks and
 * refuses: an op code, keyframe or weight row out of range; n_conn outside 0 .. n_tab; conn entries below the count outside the table;
 * parent outside -1 .. n_tab - 1; a negative weight in weight or cw; a cur outside the table.  With device memory these are the caller's
 * contract: a negative weight is absent; an op with an unknown code or a field outside its table gets status 0 and does nothing; a conn
 * entry outside the table is no link and no neighbour; a cur outside the table has no targets; nothing reads or writes outside its array.
 * The result does not depend on scheduling: one workgroup walks the log in order, every value that decides its control flow is read in
 * a barrier interval in which no thread writes it, rows are rebuilt by a sort of distinct keys, and every other kernel writes each byte
 * once.  Cost: the walk is sequential, and MSL_CONN_KF_BAD of a keyframe with c live children runs up to c rounds over its (child, stored
 * entry) pairs.  A keyframe of the reference has a handful of children; a log the limits allow but no map has -- 4 095 children with rows
 * of 4 096 -- holds one compute unit for seconds, so a caller on a shared device keeps ccap at what it reads (10 to 30).
 * Memory and synchronisation as msl_bow_transform. */
typedef struct msl_conn_op {
    int32_t op;                                      /* MSL_CONN_UPDATE or MSL_CONN_KF_BAD */
    int32_t a, b, c;                                 /* see the list above; c is ignored */
} msl_conn_op;
#define MSL_CONN_UPDATE       1
#define MSL_CONN_KF_BAD       2
#define MSL_CONN_MAX_OPS      4096   /* the most ops of one log */
#define MSL_CONN_DONE         1   /* op_status: the op was executed */
#define MSL_CONN_PARENT_SET   2   /* with MSL_CONN_DONE: the first connection set parent[a] */
#define MSL_CONN_EMPTY        4   /* MSL_CONN_UPDATE: the weight row is all zero, nothing */
#define MSL_CONN_ALREADY_BAD  8   /* the keyframe is bad, nothing */
#define MSL_CONN_KEPT        16   /* MSL_CONN_KF_BAD: the origin or a keyframe with mbNotErase, nothing */
MSL_API int msl_connections_apply(msl_match *h, int n_tab, int ccap, int n_rows, int n_ops, int tcap, int origin, int th,
                                  const int32_t *weight, const msl_conn_op *ops, int32_t *cw, int32_t *conn, int32_t *conn_w,
                                  int32_t *n_conn, int32_t *parent, uint8_t *kf_flags, msl_mem mem, uint8_t *op_status, int32_t *touched,
                                  int32_t *counts, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_connections_apply_batch(int device, int n_tab, int ccap, int n_rows, int n_ops, int tcap, int origin, int th,
                                        const int32_t *weight, const msl_conn_op *ops, int32_t *cw, int32_t *conn, int32_t *conn_w,
                                        int32_t *n_conn, int32_t *parent, uint8_t *kf_flags, msl_mem mem, uint8_t *op_status,
                                        int32_t *touched, int32_t *counts, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_fuse_targets(msl_match *h, int n_tab, int ccap, int n_items, int nn, int nn2, int tcap, const int32_t *conn,
                             const int32_t *n_conn, const uint8_t *kf_flags, const int32_t *cur, msl_mem mem, int32_t *targets,
                             int32_t *n_targets, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_fuse_targets_batch(int device, int n_tab, int ccap, int n_items, int nn, int nn2, int tcap, const int32_t *conn,
                                   const int32_t *n_conn, const uint8_t *kf_flags, const int32_t *cur, msl_mem mem, int32_t *targets,
                                   int32_t *n_targets, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- The hand-over from tracking to local mapping: the keyframe decision and the new stereo map points ----
 * msl_points_3d: the point half of the three call sites whose line half is msl_lines_3d -- StereoInitialization (src/Tracking.cc:560-572),
 * UpdateLastFrame (:1062-1104) and CreateNewKeyFrame (:1524-1569) -- with Frame::UnprojectStereo (src/Frame.cc:515-526) and the two MapPoint
 * constructors (src/MapPoint.cc:36-71), for n_frames independent frames with `cap` slots each.  Per frame f, slot i < n_kps[f]:
 *   kps_un[i]          mvKeysUn[i]: only x, y (the undistorted point: Frame::UnprojectStereo, unlike KeyFrame::UnprojectStereo) and octave are read
 *   depth[i]           mvDepth[i]                                 desc[32 i..]  row i of mDescriptors
 *   cur_held[i]        the id of mvpMapPoints[i], -1 for NULL, as in msl_local_points; pt_nobs[id] = Observations() over the point table of
 *                      n_pts rows (n_pts may be 0: every slot is NULL and pt_nobs is not read)
 *   Tcw[12]            rows 0-2 of the CV_32F mTcw; mRwc and mOw are derived from it (Frame::UpdatePoseMatrices)
 *   enable[f]          optional (NULL = every frame): a frame with 0 has no members and writes its "nothing" outputs, so msl_keyframe_decision's
 *                      need_kf gates the call on the device
 *   first_id[f]        optional: the id the frame's first new point gets in held_out
 * mode: MSL_POINT3D_ALL is StereoInitialization -- index order, every slot with depth > 0, cur_held and pt_nobs are not read (they may be
 * NULL), the KeyFrame form of the point; MSL_POINT3D_KEYFRAME is CreateNewKeyFrame -- the walk below, the KeyFrame form; MSL_POINT3D_FRAME is
 * UpdateLastFrame -- the same walk, the Frame form.
 * The walk, as the reference writes it: the members are the slots with depth > 0, in the order std::sort gives pair<float, int> (ascending
 * depth, then index).  A member is fresh when its slot is NULL or holds a point with Observations() < 1.  Every member walked counts, fresh or
 * held (nPoints), and the loop leaves after the member at position p when depth_p > th_depth && p + 1 > min_points.  Only the fresh members
 * walked get a point.
 * A fresh member's point: x3Dc = ((u - cx) * z * invfx, (v - cy) * z * invfy, z) as float products in that order, x3D = mRwc * x3Dc + mOw as
 * cv::gemm computes it (double accumulation, one rounding per element), mOw = -mRcw.t() * mtcw likewise.  KeyFrame form: what the
 * constructor, AddObservation, ComputeDistinctiveDescriptors and UpdateNormalAndDepth (src/MapPoint.cc:282-322) leave in a point with this
 * one observation -- byte for byte the rows msl_refresh_map_points computes for it: normal = (0 + normali / cv::norm(normali)) / 1, so a -0
 * component becomes +0; dist = {max / scale_factors[nlevels - 1], max = (float)cv::norm(PC) * scale_factors[octave]}.  Frame form
 * (src/MapPoint.cc:48-71): normal = (P - Ow) / cv::norm(P - Ow) as (float)((double)x * (1.0 / norm)), a -0 component stays; the same dist.
 * The descriptor is row i in both forms.
 * Out, per slot [f * cap + i], for every i < cap:
 *   pt_new             1 where a point is constructed
 *   cleared            1 where the call site NULLs (CreateNewKeyFrame) or overwrites (UpdateLastFrame) a held point without observations
 *   new_xyz[3], new_normal[3], new_dist[2], new_desc[32]   the point, in the layouts msl_match_local_points reads as mp_xyz .. mp_desc and the
 *                      point table keeps as pt_xyz .. pt_desc; zeros where no point was made
 *   held_out           cur_held as it stands (all -1 with MSL_POINT3D_ALL), with first_id[f] + j in the slot of the j-th created point, -1
 *                      there when first_id is NULL
 * Per frame: new_order[f * cap + j] the slots in creation order (the caller's nNextId++ order), -1 beyond n_new[f]; n_walked[f] the
 * reference's final nPoints (the number of members with MSL_POINT3D_ALL).  Slots at or beyond n_kps[f] get 0 / -1.
 * Pinned where the reference is undefined or not restated (tests/keyframe_model.py is the sequential model):
 *   - a NaN depth is no member (z > 0 is false), +inf is one and sorts last; its point is what IEEE arithmetic gives
 *   - depth == th_depth is not far: the test is depth > th_depth
 *   - an octave outside [0, nlevels) (an out-of-range read in the reference): as msl_refresh_map_points, UpdateNormalAndDepth writes
 *     nothing -- the KeyFrame form keeps the constructor's zero normal and zero distances; the Frame form has its normal and zero distances
 *   - device memory: an id outside [0, n_pts) counts as NULL (fresh, not cleared; held_out keeps it where no point is made); n_kps is
 *     clamped into 0 .. cap
 * Limits: n_frames >= 1, cap <= 8192, 0 <= n_pts <= 1048576, mode one of MSL_POINT3D_*, 1 <= nlevels <= MSL_MATCH_MAX_LEVELS, min_points >= 0;
 * anything else, or a NULL array other than enable / first_id (and cur_held / pt_nobs where they are not read), is refused with
 * MSL_ERR_INVALID before any launch, with msl_last_error() naming the field, and nothing is written (the _batch form refuses before it
 * touches a device).  A host-memory call (mem) also checks n_kps inside 0 .. cap and the ids below it -1 or inside the table.  One launch,
 * one workgroup per frame.  Memory and synchronisation as msl_bow_transform.
 *
 * msl_keyframe_decision: for n_frames independent frames, what Tracking::Track does between the pose of a frame and CreateNewKeyFrame, in
 * the reference's order.  Per frame f a record msl_keyframe_frame and the frame's arrays: depth, cur_held, outlier (mvbOutlier) with n_cur
 * (`cap` per frame); cur_lheld, line_outlier with n_cur_lines (`lcap`); plane_match[3 k + s] / plane_outlier[3 k + s] in
 * msl_plane_associate's / msl_pose_optimize's layout with n_planes (`pcap`; a negative plane_match is NULL).  The map: pt_nobs / pt_flags
 * (bit 0: !isBad()) over n_pts rows, ln_nobs over n_lines rows, held_id / n_kps of the keyframe table (n_tab rows of cap slots).
 *   step 1   only where flags has MSL_KF_TRACKED_LOCAL_MAP: the tail of TrackLocalMap (src/Tracking.cc:1365-1430).  found_pt[i] /
 *            found_line[j] = 1 where IncreaseFound() is called (held and not an outlier); n_inliers = mnMatchesInliers over points, lines
 *            (each with Observations() > 0 unless only_tracking) and map planes.  In place: an outlier map plane's plane_match becomes -1
 *            (its outlier byte stays); an outlier parallel or vertical plane's becomes -1 and its outlier byte 0.  A map plane that stays
 *            is the one IncreaseFound() is called on.  track_ok = !(frame_id < last_reloc_frame_id + max_frames && n_inliers < 20) &&
 *            !(n_inliers < 7).  Where the step is skipped: found_* are 0, n_inliers = n_inliers_in (the stale member), track_ok = the
 *            MSL_KF_TRACK_OK bit of flags.
 *   step 2   new_plane[f] = mbNewPlane after :429-436: some k < n_planes with plane_match[3 k] NULL and plane_outlier[3 k] == 0, or, where
 *            step 1 was skipped (SearchMapByCoefficients did not reset the member), the MSL_KF_NEW_PLANE bit.  UpdateCoefficientsAndPoints
 *            stays msl_map_plane_merge.
 *   step 3   only where track_ok: "Clean VO matches" (:450-465).  held_out / outlier_out and lheld_out / line_outlier_out are cur_held /
 *            outlier and cur_lheld / line_outlier with every held element of Observations() < 1 turned into -1 / 0; plain copies where
 *            !track_ok; -1 / 0 at and beyond the counts.
 *   step 4   only where track_ok, on the cleaned arrays: NeedNewKeyFrame (:1433-1508).  need_kf[f] the return value; counts[4 f..] =
 *            {nRefMatches, nTotal, nMap, nNonTrackedClose}; cond[f] the bits MSL_KF_C1A .. MSL_KF_C2.  nRefMatches is
 *            KeyFrame::TrackedMapPoints(nMinObs) (src/KeyFrame.cc:199-218) over row ref_kf of held_id.  counts and cond are 0 where the
 *            function returns before it computes them (!track_ok, only_tracking, local_mapping_stopped, the relocalisation test).
 * Types, as the reference has them: frame_id is the unsigned long mnId and the id sums (unsigned int + int) wrap at 2^32; ratioMap =
 * (float)((float)nMap / fmax(1.0f, nTotal)) divides in double (fmax's double overload) and rounds once; nRefMatches * 0.25 is a double
 * product, nRefMatches * thRefRatio a float product compared with (float)n_inliers; ratioMap < 0.3f and < thMapRatio are float comparisons.
 * What stays with the caller: IncreaseFound() itself, mlpTemporalPoints, the motion model, CreateNewKeyFrame's KeyFrame object, and the
 * outlier drop of :505-513 -- one element-wise where(outlier_out, -1, held) over msl_points_3d's held_out.
 * Pinned: a ref_kf outside the table gives nRefMatches 0; with device memory an id outside its table counts as NULL (not found, no inlier,
 * not cleaned: copied as it stands) and counts are clamped into 0 .. their capacity.
 * Limits: n_frames >= 1, cap <= 8192, lcap <= 256, pcap <= 64, n_tab <= 4096, n_pts <= 1048576, n_lines <= 1048576 (each at least 1); anything
 * else, or a NULL array, is refused as above.  A host-memory call also checks n_cur / n_cur_lines / n_kps inside 0 .. their capacity with
 * the ids below them -1 or inside their table, n_planes inside 0 .. pcap and ref_kf -1 or inside the table.  One launch, one workgroup per
 * frame.  Memory and synchronisation as msl_bow_transform. */
typedef struct msl_point3d_params {
    float fx, fy, cx, cy;          /* Frame::fx .. cy; invfx = 1.0f / fx, invfy = 1.0f / fy are formed by the library in float */
    float th_depth;                /* mThDepth */
    int32_t min_points;            /* 100 */
    int32_t nlevels;               /* mnScaleLevels */
    float scale_factors[MSL_MATCH_MAX_LEVELS];   /* mvScaleFactors */
} msl_point3d_params;
#define MSL_POINT3D_ALL       0  /* StereoInitialization: every slot with depth > 0, index order, KeyFrame form */
#define MSL_POINT3D_KEYFRAME  1  /* CreateNewKeyFrame: ascending (depth, index), the th_depth / min_points stop, KeyFrame form */
#define MSL_POINT3D_FRAME     2  /* UpdateLastFrame: the same walk, Frame form */
typedef struct msl_keyframe_frame {
    int32_t flags;                 /* MSL_KF_TRACKED_LOCAL_MAP | MSL_KF_TRACK_OK | MSL_KF_NEW_PLANE */
    int32_t frame_id;              /* mCurrentFrame.mnId */
    int32_t last_keyframe_id;      /* mnLastKeyFrameId */
    int32_t last_reloc_frame_id;   /* mnLastRelocFrameId */
    int32_t n_kfs;                 /* mpMap->KeyFramesInMap() */
    int32_t ref_kf;                /* the table row of mpReferenceKF */
    int32_t n_inliers_in;          /* mnMatchesInliers on entry: read where TrackLocalMap did not run */
    int32_t local_mapping_idle;    /* AcceptKeyFrames() */
    int32_t local_mapping_stopped; /* isStopped() || stopRequested() */
    int32_t keyframes_in_queue;    /* KeyframesInQueue() */
} msl_keyframe_frame;
typedef struct msl_keyframe_params {
    int32_t max_frames, min_frames;   /* mMaxFrames, mMinFrames */
    float th_depth;                   /* mThDepth */
    int32_t only_tracking;            /* mbOnlyTracking */
} msl_keyframe_params;
#define MSL_KF_TRACKED_LOCAL_MAP 1  /* flags: TrackLocalMap ran on this frame (step 1 runs) */
#define MSL_KF_TRACK_OK          2  /* flags: bOK, read where step 1 is skipped */
#define MSL_KF_NEW_PLANE         4  /* flags: mbNewPlane on entry, read where step 1 is skipped */
#define MSL_KF_C1A 1   /* cond: MaxFrames have passed since the last keyframe */
#define MSL_KF_C1B 2   /* cond: MinFrames have passed and local mapping is idle */
#define MSL_KF_C1C 4   /* cond: tracking is weak */
#define MSL_KF_C2  8   /* cond: few tracked points against the reference keyframe */
MSL_API int msl_points_3d(msl_match *h, int n_frames, int cap, int n_pts, int mode, const msl_point3d_params *params,
                          const msl_keypoint *kps_un, const float *depth, const uint8_t *desc, const int32_t *n_kps, const int32_t *cur_held,
                          const int32_t *pt_nobs, const float *Tcw, const int32_t *enable, const int32_t *first_id, msl_mem mem,
                          uint8_t *pt_new, uint8_t *cleared, float *new_xyz, float *new_normal, float *new_dist, uint8_t *new_desc,
                          int32_t *held_out, int32_t *new_order, int32_t *n_new, int32_t *n_walked, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_points_3d_batch(int device, int n_frames, int cap, int n_pts, int mode, const msl_point3d_params *params,
                                const msl_keypoint *kps_un, const float *depth, const uint8_t *desc, const int32_t *n_kps,
                                const int32_t *cur_held, const int32_t *pt_nobs, const float *Tcw, const int32_t *enable,
                                const int32_t *first_id, msl_mem mem, uint8_t *pt_new, uint8_t *cleared, float *new_xyz, float *new_normal,
                                float *new_dist, uint8_t *new_desc, int32_t *held_out, int32_t *new_order, int32_t *n_new, int32_t *n_walked,
                                msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_keyframe_decision(msl_match *h, int n_frames, int cap, int lcap, int pcap, int n_tab, int n_pts, int n_lines,
                                  const msl_keyframe_params *params, const msl_keyframe_frame *frames, const float *depth,
                                  const int32_t *n_cur, const int32_t *cur_held, const uint8_t *outlier, const int32_t *cur_lheld,
                                  const uint8_t *line_outlier, const int32_t *n_cur_lines, const int32_t *n_planes, const int32_t *pt_nobs,
                                  const uint8_t *pt_flags, const int32_t *ln_nobs, const int32_t *held_id, const int32_t *n_kps, msl_mem mem,
                                  int32_t *plane_match, uint8_t *plane_outlier, uint8_t *found_pt, uint8_t *found_line, int32_t *n_inliers,
                                  uint8_t *track_ok, uint8_t *new_plane, int32_t *held_out, uint8_t *outlier_out, int32_t *lheld_out,
                                  uint8_t *line_outlier_out, int32_t *counts, uint8_t *cond, int32_t *need_kf, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_keyframe_decision_batch(int device, int n_frames, int cap, int lcap, int pcap, int n_tab, int n_pts, int n_lines,
                                        const msl_keyframe_params *params, const msl_keyframe_frame *frames, const float *depth,
                                        const int32_t *n_cur, const int32_t *cur_held, const uint8_t *outlier, const int32_t *cur_lheld,
                                        const uint8_t *line_outlier, const int32_t *n_cur_lines, const int32_t *n_planes,
                                        const int32_t *pt_nobs, const uint8_t *pt_flags, const int32_t *ln_nobs, const int32_t *held_id,
                                        const int32_t *n_kps, msl_mem mem, int32_t *plane_match, uint8_t *plane_outlier, uint8_t *found_pt,
                                        uint8_t *found_line, int32_t *n_inliers, uint8_t *track_ok, uint8_t *new_plane, int32_t *held_out,
                                        uint8_t *outlier_out, int32_t *lheld_out, uint8_t *line_outlier_out, int32_t *counts, uint8_t *cond,
                                        int32_t *need_kf, msl_mem out_mem) MSL_NOEXCEPT;

/* ---- Keyframe planes: the plane half of keyframe creation and the Manhattan tables of Map ----
 * The two steps between msl_keyframe_decision and the next frame's msl_plane_associate / msl_manhattan_detect that a keyframe with planes
 * needs; with them the Manhattan-mode chain crosses a keyframe on one stream.  tests/kfplanes_model.py is the
 * sequential model; every output is an integer, a copy, or a pinned product, so every comparison is byte equality.
 *
 * msl_keyframe_planes: for n_frames independent new keyframes the plane loop of Tracking::CreateNewKeyFrame (src/Tracking.cc:1620-1645),
 * with mode MSL_KFPLANES_INIT that of Tracking::StereoInitialization (:594-602), and what the KeyFrame constructor and SetPose do with
 * planes (src/KeyFrame.cc:50-52, 74-86).  Per frame f a record msl_kfplanes_frame: enable (0: no in/out array of the frame is touched and
 * its outputs get their nothing values below, the need_kf gate as msl_points_3d's enable), kf_slot (the keyframe's row of the keyframe
 * tables), kf_id (mnId).  In (mem): plane_coef, plane_npts, n_planes, Tcw as for msl_plane_associate / msl_manhattan_detect (`pcap` per
 * frame), plane_outlier[3 k + s] as msl_keyframe_decision leaves it (only byte s = 0, mvbPlaneOutlier, is read).
 * In/out (out_mem): plane_match[3 k + s] as msl_keyframe_decision leaves it; the map-plane table mp_w / mp_flags / n_map as for
 * msl_plane_associate with mp_first_kf[j] = mnFirstKFid (`mcap` per frame), appended in place; row kf_slot of kf_Rwc / kf_coef / kf_npts in
 * exactly msl_manhattan_detect's layout (`kcap` rows per frame).
 * The walk over k < n_planes[f], MSL_KFPLANES_KEYFRAME: a parallel (s = 1) or vertical (s = 2) plane with plane_outlier[3 k] == 0 gets
 * AddParObservation / AddVerObservation; a held plane (s = 0) gets AddObservation and is MSL_KFPLANES_HELD; a plane that is not held and has
 * plane_outlier[3 k] != 0 is MSL_KFPLANES_SKIPPED; every other plane is new.  MSL_KFPLANES_INIT: every plane is new, no parallel or vertical
 * observation is made, and plane_match[3 k] becomes the new row (:601); in keyframe mode plane_match is left alone, as the reference leaves
 * mCurrentFrame.  New rows get the indices n_map[f], n_map[f] + 1, ... in ascending k (the creation order, GetAllMapPlanes() order):
 * mp_w = ComputePlaneWorldCoeff(k), bit for bit msl_plane_associate's pM_out; mp_flags = 1; mp_first_kf = kf_id; n_map[f] grows by n_new[f].
 * When mcap is exhausted that plane and every later new plane is MSL_KFPLANES_NO_ROOM and is not created.
 * Out (out_mem), rows k < n_planes[f]: kf_plane_match[3 k + s] the KeyFrame's mvpMapPlanes / mvpParallelPlanes / mvpVerticalPlanes (the
 * frame's, -1 for NULL, with the new row in s = 0 where one was made); plane_new[k]; obs_add[3 k + s] = 1 where AddObservation /
 * AddParObservation / AddVerObservation takes effect for (row, keyframe, k) -- the maps refuse a second entry for a keyframe
 * (src/MapPlane.cc:48-68), so only the first k that names a row in slot s is set; merge_into[k] in msl_map_plane_merge's layout (the new
 * row, -1 for every other plane: held planes were merged at :429-436); status[k] (MSL_KFPLANES_*).  Per frame: Twc[12] doubles for that
 * merge = Converter::toMatrix4d(GetPoseInverse()), the float Twc of KeyFrame::SetPose widened (Rwc = Rcw^T copied, Ow = -Rwc * tcw as one
 * cv::gemm: double accumulation, alpha = -1, one rounding); n_new[f]; set_not_erase[f] = 1 when :1637 is reached (keyframe mode only, a
 * MSL_KFPLANES_NO_ROOM plane included).  Row kf_slot: kf_Rwc = Rcw^T, kf_coef / kf_npts the frame's rows, zero at and beyond n_planes[f].
 * A frame with enable == 0: merge_into -1, plane_new / obs_add / status 0, kf_plane_match the frame's, n_new and set_not_erase 0, Twc
 * written; the map-plane table, the keyframe rows and plane_match keep their bytes.
 * Limits: n_frames in 1 .. 65535, pcap <= 64, mcap <= 4096, kcap <= 4096 (each at least 1), mode one of MSL_KFPLANES_*; anything else, or a
 * NULL array, is refused with MSL_ERR_INVALID before any launch with msl_last_error() naming the field, and nothing is written (the _batch
 * form refuses before it touches a device).  A host-memory call also checks n_planes inside 0 .. pcap, n_map inside 0 .. mcap, every
 * plane_match below n_planes -1 or inside [0, n_map), kf_slot inside [0, kcap) and kf_id >= 0.  Device memory: counts are clamped, a
 * plane_match outside [0, n_map) counts as NULL, a frame whose kf_slot is outside [0, kcap) counts as not enabled, and nothing is read or
 * written outside an array; no kernel writes rows k >= n_planes[f] of the per-plane outputs or rows of the map-plane table it does not
 * create: device-memory arrays keep their bytes there (a host-memory output is copied back whole: unspecified there).  One launch, one
 * wave per frame.
 *
 * msl_manhattan_observe: for n_frames independent keyframes the plane part of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:
 * 160-218) with Map::AddManhattanObservation / AddPartialManhattanObservation (src/Map.cc:247-275, keys compared as unordered sets).
 * In (mem): the frame records above, kf_plane_match (only s = 0 is read), plane_coef, n_planes, mp_flags, mp_first_kf, n_map,
 * params->mf_ver_th.  In/out (out_mem): full_tab / n_full (`fcap`) and part_tab / n_part (`qcap`) in exactly the layout and sort order
 * msl_manhattan_detect reads.  A new entry's kf is kf_slot and its ia, ib, ic are GetIndexInKeyFrame at insertion: the first k of
 * kf_plane_match that holds the row.
 * The loop, i < j < k: the planes held and not bad, their rows distinct, angle < mf_ver_th && angle > -mf_ver_th on the float dot product
 * of the coefficients, left to right (a dot product equal to the threshold, or NaN, does not pass: not msl_manhattan_detect's gate, which
 * passes both); the triples inside the angle12 gate; the pair added after its k loop; an existing key -- in the table or added earlier in
 * the loop -- is never replaced.  Two frame planes may hold one row; every occurrence of a key carries the same entry.
 * Out (out_mem): added_full[f], added_part[f]; set_not_erase[f] = 1 only where a key was really added (SetNotErase sits behind the
 * count() != 0 return); recent_plane[k], k < n_planes[f], the mlpRecentAddedMapPlanes pushes of :160-170 (held, not bad, mp_first_kf ==
 * kf_id); status[f] the bits MSL_MANHATTAN_FULL_NO_ROOM / MSL_MANHATTAN_PART_NO_ROOM: a table that cannot take all new keys of the keyframe
 * is left exactly as it was, its count included, and its added count is 0.  The merged tables are built in scratch of the handle and copied
 * back by the same launch.  A frame with enable == 0 (or, device memory, kf_slot outside [0, kcap)) adds nothing: zeros.
 * Limits: n_frames in 1 .. 65535, pcap <= 64, mcap <= 4096, fcap <= 65536, qcap <= 65536, kcap <= 4096 (each at least 1); refusals as above.
 * The limits hold one at a time: the call keeps 8 fcap + 6 qcap ints of scratch per frame on the handle (the merged tables and the lower
 * bounds of their new keys), 3.5 MiB per frame at fcap = qcap = 65536, so the batch is also bounded by n_frames * (8 fcap + 6 qcap) * 4 bytes
 * of free device memory; a call whose scratch cannot be allocated fails with MSL_ERR_HIP (out of memory) before any launch and changes nothing.
 * A host-memory call also checks n_planes, n_map, n_full and n_part inside 0 .. their capacity, kf_plane_match[3 k] below n_planes -1 or
 * inside [0, n_map), kf_slot and kf_id, and that both tables are sorted as msl_manhattan_detect requires; sorting device-memory tables is
 * the caller's contract.  One launch, one workgroup per frame.  Memory and synchronisation as msl_bow_transform. */
typedef struct msl_kfplanes_frame {
    int32_t enable;                /* 0: the frame makes no keyframe (need_kf) */
    int32_t kf_slot;               /* the keyframe's row of kf_Rwc / kf_coef / kf_npts, and the kf of its table entries */
    int32_t kf_id;                 /* mnId */
    int32_t _pad;
} msl_kfplanes_frame;
#define MSL_KFPLANES_KEYFRAME 0   /* mode: CreateNewKeyFrame */
#define MSL_KFPLANES_INIT     1   /* mode: StereoInitialization */
#define MSL_KFPLANES_SKIPPED  0   /* status: not held and an outlier (also: the frame is not enabled) */
#define MSL_KFPLANES_HELD     1   /* status: AddObservation on the held plane */
#define MSL_KFPLANES_NEW      2   /* status: a new map plane */
#define MSL_KFPLANES_NO_ROOM  3   /* status: a new map plane that mcap has no row for */
#define MSL_MANHATTAN_FULL_NO_ROOM 1   /* status: fcap cannot take the keyframe's new triples */
#define MSL_MANHATTAN_PART_NO_ROOM 2   /* status: qcap cannot take the keyframe's new pairs */
MSL_API int msl_keyframe_planes(msl_match *h, int n_frames, int pcap, int mcap, int kcap, int mode, const msl_kfplanes_frame *frames,
                                const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const float *Tcw,
                                const uint8_t *plane_outlier, msl_mem mem, int32_t *plane_match, float *mp_w, uint8_t *mp_flags,
                                int32_t *mp_first_kf, int32_t *n_map, float *kf_Rwc, float *kf_coef, int32_t *kf_npts,
                                int32_t *kf_plane_match, uint8_t *plane_new, uint8_t *obs_add, int32_t *merge_into, double *Twc,
                                int32_t *n_new, int32_t *set_not_erase, int32_t *status, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_keyframe_planes_batch(int device, int n_frames, int pcap, int mcap, int kcap, int mode, const msl_kfplanes_frame *frames,
                                      const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const float *Tcw,
                                      const uint8_t *plane_outlier, msl_mem mem, int32_t *plane_match, float *mp_w, uint8_t *mp_flags,
                                      int32_t *mp_first_kf, int32_t *n_map, float *kf_Rwc, float *kf_coef, int32_t *kf_npts,
                                      int32_t *kf_plane_match, uint8_t *plane_new, uint8_t *obs_add, int32_t *merge_into, double *Twc,
                                      int32_t *n_new, int32_t *set_not_erase, int32_t *status, msl_mem out_mem) MSL_NOEXCEPT;
MSL_API int msl_manhattan_observe(msl_match *h, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params,
                                  const msl_kfplanes_frame *frames, const int32_t *kf_plane_match, const float *plane_coef,
                                  const int32_t *n_planes, const uint8_t *mp_flags, const int32_t *mp_first_kf, const int32_t *n_map,
                                  msl_mem mem, int32_t *full_tab, int32_t *n_full, int32_t *part_tab, int32_t *n_part, int32_t *added_full,
                                  int32_t *added_part, int32_t *set_not_erase, uint8_t *recent_plane, int32_t *status,
                                  msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous). */
MSL_API int msl_manhattan_observe_batch(int device, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap,
                                        const msl_plane_params *params, const msl_kfplanes_frame *frames, const int32_t *kf_plane_match,
                                        const float *plane_coef, const int32_t *n_planes, const uint8_t *mp_flags,
                                        const int32_t *mp_first_kf, const int32_t *n_map, msl_mem mem, int32_t *full_tab, int32_t *n_full,
                                        int32_t *part_tab, int32_t *n_part, int32_t *added_full, int32_t *added_part,
                                        int32_t *set_not_erase, uint8_t *recent_plane, int32_t *status, msl_mem out_mem) MSL_NOEXCEPT;

/* msl_kfdb: a KeyFrameDatabase (src/KeyFrameDatabase.cc:38-66) on one device.  msl_kfdb_create returns NULL with msl_last_error() when no
 * device is usable.  msl_kfdb_add stores the BowVector of one keyframe exactly as msl_bow_transform wrote it (ascending int32 words, double
 * values, the count -- on the device for MSL_MEM_DEVICE) and returns its slot when the vector is stored; with device memory `h` is the
 * matcher handle that produced it and the call waits for h's stream, because it needs the count on the host (keyframe insertion is rare;
 * h may be NULL for host memory).  Slots are handed out in add order and never reused before msl_kfdb_clear, so the slot number is the
 * keyframe's position in every inverted list of the reference, which the order of the results depends on.  msl_kfdb_erase leaves a dead
 * slot; its storage comes back only at msl_kfdb_clear.  At most 8192 slots: the add beyond that is refused with MSL_ERR_OVERFLOW and
 * changes nothing.  add, erase, clear and the enqueueing of a query are serialised by a mutex inside (the reference's mMutex) and the
 * first three wait for the queries in flight; the database may be shared by threads and matcher handles of its device.  Waits, in full:
 * add / erase / clear block the caller (mutex held) on the last query's event and on the database's own copy stream, add with device
 * memory also on h's stream; no other stream of the device is stalled.
 * msl_kfdb_size: slots handed out since the last clear, and how many of them are live. */
typedef struct msl_kfdb msl_kfdb;
MSL_API msl_kfdb *msl_kfdb_create(int device) MSL_NOEXCEPT;
MSL_API void msl_kfdb_destroy(msl_kfdb *db) MSL_NOEXCEPT;
MSL_API int msl_kfdb_add(msl_kfdb *db, msl_match *h, const int32_t *bow_word, const double *bow_value, const int32_t *n_words, msl_mem mem,
                         int32_t *slot) MSL_NOEXCEPT;
MSL_API int msl_kfdb_erase(msl_kfdb *db, int slot) MSL_NOEXCEPT;
MSL_API int msl_kfdb_clear(msl_kfdb *db) MSL_NOEXCEPT;
MSL_API int msl_kfdb_size(msl_kfdb *db, int32_t *n_slots, int32_t *n_live) MSL_NOEXCEPT;
/* msl_reloc_candidates: n_frames consecutive calls of
 *     vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F)   (src/KeyFrameDatabase.cc:68-170)
 * with DBoW2's L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  bow_word / bow_value / n_words: msl_bow_transform's
 * BowVector outputs of the query frames (`cap` entries per frame).  covis[s * 10 ..]: GetBestCovisibilityKeyFrames(10) of the keyframe in
 * slot s as slots, in order, -1 terminated (n_slots rows; dead or out-of-range slots are skipped, as the reference skips a keyframe whose
 * mnRelocQuery differs).  Out: cand_out[f ccap ..] = vpRelocCandidates as slots in the reference's order, n_cand[f] the full count (only
 * the first ccap are written).  Optional (NULL = not wanted), n_slots entries per frame: words_out = mnRelocWords (0 for a keyframe
 * sharing no word), score_out = the float mRelocScore of this query (-1 for a keyframe not scored in it).
 * Exactly reproduced: lKFsSharingWords ordered by (first shared word, slot); minCommonWords = (int)(maxCommonWords * 0.8f), scored iff
 * mnRelocWords > minCommonWords; the L1 score summed in double over the common words in ascending order, -score / 2.0 rounded to float;
 * the covisibility accumulation in float in neighbour order over every neighbour that shares a word with this query, scored or not;
 * bestAccScore from 0 raised by >; retained when accScore > 0.75f * bestAccScore; each pBestKF emitted at its first occurrence.
 * The stale score: a neighbour that shares words but was not scored contributes the mRelocScore of the last query that scored it, so the
 * database keeps one float per slot across frames and calls (frame f sees what frames < f and earlier calls left).  A keyframe never scored
 * reads uninitialised memory in the reference; here it reads 0.0f.
 * Only L1_NORM is built (ORBvoc and the reference's configuration): a vocabulary of another scoring, or one on another device than the
 * handle's, is refused with MSL_ERR_INVALID.  Memory and synchronisation as msl_match_local_points; queries on one database are ordered
 * among themselves even across handles.  Parity is relative to a sequential CPU model. */
MSL_API int msl_reloc_candidates(msl_match *h, msl_kfdb *db, const msl_vocab *voc, int n_frames, int cap, int ccap, const int32_t *bow_word,
                                 const double *bow_value, const int32_t *n_words, const int32_t *covis, msl_mem mem, int32_t *cand_out,
                                 int32_t *n_cand, int32_t *words_out, float *score_out, msl_mem out_mem) MSL_NOEXCEPT;
/* Device-indexed convenience form (the shared per-device matcher handle, always synchronous; see msl_match_by_projection_batch). */
MSL_API int msl_reloc_candidates_batch(int device, msl_kfdb *db, const msl_vocab *voc, int n_frames, int cap, int ccap,
                                       const int32_t *bow_word, const double *bow_value, const int32_t *n_words, const int32_t *covis,
                                       msl_mem mem, int32_t *cand_out, int32_t *n_cand, int32_t *words_out, float *score_out,
                                       msl_mem out_mem) MSL_NOEXCEPT;

/* Batched form: n_frames keyframes in order, semantically n_frames consecutive msl_sf_fuse_resident calls.
 * Keyframe f's images start at base + f * <frame_stride> bytes (member_frame_stride may be 0: one shared
 * membership image); refs[n_frames] and poses (16 * n_frames floats, column-major Twc each) are host arrays.
 * generateSuperPixels() of all keyframes of a batch runs frame-batched on a second stream and overlaps the
 * per-keyframe map stage of the previous batch.  n_frames <= the capacity set below (default 1). */
MSL_API int msl_sf_set_batch_capacity(msl_sf *h, int max_frames) MSL_NOEXCEPT;
/* (All surfel entry points: the rows of ONE image must span less than 4 GB -- stride * rows < 2^32 bytes for gray, depth and membership images alike;
 * otherwise MSL_ERR_INVALID.  The kernels address an image with 32-bit byte offsets.) */
MSL_API int msl_sf_fuse_resident_batch(msl_sf *h, int n_frames, const int32_t *refs, const uint8_t *gray,
                                       size_t gray_stride, size_t gray_frame_stride, const float *depth,
                                       size_t depth_stride, size_t depth_frame_stride, const int32_t *member,
                                       size_t member_stride, size_t member_frame_stride, msl_mem img_mem,
                                       const float *poses_colmajor) MSL_NOEXCEPT;
/* The same call for RAW 16-bit depth images (the sensor's / the data set's format): keyframe f's depth is depth16 + f * depth16_frame_stride bytes,
 * rows depth16_stride bytes apart, and becomes metres on the device as (float)raw * depth_factor -- what Frame::Frame does on the host with
 * imDepth.convertTo(imDepthScaled, CV_32F, depthMapFactor) (src/Frame.cc:96-97, depthMapFactor = 1 / DepthMapFactor of the settings file,
 * src/Tracking.cc:133-137; OpenCV evaluates that conversion in float).  Half the depth bytes cross PCIe and the host loop disappears; the results
 * are bit-identical to msl_sf_fuse_resident_batch on the converted images.  img_mem applies to gray, depth16 and member alike. */
MSL_API int msl_sf_fuse_resident_batch_d16(msl_sf *h, int n_frames, const int32_t *refs, const uint8_t *gray,
                                           size_t gray_stride, size_t gray_frame_stride, const uint16_t *depth16,
                                           size_t depth16_stride, size_t depth16_frame_stride, float depth_factor,
                                           const int32_t *member, size_t member_stride, size_t member_frame_stride,
                                           msl_mem img_mem, const float *poses_colmajor) MSL_NOEXCEPT;
MSL_API int msl_sf_last_counters(msl_sf *h, int64_t counters[5]) MSL_NOEXCEPT;
MSL_API int msl_sf_sync(msl_sf *h) MSL_NOEXCEPT;
MSL_API int msl_sf_set_stream(msl_sf *h, void *hip_stream) MSL_NOEXCEPT;
/* ONE upload of the gray image for both consumers (round 6).  Tracking::GrabImageRGBD hands the same gray frame to the ORB extractor (Frame
 * constructor, src/Frame.cc:103) and, for keyframes, to the surfel fusion (src/SurfelMapping.cpp:160-166); with host images each handle would copy it
 * over PCIe.  After msl_sf_fuse_resident_batch[_d16] with MSL_MEM_HOST images, msl_sf_staged_gray returns the device address of the gray images that
 * call staged (frame f at *gray_dev + f * *frame_stride, rows *row_stride bytes apart) and a hipEvent_t, owned by the handle, that completes when
 * their copy has.  msl_orb_wait_event makes the extractor's stream wait for such an event; msl_orb_extract_batch(..., MSL_MEM_DEVICE, ...) then reads
 * the images in place.  The staged images stay valid until the SECOND next host-image batch is enqueued on the surfel handle: the caller lets the
 * extraction of batch k return before it enqueues batch k + 2 (msl_orb_extract_batch with host outputs is synchronous).  Three calls free them
 * sooner: msl_sf_set_batch_capacity with a new capacity, a host-image batch whose images take more bytes per frame than the staged ones, and a
 * device-memory msl_sf_fuse_resident_batch_d16 batch whose converted depth does not fit the staged depth slots.  Each waits for the surfel
 * handle's own streams only, not for work another handle enqueued on the images: the caller lets that work return first.  MSL_ERR_INVALID when
 * the handle's last batch had no host images, and after any of those three releases until the next host-image batch has run. */
MSL_API int msl_sf_staged_gray(msl_sf *h, const uint8_t **gray_dev, size_t *row_stride, size_t *frame_stride, void **uploaded_event) MSL_NOEXCEPT;


#ifdef __cplusplus
}
#endif
#endif /* MSL_H */
