// msl_pose.hip -- batched pose-only optimisation for gfx950: Optimizer::PoseOptimization (reference src/Optimizer.cc:53-590).
// Host side of msl_pose_optimize[_batch] and msl_pose_optimize_translation[_batch]; the device code and its description are in
// msl_pose_kernel.h.  This file instantiates k_pose<false>; msl_pose_translation.hip instantiates k_pose<true>.
#include "msl_pose_kernel.h"

namespace {

const char *pose_who(bool trans) { return trans ? "msl_pose_optimize_translation" : "msl_pose_optimize"; }

// Both optimisers: Rcw (the translation-only one's Manhattan rotation) is optional.
int check_pose(int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params, const msl_keypoint *kps, const float *un_xy,
               const float *uright, const int32_t *pt_ref, const int32_t *n_kps, const float *xyz, const double *line_fn, const double *line_xyz,
               const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w, const uint8_t *plane_has,
               const int32_t *n_planes, const float *Tcw, const float *, bool trans, msl_mem, uint8_t *outlier, uint8_t *line_outlier,
               uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good, msl_mem) {
    const char *who = pose_who(trans);
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(kps), MSL_NAMED(un_xy), MSL_NAMED(uright), MSL_NAMED(pt_ref), MSL_NAMED(n_kps), MSL_NAMED(xyz),
                         MSL_NAMED(line_fn), MSL_NAMED(line_xyz), MSL_NAMED(line_has), MSL_NAMED(n_lines), MSL_NAMED(plane_coef), MSL_NAMED(plane_w),
                         MSL_NAMED(plane_has), MSL_NAMED(n_planes), MSL_NAMED(Tcw), MSL_NAMED(outlier), MSL_NAMED(line_outlier),
                         MSL_NAMED(plane_outlier), MSL_NAMED(Tcw_out), MSL_NAMED(n_good)})) return MSL_ERR_INVALID;
    if (!at_least_one(who, "n_frames", n_frames) || !in_range(who, "cap", cap, 1, MAX_CAP) || !in_range(who, "xcap", xcap, 1, MAX_XCAP) ||
        !in_range(who, "lcap", lcap, 1, MAX_KLCAP) || !in_range(who, "pcap", pcap, 1, MAX_PCAP) || !levels_ok(who, params->nlevels)) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_pose(msl_match *h, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *prm, const msl_keypoint *kps,
                const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps, const float *xyz, const double *line_fn,
                const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w,
                const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw, const float *Rcw, bool trans, msl_mem mem, uint8_t *outlier,
                uint8_t *line_outlier, uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, n = F * cap, x = F * xcap, l = F * lcap, p = F * pcap;
    PoseDevT D{};
    D.cap = cap; D.xcap = xcap; D.lcap = lcap; D.pcap = pcap; D.prm = *prm;
    D.deltaMono = (double)(float)std::sqrt(5.991); D.deltaStereo = (double)(float)std::sqrt(7.815);   // Optimizer.cc:88-89 (const float)
    D.deltaPlane = std::sqrt(prm->plane_chi); D.deltaPlaneVP = std::sqrt(prm->plane_chi_vp);
    Stage S(h, mem, out_mem);
    D.kps = S.in(kps, n); D.unxy = S.in(un_xy, 2 * n); D.uright = S.in(uright, n); D.ptRef = S.in(pt_ref, n); D.nKps = S.in(n_kps, F);
    D.xyz = S.in(xyz, 3 * x); D.lineFn = S.in(line_fn, 3 * l); D.lineXyz = S.in(line_xyz, 6 * l); D.lineHas = S.in(line_has, l);
    D.nLines = S.in(n_lines, F); D.planeCoef = S.in(plane_coef, 4 * p); D.planeW = S.in(plane_w, 12 * p); D.planeHas = S.in(plane_has, p);
    D.nPlanes = S.in(n_planes, F); D.Tcw = S.in(Tcw, 12 * F);
    D.Rcw = S.in(Rcw, 9 * F);                                                    // optional
    D.outlier = S.inout(outlier, n); D.lineOutlier = S.inout(line_outlier, l); D.planeOutlier = S.inout(plane_outlier, 3 * p);
    D.TcwOut = S.out(Tcw_out, 12 * F); D.nGood = S.out(n_good, F);
    MSL_HIP_TRY(S.error());
    if (trans) {
        MSL_HIP_TRY(launch_pose_translation(D, n_frames, st));
    } else {
        hipLaunchKernelGGL(k_pose<false>, dim3((unsigned)n_frames), dim3(NT), 0, st, static_cast<const PoseDev &>(D));
        MSL_HIP_TRY(hipGetLastError());
    }
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

constexpr const float *NO_RCW = nullptr;   // msl_pose_optimize has no Manhattan rotation

}  // namespace

extern "C" {

int msl_pose_optimize(msl_match *h, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params, const msl_keypoint *kps,
                      const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps, const float *xyz, const double *line_fn,
                      const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w,
                      const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw, msl_mem mem, uint8_t *outlier, uint8_t *line_outlier,
                      uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good, msl_mem out_mem) noexcept {
    try {
    return handle_form(pose_who(false), check_pose, launch_pose, h, n_frames, cap, xcap, lcap, pcap, params, kps, un_xy, uright, pt_ref, n_kps, xyz, line_fn,
                       line_xyz, line_has, n_lines, plane_coef, plane_w, plane_has, n_planes, Tcw, NO_RCW, false, mem, outlier, line_outlier, plane_outlier,
                       Tcw_out, n_good, out_mem);
    } MSL_ABI_CATCH_INT
}

// In the _batch forms the outlier flags are inputs too: device-memory ones are read as well.
int msl_pose_optimize_batch(int device, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                            const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps,
                            const float *xyz, const double *line_fn, const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines,
                            const float *plane_coef, const float *plane_w, const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw,
                            msl_mem mem, uint8_t *outlier, uint8_t *line_outlier, uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good,
                            msl_mem out_mem) noexcept {
    try {
    return batch_form(check_pose, launch_pose, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, cap, xcap, lcap, pcap, params, kps, un_xy,
                      uright, pt_ref, n_kps, xyz, line_fn, line_xyz, line_has, n_lines, plane_coef, plane_w, plane_has, n_planes, Tcw, NO_RCW, false, mem,
                      outlier, line_outlier, plane_outlier, Tcw_out, n_good, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_pose_optimize_translation(msl_match *h, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                                  const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps,
                                  const float *xyz, const double *line_fn, const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines,
                                  const float *plane_coef, const float *plane_w, const uint8_t *plane_has, const int32_t *n_planes,
                                  const float *Tcw, const float *Rcw, msl_mem mem, uint8_t *outlier, uint8_t *line_outlier,
                                  uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good, msl_mem out_mem) noexcept {
    try {
    return handle_form(pose_who(true), check_pose, launch_pose, h, n_frames, cap, xcap, lcap, pcap, params, kps, un_xy, uright, pt_ref, n_kps, xyz, line_fn,
                       line_xyz, line_has, n_lines, plane_coef, plane_w, plane_has, n_planes, Tcw, Rcw, true, mem, outlier, line_outlier, plane_outlier,
                       Tcw_out, n_good, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_pose_optimize_translation_batch(int device, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                                        const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref,
                                        const int32_t *n_kps, const float *xyz, const double *line_fn, const double *line_xyz,
                                        const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w,
                                        const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw, const float *Rcw, msl_mem mem,
                                        uint8_t *outlier, uint8_t *line_outlier, uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good,
                                        msl_mem out_mem) noexcept {
    try {
    return batch_form(check_pose, launch_pose, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, cap, xcap, lcap, pcap, params, kps, un_xy,
                      uright, pt_ref, n_kps, xyz, line_fn, line_xyz, line_has, n_lines, plane_coef, plane_w, plane_has, n_planes, Tcw, Rcw, true, mem, outlier,
                      line_outlier, plane_outlier, Tcw_out, n_good, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
