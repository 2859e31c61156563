// msl_pose.hip -- batched pose-only optimisation for gfx950: Optimizer::PoseOptimization (reference src/Optimizer.cc:53-590).
// Host side of msl_pose_optimize[_batch] and msl_pose_optimize_translation[_batch]; the device code and its description are in
// msl_pose_kernel.h.  This file instantiates k_pose<false>; msl_pose_translation.hip instantiates k_pose<true>.
#include "msl_pose_kernel.h"

namespace {

int run_pose(msl_match *h, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *prm, const msl_keypoint *kps,
             const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps, const float *xyz, const double *line_fn,
             const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w,
             const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw, const float *Rcw, bool trans, msl_mem mem, uint8_t *outlier,
             uint8_t *line_outlier, uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good, msl_mem out_mem) {
    const char *name = trans ? "msl_pose_optimize_translation" : "msl_pose_optimize";
    if (!h || n_frames < 1 || cap < 1 || cap > MAX_CAP || xcap < 1 || xcap > MAX_XCAP || lcap < 1 || lcap > MAX_LCAP || pcap < 1 ||
        pcap > MAX_PCAP || !prm || prm->nlevels < 1 || prm->nlevels > MSL_MATCH_MAX_LEVELS || !kps || !un_xy || !uright || !pt_ref || !n_kps ||
        !xyz || !line_fn || !line_xyz || !line_has || !n_lines || !plane_coef || !plane_w || !plane_has || !n_planes || !Tcw || !outlier ||
        !line_outlier || !plane_outlier || !Tcw_out || !n_good) {
        set_error("%s: invalid argument (1 <= cap <= %d, xcap <= %d, lcap <= %d, pcap <= %d, nlevels <= %d)", name, MAX_CAP, MAX_XCAP,
                  MAX_LCAP, MAX_PCAP, MSL_MATCH_MAX_LEVELS);
        return MSL_ERR_INVALID;
    }
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, n = F * cap, x = F * xcap, l = F * lcap, p = F * pcap;
    PoseDevT D{};
    D.cap = cap; D.xcap = xcap; D.lcap = lcap; D.pcap = pcap; D.prm = *prm;
    D.deltaMono = (double)(float)std::sqrt(5.991); D.deltaStereo = (double)(float)std::sqrt(7.815);   // Optimizer.cc:88-89 (const float)
    D.deltaPlane = std::sqrt(prm->plane_chi); D.deltaPlaneVP = std::sqrt(prm->plane_chi_vp);
    const void *src[15] = {kps, un_xy, uright, pt_ref, n_kps, xyz, line_fn, line_xyz, line_has, n_lines, plane_coef, plane_w, plane_has, n_planes, Tcw};
    const size_t bytes[15] = {sizeof(msl_keypoint) * n, 8 * n, 4 * n, 4 * n, 4 * F, 12 * x, 24 * l, 48 * l, l, 4 * F, 16 * p, 48 * p, p, 4 * F, 48 * F};
    void *dev[15];
    MSL_HIP_TRY(stage(src, bytes, 15, 15, mem, h->poseIn, st, dev));
    D.kps = (const msl_keypoint *)dev[0]; D.unxy = (const float *)dev[1]; D.uright = (const float *)dev[2]; D.ptRef = (const int32_t *)dev[3];
    D.nKps = (const int32_t *)dev[4]; D.xyz = (const float *)dev[5]; D.lineFn = (const double *)dev[6]; D.lineXyz = (const double *)dev[7];
    D.lineHas = (const uint8_t *)dev[8]; D.nLines = (const int32_t *)dev[9]; D.planeCoef = (const float *)dev[10]; D.planeW = (const float *)dev[11];
    D.planeHas = (const uint8_t *)dev[12]; D.nPlanes = (const int32_t *)dev[13]; D.Tcw = (const float *)dev[14];
    if (Rcw) {                                                                   // optional: staged like the other inputs
        const void *r[1] = {Rcw};
        const size_t rb[1] = {36 * F};
        void *dr[1];
        MSL_HIP_TRY(stage(r, rb, 1, 1, mem, &h->poseIn[15], st, dr));
        D.Rcw = (const float *)dr[0];
    }
    void *out[5] = {outlier, line_outlier, plane_outlier, Tcw_out, n_good}, *dout[5];
    const size_t outBytes[5] = {n, l, 3 * p, 48 * F, 4 * F};
    MSL_HIP_TRY(stage(out, outBytes, 5, 3, out_mem, h->poseOut, st, dout));   // the outlier flags are in/out
    D.outlier = (uint8_t *)dout[0]; D.lineOutlier = (uint8_t *)dout[1]; D.planeOutlier = (uint8_t *)dout[2];
    D.TcwOut = (float *)dout[3]; D.nGood = (int32_t *)dout[4];
    if (trans) {
        MSL_HIP_TRY(launch_pose_translation(D, n_frames, st));
    } else {
        hipLaunchKernelGGL(k_pose<false>, dim3((unsigned)n_frames), dim3(NT), 0, st, static_cast<const PoseDev &>(D));
        MSL_HIP_TRY(hipGetLastError());
    }
    MSL_HIP_TRY(finish_call(out, dout, outBytes, 5, mem, out_mem, st));
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_pose_optimize(msl_match *h, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params, const msl_keypoint *kps,
                      const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps, const float *xyz, const double *line_fn,
                      const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines, const float *plane_coef, const float *plane_w,
                      const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw, msl_mem mem, uint8_t *outlier, uint8_t *line_outlier,
                      uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good, msl_mem out_mem) noexcept {
    try {
    return run_pose(h, n_frames, cap, xcap, lcap, pcap, params, kps, un_xy, uright, pt_ref, n_kps, xyz, line_fn, line_xyz, line_has, n_lines,
                    plane_coef, plane_w, plane_has, n_planes, Tcw, nullptr, false, mem, outlier, line_outlier, plane_outlier, Tcw_out, n_good,
                    out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_pose_optimize_batch(int device, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                            const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps,
                            const float *xyz, const double *line_fn, const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines,
                            const float *plane_coef, const float *plane_w, const uint8_t *plane_has, const int32_t *n_planes, const float *Tcw,
                            msl_mem mem, uint8_t *outlier, uint8_t *line_outlier, uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good,
                            msl_mem out_mem) noexcept {
    try {
    // the outlier flags are inputs too: device-memory ones are read as well
    return on_default_handle(device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, [&](msl_match *h) {
        return run_pose(h, n_frames, cap, xcap, lcap, pcap, params, kps, un_xy, uright, pt_ref, n_kps, xyz, line_fn, line_xyz, line_has, n_lines,
                        plane_coef, plane_w, plane_has, n_planes, Tcw, nullptr, false, mem, outlier, line_outlier, plane_outlier, Tcw_out, n_good,
                        out_mem);
    });
    } MSL_ABI_CATCH_INT
}

int msl_pose_optimize_translation(msl_match *h, int n_frames, int cap, int xcap, int lcap, int pcap, const msl_pose_params *params,
                                  const msl_keypoint *kps, const float *un_xy, const float *uright, const int32_t *pt_ref, const int32_t *n_kps,
                                  const float *xyz, const double *line_fn, const double *line_xyz, const uint8_t *line_has, const int32_t *n_lines,
                                  const float *plane_coef, const float *plane_w, const uint8_t *plane_has, const int32_t *n_planes,
                                  const float *Tcw, const float *Rcw, msl_mem mem, uint8_t *outlier, uint8_t *line_outlier,
                                  uint8_t *plane_outlier, float *Tcw_out, int32_t *n_good, msl_mem out_mem) noexcept {
    try {
    return run_pose(h, n_frames, cap, xcap, lcap, pcap, params, kps, un_xy, uright, pt_ref, n_kps, xyz, line_fn, line_xyz, line_has, n_lines,
                    plane_coef, plane_w, plane_has, n_planes, Tcw, Rcw, true, mem, outlier, line_outlier, plane_outlier, Tcw_out, n_good, out_mem);
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
    return on_default_handle(device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, [&](msl_match *h) {
        return run_pose(h, n_frames, cap, xcap, lcap, pcap, params, kps, un_xy, uright, pt_ref, n_kps, xyz, line_fn, line_xyz, line_has, n_lines,
                        plane_coef, plane_w, plane_has, n_planes, Tcw, Rcw, true, mem, outlier, line_outlier, plane_outlier, Tcw_out, n_good,
                        out_mem);
    });
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
