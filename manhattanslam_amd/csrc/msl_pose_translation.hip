// msl_pose_translation.hip -- k_pose<true>: batched Optimizer::TranslationOptimization (reference src/Optimizer.cc:592-1009, Manhattan
// mode) for gfx950.  The device code is msl_pose_kernel.h; the entry points msl_pose_optimize_translation[_batch] are in msl_pose.hip.
// This instantiation has its own translation unit so that k_pose<false> compiles exactly as it did alone (see msl_pose_kernel.h).
#include "msl_pose_kernel.h"

namespace msl {

hipError_t launch_pose_translation(const PoseDevT &D, int n_frames, hipStream_t st) {
    hipLaunchKernelGGL(k_pose<true>, dim3((unsigned)n_frames), dim3(NT), 0, st, D);
    return hipGetLastError();
}

}  // namespace msl
