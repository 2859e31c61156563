// msl_sf_superpixel.hip -- frame-batched superpixel stage of the surfel fusion for gfx950 (MI355X).
//
// generateSuperPixels() of a keyframe (reference src/SurfelFusion.cpp:333-773) depends only on that keyframe's images, never on the
// map, so it is FRAME-BATCHED (one launch sequence per batch of F keyframes, XCD-aware 1-D grids) on the handle's "pre" stream:
//     kb_seed_init                        one thread per 8x8 superpixel seed                  (:528-584)   msl_sf_sp_assign.hip
//     3 x { kb_assign                     one wave per three dual cells: argmin over <= 4 seeds (:333-415) msl_sf_sp_assign.hip
//           [kb_prop_lds,                 raster-order `stable` semantics as a min-fixpoint   (App. B.7.1)
//            kb_commit_px]                  over a compact worklist of the only pixels that can extend a chain (one launch, LDS)
//           kb_update_seeds               16 lanes per seed: ordered window gather, Huber mean (:428-515)  msl_sf_sp_seeds.hip
//           kb_commit_seeds }             chunk-abort (`return`) semantics: restore-only      (App. B.7.2)
//     kb_seed_plane                       16 lanes per seed: back-projection, pixel normals, Huber plane   msl_sf_sp_plane.hip
//                                         fit with FP64 4x4 normal equations                  (:91-165, :597-773)
// What the map stage (msl_sf_map.hip) reads of a keyframe is written here: tex (one 8-byte texel per pixel), fuseRec (three 16-byte
// words per seed, one plane per word), cand / candOk (the surfel a seed would spawn).
//
// Every float expression keeps the reference's evaluation order and float/double promotions; compiled with -ffp-contract=off.
//
// Here: the launch sequence, and the conversion of raw 16-bit depth that stages a batch's input.  The exact-arithmetic pins and the 16-lane row
// operations the three kernel units share: msl_sf_sp_dev.h.

#include "msl_sf_sp_dev.h"

namespace {

// Raw 16-bit depth (what the sensor / the data set's PNG holds) -> metres, on the device: imDepth.convertTo(imDepthScaled, CV_32F, depthMapFactor) of
// src/Frame.cc:96-97.  OpenCV's 16U -> 32F conversion with a scale works in float: dst = (float)src * (float)alpha + 0.0f (one rounding: the float
// product), which is what this kernel evaluates; a third of the bytes cross PCIe (2 instead of 4 per pixel) and the host loop disappears.
__global__ __launch_bounds__(256) void kb_depth_u16(const uint8_t *src, size_t srcStride, size_t srcFrameStride, float *dst, size_t dstFrameStride, int W, int H,
                                                    float factor) {
    const int frame = blockIdx.y;
    const int npx = W * H;
    const uint8_t *sf = src + (size_t)frame * srcFrameStride;
    float *df = dst + (size_t)frame * dstFrameStride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npx; i += gridDim.x * 256) {
        const int row = i / W, col = i - row * W;
        const unsigned raw = *reinterpret_cast<const uint16_t *>(sf + (size_t)row * srcStride + 2 * (size_t)col);
        df[i] = (float)raw * factor;
    }
}

}  // namespace

namespace msl {
namespace sf {

void sp_launch_depth_u16(hipStream_t st, const void *src, size_t srcStride, size_t srcFrameStride, float *dst, size_t dstFrameStride, int W, int H, int nFrames,
                         float factor) {
    const unsigned bx = (unsigned)std::min(((long long)W * H + 1023) / 1024, 1024ll);   // four pixels per thread
    hipLaunchKernelGGL(kb_depth_u16, dim3(bx, (unsigned)nFrames), dim3(256), 0, st, (const uint8_t *)src, srcStride, srcFrameStride, dst, dstFrameStride, W, H, factor);
}

// Superpixel stage of nFrames keyframes; P's per-slot pointers address the first of them (blockIdx.y / xcd_slot() == 0).
void sp_launch_stage(KernelProfiler &prof, hipStream_t sp, const SfDev &P, int n, bool propLds) {
    sp_launch_seed_init(prof, sp, P, n);
    for (int it = 0; it < 3; it++) {
        sp_launch_pixel_pass(prof, sp, P, n, it, propLds);
        sp_launch_seed_pass(prof, sp, P, n, it);
    }
    sp_launch_plane(prof, sp, P, n);
}

}  // namespace sf
}  // namespace msl
