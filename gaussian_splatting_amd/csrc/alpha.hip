// alpha.hip -- the accumulated-alpha (silhouette) map of a finished forward: A = 1 - final_T.
//
// render_fwd keeps final_T (the transmittance after each pixel's last contributor) in the image
// buffer's tile-major planes (gsr_common.h tile_px) for the backward's background term; this kernel
// turns that plane into a row-major [1,H,W] output.  It is a launch of its own, queued by
// gsr_render_alpha after the forward (and after the forward's tile redo, so it reads final values):
// render_fwd is not touched and a forward that asks for no alpha launches nothing.
//
// One workgroup per strip of 64 x 16 pixels (four tiles side by side), four waves: wave w writes rows
// w, w + 4, w + 8, w + 12 of the strip, its 64 lanes 64 consecutive pixels of one image row -- one
// 256-byte store per wave and row.  The reads gather 32-byte runs (8 pixels of a quadrant row) out of
// the tiles' planes; the four waves of a group read the four rows that share each 128-byte line in
// the same iteration, so the gather is served by the CU's cache.  Pixels of partial edge tiles (never
// written by the forward) are masked.
#include "kernels.h"

namespace gsr {

constexpr int kAlphaStripW = 64;  // pixels per strip row: one wave, four tiles

__global__ void __launch_bounds__(256) render_alpha_kernel(const float* __restrict__ final_T,
                                                           float* __restrict__ out_alpha, int W, int H, uint32_t gx) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int x = blockIdx.x * kAlphaStripW + lane;
    if (x >= W) return;
    const uint32_t tile = blockIdx.y * gx + (uint32_t)(x >> 4);
    const int qx = (x & 15) >> 3, lx = x & 7;
#pragma unroll
    for (int i = 0; i < kTile / 4; i++) {
        const int ty = wave + 4 * i;  // row inside the tile
        const int y = blockIdx.y * kTile + ty;
        if (y < H) out_alpha[(size_t)y * W + x] = 1.f - final_T[tile_px(tile, (ty >> 3) * 2 + qx, (ty & 7) * 8 + lx)];
    }
}

hipError_t launch_render_alpha(const float* final_T, float* out_alpha, int W, int H, hipStream_t stream) {
    const uint32_t gx = (W + kTile - 1) / kTile, gy = (H + kTile - 1) / kTile;
    if (gx == 0 || gy == 0) return hipSuccess;
    hipLaunchKernelGGL(render_alpha_kernel, dim3((W + kAlphaStripW - 1) / kAlphaStripW, gy), dim3(256), 0, stream,
                       final_T, out_alpha, W, H, gx);
    return hipGetLastError();
}

}  // namespace gsr
