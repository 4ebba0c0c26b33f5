// camera.h -- launch arguments of the camera backward (camera.hip) and the one thing it needs from the
// forward's geometry buffer, whose layout api.hip owns.
#pragma once

#include "gsr_common.h"

namespace gsr {

struct CameraBwdArgs {
    int P, D, M;
    const float* means3D;
    const float* shs;  // as PreprocessArgs::shs; null with precomputed colours
    const float* dc;   // [P,1,3] or null
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    float scale_modifier;
    const float* viewmatrix;
    const float* projmatrix;
    const float* campos;
    float tan_fovx, tan_fovy, focal_x, focal_y;
    int antialiasing;
    const int* radii;
    const uint8_t* clamped;      // GeomState::clamped (read with SH colours only)
    const float* dL_dmean2D;     // [P,3]
    const float* dL_dconic;      // [P,4]
    const float* dL_dopacity;    // [P]
    const float* dL_dcolor;      // [P,3]
    const float* dL_dinvdepth;   // [P] or null
    float* slab;                 // [camera_slab_rows(P)][kCamSlabRow] workgroup partials
    float* dL_dviewmatrix;       // 16
    float* dL_dprojmatrix;       // 16
    float* dL_dcampos;           // 3
};

constexpr int kCamThreads = 1024;   // one lane per Gaussian, sixteen waves per workgroup
constexpr int kCamSlabRow = 32;     // floats per workgroup in the slab: the 27 partials, padded to 128 bytes
inline size_t camera_slab_rows(int P) { return ((size_t)P + kCamThreads - 1) / kCamThreads; }

// camera.hip: the per-Gaussian pass into the slab, then the fixed-order fp64 sum of the slab into the 35 outputs
hipError_t launch_camera_backward(const CameraBwdArgs& a, hipStream_t stream);
// api.hip: the SH clamp flags inside a forward's geometry buffer
const uint8_t* geom_clamped(const void* geom_buffer, int P, int width, int height);

}  // namespace gsr
