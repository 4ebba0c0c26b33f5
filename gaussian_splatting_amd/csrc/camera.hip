// camera.hip -- camera-pose gradients: dL/dviewmatrix [16], dL/dprojmatrix [16], dL/dcampos [3]
// (gsr_camera_backward, include/gsr.h; no reference counterpart).
//
// The camera backward runs after the ordinary backward, on the same stream, as a pure function of what that
// backward documents as its outputs -- the per-Gaussian screen-space gradients dL/dmean2D, dL/dconic,
// dL/dopacity, dL/dcolour, dL/dinvdepth -- plus the inputs, the radii and the geometry buffer's SH clamp
// flags.  It does not depend on which path the backward took (records or atomics, live list, zero fill).
//
//   camera_bwd_kernel     one lane per Gaussian, 1024 per workgroup: the Gaussian's contribution
//                         (camera_math.h) in 27 registers; then a wave64 sum (DPP), the workgroup's sixteen
//                         wave totals added in wave order through LDS, and one plain vector store of the 27
//                         partials into the workgroup's row of the slab (977 rows at 1M Gaussians).
//   camera_reduce_kernel  one workgroup: the slab's rows summed in a fixed order in fp64, and all 35 outputs
//                         written, the structural zeros (viewmatrix[:,3], projmatrix[:,2]) included.
// No float atomics and no hand-off between workgroups inside a launch: for given per-Gaussian inputs the result
// is the same bit for bit on every run.
// Compiled with backward.hip's per-file flags (build.py FILE_FLAGS), like every user of gauss_bwd_math.h.
#include "camera.h"
#include "camera_math.h"
#include "host.h"

namespace gsr {

constexpr int kCamWaves = kCamThreads / 64;
static_assert(kCamAcc <= kCamSlabRow, "a slab row holds the partials");

__global__ void __launch_bounds__(kCamThreads) camera_bwd_kernel(CameraBwdArgs a) {
    float acc[kCamAcc];
#pragma unroll
    for (int i = 0; i < kCamAcc; i++) acc[i] = 0.f;
    // the camera through LDS: 35 wave-uniform values that would otherwise sit in scalar registers from here to
    // their last use, beside the arguments' pointers
    __shared__ float s_cam[36];
    if (threadIdx.x < 16) s_cam[threadIdx.x] = a.viewmatrix[threadIdx.x];
    else if (threadIdx.x < 32) s_cam[threadIdx.x] = a.projmatrix[threadIdx.x - 16];
    else if (threadIdx.x < 35) s_cam[threadIdx.x] = a.campos ? a.campos[threadIdx.x - 32] : 0.f;
    __syncthreads();
    const ViewCam cam{s_cam,     s_cam + 16, s_cam + 32,     a.tan_fovx, a.tan_fovy,
                      a.focal_x, a.focal_y,  a.antialiasing, a.dL_dinvdepth != nullptr};
    const bool do_sh = a.shs || a.dc;
    const ShAddr sh_src{a.shs, a.dc, a.M};
    // (one Gaussian per lane, no loop over several: with every argument pointer live around a loop the scalar
    // registers spilled.  Large workgroups instead keep the slab short.)
    const uint32_t gu = blockIdx.x * (uint32_t)kCamThreads + threadIdx.x;
    const int g = (int)gu;
    // culled: its rows of the gradient arrays may hold anything; nothing of it is read
    if (gu < (uint32_t)a.P && a.radii[g] > 0) {
        CamGrads cg;
        cg.m2x = a.dL_dmean2D[3 * (size_t)g];
        cg.m2y = a.dL_dmean2D[3 * (size_t)g + 1];
        const float4 dcon = reinterpret_cast<const float4*>(a.dL_dconic)[g];
        cg.dca = dcon.x;
        cg.dcb = dcon.y;
        cg.dcc = dcon.w;
        cg.dop = a.dL_dopacity[g];
        cg.dcol = make_float3(a.dL_dcolor[3 * (size_t)g], a.dL_dcolor[3 * (size_t)g + 1], a.dL_dcolor[3 * (size_t)g + 2]);
        cg.dinvd = a.dL_dinvdepth ? a.dL_dinvdepth[g] : 0.f;
        // visible but behind saturated pixels everywhere (most of a full-size frame): every term is zero, and
        // none of its geometry or SH row is read
        const bool any = (cg.m2x != 0.f) | (cg.m2y != 0.f) | (cg.dca != 0.f) | (cg.dcb != 0.f) | (cg.dcc != 0.f) |
                         (cg.dop != 0.f) | (cg.dcol.x != 0.f) | (cg.dcol.y != 0.f) | (cg.dcol.z != 0.f) |
                         (cg.dinvd != 0.f);
        if (any) {
            GaussIn gi;
            gi.have_scales = a.scales != nullptr;
            gi.mean = make_float3(a.means3D[3 * (size_t)g], a.means3D[3 * (size_t)g + 1], a.means3D[3 * (size_t)g + 2]);
            gi.sc3 = make_float3(0.f, 0.f, 0.f);
            gi.q = make_float4(1.f, 0.f, 0.f, 0.f);
            if (a.scales) {
                gi.sc3 = make_float3(a.scales[3 * (size_t)g], a.scales[3 * (size_t)g + 1], a.scales[3 * (size_t)g + 2]);
                gi.q = make_float4(a.rotations[4 * (size_t)g], a.rotations[4 * (size_t)g + 1], a.rotations[4 * (size_t)g + 2],
                                   a.rotations[4 * (size_t)g + 3]);
            }
            gi.cov3D = a.cov3D_precomp ? a.cov3D_precomp + 6 * (size_t)g : nullptr;
            gi.scale_modifier = a.scale_modifier;
            gi.opacity = a.opacities + g;
            const uint8_t cm = do_sh ? a.clamped[g] : 0;
            camera_contrib(cam, gi, cg, cm, do_sh, a.D, a.M, ShReadOnly{sh_src, g}, acc);
        }
    }

    // wave sums (valid in lane 63), the waves' totals through LDS in wave order, one row of the slab
    __shared__ float s_part[kCamWaves][kCamSlabRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < kCamAcc; i++) {
        const float v = wave_sum_to_lane63(acc[i]);
        if (lane == 63) s_part[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kCamSlabRow) {
        float s = 0.f;
        if (threadIdx.x < kCamAcc)
            for (int w = 0; w < kCamWaves; w++) s += s_part[w][threadIdx.x];
        a.slab[(size_t)blockIdx.x * kCamSlabRow + threadIdx.x] = s;
    }
}

// rows: the slab's rows (0: no Gaussians, every output zero).  Thread (grp, col) = (t / 32, t % 32) sums column
// col of rows grp, grp + 8, ... in fp64; thread col then adds the eight group sums in group order.
constexpr int kCamRedThreads = 256;
constexpr int kCamRedGroups = kCamRedThreads / kCamSlabRow;
__global__ void __launch_bounds__(kCamRedThreads) camera_reduce_kernel(const float* __restrict__ slab, int rows,
                                                                       float* __restrict__ dV, float* __restrict__ dPm,
                                                                       float* __restrict__ dC) {
    __shared__ double s_grp[kCamRedGroups][kCamSlabRow];
    __shared__ float s_tot[kCamSlabRow];
    const int col = threadIdx.x % kCamSlabRow, grp = threadIdx.x / kCamSlabRow;
    double s = 0.0;
    for (int r = grp; r < rows; r += kCamRedGroups) s += (double)slab[(size_t)r * kCamSlabRow + col];
    s_grp[grp][col] = s;
    __syncthreads();
    if (threadIdx.x < kCamSlabRow) {
        double tot = 0.0;
        for (int k = 0; k < kCamRedGroups; k++) tot += s_grp[k][threadIdx.x];
        s_tot[threadIdx.x] = (float)tot;
    }
    __syncthreads();
    // accumulator layout: camera_math.h
    const int k = threadIdx.x;
    if (k < 16) {
        const int r = k & 3, c = k >> 2;
        dV[k] = r == 3 ? 0.f : s_tot[3 * c + r];
    } else if (k < 32) {
        const int r = k & 3, c = (k - 16) >> 2;
        dPm[k - 16] = r == 2 ? 0.f : s_tot[12 + 3 * c + (r == 3 ? 2 : r)];
    } else if (k < 35) {
        dC[k - 32] = s_tot[24 + (k - 32)];
    }
}

hipError_t launch_camera_backward(const CameraBwdArgs& a, hipStream_t stream) {
    const int rows = a.P > 0 ? (int)camera_slab_rows(a.P) : 0;
    if (rows > 0) {
        hipLaunchKernelGGL(camera_bwd_kernel, dim3(rows), dim3(kCamThreads), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(camera_reduce_kernel, dim3(1), dim3(kCamRedThreads), 0, stream, a.slab, rows, a.dL_dviewmatrix,
                       a.dL_dprojmatrix, a.dL_dcampos);
    return hipGetLastError();
}

}  // namespace gsr

// ---- C entry point (include/gsr.h) --------------------------------------------------------------------
using namespace gsr;

extern "C" {

int gsr_camera_backward(int P, int D, int M, int width, int height, const float* means3D, const float* dc,
                        const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                        float scale_modifier, const float* rotations, const float* cov3D_precomp,
                        const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                        float tan_fovy, const int* radii, const void* geom_buffer, const float* dL_dmean2D,
                        const float* dL_dconic, const float* dL_dopacity, const float* dL_dcolor,
                        const float* dL_dinvdepth, int antialiasing, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                        void* stream, float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos) {
    clear_error();
    if (P < 0 || width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGUMENT, "camera_backward: invalid sizes P=%d W=%d H=%d", P, width, height);
    if (!dL_dviewmatrix || !dL_dprojmatrix || !dL_dcampos)
        return fail(GSR_ERR_ARGUMENT, "camera_backward: missing output");
    CameraBwdArgs a{};
    a.P = P;
    a.dL_dviewmatrix = dL_dviewmatrix;
    a.dL_dprojmatrix = dL_dprojmatrix;
    a.dL_dcampos = dL_dcampos;
    if (P > 0) {
        if (!means3D || !opacities || !radii || !viewmatrix || !projmatrix || !geom_buffer)
            return fail(GSR_ERR_ARGUMENT, "camera_backward: missing required pointer");
        if (!dL_dmean2D || !dL_dconic || !dL_dopacity || !dL_dcolor)
            return fail(GSR_ERR_ARGUMENT, "camera_backward: missing a per-Gaussian gradient array");
        if (reinterpret_cast<uintptr_t>(dL_dconic) & 15)
            return fail(GSR_ERR_ARGUMENT, "camera_backward: dL_dconic must be 16-byte aligned");
        if ((scales == nullptr) != (rotations == nullptr) || (scales == nullptr) == (cov3D_precomp == nullptr))
            return fail(GSR_ERR_ARGUMENT, "camera_backward: provide scales+rotations or a precomputed covariance");
        if (colors_precomp) {  // no SH evaluation: dL/dcampos is zero
            dc = shs = nullptr;
            M = 0;
        } else {
            if (!dc && !shs) return fail(GSR_ERR_ARGUMENT, "camera_backward: provide SHs or precomputed colours");
            if (dc && M > 0 && !shs) return fail(GSR_ERR_ARGUMENT, "camera_backward: %d rest SH coefficients but no shs", M);
            if (dc) M += 1;  // as in the forward
            if (D < 0 || D > 3 || (D + 1) * (D + 1) > M)
                return fail(GSR_ERR_ARGUMENT, "camera_backward: SH degree %d needs %d coefficients, got %d", D,
                            (D + 1) * (D + 1), M);
            if (!campos) return fail(GSR_ERR_ARGUMENT, "camera_backward: campos required for SHs");
            if (M <= (dc ? 1 : 0)) shs = nullptr;
        }
        a.D = D;
        a.M = M;
        a.means3D = means3D;
        a.shs = shs;
        a.dc = dc;
        a.opacities = opacities;
        a.scales = scales;
        a.rotations = rotations;
        a.cov3D_precomp = cov3D_precomp;
        a.scale_modifier = scale_modifier;
        a.viewmatrix = viewmatrix;
        a.projmatrix = projmatrix;
        a.campos = campos;
        a.tan_fovx = tan_fovx;
        a.tan_fovy = tan_fovy;
        a.focal_x = width / (2.0f * tan_fovx);
        a.focal_y = height / (2.0f * tan_fovy);
        a.antialiasing = antialiasing;
        a.radii = radii;
        a.clamped = geom_clamped(geom_buffer, P, width, height);
        a.dL_dmean2D = dL_dmean2D;
        a.dL_dconic = dL_dconic;
        a.dL_dopacity = dL_dopacity;
        a.dL_dcolor = dL_dcolor;
        a.dL_dinvdepth = dL_dinvdepth;
        const size_t bytes = (size_t)camera_slab_rows(P) * kCamSlabRow * sizeof(float);
        a.slab = static_cast<float*>(call_alloc(scratch_alloc, scratch_ctx, bytes));
        if (!a.slab) return fail(GSR_ERR_ALLOC, "camera_backward: scratch allocation failed");
    }
    HIP_TRY(launch_camera_backward(a, (hipStream_t)stream), "camera_backward");
    return GSR_OK;
}

}  // extern "C"
