// camera_math.h -- one Gaussian's contribution to the camera gradients (device code, camera.hip).
//
// view_backward (gauss_bwd_math.h) forms dL/dt, dL/dA and the SH direction gradient of a Gaussian, folds them
// into dL/dmean3D and drops them.  camera_contrib forms the same three from the per-Gaussian screen-space
// gradients the backward has already written (dL/dmean2D, dL/dconic, dL/dopacity, dL/dcolour, dL/dinvdepth)
// and adds what they mean for the camera into 27 accumulators:
//   acc[3c + r]          dL/dviewmatrix[4c + r]          r = 0..2, c = 0..3   (column 3 is never read)
//   acc[12 + 3c + k]     dL/dprojmatrix[4c + {0,1,3}[k]]           c = 0..3   (column 2 is never read)
//   acc[24 + i]          dL/dcampos[i]
// It restates view_backward's cov2D chain instead of sharing it: view_backward's instantiations, their
// register budgets and their rounding (the bitwise equalities between the backward's paths) stay as they are.
// The SH polynomial is shared (sh_dir_backward over an accessor that reads and stores nothing).
// Conventions are dL/dmean3D's: a clamped t.x / t.y is a constant in J, the antialiasing term is the
// reference's formula at the dilated covariance, no gradient through culling or the radius.
#pragma once

#include "gauss_bwd_math.h"

namespace gsr {

constexpr int kCamAcc = 27;

// SH coefficients read from the inputs; the dL/dSH values sh_backward forms on the way are dropped.
struct ShReadOnly {
    ShAddr src;
    int idx;
    __device__ float3 load(int k) const {
        const float* c = src.coef(idx, k);
        return make_float3(c[0], c[1], c[2]);
    }
    __device__ void store(int, float3) const {}
};

// g: the screen-space gradients of one visible Gaussian (radius > 0):
//   m2x, m2y  dL/dmean2D (NDC units)      dca, dcb, dcc  dL/dconic (the reference's convention)
//   dop       dL/dopacity as stored (with antialiasing: the raw gradient times h)
//   dcol      dL/dcolour                  dinvd          dL/dinvdepth (read when c.have_invdepth)
struct CamGrads {
    float m2x, m2y, dca, dcb, dcc, dop, dinvd;
    float3 dcol;
};

template <class ShAcc>
__device__ __forceinline__ void camera_contrib(const ViewCam& c, const GaussIn& gi, const CamGrads& g, uint8_t cm,
                                               bool do_sh, int D, int M, const ShAcc& sh, float (&acc)[kCamAcc]) {
    const float* V = c.V;
    const float3 mean = gi.mean;
    const float m[4] = {mean.x, mean.y, mean.z, 1.f};
    float3 t = xform_point_4x3(mean, V);
    // (a visible Gaussian has t.z > 0.2; anything else here is a row of another forward: no contribution)
    if (t.z > 0.f) {
        // ---- computeCov2DCUDA, as view_backward
        const float limx = 1.3f * c.tan_fovx, limy = 1.3f * c.tan_fovy;
        const float txtz = t.x / t.z, tytz = t.y / t.z;
        t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
        t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
        const float x_grad_mul = txtz < -limx || txtz > limx ? 0.f : 1.f;
        const float y_grad_mul = tytz < -limy || tytz > limy ? 0.f : 1.f;
        const float fx = c.focal_x, fy = c.focal_y;
        const float j00 = fx / t.z, j02 = -(fx * t.x) / (t.z * t.z);
        const float j11 = fy / t.z, j12 = -(fy * t.y) / (t.z * t.z);
        const float A0[3] = {j00 * V[0] + j02 * V[2], j00 * V[4] + j02 * V[6], j00 * V[8] + j02 * V[10]};
        const float A1[3] = {j11 * V[1] + j12 * V[2], j11 * V[5] + j12 * V[6], j11 * V[9] + j12 * V[10]};

        float cov[6];
        if (gi.cov3D) {
            for (int k = 0; k < 6; k++) cov[k] = gi.cov3D[k];
        } else {
            const float r_ = gi.q.x, x = gi.q.y, y = gi.q.z, z = gi.q.w;
            const float sx = gi.scale_modifier * gi.sc3.x, sy = gi.scale_modifier * gi.sc3.y,
                        sz = gi.scale_modifier * gi.sc3.z;
            const float L00 = (1.f - 2.f * (y * y + z * z)) * sx, L01 = 2.f * (x * y - r_ * z) * sy,
                        L02 = 2.f * (x * z + r_ * y) * sz;
            const float L10 = 2.f * (x * y + r_ * z) * sx, L11 = (1.f - 2.f * (x * x + z * z)) * sy,
                        L12 = 2.f * (y * z - r_ * x) * sz;
            const float L20 = 2.f * (x * z - r_ * y) * sx, L21 = 2.f * (y * z + r_ * x) * sy,
                        L22 = (1.f - 2.f * (x * x + y * y)) * sz;
            cov[0] = L00 * L00 + L01 * L01 + L02 * L02;
            cov[1] = L00 * L10 + L01 * L11 + L02 * L12;
            cov[2] = L00 * L20 + L01 * L21 + L02 * L22;
            cov[3] = L10 * L10 + L11 * L11 + L12 * L12;
            cov[4] = L10 * L20 + L11 * L21 + L12 * L22;
            cov[5] = L20 * L20 + L21 * L21 + L22 * L22;
        }
        const float SA0[3] = {cov[0] * A0[0] + cov[1] * A0[1] + cov[2] * A0[2],
                              cov[1] * A0[0] + cov[3] * A0[1] + cov[4] * A0[2],
                              cov[2] * A0[0] + cov[4] * A0[1] + cov[5] * A0[2]};
        const float SA1[3] = {cov[0] * A1[0] + cov[1] * A1[1] + cov[2] * A1[2],
                              cov[1] * A1[0] + cov[3] * A1[1] + cov[4] * A1[2],
                              cov[2] * A1[0] + cov[4] * A1[1] + cov[5] * A1[2]};
        float c_xx = A0[0] * SA0[0] + A0[1] * SA0[1] + A0[2] * SA0[2];
        const float c_xy = A0[0] * SA1[0] + A0[1] * SA1[1] + A0[2] * SA1[2];
        float c_yy = A1[0] * SA1[0] + A1[1] * SA1[1] + A1[2] * SA1[2];

        constexpr float h_var = 0.3f;
        float dL_dc_xx = 0.f, dL_dc_xy = 0.f, dL_dc_yy = 0.f;
        const float det_cov = c_xx * c_yy - c_xy * c_xy;
        c_xx += h_var;
        c_yy += h_var;
        if (c.antialiasing) {
            // view_backward: d_h = raw * opacity, d_inside_root = d_h / (2 h) unless h is clamped.  The stored
            // dL/dopacity is raw * h and h^2 is the ratio, so d_inside_root = stored * opacity / (2 ratio).
            const float ratio = det_cov / (c_xx * c_yy - c_xy * c_xy);
            const float d_inside_root = ratio <= 0.000025f ? 0.f : g.dop * *gi.opacity / (2.f * ratio);
            const float x = c_xx, y = c_yy, z = c_xy, w = h_var;
            const float qd = w * w + w * (x + y) + x * y - z * z;
            const float denom_f = d_inside_root / (qd * qd);
            dL_dc_xx = w * (w * y + y * y + z * z) * denom_f;
            dL_dc_yy = w * (w * x + x * x + z * z) * denom_f;
            dL_dc_xy = -2.f * w * z * (w + x + y) * denom_f;
        }
        const float denom = c_xx * c_yy - c_xy * c_xy;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
        if (denom2inv != 0.f) {
            dL_dc_xx += denom2inv * (-c_yy * c_yy * g.dca + 2.f * c_xy * c_yy * g.dcb + (denom - c_xx * c_yy) * g.dcc);
            dL_dc_yy += denom2inv * (-c_xx * c_xx * g.dcc + 2.f * c_xx * c_xy * g.dcb + (denom - c_xx * c_yy) * g.dca);
            dL_dc_xy += denom2inv * 2.f * (c_xy * c_yy * g.dca - (denom + 2.f * c_xy * c_xy) * g.dcb + c_xx * c_xy * g.dcc);
        }

        // cov2D = A Sigma A^T -> dL/dA; A = J Rv -> dL/dJ (-> dL/dt) and dL/dRv (the rotation chain)
        float dA0[3], dA1[3];
        for (int k = 0; k < 3; k++) {
            dA0[k] = 2.f * dL_dc_xx * SA0[k] + dL_dc_xy * SA1[k];
            dA1[k] = 2.f * dL_dc_yy * SA1[k] + dL_dc_xy * SA0[k];
        }
        const float dJ00 = dA0[0] * V[0] + dA0[1] * V[4] + dA0[2] * V[8];
        const float dJ02 = dA0[0] * V[2] + dA0[1] * V[6] + dA0[2] * V[10];
        const float dJ11 = dA1[0] * V[1] + dA1[1] * V[5] + dA1[2] * V[9];
        const float dJ12 = dA1[0] * V[2] + dA1[1] * V[6] + dA1[2] * V[10];
        const float tz = 1.f / t.z, tz2 = tz * tz, tz3 = tz2 * tz;
        float dt[3];
        dt[0] = x_grad_mul * -fx * tz2 * dJ02;
        dt[1] = y_grad_mul * -fy * tz2 * dJ12;
        dt[2] = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2.f * fx * t.x) * tz3 * dJ02 + (2.f * fy * t.y) * tz3 * dJ12;
        if (c.have_invdepth) dt[2] -= g.dinvd * tz2;
        // t[r] = sum_c V[4c + r] m[c]
        for (int col = 0; col < 4; col++)
            for (int r = 0; r < 3; r++) acc[3 * col + r] += dt[r] * m[col];
        // A0[c] = j00 V[4c] + j02 V[4c + 2],  A1[c] = j11 V[4c + 1] + j12 V[4c + 2]
        for (int col = 0; col < 3; col++) {
            acc[3 * col + 0] += j00 * dA0[col];
            acc[3 * col + 1] += j11 * dA1[col];
            acc[3 * col + 2] += j02 * dA0[col] + j12 * dA1[col];
        }
    }

    // ---- screen position: ndc = (h.x, h.y) / (h.w + 1e-7), h[r] = sum_c Pm[4c + r] m[c]
    {
        const float4 h = xform_point_4x4(mean, c.Pm);
        const float w = 1.0f / (h.w + 0.0000001f);
        const float dh[3] = {g.m2x * w, g.m2y * w, -(g.m2x * h.x + g.m2y * h.y) * w * w};
        for (int col = 0; col < 4; col++)
            for (int k = 0; k < 3; k++) acc[12 + 3 * col + k] += dh[k] * m[col];
    }

    // ---- SH view direction: dir = normalize(mean - campos), so dL/dcampos = -(the term dL/dmean3D gets)
    if (do_sh) {
        const float3 v = make_float3(mean.x - c.campos[0], mean.y - c.campos[1], mean.z - c.campos[2]);
        // (mean == campos has no direction; 1e-12: the cube of the squared length stays a normal float)
        if (v.x * v.x + v.y * v.y + v.z * v.z > 1e-12f) {
            const float3 gm = make_float3((cm & 1) ? 0.f : g.dcol.x, (cm & 2) ? 0.f : g.dcol.y, (cm & 4) ? 0.f : g.dcol.z);
            float3 dm = make_float3(0.f, 0.f, 0.f);
            sh_dir_backward(sh, D, M, v, gm, dm);
            acc[24] -= dm.x;
            acc[25] -= dm.y;
            acc[26] -= dm.z;
        }
    }
}

}  // namespace gsr
