// gauss_bwd_math.h -- the per-Gaussian backward math (device code) shared by backward.hip (one view) and
// views.hip (the same Gaussian over several views): the SH colour backward and view_backward.  Both files are
// compiled with the same per-file flags (build.py FILE_FLAGS), so an expression here rounds the same way in
// both and the view exchange's gradients equal the single-view backward's bit for bit.
#pragma once

#include "kernels.h"

namespace gsr {

// ---- 2. SH colour backward, one coefficient at a time ---------------------------
// Row accessors: coefficient k of this thread's Gaussian (3 floats).
struct ShLds {
    float* row;  // LDS row, padded stride
    __device__ float3 load(int k) const { return make_float3(row[3 * k], row[3 * k + 1], row[3 * k + 2]); }
    __device__ void store(int k, float3 v) const {
        row[3 * k] = v.x;
        row[3 * k + 1] = v.y;
        row[3 * k + 2] = v.z;
    }
};
struct ShGlobal {
    ShAddr src;
    ShGradAddr dst;
    int idx;
    __device__ float3 load(int k) const {
        const float* c = src.coef(idx, k);
        return make_float3(c[0], c[1], c[2]);
    }
    __device__ void store(int k, float3 v) const {
        float* c = dst.coef(idx, k);
        c[0] = v.x;
        c[1] = v.y;
        c[2] = v.z;
    }
};

// For each coefficient k < (deg+1)^2: dL/dsh_k = B_k(dir) * g, and
// d(colour . g)/d(dir) += grad B_k(dir) * (sh_k . g)  (CR/backward.cu:43-127).
// Coefficients k >= (deg+1)^2 (up to M) get zero gradients.
template <class Acc>
__device__ __forceinline__ void sh_backward(const Acc& acc, int deg, int M, float x, float y, float z, float3 g,
                                            float& ddx, float& ddy, float& ddz) {
    ddx = ddy = ddz = 0.f;
    auto term = [&](int k, float B, float bx, float by, float bz) {
        const float3 s = acc.load(k);
        const float sg = s.x * g.x + s.y * g.y + s.z * g.z;
        ddx += bx * sg;
        ddy += by * sg;
        ddz += bz * sg;
        acc.store(k, make_float3(B * g.x, B * g.y, B * g.z));
    };
    term(0, SH_C0, 0.f, 0.f, 0.f);
    int K = 1;
    if (deg > 0) {
        term(1, -SH_C1 * y, 0.f, -SH_C1, 0.f);
        term(2, SH_C1 * z, 0.f, 0.f, SH_C1);
        term(3, -SH_C1 * x, -SH_C1, 0.f, 0.f);
        K = 4;
        if (deg > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            term(4, SH_C2_0 * xy, SH_C2_0 * y, SH_C2_0 * x, 0.f);
            term(5, SH_C2_1 * yz, 0.f, SH_C2_1 * z, SH_C2_1 * y);
            term(6, SH_C2_2 * (2.f * zz - xx - yy), SH_C2_2 * -2.f * x, SH_C2_2 * -2.f * y, SH_C2_2 * 4.f * z);
            term(7, SH_C2_3 * xz, SH_C2_3 * z, 0.f, SH_C2_3 * x);
            term(8, SH_C2_4 * (xx - yy), SH_C2_4 * 2.f * x, SH_C2_4 * -2.f * y, 0.f);
            K = 9;
            if (deg > 2) {
                term(9, SH_C3_0 * y * (3.f * xx - yy), SH_C3_0 * 6.f * xy, SH_C3_0 * 3.f * (xx - yy), 0.f);
                term(10, SH_C3_1 * xy * z, SH_C3_1 * yz, SH_C3_1 * xz, SH_C3_1 * xy);
                term(11, SH_C3_2 * y * (4.f * zz - xx - yy), SH_C3_2 * -2.f * xy, SH_C3_2 * (-3.f * yy + 4.f * zz - xx),
                     SH_C3_2 * 8.f * yz);
                term(12, SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy), SH_C3_3 * -6.f * xz, SH_C3_3 * -6.f * yz,
                     SH_C3_3 * 3.f * (2.f * zz - xx - yy));
                term(13, SH_C3_4 * x * (4.f * zz - xx - yy), SH_C3_4 * (-3.f * xx + 4.f * zz - yy), SH_C3_4 * -2.f * xy,
                     SH_C3_4 * 8.f * xz);
                term(14, SH_C3_5 * z * (xx - yy), SH_C3_5 * 2.f * xz, SH_C3_5 * -2.f * yz, SH_C3_5 * (xx - yy));
                term(15, SH_C3_6 * x * (xx - 3.f * yy), SH_C3_6 * 3.f * (xx - yy), SH_C3_6 * -6.f * xy, 0.f);
                K = 16;
            }
        }
    }
    for (int k = K; k < M; k++) acc.store(k, make_float3(0.f, 0.f, 0.f));
}

__device__ __forceinline__ void store3(float* p, int i, float x, float y, float z) {
    p[3 * i] = x;
    p[3 * i + 1] = y;
    p[3 * i + 2] = z;
}

constexpr int kShStride = 52;  // padded LDS row stride: conflict-free ds_read/write_b128

// ---- per-view gradient math (one Gaussian, one view) ----------------------------
// computeCov2DCUDA with its re-derived tail, the screen-space mean chain, the SH colour
// backward and the scale/rotation backward, from the view's summed render gradients.  The one
// copy of this math: gauss_bwd_kernel runs it once per Gaussian, gauss_bwd_views_kernel once
// per (Gaussian, view).  The outputs leave through the caller's sink as soon as each is formed
// (the single-view kernel stores them there and then, which keeps its register peak down; the
// multi-view kernel sums them over the views).  Sink interface:
//   dop(float)  dcov(const float (&)[6])  dmean(float3)  scale_rot(bool have, float3, float4)
//   sh_defer(float3 view vector, float3 masked colour gradient)   (kShDefer only)
struct ViewCam {
    const float* V;       // viewmatrix, 16 floats (column-major)
    const float* Pm;      // projmatrix
    const float* campos;  // 3
    float tan_fovx, tan_fovy, focal_x, focal_y;
    int antialiasing, have_invdepth;
};
struct GaussIn {
    float3 mean;
    bool have_scales;
    float3 sc3;            // scales (when have_scales)
    float4 q;              // rotation (when have_scales)
    const float* cov3D;    // 6 floats, or null
    float scale_modifier;
    const float* opacity;  // the Gaussian's opacity (read by the AA chain only)
};
// SH colour backward of view_backward (when do_sh: the colours came from SH, not precomputed):
// now (through the accessor, adding the view-direction term to dL/dmean3D), or deferred (the
// caller runs it later from what sink.sh_defer receives, then stores dL/dmean3D itself).
enum { kShNow = 1, kShDefer = 2 };

// d(normalize(v))/dv applied to the direction gradient (dnormvdv, CR/auxiliary.h:129-139),
// added to dmean.
__device__ __forceinline__ void add_dir_grad(float3 v, float ddx, float ddy, float ddz, float3& dmean) {
    const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
    const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    dmean.x += ((sum2 - v.x * v.x) * ddx - v.y * v.x * ddy - v.z * v.x * ddz) * invsum32;
    dmean.y += (-v.x * v.y * ddx + (sum2 - v.y * v.y) * ddy - v.z * v.y * ddz) * invsum32;
    dmean.z += (-v.x * v.z * ddx - v.y * v.z * ddy + (sum2 - v.z * v.z) * ddz) * invsum32;
}

// SH colour backward for view vector v (mean - campos) and colour gradient g: dL/dSH through the
// accessor, the direction term added to dmean (CR/backward.cu:12-146).
template <class ShAcc>
__device__ __forceinline__ void sh_dir_backward(const ShAcc& sh, int D, int M, float3 v, float3 g, float3& dmean) {
    const float len = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    float ddx, ddy, ddz;
    sh_backward(sh, D, M, v.x / len, v.y / len, v.z / len, g, ddx, ddy, ddz);
    add_dir_grad(v, ddx, ddy, ddz, dmean);
}

template <int SHM, class ShAcc, class Sink>
__device__ __forceinline__ void view_backward(const ViewCam& c, const GaussIn& gi, float4 sa, float4 sb, float2 sc,
                                              uint8_t cm, bool do_sh, int D, int M, const ShAcc& sh, Sink& out) {
    const float3 dcol = make_float3(sa.x, sa.y, sa.z);
    const float dinvd = sa.w;
    const float m2x = sb.x, m2y = sb.y;
    float dop = sb.z;
    const float dca = sc.x, dcb = sb.w, dcc = sc.y;  // dL/dconic, the reference's convention
    // ---- computeCov2DCUDA
    const float* V = c.V;
    const float3 mean = gi.mean;
    float3 t = xform_point_4x3(mean, V);
    const float limx = 1.3f * c.tan_fovx, limy = 1.3f * c.tan_fovy;
    const float txtz = t.x / t.z, tytz = t.y / t.z;
    t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
    t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
    const float x_grad_mul = txtz < -limx || txtz > limx ? 0.f : 1.f;
    const float y_grad_mul = tytz < -limy || tytz > limy ? 0.f : 1.f;
    const float fx = c.focal_x, fy = c.focal_y;
    const float j00 = fx / t.z, j02 = -(fx * t.x) / (t.z * t.z);
    const float j11 = fy / t.z, j12 = -(fy * t.y) / (t.z * t.z);
    // A = J * Rv, rows A0 (x) and A1 (y); Rv rows (V0,V4,V8) (V1,V5,V9) (V2,V6,V10)
    const float A0[3] = {j00 * V[0] + j02 * V[2], j00 * V[4] + j02 * V[6], j00 * V[8] + j02 * V[10]};
    const float A1[3] = {j11 * V[1] + j12 * V[2], j11 * V[5] + j12 * V[6], j11 * V[9] + j12 * V[10]};

    float cov[6];
    const float3 sc3 = gi.sc3;
    const float4 q = gi.q;
    if (gi.cov3D) {
        for (int k = 0; k < 6; k++) cov[k] = gi.cov3D[k];
    } else {
        const float r_ = q.x, x = q.y, y = q.z, z = q.w;
        const float sx = gi.scale_modifier * sc3.x, sy = gi.scale_modifier * sc3.y, sz = gi.scale_modifier * sc3.z;
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
    float d_inside_root = 0.f;
    if (c.antialiasing) {
        const float det_cov = c_xx * c_yy - c_xy * c_xy;
        c_xx += h_var;
        c_yy += h_var;
        const float det_cov_plus_h_cov = c_xx * c_yy - c_xy * c_xy;
        const float h = sqrtf(fmaxf(0.000025f, det_cov / det_cov_plus_h_cov));
        const float d_h = dop * *gi.opacity;
        dop = dop * h;
        d_inside_root = (det_cov / det_cov_plus_h_cov) <= 0.000025f ? 0.f : d_h / (2.f * h);
    } else {
        c_xx += h_var;
        c_yy += h_var;
    }
    float dL_dc_xx = 0.f, dL_dc_xy = 0.f, dL_dc_yy = 0.f;
    if (c.antialiasing) {
        // the reference's formula (CR/backward.cu:256-270), at the dilated x, y as written there
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
        dL_dc_xx += denom2inv * (-c_yy * c_yy * dca + 2.f * c_xy * c_yy * dcb + (denom - c_xx * c_yy) * dcc);
        dL_dc_yy += denom2inv * (-c_xx * c_xx * dcc + 2.f * c_xx * c_xy * dcb + (denom - c_xx * c_yy) * dca);
        dL_dc_xy += denom2inv * 2.f * (c_xy * c_yy * dca - (denom + 2.f * c_xy * c_xy) * dcb + c_xx * c_xy * dcc);
    }
    out.dop(dop);

    // tail: cov2D = A Sigma A^T  ->  dL/dcov3D (6 stored entries) and dL/dA
    const float ga = dL_dc_xx, gb = dL_dc_xy, gc = dL_dc_yy;
    float dcov[6];
    dcov[0] = A0[0] * A0[0] * ga + A0[0] * A1[0] * gb + A1[0] * A1[0] * gc;
    dcov[3] = A0[1] * A0[1] * ga + A0[1] * A1[1] * gb + A1[1] * A1[1] * gc;
    dcov[5] = A0[2] * A0[2] * ga + A0[2] * A1[2] * gb + A1[2] * A1[2] * gc;
    dcov[1] = 2.f * A0[0] * A0[1] * ga + (A0[0] * A1[1] + A0[1] * A1[0]) * gb + 2.f * A1[0] * A1[1] * gc;
    dcov[2] = 2.f * A0[0] * A0[2] * ga + (A0[0] * A1[2] + A0[2] * A1[0]) * gb + 2.f * A1[0] * A1[2] * gc;
    dcov[4] = 2.f * A0[2] * A0[1] * ga + (A0[1] * A1[2] + A0[2] * A1[1]) * gb + 2.f * A1[1] * A1[2] * gc;
    out.dcov(dcov);

    float dA0[3], dA1[3];
    for (int k = 0; k < 3; k++) {
        dA0[k] = 2.f * ga * SA0[k] + gb * SA1[k];
        dA1[k] = 2.f * gc * SA1[k] + gb * SA0[k];
    }
    const float dJ00 = dA0[0] * V[0] + dA0[1] * V[4] + dA0[2] * V[8];
    const float dJ02 = dA0[0] * V[2] + dA0[1] * V[6] + dA0[2] * V[10];
    const float dJ11 = dA1[0] * V[1] + dA1[1] * V[5] + dA1[2] * V[9];
    const float dJ12 = dA1[0] * V[2] + dA1[1] * V[6] + dA1[2] * V[10];
    const float tz = 1.f / t.z, tz2 = tz * tz, tz3 = tz2 * tz;
    const float dL_dtx = x_grad_mul * -fx * tz2 * dJ02;
    const float dL_dty = y_grad_mul * -fy * tz2 * dJ12;
    float dL_dtz =
        -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2.f * fx * t.x) * tz3 * dJ02 + (2.f * fy * t.y) * tz3 * dJ12;
    if (c.have_invdepth) dL_dtz -= dinvd / (t.z * t.z);
    // transformVec4x3Transpose (CR/auxiliary.h:109-117)
    float3 dmean = make_float3(V[0] * dL_dtx + V[1] * dL_dty + V[2] * dL_dtz,
                               V[4] * dL_dtx + V[5] * dL_dty + V[6] * dL_dtz,
                               V[8] * dL_dtx + V[9] * dL_dty + V[10] * dL_dtz);

    // ---- screen-space mean -> 3-D mean through the projection (CR/backward.cu:403-420)
    const float* Pm = c.Pm;
    const float4 m_hom = xform_point_4x4(mean, Pm);
    const float m_w = 1.0f / (m_hom.w + 0.0000001f);
    const float mul1 = m_hom.x * m_w * m_w, mul2 = m_hom.y * m_w * m_w;
    dmean.x += (Pm[0] * m_w - Pm[3] * mul1) * m2x + (Pm[1] * m_w - Pm[3] * mul2) * m2y;
    dmean.y += (Pm[4] * m_w - Pm[7] * mul1) * m2x + (Pm[5] * m_w - Pm[7] * mul2) * m2y;
    dmean.z += (Pm[8] * m_w - Pm[11] * mul1) * m2x + (Pm[9] * m_w - Pm[11] * mul2) * m2y;

    // ---- SH colour backward (CR/backward.cu:12-146), the clamp mask zeroing its channels (:26-28)
    if (do_sh) {
        const float3 v = make_float3(mean.x - c.campos[0], mean.y - c.campos[1], mean.z - c.campos[2]);
        const float3 g = make_float3((cm & 1) ? 0.f : dcol.x, (cm & 2) ? 0.f : dcol.y, (cm & 4) ? 0.f : dcol.z);
        if constexpr (SHM == kShNow)
            sh_dir_backward(sh, D, M, v, g, dmean);
        else
            out.sh_defer(v, g);
    }
    out.dmean(dmean);

    // ---- scale / rotation backward (CR/backward.cu:296-365, called when scales are given, :427-428)
    if (gi.have_scales) {
        const float r_ = q.x, x = q.y, y = q.z, z = q.w;
        // Rg[col][row] = the reference's GLM rotation (R_std transposed)
        const float Rg[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r_ * z), 2.f * (x * z + r_ * y)},
                                {2.f * (x * y + r_ * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r_ * x)},
                                {2.f * (x * z - r_ * y), 2.f * (y * z + r_ * x), 1.f - 2.f * (x * x + y * y)}};
        const float s[3] = {gi.scale_modifier * sc3.x, gi.scale_modifier * sc3.y, gi.scale_modifier * sc3.z};
        const float dS[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                                {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                                {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
        // dMt[r][c] = dL_dM[c][r], dL_dM = 2 M dSigma (GLM product), M[k][r] = s_r Rg[k][r]
        float dMt[3][3];
        for (int c = 0; c < 3; c++)
            for (int rr = 0; rr < 3; rr++)
                dMt[rr][c] = 2.f * s[rr] * (Rg[0][rr] * dS[c][0] + Rg[1][rr] * dS[c][1] + Rg[2][rr] * dS[c][2]);
        // dot(Rt[i], dL_dMt[i]) -- the reference leaves the scale modifier out here
        const float ds0 = Rg[0][0] * dMt[0][0] + Rg[1][0] * dMt[0][1] + Rg[2][0] * dMt[0][2];
        const float ds1 = Rg[0][1] * dMt[1][0] + Rg[1][1] * dMt[1][1] + Rg[2][1] * dMt[1][2];
        const float ds2 = Rg[0][2] * dMt[2][0] + Rg[1][2] * dMt[2][1] + Rg[2][2] * dMt[2][2];
        const float3 dscale = make_float3(ds0, ds1, ds2);
        for (int i = 0; i < 3; i++)
            for (int kk = 0; kk < 3; kk++) dMt[i][kk] *= s[i];
        float4 dq;
        dq.x = 2.f * z * (dMt[0][1] - dMt[1][0]) + 2.f * y * (dMt[2][0] - dMt[0][2]) +
               2.f * x * (dMt[1][2] - dMt[2][1]);
        dq.y = 2.f * y * (dMt[1][0] + dMt[0][1]) + 2.f * z * (dMt[2][0] + dMt[0][2]) +
               2.f * r_ * (dMt[1][2] - dMt[2][1]) - 4.f * x * (dMt[2][2] + dMt[1][1]);
        dq.z = 2.f * x * (dMt[1][0] + dMt[0][1]) + 2.f * r_ * (dMt[2][0] - dMt[0][2]) +
               2.f * z * (dMt[1][2] + dMt[2][1]) - 4.f * y * (dMt[2][2] + dMt[0][0]);
        dq.w = 2.f * r_ * (dMt[0][1] - dMt[1][0]) + 2.f * x * (dMt[2][0] + dMt[0][2]) +
               2.f * y * (dMt[1][2] + dMt[2][1]) - 4.f * z * (dMt[1][1] + dMt[0][0]);
        out.scale_rot(true, dscale, dq);
    } else {
        out.scale_rot(false, make_float3(0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

}  // namespace gsr
