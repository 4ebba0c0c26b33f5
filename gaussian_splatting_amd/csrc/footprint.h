// footprint.h -- conservative tests of a splat's alpha >= 1/255 footprint against the
// 8x8 quadrants of a 16x16 tile.  The forward render runs them while staging (one list entry
// per lane) for the quadrants its wave owns, and walks an entry only in the quadrants the
// footprint reaches.  Inputs are the first three rows of the splat record (gsr_common.h).
#pragma once

#include "gsr_common.h"

namespace gsr {

// clamp(v, lo, hi) for lo <= hi as one v_med3_f32
__device__ __forceinline__ float clamp_med3(float v, float lo, float hi) { return __builtin_amdgcn_fmed3f(v, lo, hi); }

// The ellipse side of the test: per-splat values, computed once per staged entry.
struct FootprintForm {
    float a, b, c;  // conic
    float ra, rc;   // ~1/a, ~1/c
    float lim;      // Q <= lim  <=>  alpha >= 1/255, with the box's margin (preprocess.hip)
    bool exact;     // false: degenerate conic or opacity, the box decides alone
};

// ra and rc only place a clamped parabola vertex: an error of d in the vertex moves the edge's
// minimum by (a or c) d^2, so the raw v_rcp_f32 (1 ulp) serves.  lim = 2 (max(0, ln(255 o)) 1.001 + 0.01)
// from the raw v_log_f32 (1 ulp, no denormal inputs: an entry with a box has 255 o >= 0.999); both
// errors are ~1e-7 relative against a margin of 1e-3 relative plus 0.02 absolute.
__device__ __forceinline__ FootprintForm footprint_form(float4 v0, float4 v1) {
    FootprintForm f;
    f.a = v0.z, f.b = v0.w, f.c = v1.x;
    const float o = v1.y;
    f.exact = (f.a > 0.f && f.c > 0.f && f.a * f.c - f.b * f.b > 0.f) && (o > 0.f);
    f.ra = __builtin_amdgcn_rcpf(f.a), f.rc = __builtin_amdgcn_rcpf(f.c);
    constexpr float kLn2 = 0.6931471805599453f;
    f.lim = fmaxf(0.f, __builtin_amdgcn_logf(255.f * o)) * (2.f * 1.001f * kLn2) + 0.02f;
    return f;
}

// Does the conic's quadratic form Q(d) = a dx^2 + 2 b dx dy + c dy^2 (power = -Q/2) stay above lim on
// the whole pixel-centre rectangle [x0, x0+7] x [y0, y0+7] of offsets d = p - mean?
// Q is convex with its minimum (0) at the mean, so from any point the direction to the mean descends:
// a constrained minimum sits where that direction leaves the rectangle, on an edge that faces the mean,
// x = cx = clamp(0, x0, x1) or y = cy = clamp(0, y0, y1).  On such an edge Q is a 1-D parabola, least at
// its clamped vertex.  With the mean inside, cx = cy = 0 and both values are 0: no special case, no
// divergence.  (When the rectangle straddles the mean's column or row, cx or cy is 0 and that value is
// Q on a line through the rectangle: never below the minimum.)
// Two compares, not a minimum: a NaN from a conic at the edge of the number range keeps the quadrant.
__device__ __forceinline__ bool rect_misses(const FootprintForm& f, float x0, float y0) {
    const float x1 = x0 + 7.f, y1 = y0 + 7.f;
    const float cx = clamp_med3(0.f, x0, x1), cy = clamp_med3(0.f, y0, y1);
    const float dy = clamp_med3(-f.b * cx * f.rc, y0, y1);
    const float qv = f.a * cx * cx + (2.f * f.b * cx + f.c * dy) * dy;  // least Q on x = cx
    const float dx = clamp_med3(-f.b * cy * f.ra, x0, x1);
    const float qh = f.c * cy * cy + (2.f * f.b * cy + f.a * dx) * dx;  // least Q on y = cy
    return qv > f.lim && qh > f.lim;
}

// Footprint mask of the NQ quadrants one render wave owns: NQ = 4 the whole tile (bit k: quadrant k, at
// (k & 1, k >> 1)), NQ = 2 a half tile's left and right quadrant, NQ = 1 a single quadrant; (qx0, qy0) is
// the pixel origin of the first of them.  A quadrant's bit is set when the footprint box overlaps it and
// the ellipse Q <= lim reaches one of its pixel centres; a degenerate conic keeps the box result.
template <int NQ>
__device__ __forceinline__ uint32_t quad_bits(float4 v0, float4 v1, float4 v2, int qx0, int qy0) {
    const uint32_t bx = __float_as_uint(v1.w), by = __float_as_uint(v2.w);
    const int bx0 = unpack_lo(bx), bx1 = unpack_hi(bx), by0 = unpack_lo(by), by1 = unpack_hi(by);
    const FootprintForm f = footprint_form(v0, v1);
    uint32_t q = 0;
#pragma unroll
    for (int k = 0; k < NQ; k++) {
        const int ox = NQ == 1 ? 0 : (k & 1) * 8, oy = NQ == 4 ? (k >> 1) * 8 : 0;
        const bool box = bx0 <= qx0 + ox + 7 && bx1 >= qx0 + ox && by0 <= qy0 + oy + 7 && by1 >= qy0 + oy;
        // (the pixel coordinate is converted, then the mean subtracted: the offsets the per-pixel walk forms)
        const bool miss = f.exact && rect_misses(f, (float)(qx0 + ox) - v0.x, (float)(qy0 + oy) - v0.y);
        if (box && !miss) q |= 1u << k;
    }
    return q;
}

// One quadrant's bit: does the alpha >= 1/255 footprint (box, then ellipse) reach a pixel centre of
// the 8x8 quadrant at (qx0, qy0)?
__device__ __forceinline__ bool quad_hit(float4 v0, float4 v1, float4 v2, int qx0, int qy0) {
    return quad_bits<1>(v0, v1, v2, qx0, qy0) != 0u;
}

}  // namespace gsr
