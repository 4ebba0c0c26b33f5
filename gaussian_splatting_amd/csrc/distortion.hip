// distortion.hip -- the depth-distortion map of a finished forward's blend weights for a per-Gaussian scalar t, and
// its backward (include/gsr.h gsr_render_distortion / gsr_render_distortion_backward).
//
// Per pixel, over the contributing entries 1..n in the forward's list order with w_i = alpha_i T_i,
//     D = 2 sum_i w_i (t_i A_{i-1} - B_{i-1}),   A_k = sum_{j<=k} w_j,   B_k = sum_{j<=k} w_j t_j
// (= sum_{i,j} w_i w_j |t_i - t_j| for t non-decreasing along the list).  The walk is features.hip's: one wave64 per
// tile walks the tile's WHOLE list from its head, entries staged 64 at a time into LDS with each entry's t beside its
// conic, only entries with a non-zero blend mask walked and only the quadrants whose bit is set evaluated, alpha and
// T recomputed in the forward's order with the exponent spelled as contrib.hip spells it, each pixel stopped at its
// n_contrib.  Every weight therefore depends on the forward's discrete state alone.
//
// D and its gradients depend on differences of t only, so both kernels take t ABOUT THE PIXEL'S FIRST CONTRIBUTOR'S
// (t_i - t_1, found identically by both: the entry blended while T is still 1).  B and the products t A then have the
// size of the depth spread among the pixel's contributors, not of the depth itself, and float32 loses nothing to the
// cancellation in t_i A - B: on a 10000-entry list the geometry sums came out 500 times closer to float64.
//
// Forward: T, A, B, D of the four quadrant slots stay in registers; D and the moments (A_n and B_n, the latter about
// t_1) of every pixel of the image are written once by the one wave that owns it -- no atomics, bitwise reproducible.
// Backward: with the pixel's totals A_n, B_n, D (inputs), upstream U and the prefix sums BEFORE entry i,
//     g_i = dD/dw_i = 2 (t_i (2 A_prev - A_n) + B_n - 2 B_prev),      dD/dt_i = 2 w_i (2 A_prev + w_i - A_n),
//     dL/dalpha_i = U (T_i g_i - (2 D - sum_{h<=i} w_h g_h) / (1 - alpha_i))
// (sum_h w_h g_h = 2 D: D is homogeneous of degree 2 in w), so the suffix sum is had front to back as in
// features_bwd_kernel.  Per walked entry the wave makes one 8-value reduce-scatter -- the six screen-space sums of
// render.hip's render_bwd and the dL/dt term -- and after each batch flushes the written entries with NO-RETURN FLOAT
// ATOMICS: eight lanes per entry, one add into dL_dt[g] and six into floats 4..9 of the Gaussian's scratch accumulator
// row (GeomState::acc's layout, which launch_gauss_live_views turns into a view block), plus its touched bit.  Without
// GEOM the kernel forms dL/dt alone.  Both outputs are zeroed by the caller and not bitwise reproducible.
//
// The helpers restate features.hip's (private to their translation units); this file is built with render.hip's
// flags so that the exponent and alpha round as they do there.
#include "kernels.h"

namespace gsr {
namespace {

constexpr int kBatch = 64;  // list entries staged per round (one per lane)
constexpr float kLog2e = 1.4426950408889634f;
constexpr uint32_t kNoGauss = 0xffffffffu;

__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// (A, B, C, quads): the staged conic of render.hip stage_conic
__device__ __forceinline__ float4 stage_conic(float4 v0, float4 v1, uint32_t qm) {
    return make_float4(-0.5f * kLog2e * v0.z, -kLog2e * v0.w, -0.5f * kLog2e * v1.x, __uint_as_float(qm));
}

__device__ __forceinline__ void unit_sync() { wave_lds_sync(); }

// Reduce-scatter of eight per-lane values over the wave (features.hip reduce8): the lanes with (lane & 7) == 0 end
// up with value reduced_index8(lane).
__device__ __forceinline__ float reduce8(const float (&v)[8], int lane) {
    float h[4], r[2];
#pragma unroll
    for (int i = 0; i < 4; i++) h[i] = half_fold(v[2 * i], v[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 2; i++) r[i] = row_fold(h[2 * i], h[2 * i + 1]);
    return half_row_allsum(eight_fold(r[0], r[1], (lane & 8) != 0));
}
__device__ __forceinline__ int reduced_index8(int lane) {
    const int row = lane >> 4;
    return 4 * ((lane >> 3) & 1) + 2 * (row & 1) + (row >> 1);
}

// The tile's list as far as any pixel of the tile blends it, or nothing for a tile, a range or a limit that is not
// this forward's (foreign buffers must not send the walk out of bounds).
struct TileWalk {
    uint2 range;
    int limit;
    int slim[4];
    uint32_t live;  // slots with a contributor at all
    int next_lim;   // smallest slot limit among them
};
__device__ __forceinline__ TileWalk tile_walk(const FeatureArgs& a, uint32_t tile, const int (&nc)[4]) {
    TileWalk t;
    t.range = a.ranges[tile];
    const bool ok = t.range.x <= t.range.y && t.range.y <= a.n_entries;
    const int n = ok ? (int)(t.range.y - t.range.x) : 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        t.slim[q] = min(n, __builtin_amdgcn_readlane((int)wave_incl_max((uint32_t)nc[q]), 63));  // max over the wave
    t.limit = max(max(t.slim[0], t.slim[1]), max(t.slim[2], t.slim[3]));
    t.live = 0;
    t.next_lim = t.limit;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (t.slim[q] > 0) {
            t.live |= 1u << q;
            t.next_lim = min(t.next_lim, t.slim[q]);
        }
    return t;
}
// At list position pos: retires the slots whose last contributor has passed (uniform).
__device__ __forceinline__ void retire(TileWalk& t, int pos) {
    if (pos < t.next_lim) return;
    t.next_lim = t.limit;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (pos >= t.slim[q]) t.live &= ~(1u << q);
        else t.next_lim = min(t.next_lim, t.slim[q]);
    }
}

// One batch's entries into LDS: position, opacity and t, and the staged conic of lane's entry, its Gaussian
// (kNoGauss for an entry that is not walked).  Returns the lane's entry's blend mask (0: not walked).
__device__ __forceinline__ uint32_t stage_batch(const FeatureArgs& a, uint32_t ent, bool has, int lane, float4* s_xy,
                                                float4* s_cq, uint32_t* s_gid, float4* raw) {
    uint32_t qm = 0, g = kNoGauss;
    if (has) {
        const uint32_t e = ent >> kEntryMaskBits;
        if ((ent & kEntryMask) && e < a.n_gauss) {  // (an entry no pixel blended is not walked)
            const float4* rec = a.rec + (size_t)kRecRows * e;
            const float4 v0 = rec[0], v1 = rec[1];
            s_xy[lane] = make_float4(v0.x, v0.y, v1.y, a.features[e]);
            qm = ent & kEntryMask;
            s_cq[lane] = stage_conic(v0, v1, qm);
            if (raw) *raw = make_float4(v0.z, v0.w, v1.x, v1.y);  // conic a, b, c and opacity, for the flush
            g = e;
        }
    }
    if (s_gid) s_gid[lane] = g;
    unit_sync();
    return qm;
}

}  // namespace

__global__ void __launch_bounds__(64) distortion_fwd_kernel(DistortionArgs da) {
    const FeatureArgs& a = da.walk;
    const uint32_t tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int tile_x0 = (int)(tile % a.gx) * kTile, tile_y0 = (int)(tile / a.gx) * kTile;
    const int lx = lane & 7, ly = lane >> 3;
    const float pxf0 = (float)(tile_x0 + lx), pyf0 = (float)(tile_y0 + ly);  // this lane's pixel in quadrant 0

    __shared__ float4 s_xy[kBatch], s_cq[kBatch];  // (x, y, opacity, t), (A, B, C, quads)

    float T[4], A[4], B[4], D[4], t1[4];
    int nc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int px = tile_x0 + (q & 1) * 8 + lx, py = tile_y0 + (q >> 1) * 8 + ly;
        const uint32_t c = a.n_contrib[tile_px(tile, q, lane)];
        nc[q] = px < a.W && py < a.H ? (int)c : 0;
        T[q] = 1.f;
        A[q] = B[q] = D[q] = t1[q] = 0.f;
    }
    TileWalk tw = tile_walk(a, tile, nc);
    const int limit = tw.limit;
    uint32_t ent_next = lane < limit ? a.gid_sorted[tw.range.x + lane] : 0u;  // the next batch's entry
    for (int b0 = 0; b0 < limit; b0 += kBatch) {
        const bool has = b0 + lane < limit;
        const uint32_t ent = ent_next;
        if (b0 + kBatch + lane < limit) ent_next = a.gid_sorted[tw.range.x + b0 + kBatch + lane];
        const uint32_t qm = stage_batch(a, ent, has, lane, s_xy, s_cq, nullptr, nullptr);
        unsigned long long todo = __ballot(qm != 0);
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int pos = b0 + j;
            const float4 xy = s_xy[j], cq = s_cq[j];
            retire(tw, pos);
            const uint32_t m = uniform_u32(__float_as_uint(cq.w)) & tw.live;
            if (m == 0) continue;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (!(m & (1u << q))) continue;  // uniform
                const float dx = xy.x - (pxf0 + (float)((q & 1) * 8)), dy = xy.y - (pyf0 + (float)((q >> 1) * 8));
                // render_fwd's exponent with the two fused multiply-adds spelled out as in contrib.hip, so alpha, and
                // with it T, is the forward's bit for bit
                const float p2 = fmaf(dx, fmaf(dx, cq.x, cq.y * dy), (cq.z * dy) * dy);
                const float G = __builtin_amdgcn_exp2f(p2);
                const float ac = fminf(0.99f, xy.z * G);
                const bool on = (p2 <= 0.f) & (ac >= 1.0f / 255.0f) & (pos < nc[q]);
                if (!__ballot(on)) continue;  // uniform
                const float alpha = on ? ac : 0.f;
                const float w = alpha * T[q];  // (w = 0 leaves A, B and D unchanged)
                if (on && T[q] == 1.f) t1[q] = xy.w;  // the pixel's first contributor (T < 1 after it)
                const float t = xy.w - t1[q];
                D[q] = fmaf(w, fmaf(t, A[q], -B[q]), D[q]);
                A[q] += w;
                B[q] = fmaf(w, t, B[q]);
                T[q] *= 1.f - alpha;  // alpha = 0 leaves T unchanged
            }
        }
        unit_sync();  // (the batch's LDS rows are read for the last time)
    }
    const size_t N = (size_t)a.W * a.H;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int px = tile_x0 + (q & 1) * 8 + lx, py = tile_y0 + (q >> 1) * 8 + ly;
        if (px < a.W && py < a.H) {
            const size_t pix = (size_t)py * a.W + px;
            a.out[pix] = 2.f * D[q];
            da.moments[pix] = A[q];
            da.moments[N + pix] = B[q];
        }
    }
}

// GEOM: also the screen-space sums of the distortion loss (FeatureArgs::acc / touched non-null; the launcher picks
// the instantiation by the pointer).  Without it the kernel forms dL/dt only and never reads the map.
template <bool GEOM>
__global__ void __launch_bounds__(64) distortion_bwd_kernel(DistortionArgs da) {
    const FeatureArgs& a = da.walk;
    const uint32_t tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int tile_x0 = (int)(tile % a.gx) * kTile, tile_y0 = (int)(tile / a.gx) * kTile;
    const int lx = lane & 7, ly = lane >> 3;
    const float pxf0 = (float)(tile_x0 + lx), pyf0 = (float)(tile_y0 + ly);

    __shared__ float4 s_xy[kBatch], s_cq[kBatch];
    __shared__ uint32_t s_gid[kBatch];
    // per entry: the six reduced sums and the dL/dt term (float 6); without GEOM the dL/dt term alone
    __shared__ __attribute__((aligned(16))) float s_sum[GEOM ? kBatch * 8 : kBatch];
    __shared__ uint32_t s_wj[kBatch];  // written entries' slots

    const size_t N = (size_t)a.W * a.H;
    float T[4], Ap[4], Bp[4], An[4], Bn[4], U[4], gB[4], t1[4];
    int nc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {  // (an outside pixel reads a clamped, valid address and is zeroed)
        const int px = tile_x0 + (q & 1) * 8 + lx, py = tile_y0 + (q >> 1) * 8 + ly;
        const bool in = px < a.W && py < a.H;
        const size_t pix = (size_t)min(py, a.H - 1) * a.W + min(px, a.W - 1);
        const uint32_t c = a.n_contrib[tile_px(tile, q, lane)];
        nc[q] = in ? (int)c : 0;
        T[q] = 1.f;
        Ap[q] = Bp[q] = t1[q] = 0.f;
        const float u = a.dL_dfmap[pix];
        U[q] = in ? u : 0.f;
        An[q] = da.moments[pix];
        Bn[q] = da.moments[N + pix];
        // U sum_h w_h g_h = 2 U D over the whole list: shrinks to "strictly behind this entry" as the walk proceeds
        gB[q] = GEOM ? 2.f * U[q] * a.fmap[pix] : 0.f;
    }
    TileWalk tw = tile_walk(a, tile, nc);
    const int limit = tw.limit;
    const int k8 = reduced_index8(lane);
    uint32_t ent_next = lane < limit ? a.gid_sorted[tw.range.x + lane] : 0u;
    for (int b0 = 0; b0 < limit; b0 += kBatch) {
        const bool has = b0 + lane < limit;
        const uint32_t ent = ent_next;
        if (b0 + kBatch + lane < limit) ent_next = a.gid_sorted[tw.range.x + b0 + kBatch + lane];
        float4 raw = make_float4(0.f, 0.f, 0.f, 0.f);
        const uint32_t qm = stage_batch(a, ent, has, lane, s_xy, s_cq, s_gid, GEOM ? &raw : nullptr);
        unsigned long long todo = __ballot(qm != 0);
        unsigned long long written = 0;
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int pos = b0 + j;
            const float4 xy = s_xy[j], cq = s_cq[j];
            retire(tw, pos);
            const uint32_t m = uniform_u32(__float_as_uint(cq.w)) & tw.live;
            if (m == 0) continue;
            float r[8];
#pragma unroll
            for (int k = 0; k < 8; k++) r[k] = 0.f;
            bool contrib = false;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (!(m & (1u << q))) continue;  // uniform
                const float dx = xy.x - (pxf0 + (float)((q & 1) * 8)), dy = xy.y - (pyf0 + (float)((q >> 1) * 8));
                const float p2 = fmaf(dx, fmaf(dx, cq.x, cq.y * dy), (cq.z * dy) * dy);  // (as the forward kernel's)
                const float G = __builtin_amdgcn_exp2f(p2);
                const float ac = fminf(0.99f, xy.z * G);
                const bool on = (p2 <= 0.f) & (ac >= 1.0f / 255.0f) & (pos < nc[q]);
                if (!__ballot(on)) continue;  // uniform
                contrib = true;
                const float alpha = on ? ac : 0.f;
                const float w = alpha * T[q];
                if (on && T[q] == 1.f) t1[q] = xy.w;  // (as the forward kernel's)
                const float t = xy.w - t1[q];
                const float c = 2.f * Ap[q] - An[q];
                r[6] = fmaf(U[q], 2.f * w * (c + w), r[6]);  // (w = 0: nothing)
                const float one_m_a = 1.f - alpha;
                if (GEOM) {  // render_bwd's per-pixel terms with U g in place of dL/dpix . colour
                    const float s = U[q] * (2.f * (fmaf(t, c, Bn[q]) - 2.f * Bp[q]));
                    gB[q] -= w * s;
                    const float dLda = T[q] * s - gB[q] * __builtin_amdgcn_rcpf(one_m_a);
                    const float u = on ? dLda * G : 0.f;
                    const float udx = u * dx, udy = u * dy;
                    r[0] += udx;
                    r[1] += udy;
                    r[2] += udx * dx;
                    r[3] += udx * dy;
                    r[4] += udy * dy;
                    r[5] += u;
                }
                Ap[q] += w;
                Bp[q] = fmaf(w, t, Bp[q]);
                T[q] *= one_m_a;  // alpha = 0 leaves T unchanged
            }
            if (contrib) {  // uniform
                if (GEOM) {
                    const float g = reduce8(r, lane);
                    if ((lane & 7) == 0) s_sum[j * 8 + k8] = g;
                } else {
                    const float g = wave_sum_to_lane63(r[6]);
                    if (lane == 63) s_sum[j] = g;
                }
                written |= 1ull << j;
            }
        }
        unit_sync();
        const bool mine = has && ((written >> lane) & 1ull);
        if (!GEOM) {  // one add per written entry (no value returned: fire and forget)
            if (mine) (void)atomicAdd(a.dL_dfeatures + (ent >> kEntryMaskBits), s_sum[lane]);
        } else {
            if (mine) {  // this entry's place in the list of written entries
                s_wj[__popcll(written & ((1ull << lane) - 1ull))] = (uint32_t)lane;
                // the sums in their final form (render_bwd's flush): dL/dmean2D in NDC units, dL/dopacity_eff,
                // dL/dconic with the reference's -0.5 factors, in the order of accumulator row floats 4..9
                const float4 S = reinterpret_cast<const float4*>(s_sum)[lane * 2];
                const float s8 = s_sum[lane * 8 + 4], s9 = s_sum[lane * 8 + 5];
                const float ca = raw.x, cb = raw.y, cc = raw.z, o = raw.w;
                reinterpret_cast<float4*>(s_sum)[lane * 2] =
                    make_float4(-0.5f * (float)a.W * o * (ca * S.x + cb * S.y),
                                -0.5f * (float)a.H * o * (cc * S.y + cb * S.x), s9, -0.5f * o * S.w);
                s_sum[lane * 8 + 4] = -0.5f * o * S.z;
                s_sum[lane * 8 + 5] = -0.5f * o * s8;
                const uint32_t e = ent >> kEntryMaskBits;
                (void)atomicOr(a.touched + (e >> 5), 1u << (e & 31u));  // OR is order-free
            }
            unit_sync();
            // one wave instruction per eight listed entries: lane 8 k + v adds value v of listed entry k
            const int nw = __popcll(written), sub = lane >> 3, v = lane & 7;
            for (int k0 = 0; k0 < nw; k0 += 8) {  // uniform
                const int k = k0 + sub;
                if (k < nw) {
                    const int j = (int)s_wj[k];
                    const uint32_t g = s_gid[j];
                    if (v < 6) (void)atomicAdd(a.acc + (size_t)g * (4 * kAccRow4) + 4 + v, s_sum[j * 8 + v]);
                    else if (v == 6) (void)atomicAdd(a.dL_dfeatures + g, s_sum[j * 8 + 6]);
                }
            }
        }
        unit_sync();
    }
}

hipError_t launch_distortion_fwd(const DistortionArgs& a, hipStream_t stream) {
    const uint32_t tiles = a.walk.gx * a.walk.gy;
    if (tiles == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(distortion_fwd_kernel, dim3(tiles), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_distortion_bwd(const DistortionArgs& a, hipStream_t stream) {
    const uint32_t tiles = a.walk.gx * a.walk.gy;
    if (tiles == 0) return hipErrorInvalidValue;
    if (a.walk.acc && a.walk.touched)
        hipLaunchKernelGGL((distortion_bwd_kernel<true>), dim3(tiles), dim3(kWave), 0, stream, a);
    else
        hipLaunchKernelGGL((distortion_bwd_kernel<false>), dim3(tiles), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

}  // namespace gsr
