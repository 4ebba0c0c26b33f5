// features.hip -- N-channel per-Gaussian feature vectors blended with a finished forward's own weights, and the
// backward of that blend (include/gsr.h gsr_render_features / gsr_render_features_backward).
//
// Two passes of their own over what the forward left behind, read-only on its buffers: the sorted tile lists with
// the blend masks, the splat records and n_contrib.  One wave64 per (tile, chunk of kFeatChunk channels) walks the
// tile's WHOLE list from its head: entries staged 64 at a time into LDS with the chunk of each entry's feature row
// beside its conic, only entries with a non-zero blend mask walked and only the quadrants whose bit is set
// evaluated, alpha and T recomputed in the forward's order with the exponent spelled as contrib.hip spells it,
// each pixel stopped at its n_contrib.  Every weight therefore depends on the forward's discrete state alone (list
// order, blend masks, n_contrib), not on its checkpoints: the map is the same bits after a half-tile, a whole-tile
// or a no_backward forward and for copies of the buffers.  The blend is linear in the channels, so a chunk is an
// independent render and the chunks' shares of the per-Gaussian sums simply add.
//
// Forward: the chunk's 4 x kFeatChunk accumulators stay in registers, every pixel of the image is written once by
// the one wave that owns it -- no atomics, bitwise reproducible.
// Backward: per entry the wave reduces w U[c] over its pixels for the chunk's channels (a reduce-scatter: lane
// swaps and DPP folds, no LDS) and, in the GEOM instantiation, the six screen-space sums of render.hip's
// render_bwd for dL/dalpha = T s - (sum_{h>g} w_h s_h) / (1 - alpha), s = sum_c U[c] F[c], the suffix sum had front
// to back as U . Fmap - sum_{h<=g} w_h s_h (render_bwd's prefix form; Fmap is an input).  After each batch the
// written entries are flushed with NO-RETURN FLOAT ATOMICS: sixteen lanes per entry add its chunk of dL_dF (64
// contiguous bytes, four entries per wave instruction), and six lanes per entry add the sums in their final form
// into floats 4..9 of the Gaussian's scratch accumulator row (the layout of GeomState::acc, which
// launch_gauss_live_views turns into a view block) and set its touched bit.  Both outputs are zeroed by the caller;
// their summation order over a Gaussian's tile instances follows the hardware, so they are not bitwise reproducible.
//
// The helpers restate render.hip's and contrib.hip's (private to their translation units); this file is built with
// render.hip's flags so that the exponent and alpha round as they do there.
#include "kernels.h"

#include <algorithm>

namespace gsr {
namespace {

constexpr int kBatch = 64;  // list entries staged per round (one per lane)
constexpr int kCh = kFeatChunk;
constexpr float kLog2e = 1.4426950408889634f;
constexpr uint32_t kNoGauss = 0xffffffffu;
static_assert(kCh == 16, "the reduce-scatter below folds sixteen values; the flush gives an entry sixteen lanes");

__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// (A, B, C, quads): the staged conic of render.hip stage_conic
__device__ __forceinline__ float4 stage_conic(float4 v0, float4 v1, uint32_t qm) {
    return make_float4(-0.5f * kLog2e * v0.z, -kLog2e * v0.w, -0.5f * kLog2e * v1.x, __uint_as_float(qm));
}

__device__ __forceinline__ void unit_sync() { wave_lds_sync(); }

// four_fold(x, y, hi4) with hi4 = (lane & 4): on every 8-lane half row, lanes 0-3 get x[l] + x[7 - l] and lanes
// 4-7 get y[l] + y[7 - l] (DPP row_half_mirror: each value's eight partials end up in four lanes)
__device__ __forceinline__ float four_fold(float x, float y, bool hi4) {
    const float a = hi4 ? y : x, b = hi4 ? x : y;
    return a + dpp_f32<0x141, 0xf, true>(b);
}
// Sum over each aligned group of four lanes, in every lane of it (quad_perm [1,0,3,2], [2,3,0,1]).
__device__ __forceinline__ float quad_allsum(float v) {
    v += dpp_f32<0xB1, 0xf, true>(v);
    v += dpp_f32<0x4E, 0xf, true>(v);
    return v;
}

// Reduce-scatter of sixteen per-lane values over the wave: four halving steps (32-, 16-, 8- and 4-lane folds) leave
// one register in which every aligned group of four lanes holds four partials of one value, and two DPP steps finish
// it.  The value a lane ends up with is reduced_index16(lane).
__device__ __forceinline__ float reduce16(const float (&v)[16], int lane) {
    float h[8], r[4], e[2];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = half_fold(v[2 * i], v[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = row_fold(h[2 * i], h[2 * i + 1]);
    const bool hi8 = (lane & 8) != 0, hi4 = (lane & 4) != 0;
#pragma unroll
    for (int i = 0; i < 2; i++) e[i] = eight_fold(r[2 * i], r[2 * i + 1], hi8);
    return quad_allsum(four_fold(e[0], e[1], hi4));
}
__device__ __forceinline__ int reduced_index16(int lane) {
    const int row = lane >> 4;
    return 8 * ((lane >> 2) & 1) + 4 * ((lane >> 3) & 1) + 2 * (row & 1) + (row >> 1);
}
// The same for eight values (three halving steps, then the 8-lane half row's sum): reduced_index8(lane).
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
};
__device__ __forceinline__ TileWalk tile_walk(const FeatureArgs& a, uint32_t tile, const int (&nc)[4]) {
    TileWalk t;
    t.range = a.ranges[tile];
    const bool ok = t.range.x <= t.range.y && t.range.y <= a.n_entries;
    const int n = ok ? (int)(t.range.y - t.range.x) : 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        t.slim[q] = min(n, __builtin_amdgcn_readlane((int)wave_incl_max((uint32_t)nc[q]), 63));  // DPP max over the wave
    t.limit = max(max(t.slim[0], t.slim[1]), max(t.slim[2], t.slim[3]));
    return t;
}

// One batch's entries into LDS: position, opacity and staged conic of lane's entry, its Gaussian (kNoGauss for an
// entry that is not walked), then the chunk of every walked entry's feature row, sixteen lanes per row (64
// contiguous bytes a row; zeros past the last channel).  Returns the lane's entry's blend mask (0: not walked).
__device__ __forceinline__ uint32_t stage_batch(const FeatureArgs& a, uint32_t ent, bool has, int lane, int c0, int nch,
                                                float4* s_xy, float4* s_cq, uint32_t* s_gid, float* s_f, float4* raw) {
    uint32_t qm = 0, g = kNoGauss;
    if (has) {
        const uint32_t e = ent >> kEntryMaskBits;
        if ((ent & kEntryMask) && e < a.n_gauss) {  // (an entry no pixel blended is not walked)
            const float4* rec = a.rec + (size_t)kRecRows * e;
            const float4 v0 = rec[0], v1 = rec[1];
            s_xy[lane] = make_float4(v0.x, v0.y, v1.y, 0.f);
            qm = ent & kEntryMask;
            s_cq[lane] = stage_conic(v0, v1, qm);
            if (raw) *raw = make_float4(v0.z, v0.w, v1.x, v1.y);  // conic a, b, c and opacity, for the flush
            g = e;
        }
    }
    s_gid[lane] = g;
    unit_sync();
#pragma unroll
    for (int i = 0; i < kCh; i++) {
        const int idx = i * kBatch + lane, j = idx / kCh, k = idx % kCh;
        const uint32_t gj = s_gid[j];
        s_f[idx] = gj != kNoGauss && k < nch ? a.features[(size_t)gj * a.C + c0 + k] : 0.f;
    }
    unit_sync();
    return qm;
}

}  // namespace

__global__ void __launch_bounds__(64) features_fwd_kernel(FeatureArgs a) {
    const uint32_t tile = blockIdx.x;
    const int c0 = (int)blockIdx.y * kCh, nch = min(kCh, a.C - c0);
    const int lane = threadIdx.x;
    const int tile_x0 = (int)(tile % a.gx) * kTile, tile_y0 = (int)(tile / a.gx) * kTile;
    const int lx = lane & 7, ly = lane >> 3;
    const float pxf0 = (float)(tile_x0 + lx), pyf0 = (float)(tile_y0 + ly);  // this lane's pixel in quadrant 0

    __shared__ float4 s_xy[kBatch], s_cq[kBatch];  // (x, y, opacity, -), (A, B, C, quads)
    __shared__ uint32_t s_gid[kBatch];
    __shared__ __attribute__((aligned(16))) float s_f[kBatch * kCh];  // the chunk of each entry's feature row

    float T[4], acc[4][kCh];
    int nc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int px = tile_x0 + (q & 1) * 8 + lx, py = tile_y0 + (q >> 1) * 8 + ly;
        const uint32_t c = a.n_contrib[tile_px(tile, q, lane)];
        nc[q] = px < a.W && py < a.H ? (int)c : 0;
        T[q] = 1.f;
#pragma unroll
        for (int k = 0; k < kCh; k++) acc[q][k] = 0.f;
    }
    const TileWalk tw = tile_walk(a, tile, nc);
    const int limit = tw.limit;
    uint32_t live = 0;     // slots still reachable at the current position (uniform)
    int next_lim = limit;  // smallest slot limit among live slots
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (tw.slim[q] > 0) {
            live |= 1u << q;
            next_lim = min(next_lim, tw.slim[q]);
        }
    uint32_t ent_next = lane < limit ? a.gid_sorted[tw.range.x + lane] : 0u;  // the next batch's entry
    for (int b0 = 0; b0 < limit; b0 += kBatch) {
        const bool has = b0 + lane < limit;
        const uint32_t ent = ent_next;
        if (b0 + kBatch + lane < limit) ent_next = a.gid_sorted[tw.range.x + b0 + kBatch + lane];
        const uint32_t qm = stage_batch(a, ent, has, lane, c0, nch, s_xy, s_cq, s_gid, s_f, nullptr);
        unsigned long long todo = __ballot(qm != 0);
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int pos = b0 + j;
            const float4 xy = s_xy[j], cq = s_cq[j];
            if (pos >= next_lim) {  // uniform: retire the slots whose last contributor has passed
                next_lim = limit;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (pos >= tw.slim[q]) live &= ~(1u << q);
                    else next_lim = min(next_lim, tw.slim[q]);
                }
            }
            const uint32_t m = uniform_u32(__float_as_uint(cq.w)) & live;
            if (m == 0) continue;
            float f[kCh];
#pragma unroll
            for (int k4 = 0; k4 < kCh / 4; k4++) {
                const float4 v = reinterpret_cast<const float4*>(s_f)[j * (kCh / 4) + k4];
                f[4 * k4] = v.x; f[4 * k4 + 1] = v.y; f[4 * k4 + 2] = v.z; f[4 * k4 + 3] = v.w;
            }
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
                const float w = alpha * T[q];
#pragma unroll
                for (int k = 0; k < kCh; k++) acc[q][k] = fmaf(w, f[k], acc[q][k]);
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
            float* o = a.out + (size_t)c0 * N + (size_t)py * a.W + px;
#pragma unroll
            for (int k = 0; k < kCh; k++)
                if (k < nch) o[(size_t)k * N] = acc[q][k];
        }
    }
}

// GEOM: also the screen-space sums of the feature loss (FeatureArgs::acc / touched non-null; the launcher picks the
// instantiation by the pointer).  Without it the kernel does the dL_dF work only and never reads Fmap.
template <bool GEOM>
__global__ void __launch_bounds__(64) features_bwd_kernel(FeatureArgs a) {
    const uint32_t tile = blockIdx.x;
    const int c0 = (int)blockIdx.y * kCh, nch = min(kCh, a.C - c0);
    const int lane = threadIdx.x;
    const int tile_x0 = (int)(tile % a.gx) * kTile, tile_y0 = (int)(tile / a.gx) * kTile;
    const int lx = lane & 7, ly = lane >> 3;
    const float pxf0 = (float)(tile_x0 + lx), pyf0 = (float)(tile_y0 + ly);

    __shared__ float4 s_xy[kBatch], s_cq[kBatch];
    __shared__ uint32_t s_gid[kBatch];
    __shared__ __attribute__((aligned(16))) float s_f[kBatch * kCh];
    __shared__ __attribute__((aligned(16))) float s_df[kBatch * kCh];  // per entry: the chunk's reduced w U sums
    __shared__ __attribute__((aligned(16))) float s_geo[GEOM ? kBatch * 8 : 8];  // per entry: the six reduced sums
    __shared__ uint32_t s_wj[kBatch];  // written entries' slots

    const size_t N = (size_t)a.W * a.H;
    float T[4], gB[4], U[4][kCh];
    int nc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {  // (an outside pixel reads a clamped, valid address and is zeroed)
        const int px = tile_x0 + (q & 1) * 8 + lx, py = tile_y0 + (q >> 1) * 8 + ly;
        const bool in = px < a.W && py < a.H;
        const size_t pix = (size_t)min(py, a.H - 1) * a.W + min(px, a.W - 1);
        const uint32_t c = a.n_contrib[tile_px(tile, q, lane)];
        nc[q] = in ? (int)c : 0;
        T[q] = 1.f;
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < kCh; k++) {
            const size_t at = (size_t)(c0 + min(k, nch - 1)) * N + pix;
            const float u = a.dL_dfmap[at];
            U[q][k] = in && k < nch ? u : 0.f;
            if (GEOM) dot += U[q][k] * a.fmap[at];
        }
        // dL/dFmap . (what the forward accumulated), no background term: shrinks to "strictly behind this entry"
        // as the walk proceeds
        gB[q] = dot;
    }
    const TileWalk tw = tile_walk(a, tile, nc);
    const int limit = tw.limit;
    uint32_t live = 0;
    int next_lim = limit;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (tw.slim[q] > 0) {
            live |= 1u << q;
            next_lim = min(next_lim, tw.slim[q]);
        }
    const int k16 = reduced_index16(lane), k8 = reduced_index8(lane);
    uint32_t ent_next = lane < limit ? a.gid_sorted[tw.range.x + lane] : 0u;
    for (int b0 = 0; b0 < limit; b0 += kBatch) {
        const bool has = b0 + lane < limit;
        const uint32_t ent = ent_next;
        if (b0 + kBatch + lane < limit) ent_next = a.gid_sorted[tw.range.x + b0 + kBatch + lane];
        float4 raw = make_float4(0.f, 0.f, 0.f, 0.f);
        const uint32_t qm = stage_batch(a, ent, has, lane, c0, nch, s_xy, s_cq, s_gid, s_f, GEOM ? &raw : nullptr);
        unsigned long long todo = __ballot(qm != 0);
        unsigned long long written = 0;
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int pos = b0 + j;
            const float4 xy = s_xy[j], cq = s_cq[j];
            if (pos >= next_lim) {
                next_lim = limit;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (pos >= tw.slim[q]) live &= ~(1u << q);
                    else next_lim = min(next_lim, tw.slim[q]);
                }
            }
            const uint32_t m = uniform_u32(__float_as_uint(cq.w)) & live;
            if (m == 0) continue;
            float f[kCh], df[kCh], r[8];
#pragma unroll
            for (int k4 = 0; k4 < kCh / 4; k4++) {
                const float4 v = reinterpret_cast<const float4*>(s_f)[j * (kCh / 4) + k4];
                f[4 * k4] = v.x; f[4 * k4 + 1] = v.y; f[4 * k4 + 2] = v.z; f[4 * k4 + 3] = v.w;
            }
#pragma unroll
            for (int k = 0; k < kCh; k++) df[k] = 0.f;
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
#pragma unroll
                for (int k = 0; k < kCh; k++) df[k] = fmaf(w, U[q][k], df[k]);
                const float one_m_a = 1.f - alpha;
                if (GEOM) {  // render_bwd's per-pixel terms with s in place of dL/dpix . colour
                    float sdot = 0.f;
#pragma unroll
                    for (int k = 0; k < kCh; k++) sdot = fmaf(U[q][k], f[k], sdot);
                    gB[q] -= w * sdot;
                    const float dLda = T[q] * sdot - gB[q] * __builtin_amdgcn_rcpf(one_m_a);
                    const float u = on ? dLda * G : 0.f;
                    const float udx = u * dx, udy = u * dy;
                    r[0] += udx;
                    r[1] += udy;
                    r[2] += udx * dx;
                    r[3] += udx * dy;
                    r[4] += udy * dy;
                    r[5] += u;
                }
                T[q] *= one_m_a;  // alpha = 0 leaves T unchanged
            }
            if (contrib) {  // uniform
                const float d = reduce16(df, lane);
                if ((lane & 3) == 0) s_df[j * kCh + k16] = d;
                if (GEOM) {
                    const float g = reduce8(r, lane);
                    if ((lane & 7) == 0) s_geo[j * 8 + k8] = g;
                }
                written |= 1ull << j;
            }
        }
        unit_sync();
        if (has && ((written >> lane) & 1ull)) {  // this entry's place in the list of written entries
            s_wj[__popcll(written & ((1ull << lane) - 1ull))] = (uint32_t)lane;
            if (GEOM) {
                // the sums in their final form (render_bwd's flush): dL/dmean2D in NDC units, dL/dopacity_eff,
                // dL/dconic with the reference's -0.5 factors, in the order of accumulator row floats 4..9
                const float4 B = reinterpret_cast<const float4*>(s_geo)[lane * 2];
                const float s8 = s_geo[lane * 8 + 4], s9 = s_geo[lane * 8 + 5];
                const float ca = raw.x, cb = raw.y, cc = raw.z, o = raw.w;
                reinterpret_cast<float4*>(s_geo)[lane * 2] =
                    make_float4(-0.5f * (float)a.W * o * (ca * B.x + cb * B.y),
                                -0.5f * (float)a.H * o * (cc * B.y + cb * B.x), s9, -0.5f * o * B.w);
                s_geo[lane * 8 + 4] = -0.5f * o * B.z;
                s_geo[lane * 8 + 5] = -0.5f * o * s8;
                const uint32_t e = ent >> kEntryMaskBits;
                (void)atomicOr(a.touched + (e >> 5), 1u << (e & 31u));  // OR is order-free
            }
        }
        unit_sync();
        // one wave instruction per four listed entries: lane 16 k + v adds value v of listed entry k
        const int nw = __popcll(written), sub = lane >> 4, v = lane & 15;
        for (int k0 = 0; k0 < nw; k0 += 4) {  // uniform
            const int k = k0 + sub;
            if (k < nw) {
                const int j = (int)s_wj[k];
                const uint32_t g = s_gid[j];
                // (no value returned: fire and forget)
                if (v < nch) (void)atomicAdd(a.dL_dfeatures + (size_t)g * a.C + c0 + v, s_df[j * kCh + v]);
                if (GEOM && v < 6) (void)atomicAdd(a.acc + (size_t)g * (4 * kAccRow4) + 4 + v, s_geo[j * 8 + v]);
            }
        }
        unit_sync();
    }
}

static bool features_grid(const FeatureArgs& a, dim3* grid) {
    const uint32_t tiles = a.gx * a.gy;
    const uint32_t chunks = (uint32_t)((a.C + kCh - 1) / kCh);
    if (tiles == 0 || chunks == 0 || chunks > 65535u) return false;
    *grid = dim3(tiles, chunks);
    return true;
}

hipError_t launch_features_fwd(const FeatureArgs& a, hipStream_t stream) {
    dim3 grid;
    if (!features_grid(a, &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(features_fwd_kernel, grid, dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_features_bwd(const FeatureArgs& a, hipStream_t stream) {
    dim3 grid;
    if (!features_grid(a, &grid)) return hipErrorInvalidValue;
    if (a.acc && a.touched)
        hipLaunchKernelGGL((features_bwd_kernel<true>), grid, dim3(kWave), 0, stream, a);
    else
        hipLaunchKernelGGL((features_bwd_kernel<false>), grid, dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

}  // namespace gsr
