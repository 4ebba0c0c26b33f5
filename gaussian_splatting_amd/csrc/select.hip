// select.hip -- per-pixel SELECTIONS from a finished forward's blend weights: the median contributor (the one at which
// the transmittance crosses one half) with a per-Gaussian scalar t copied from it, and the K contributors of largest
// weight (include/gsr.h gsr_render_select / gsr_render_median_backward).
//
// The walk is distortion.hip's: one wave64 per tile walks the tile's WHOLE list from its head, entries staged 64 at a
// time into LDS with each entry's t beside its conic and its Gaussian index beside both, only entries with a non-zero
// blend mask walked and only the quadrants whose bit is set evaluated, alpha and T recomputed in the forward's order
// with the exponent spelled as contrib.hip spells it, each pixel stopped at its n_contrib.  Every weight therefore
// depends on the forward's discrete state alone, and so does every selection.
//
// Per quadrant slot a lane keeps in registers T, the median's Gaussian and t (overwritten while T > 0.5 before T is
// multiplied: the last contributor with T > 0.5 stays), and KMAX (weight, Gaussian) pairs sorted by descending weight.
// A new weight goes behind every kept weight >= it (a later entry displaces only on strict >, so equal weights keep
// list order), by compare-selects over statically indexed registers; an entry that beats no lane's K-th weight is
// skipped by the whole wave.  Every pixel of the image is written once by the one wave that owns it, with plain vector
// stores: no atomics, bitwise reproducible.
//
// median_bwd_kernel scatters the upstream gradient of the median map into dL_dt[median_ids[pix]], one thread per pixel
// with a no-return float atomic: the map is a copy of t, piecewise constant in the weights.
//
// The helpers restate distortion.hip's (private to their translation units); this file is built with render.hip's
// flags so that the exponent and alpha round as they do there.
#include "kernels.h"

namespace gsr {
namespace {

constexpr int kBatch = 64;  // list entries staged per round (one per lane)
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// (A, B, C, quads): the staged conic of render.hip stage_conic
__device__ __forceinline__ float4 stage_conic(float4 v0, float4 v1, uint32_t qm) {
    return make_float4(-0.5f * kLog2e * v0.z, -kLog2e * v0.w, -0.5f * kLog2e * v1.x, __uint_as_float(qm));
}

__device__ __forceinline__ void unit_sync() { wave_lds_sync(); }

// distortion.hip's TileWalk / tile_walk / retire
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
__device__ __forceinline__ void retire(TileWalk& t, int pos) {
    if (pos < t.next_lim) return;
    t.next_lim = t.limit;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (pos >= t.slim[q]) t.live &= ~(1u << q);
        else t.next_lim = min(t.next_lim, t.slim[q]);
    }
}

// One batch's entries into LDS: position, opacity and t (0 without MEDIAN: t may be null), the staged conic and the
// Gaussian index of lane's entry.  Returns the lane's entry's blend mask (0: not walked, nothing staged).
template <bool MEDIAN>
__device__ __forceinline__ uint32_t stage_batch(const FeatureArgs& a, uint32_t ent, bool has, int lane, float4* s_xy,
                                                float4* s_cq, int* s_gid) {
    uint32_t qm = 0;
    if (has) {
        const uint32_t e = ent >> kEntryMaskBits;
        if ((ent & kEntryMask) && e < a.n_gauss) {  // (an entry no pixel blended is not walked)
            const float4* rec = a.rec + (size_t)kRecRows * e;
            const float4 v0 = rec[0], v1 = rec[1];
            s_xy[lane] = make_float4(v0.x, v0.y, v1.y, MEDIAN ? a.features[e] : 0.f);
            qm = ent & kEntryMask;
            s_cq[lane] = stage_conic(v0, v1, qm);
            s_gid[lane] = (int)e;
        }
    }
    unit_sync();
    return qm;
}

// The KMAX kept (weight, Gaussian) pairs of one pixel, descending; w goes behind every kept weight >= w.
template <int KMAX>
__device__ __forceinline__ void topk_insert(float (&wk)[KMAX > 0 ? KMAX : 1], int (&ik)[KMAX > 0 ? KMAX : 1], float w,
                                            int g) {
    bool ge[KMAX > 0 ? KMAX : 1];
#pragma unroll
    for (int k = 0; k < KMAX; k++) ge[k] = wk[k] >= w;  // (a prefix of trues: the array is sorted)
#pragma unroll
    for (int k = KMAX - 1; k >= 0; k--) {
        const bool here = k == 0 || ge[k - 1];  // with !ge[k]: the new pair's rank
        const float wp = k > 0 ? wk[k - 1] : 0.f;
        const int ip = k > 0 ? ik[k - 1] : -1;
        wk[k] = ge[k] ? wk[k] : here ? w : wp;
        ik[k] = ge[k] ? ik[k] : here ? g : ip;
    }
}

}  // namespace

// KMAX: pairs kept per pixel (the first a.K planes are written); MEDIAN: the median outputs, and t is read.
template <int KMAX, bool MEDIAN>
__global__ void __launch_bounds__(64) select_fwd_kernel(SelectArgs sa) {
    const FeatureArgs& a = sa.walk;
    constexpr int KR = KMAX > 0 ? KMAX : 1;
    const uint32_t tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int tile_x0 = (int)(tile % a.gx) * kTile, tile_y0 = (int)(tile / a.gx) * kTile;
    const int lx = lane & 7, ly = lane >> 3;
    const float pxf0 = (float)(tile_x0 + lx), pyf0 = (float)(tile_y0 + ly);  // this lane's pixel in quadrant 0

    __shared__ float4 s_xy[kBatch], s_cq[kBatch];  // (x, y, opacity, t), (A, B, C, quads)
    __shared__ int s_gid[kBatch];

    float T[4], mt[4], wk[4][KR];
    int mi[4], ik[4][KR], nc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int px = tile_x0 + (q & 1) * 8 + lx, py = tile_y0 + (q >> 1) * 8 + ly;
        const uint32_t c = a.n_contrib[tile_px(tile, q, lane)];
        nc[q] = px < a.W && py < a.H ? (int)c : 0;
        T[q] = 1.f;
        mt[q] = 0.f;
        mi[q] = -1;
#pragma unroll
        for (int k = 0; k < KR; k++) {
            wk[q][k] = 0.f;
            ik[q][k] = -1;
        }
    }
    TileWalk tw = tile_walk(a, tile, nc);
    const int limit = tw.limit;
    uint32_t ent_next = lane < limit ? a.gid_sorted[tw.range.x + lane] : 0u;  // the next batch's entry
    for (int b0 = 0; b0 < limit; b0 += kBatch) {
        const bool has = b0 + lane < limit;
        const uint32_t ent = ent_next;
        if (b0 + kBatch + lane < limit) ent_next = a.gid_sorted[tw.range.x + b0 + kBatch + lane];
        const uint32_t qm = stage_batch<MEDIAN>(a, ent, has, lane, s_xy, s_cq, s_gid);
        unsigned long long todo = __ballot(qm != 0);
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int pos = b0 + j;
            const float4 xy = s_xy[j], cq = s_cq[j];
            const int g = s_gid[j];
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
                if constexpr (MEDIAN) {
                    const bool front = on && T[q] > 0.5f;  // (before T is multiplied: 2DGS's rule)
                    mi[q] = front ? g : mi[q];
                    mt[q] = front ? xy.w : mt[q];
                }
                if constexpr (KMAX > 0) {
                    const float w = alpha * T[q];
                    // (a lane whose w does not beat its K-th weight keeps its pairs; so does a whole wave of them)
                    if (__ballot(on && w > wk[q][KR - 1])) topk_insert<KMAX>(wk[q], ik[q], on ? w : 0.f, g);
                }
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
            if constexpr (MEDIAN) {
                sa.out_median[pix] = mt[q];
                sa.out_median_ids[pix] = mi[q];
            }
#pragma unroll
            for (int k = 0; k < KMAX; k++)
                if (k < sa.K) {  // uniform
                    sa.out_topk_ids[(size_t)k * N + pix] = ik[q][k];
                    sa.out_topk_weights[(size_t)k * N + pix] = wk[q][k];
                }
        }
    }
}

// One thread per pixel: dL_dt[median_ids[pix]] += U[pix] (dL_dt zeroed by the launcher; the hardware's order).
__global__ void __launch_bounds__(256) median_bwd_kernel(int P, size_t N, const int* __restrict__ ids,
                                                         const float* __restrict__ U, float* dL_dt) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= N) return;
    const int g = ids[pix];
    if (g >= 0 && g < P) (void)atomicAdd(dL_dt + g, U[pix]);  // no value returned: fire and forget
}

template <int KMAX>
static hipError_t launch_select(const SelectArgs& a, uint32_t tiles, hipStream_t stream) {
    if (a.out_median)
        hipLaunchKernelGGL((select_fwd_kernel<KMAX, true>), dim3(tiles), dim3(kWave), 0, stream, a);
    else
        hipLaunchKernelGGL((select_fwd_kernel<KMAX, false>), dim3(tiles), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_select_fwd(const SelectArgs& a, hipStream_t stream) {
    const uint32_t tiles = a.walk.gx * a.walk.gy;
    if (tiles == 0 || a.K < 0 || a.K > kSelectMaxK || (a.K == 0 && !a.out_median)) return hipErrorInvalidValue;
    if (a.K == 0) return launch_select<0>(a, tiles, stream);
    if (a.K == 1) return launch_select<1>(a, tiles, stream);
    if (a.K == 2) return launch_select<2>(a, tiles, stream);
    if (a.K <= 4) return launch_select<4>(a, tiles, stream);
    return launch_select<8>(a, tiles, stream);
}

hipError_t launch_median_bwd(int P, int W, int H, const int* median_ids, const float* dL_dmedian, float* dL_dt,
                             hipStream_t stream) {
    const size_t N = (size_t)W * H;
    if (N == 0 || P <= 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(dL_dt, 0, sizeof(float) * (size_t)P, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(median_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, P, N, median_ids,
                       dL_dmedian, dL_dt);
    return hipGetLastError();
}

}  // namespace gsr
