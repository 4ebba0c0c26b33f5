// contrib.hip -- per-Gaussian contribution statistics of a finished forward (include/gsr.h gsr_contrib_stats):
// for every Gaussian the sum, the maximum and the number of the blend weights w = alpha * T the forward used,
// and optionally their sum weighted by a per-pixel map.
//
// A pass of its own over what the forward left for its backward, read-only: one wave64 per unit (tile, segment)
// of the backward's work list, started from the unit's blend checkpoint (its T plane alone; or, see CKPT below, from
// the head of the tile's list with a walk for T alone up to the unit's start), entries staged 64 at
// a time into LDS, only entries with a non-zero blend mask walked and only the quadrants whose bit is set
// evaluated, alpha and T recomputed in the forward's order, each pixel stopped at its n_contrib -- the walk of
// render.hip's render_bwd with the gradient arithmetic taken out.  The (pixel, entry) pairs that contribute are
// exactly those render_bwd forms a gradient term for.
//
// Per entry the wave reduces its pixels' weights (two lane-swap halvings and DPP row sums for the two sums, a DPP
// max, a scalar population count for the pixel count) into one 16-byte LDS row; after a batch the written rows
// are compacted and flushed into the Gaussians' output rows with no-return atomics, SIXTEEN entries per wave
// instruction (lane 4 k + v handles value v of listed entry k): float add for the sums, unsigned max on the bits
// of the maximum (w > 0 orders as its bit pattern), unsigned add for the count.  The summation order of the two
// sums over a Gaussian's tile instances follows the hardware; the maximum and the count do not depend on it.
//
// The helpers below restate render.hip's (which keeps them private to its translation unit); this file is built
// with render.hip's flags so that the exponent and alpha round as they do there.
#include "kernels.h"

#include <algorithm>

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

}  // namespace

// WEIGHTED: a per-pixel weight map is loaded in the prologue and a fourth value, sum w m(pix), is formed; the
// launcher picks the instantiation by the pointer (the project's rule for nullable prologue loads).
// STRIDED: as render_bwd's (a block takes units i, i + G, ...).
// CKPT: the unit starts from the forward's blend checkpoint (ContribArgs::ckpt non-null).  That is exact only when the
// checkpoint's T was formed with this kernel's arithmetic, i.e. by the half-tile / quadrant forward, whose exponent the
// compiler contracts as spelled out below; the whole-tile forward ("fwd_quads" 4) is compiled to another contraction
// of the same source line, so its T differs in the last bits.  Without CKPT (the launcher picks by the pointer; api.hip
// passes null unless it knows the buffers' forward was a half-tile one) the unit first re-walks the entries
// [0, start) of its tile, updating T alone -- no sums, no flush -- so every weight depends only on the forward's
// discrete state (list order, blend masks, n_contrib) and weight_max / pixel_count are the same bits whichever
// forward kernel, segment length or grid ran.  After a half-tile forward both forms give the same bits.
template <bool STRIDED, bool WEIGHTED, bool CKPT>
__global__ void __launch_bounds__(64) contrib_stats_kernel(ContribArgs a) {
    static_assert(kUnitLists * kUnitShards <= kWave, "one lane per list counter");
    constexpr int nl = kUnitLists * kUnitShards;
    const uint32_t incl = wave_incl_sum(threadIdx.x < nl ? a.unit_cnt[threadIdx.x * kUnitCntStride] : 0u);
    const uint32_t tiles = a.gx * a.gy;
    for (uint32_t i = blockIdx.x;; i += gridDim.x) {
        uint2 unit;
        {  // the list holding unit i (render_bwd's lookup)
            const int lane = threadIdx.x;
            const int l = __popcll(__ballot(lane < nl && incl <= i));
            if (l >= nl) return;  // past the lists (the grid is sized for the worst case)
            const uint32_t before = l ? (uint32_t)__builtin_amdgcn_readlane((int)incl, l - 1) : 0u;
            const uint32_t k = i - before;
            if (l < kUnitShards)
                unit = a.unit_full[(size_t)l * a.full_cap + k];
            else
                unit = a.unit_part[(size_t)(l - kUnitShards) * unit_part_cap(tiles) + k];
        }
        const uint32_t tile = unit.x;
        const int start = (int)unit.y * kCkStride;
        int lane_o = threadIdx.x;
        if (STRIDED) asm volatile("" : "+v"(lane_o));  // (as render_bwd: lane constants formed per unit)
        const int lane = lane_o;
        // (a work list that is not this forward's -- foreign buffers -- must not send the walk out of bounds)
        const uint2 range = tile < tiles ? a.ranges[tile] : make_uint2(0u, 0u);
        const int n = (int)(range.y - range.x);
        if (start < n) {
            const int tile_x0 = (int)(tile % a.gx) * kTile, tile_y0 = (int)(tile / a.gx) * kTile;
            const int lx = lane & 7, ly = lane >> 3;
            const float pxf0 = (float)(tile_x0 + lx), pyf0 = (float)(tile_y0 + ly);  // this lane's pixel in quadrant 0

            __shared__ float4 s_xy[kBatch], s_cq[kBatch];  // (x, y, opacity, -), (A, B, C, quads)
            __shared__ uint32_t s_acc[kBatch][4];          // per entry: sum, max, count, weighted sum (bits)
            __shared__ uint32_t s_wgid[kBatch], s_wj[kBatch];  // written entries' Gaussian, slot

            float T[4], pm[4];
            int nc[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {  // (an outside pixel reads a clamped, valid address and is zeroed)
                const int px = tile_x0 + (q & 1) * 8 + lx, py = tile_y0 + (q >> 1) * 8 + ly;
                const bool in = px < a.W && py < a.H;
                const size_t pix = (size_t)min(py, a.H - 1) * a.W + min(px, a.W - 1);
                const uint32_t c = a.n_contrib[tile_px(tile, q, lane)];
                pm[q] = WEIGHTED ? a.pixel_weight[pix] : 0.f;
                if (CKPT) {  // blend state at `start`: the forward's checkpoint (gsr_common.h), or the empty state
                    const float* ck = a.ckpt + (size_t)((range.x + (uint32_t)start) / kCkStride) * kCkFloats + lane;
                    T[q] = start > 0 ? ck[q * 64] : 1.f;
                } else {
                    T[q] = 1.f;  // the walk below starts at the head of the list
                }
                nc[q] = in ? (int)c : 0;
            }
            int slim[4];
#pragma unroll
            for (int q = 0; q < 4; q++)
                slim[q] = __builtin_amdgcn_readlane((int)wave_incl_max((uint32_t)nc[q]), 63);  // DPP max over the wave
            const int limit = min(n, max(max(slim[0], slim[1]), max(slim[2], slim[3])));
            const int end = min(limit, start + (int)uniform_u32(*a.seg_ck) * kCkStride);  // the forward's segments
            uint32_t live = 0;     // slots still reachable at the current position (uniform)
            int next_lim = limit;  // smallest slot limit among live slots
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (slim[q] > start) {
                    live |= 1u << q;
                    next_lim = min(next_lim, slim[q]);
                }
            // where this lane's part of an entry's reduced row lands: lane 0 the sum, lane 63 the maximum, lane 1
            // the count, lane 32 the weighted sum
            const bool acc_wr = lane == 0 || lane == 1 || lane == 32 || lane == 63;
            const int acc_off = lane == 0 ? 0 : lane == 63 ? 1 : lane == 1 ? 2 : 3;

            const int first = CKPT ? start : 0;  // (start is a multiple of the batch: a batch is wholly before it or not)
            uint32_t ent_next = first + lane < end ? a.gid_sorted[range.x + first + lane] : 0u;  // the next batch's entry
            for (int b0 = first; b0 < end; b0 += kBatch) {
                const bool pre = !CKPT && b0 < start;  // uniform: a batch walked for T alone
                const bool has = b0 + lane < end;
                uint32_t qm = 0, e = 0;
                if (has) {
                    const uint32_t ent = ent_next;  // Gaussian << 4 | blend mask
                    e = ent >> kEntryMaskBits;
                    if ((ent & kEntryMask) && e < a.n_gauss) {  // (an entry no pixel blended is not walked)
                        const float4* rec = a.rec + (size_t)kRecRows * e;
                        const float4 v0 = rec[0], v1 = rec[1];
                        s_xy[lane] = make_float4(v0.x, v0.y, v1.y, 0.f);
                        qm = ent & kEntryMask;
                        s_cq[lane] = stage_conic(v0, v1, qm);
                    }
                }
                if (b0 + kBatch + lane < end) ent_next = a.gid_sorted[range.x + b0 + kBatch + lane];
                unit_sync();
                unsigned long long todo = __ballot(qm != 0);
                unsigned long long written = 0;
                while (todo) {
                    const int j = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const int pos = b0 + j;
                    const float4 xy = s_xy[j], cq = s_cq[j];
                    if (pos >= next_lim) {  // uniform: retire the slots whose last contributor has passed
                        next_lim = limit;
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            if (pos >= slim[q]) live &= ~(1u << q);
                            else next_lim = min(next_lim, slim[q]);
                        }
                    }
                    const uint32_t m = uniform_u32(__float_as_uint(cq.w)) & live;
                    if (m == 0) continue;
                    float s = 0.f, mx = 0.f, sw = 0.f;
                    uint32_t cnt = 0;  // uniform
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if (!(m & (1u << q))) continue;  // uniform
                        const float dx = xy.x - (pxf0 + (float)((q & 1) * 8)), dy = xy.y - (pyf0 + (float)((q >> 1) * 8));
                        // render_fwd's exponent dx (A dx + B dy) + C dy^2 with the two fused multiply-adds spelled out
                        // as the compiler forms them there, so alpha, and with it T, is the forward's bit for bit
                        const float p2 = fmaf(dx, fmaf(dx, cq.x, cq.y * dy), (cq.z * dy) * dy);
                        // the forward's skip tests and "the forward stopped this pixel before `pos`" as one mask
                        const float G = __builtin_amdgcn_exp2f(p2);
                        const float ac = fminf(0.99f, xy.z * G);
                        const bool on = (p2 <= 0.f) & (ac >= 1.0f / 255.0f) & (pos < nc[q]);
                        const unsigned long long onb = __ballot(on);
                        if (!onb) continue;  // uniform
                        cnt += (uint32_t)__popcll(onb);
                        const float alpha = on ? ac : 0.f;
                        const float w = alpha * T[q];
                        s += w;
                        mx = fmaxf(mx, w);
                        if (WEIGHTED) sw += w * pm[q];
                        T[q] *= 1.f - alpha;  // alpha = 0 leaves T unchanged
                    }
                    if (cnt && !pre) {  // uniform
                        // the two sums: lanes 0-31 of h hold s, lanes 32-63 sw; rows 0 + 1 -> row 0, rows 2 + 3 ->
                        // row 2; then each 16-lane row's total in all its lanes
                        const float h = half_fold(s, sw);
                        const float f = row_allsum(row_fold(h, h));
                        const uint32_t mxb = wave_incl_max(__float_as_uint(mx));  // lane 63 (w >= 0: bits order as floats)
                        if (acc_wr) s_acc[j][acc_off] = lane == 63 ? mxb : lane == 1 ? cnt : __float_as_uint(f);
                        written |= 1ull << j;
                    }
                }
                unit_sync();
                if (pre) continue;  // uniform (nothing written: no flush)
                if (has && ((written >> lane) & 1ull)) {  // this entry's place in the list of written entries
                    const int slot = __popcll(written & ((1ull << lane) - 1ull));
                    s_wgid[slot] = e;
                    s_wj[slot] = (uint32_t)lane;
                }
                unit_sync();
                // one wave instruction per sixteen listed entries and kind of atomic: lane 4 k + v, value v of entry k
                const int nw = __popcll(written), sub = lane >> 2, v = lane & 3;
                for (int k0 = 0; k0 < nw; k0 += 16) {  // uniform
                    const int k = k0 + sub;
                    if (k < nw) {
                        const uint32_t bits = s_acc[s_wj[k]][v];
                        uint32_t* dst = reinterpret_cast<uint32_t*>(a.stats) + (size_t)s_wgid[k] * 4 + v;
                        // (no value returned: fire and forget)
                        if (v == 1) (void)atomicMax(dst, bits);
                        else if (v == 2) (void)atomicAdd(dst, bits);
                        else if (v == 0 || WEIGHTED) (void)atomicAdd(reinterpret_cast<float*>(dst), __uint_as_float(bits));
                    }
                }
                unit_sync();
            }
        }
        if (!STRIDED) break;  // one unit per block
    }
}

constexpr uint32_t kContribGridTiles = 2, kContribStrideRatio = 4;  // render.hip kBwdGridTiles / kBwdStrideRatio
hipError_t launch_contrib_stats(const ContribArgs& a, size_t max_units, hipStream_t stream, int grid_mode) {
    if (max_units == 0) return hipSuccess;
    const size_t strided_units = std::min(max_units, (size_t)kContribGridTiles * a.gx * a.gy);
    const bool strided = grid_mode == 2 || (grid_mode == 0 && max_units > kContribStrideRatio * strided_units);
    const uint32_t grid = (uint32_t)(strided ? strided_units : max_units);
#define GSR_CONTRIB_LAUNCH(S, W, C) \
    hipLaunchKernelGGL((contrib_stats_kernel<S, W, C>), dim3(grid), dim3(kWave), 0, stream, a)
    const int variant = (strided ? 4 : 0) | (a.pixel_weight ? 2 : 0) | (a.ckpt ? 1 : 0);
    switch (variant) {
        case 0: GSR_CONTRIB_LAUNCH(false, false, false); break;
        case 1: GSR_CONTRIB_LAUNCH(false, false, true); break;
        case 2: GSR_CONTRIB_LAUNCH(false, true, false); break;
        case 3: GSR_CONTRIB_LAUNCH(false, true, true); break;
        case 4: GSR_CONTRIB_LAUNCH(true, false, false); break;
        case 5: GSR_CONTRIB_LAUNCH(true, false, true); break;
        case 6: GSR_CONTRIB_LAUNCH(true, true, false); break;
        default: GSR_CONTRIB_LAUNCH(true, true, true); break;
    }
#undef GSR_CONTRIB_LAUNCH
    return hipGetLastError();
}

}  // namespace gsr
