// views.hip -- the multi-GPU view exchange (distributed.py ViewExchange; include/gsr.h): filling a view block
// from a screen-space backward, packing, unpacking and indexing sparse view blocks, the live list of the
// Gaussians some view flags, and the per-Gaussian backward over several views' gathered sums.  The kernels
// come first, the C entry points are at the end of the file.
// Compiled with backward.hip's per-file flags (build.py FILE_FLAGS): view_backward (gauss_bwd_math.h) must
// round here as it does there.
#include "gauss_bwd_math.h"
#include "host.h"

namespace gsr {

// multi-view backward over gathered view blocks (section 2)
struct ViewsBwdArgs {
    int P, D, M;
    const float* means3D;
    const float* shs;
    const float* dc;
    const float* opacities;
    const float* scales;
    const float* rotations;
    float scale_modifier;
    int n_views;
    const float* blocks;  // [n_views][block_floats]: view blocks, or packed blocks when `flags` is set
    size_t block_floats;
    // Packed mode (gsr_view_block_index): the flag word of Gaussian g in view v is flags[v * P + g],
    // its entry index in view v's packed block << 4 | the block's flag bits; the sums are read from
    // that packed entry, the camera from the packed block's header.  Null: dense view blocks.
    const uint32_t* flags;
    // with flags: the live list of Gaussians some view flags (launch_views_live), or null; with it
    // the kernel runs a lane per listed Gaussian and the outputs must be zero beforehand
    const uint32_t* live;
    const uint32_t* live_count;
    uint32_t live_cap;
    float* dL_dmean3D;
    float* dL_dsh;
    float* dL_ddc;
    float* dL_dopacity;
    float* dL_dscale;
    float* dL_drot;
};

// ---- 1. a view block from a screen-space backward ---------------------------------
// The atomic backward into a view block (gsr_backward_args.view_block, multi-GPU view exchange): one lane
// per Gaussian writes its dense sums -- its accumulator row if its touched bit is set (the row then zeroed),
// zeros otherwise -- and its flag word, as gauss_reduce does for a view block; the words it read are cleared.
__global__ void __launch_bounds__(64) gauss_live_views_kernel(int P, uint32_t* __restrict__ touched,
                                                              float4* __restrict__ acc, const int* __restrict__ radii,
                                                              const uint8_t* __restrict__ clamped, GradRecs sums,
                                                              uint32_t* __restrict__ flags) {
    const int lane = threadIdx.x;
    const uint32_t g = blockIdx.x * 64u + (uint32_t)lane;
    if (g >= (uint32_t)P) return;
    const uint32_t w = touched[g >> 5];
    const bool lv = (w >> (g & 31u)) & 1u;
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra;
    float4* row = acc + (size_t)g * kAccRow4;
    if (lv) {
        ra = row[0];
        rb = row[1];
        rc = row[2];
    }
    const int rad = radii[g];
    const uint8_t cm = clamped[g];
    sums.a[g] = ra;
    sums.b[g] = rb;
    sums.c[g] = make_float2(rc.x, rc.y);
    flags[g] = (rad > 0 ? 1u : 0u) | ((uint32_t)(cm & 7u) << 1);
    if (lv) row[0] = row[1] = row[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((lane & 31) == 0 && w) touched[g >> 5] = 0u;  // (after every lane's read: the stores depend on w)
}

hipError_t launch_gauss_live_views(int P, uint32_t* touched, float4* acc, const int* radii, const uint8_t* clamped,
                                   const GradRecs& sums, uint32_t* flags, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(gauss_live_views_kernel, dim3((uint32_t)(((size_t)P + 63) / 64)), dim3(64), 0, stream, P, touched,
                       acc, radii, clamped, sums, flags);
    return hipGetLastError();
}

// ---- 2. the per-Gaussian backward over several views' summed render gradients ---
// Multi-GPU (distributed.py ViewExchange): every rank all-gathers the
// other ranks' per-Gaussian render-gradient sums (a "view block": camera header, 10 floats
// and a flag word per Gaussian, kViewBlock* in gsr_common.h) instead of all-reducing the
// 59-float parameter gradients, and runs this kernel once: one lane per Gaussian loops over
// the views, evaluates view_backward for each view in which the Gaussian is visible, and
// sums the parameter gradients in registers.  Every rank runs it on the same gathered bytes,
// so the replicas' gradients are bitwise identical.
// Phase 1 reads the staged (or global) SH rows for the view-direction gradient and drops
// the per-coefficient products; phase 2 forms dL/dSH_k = sum over views of B_k(dir_v) g_v
// one SH band at a time (bands are compile-time, so the band's accumulators stay in
// registers), recomputing dir_v and g_v from the view blocks -- dL/dSH does not depend on
// the SH values, so the 48 accumulators of all coefficients are never live at once.
template <bool LDS>
struct ShReadOnly {
    const float* lds_row;  // staged row (LDS variants)
    ShAddr src;            // global rows otherwise
    int idx;
    __device__ __forceinline__ float3 load(int k) const {
        if constexpr (LDS) return make_float3(lds_row[3 * k], lds_row[3 * k + 1], lds_row[3 * k + 2]);
        const float* c = src.coef(idx, k);
        return make_float3(c[0], c[1], c[2]);
    }
    __device__ __forceinline__ void store(int, float3) const {}
};
// A view's flag word and summed render gradients for Gaussian idx: from a dense view block, or
// (packed mode, a.flags set) the flag array and the packed entry it indexes (entry layout:
// index bits, a.xyz | a.w, b.xyz | b.w, c.xy, flag bits -- view_pack_scatter_kernel).
template <bool PACKED>
__device__ __forceinline__ uint32_t view_flag(const ViewsBwdArgs& a, const float* blk, int v, int idx) {
    if constexpr (PACKED) return a.flags[(size_t)v * a.P + idx];
    return reinterpret_cast<const uint32_t*>(blk + kViewBlockHeader + 10 * (size_t)a.P)[idx];
}
template <bool PACKED>
__device__ __forceinline__ void view_sums(const ViewsBwdArgs& a, const float* blk, uint32_t flags, int idx,
                                          float4& sa, float4& sb, float2& sc) {
    if constexpr (PACKED) {
        const float4* e = reinterpret_cast<const float4*>(blk + kViewBlockHeader + (size_t)kViewPackEntry * (flags >> 4));
        const float4 e0 = e[0], e1 = e[1], e2 = e[2];
        sa = make_float4(e0.y, e0.z, e0.w, e1.x);
        sb = make_float4(e1.y, e1.z, e1.w, e2.x);
        sc = make_float2(e2.y, e2.z);
    } else {
        const float* sums = blk + kViewBlockHeader;
        sa = reinterpret_cast<const float4*>(sums)[idx];
        sb = reinterpret_cast<const float4*>(sums + 4 * (size_t)a.P)[idx];
        sc = reinterpret_cast<const float2*>(sums + 8 * (size_t)a.P)[idx];
    }
}
template <bool PACKED>
__device__ __forceinline__ float4 view_sums_a(const ViewsBwdArgs& a, const float* blk, uint32_t flags, int idx) {
    if constexpr (PACKED) {
        const float4* e = reinterpret_cast<const float4*>(blk + kViewBlockHeader + (size_t)kViewPackEntry * (flags >> 4));
        const float4 e0 = e[0], e1 = e[1];
        return make_float4(e0.y, e0.z, e0.w, e1.x);
    }
    return reinterpret_cast<const float4*>(blk + kViewBlockHeader)[idx];
}

template <int K0, int K1>
struct ShBand {  // accumulates B_k g for K0 <= k < K1; SH values are not needed (read as 0)
    float* acc;
    __device__ __forceinline__ float3 load(int) const { return make_float3(0.f, 0.f, 0.f); }
    __device__ __forceinline__ void store(int k, float3 v) const {
        if (k >= K0 && k < K1) {
            acc[3 * (k - K0)] += v.x;
            acc[3 * (k - K0) + 1] += v.y;
            acc[3 * (k - K0) + 2] += v.z;
        }
    }
};

// dL/dSH of band [K0, K1) for lane idx, summed over the views it is visible in; written to
// the lane's LDS row (LDS variants) or straight to global memory
template <int K0, int K1, int SH_MODE, bool PACKED>
__device__ __forceinline__ void views_sh_band(const ViewsBwdArgs& a, int idx, float3 mean, float* row,
                                              const ShGradAddr& dst) {
    float acc[3 * (K1 - K0)];
#pragma unroll
    for (int i = 0; i < 3 * (K1 - K0); i++) acc[i] = 0.f;
#pragma unroll 1
    for (int v = 0; v < a.n_views; v++) {
        const float* blk = a.blocks + (size_t)v * a.block_floats;
        const uint32_t flags = view_flag<PACKED>(a, blk, v, idx);
        if (!(flags & 1u)) continue;
        const float* cp = blk + kViewCamPos;
        const float3 d = make_float3(mean.x - cp[0], mean.y - cp[1], mean.z - cp[2]);
        const float len = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
        const float4 sa = view_sums_a<PACKED>(a, blk, flags, idx);
        const float3 g = make_float3((flags & 2u) ? 0.f : sa.x, (flags & 4u) ? 0.f : sa.y, (flags & 8u) ? 0.f : sa.z);
        float ddx, ddy, ddz;
        sh_backward(ShBand<K0, K1>{acc}, a.D, a.M, d.x / len, d.y / len, d.z / len, g, ddx, ddy, ddz);
    }
#pragma unroll
    for (int k = K0; k < K1; k++) {
        const float x = acc[3 * (k - K0)], y = acc[3 * (k - K0) + 1], z = acc[3 * (k - K0) + 2];
        if constexpr (SH_MODE != kShGlobal) {
            row[3 * k] = x;
            row[3 * k + 1] = y;
            row[3 * k + 2] = z;
        } else if (k < a.M) {
            float* c = dst.coef(idx, k);
            c[0] = x;
            c[1] = y;
            c[2] = z;
        }
    }
}

// 3 waves per SIMD (the LDS limit of the SH staging): the register allocator then spills a
// few values but the per-view latency chains overlap better (8 views: 0.50 -> 0.44 ms, r1af)
template <int SH_MODE, bool PACKED, bool LIST = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) gauss_bwd_views_kernel(ViewsBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float s_sh[SH_MODE != kShGlobal ? 64 * kShStride : 4];
    const int lane = threadIdx.x;
    const int g0 = blockIdx.x * 64;
    int idx = g0 + lane;
    if constexpr (LIST) {  // a lane per Gaussian some view flags (the outputs were zeroed beforehand)
        const uint32_t shard = blockIdx.x % kLiveShards, k0 = (blockIdx.x / kLiveShards) * 64;
        const uint32_t n = a.live_count[shard * kLiveCntStride];
        if (k0 >= n) return;  // uniform: past the shard's list
        idx = k0 + lane < n ? (int)a.live[(size_t)shard * a.live_cap + k0 + lane] : a.P;
    }
    const int nvalid = min(64, a.P - g0);
    const int M = a.M;
    const ShAddr sh_src{a.shs, a.dc, M};
    const ShGradAddr sh_dst{a.dL_dsh, a.dL_ddc, M};
    if constexpr (SH_MODE != kShGlobal) {
        if constexpr (LIST)
            sh_gather_in<64, 64, SH_MODE == kShLdsSplit>(sh_src, idx < a.P ? idx : -1, 0, s_sh, kShStride, lane);
        else
            sh_stage_in<64, 64, SH_MODE == kShLdsSplit>(sh_src, g0, nvalid, s_sh, kShStride, lane);
        __syncthreads();
    }
    const bool valid = idx < a.P;
    float3 mean = make_float3(0.f, 0.f, 0.f);
    // ---- phase 1: geometry gradients, summed over views
    if (valid) {
        GaussIn gi;
        gi.mean = make_float3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
        mean = gi.mean;
        gi.have_scales = true;
        gi.sc3 = make_float3(a.scales[3 * idx], a.scales[3 * idx + 1], a.scales[3 * idx + 2]);
        gi.q = reinterpret_cast<const float4*>(a.rotations)[idx];
        gi.cov3D = nullptr;
        gi.scale_modifier = a.scale_modifier;
        gi.opacity = a.opacities + idx;
        const ShReadOnly<SH_MODE != kShGlobal> shr{SH_MODE != kShGlobal ? &s_sh[lane * kShStride] : nullptr, sh_src,
                                                   idx};
        // the parameter gradients summed over the views (dL/dcov3D is not an output here)
        struct Sink {
            float3 dmean_sum = make_float3(0.f, 0.f, 0.f), dscale_sum = make_float3(0.f, 0.f, 0.f);
            float4 drot_sum = make_float4(0.f, 0.f, 0.f, 0.f);
            float dop_sum = 0.f;
            __device__ __forceinline__ void dop(float v) { dop_sum += v; }
            __device__ __forceinline__ void dcov(const float (&)[6]) {}
            __device__ __forceinline__ void sh_defer(float3, float3) {}
            __device__ __forceinline__ void dmean(float3 m) {
                dmean_sum.x += m.x; dmean_sum.y += m.y; dmean_sum.z += m.z;
            }
            __device__ __forceinline__ void scale_rot(bool, float3 ds, float4 dq) {
                dscale_sum.x += ds.x; dscale_sum.y += ds.y; dscale_sum.z += ds.z;
                drot_sum.x += dq.x; drot_sum.y += dq.y; drot_sum.z += dq.z; drot_sum.w += dq.w;
            }
        } sink;
        uint32_t flags_next = a.n_views > 0 ? view_flag<PACKED>(a, a.blocks, 0, idx) : 0u;
#pragma unroll 1
        for (int v = 0; v < a.n_views; v++) {
            const float* blk = a.blocks + (size_t)v * a.block_floats;
            const uint32_t flags = flags_next;
            if (v + 1 < a.n_views) flags_next = view_flag<PACKED>(a, blk + a.block_floats, v + 1, idx);
            if (!(flags & 1u)) continue;  // not visible in view v: no gradient from it
            const ViewCam cam{blk + kViewCamView, blk + kViewCamProj, blk + kViewCamPos, blk[kViewCamTanX],
                              blk[kViewCamTanY],  blk[kViewCamFocalX], blk[kViewCamFocalY],
                              (int)__float_as_uint(blk[kViewCamAA]), (int)__float_as_uint(blk[kViewCamInvDepth])};
            float4 sa, sb;
            float2 sc;
            view_sums<PACKED>(a, blk, flags, idx, sa, sb, sc);
            view_backward<kShNow>(cam, gi, sa, sb, sc, (uint8_t)((flags >> 1) & 7u), true, a.D, M, shr, sink);
        }
        store3(a.dL_dmean3D, idx, sink.dmean_sum.x, sink.dmean_sum.y, sink.dmean_sum.z);
        a.dL_dopacity[idx] = sink.dop_sum;
        store3(a.dL_dscale, idx, sink.dscale_sum.x, sink.dscale_sum.y, sink.dscale_sum.z);
        reinterpret_cast<float4*>(a.dL_drot)[idx] = sink.drot_sum;
    }
    // ---- phase 2: dL/dSH band by band (CR/backward.cu:43-127 products, summed over views)
    if constexpr (SH_MODE != kShGlobal) __syncthreads();  // the staged SH rows are read for the last time
    float* row = SH_MODE != kShGlobal ? &s_sh[lane * kShStride] : nullptr;
    if (valid) {
        // one walk over the views for every band: phase 1's registers are dead here, so the 48
        // accumulators fit under its peak (four walks -- one per band -- cost 0.12 of 0.28 ms at 8
        // views, r3z)
        if (a.D > 2) views_sh_band<0, 16, SH_MODE, PACKED>(a, idx, mean, row, sh_dst);
        else if (a.D > 1) views_sh_band<0, 9, SH_MODE, PACKED>(a, idx, mean, row, sh_dst);
        else if (a.D > 0) views_sh_band<0, 4, SH_MODE, PACKED>(a, idx, mean, row, sh_dst);
        else views_sh_band<0, 1, SH_MODE, PACKED>(a, idx, mean, row, sh_dst);
        const int K = (a.D + 1) * (a.D + 1);
        if constexpr (SH_MODE != kShGlobal) {
            for (int k = K; k < 16; k++) row[3 * k] = row[3 * k + 1] = row[3 * k + 2] = 0.f;
        } else {
            for (int k = K; k < M; k++) {
                float* c = sh_dst.coef(idx, k);
                c[0] = c[1] = c[2] = 0.f;
            }
        }
    }
    if constexpr (SH_MODE != kShGlobal) {
        __syncthreads();
        if constexpr (LIST)
            sh_gather_out<64, 64, SH_MODE == kShLdsSplit>(sh_dst, idx < a.P ? idx : -1, 0, s_sh, kShStride, lane);
        else
            sh_stage_out<64, 64, SH_MODE == kShLdsSplit>(sh_dst, g0, nvalid, s_sh, kShStride, lane);
    }
}

static hipError_t launch_gauss_bwd_views(const ViewsBwdArgs& a, hipStream_t stream) {
    if (a.P == 0) return hipSuccess;
    const dim3 grid((a.P + 63) / 64), block(64);
    const bool lds = a.shs && a.dL_dsh && a.M == 16 && (!a.dc || a.dL_ddc) &&
                     ((reinterpret_cast<uintptr_t>(a.shs) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(a.dL_dsh) & 15) == 0);
    if (a.flags && a.live) {  // packed blocks, a lane per Gaussian some view flags (outputs pre-zeroed)
        const dim3 lgrid(kLiveShards * ((a.live_cap + 63) / 64));
        if (lds && a.dc)
            hipLaunchKernelGGL((gauss_bwd_views_kernel<kShLdsSplit, true, true>), lgrid, block, 0, stream, a);
        else if (lds)
            hipLaunchKernelGGL((gauss_bwd_views_kernel<kShLdsCombined, true, true>), lgrid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((gauss_bwd_views_kernel<kShGlobal, true, true>), lgrid, block, 0, stream, a);
    } else if (a.flags) {  // packed blocks (gsr_view_block_index)
        if (lds && a.dc)
            hipLaunchKernelGGL((gauss_bwd_views_kernel<kShLdsSplit, true>), grid, block, 0, stream, a);
        else if (lds)
            hipLaunchKernelGGL((gauss_bwd_views_kernel<kShLdsCombined, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((gauss_bwd_views_kernel<kShGlobal, true>), grid, block, 0, stream, a);
    } else if (lds && a.dc) {
        hipLaunchKernelGGL((gauss_bwd_views_kernel<kShLdsSplit, false>), grid, block, 0, stream, a);
    } else if (lds) {
        hipLaunchKernelGGL((gauss_bwd_views_kernel<kShLdsCombined, false>), grid, block, 0, stream, a);
    } else {
        hipLaunchKernelGGL((gauss_bwd_views_kernel<kShGlobal, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

// The header of a view block: the camera, as gauss_bwd_views_kernel reads it.
__global__ void view_header_kernel(float* blk, const float* view, const float* proj, const float* campos,
                                   float tan_fovx, float tan_fovy, float focal_x, float focal_y, int antialiasing,
                                   int have_invdepth) {
    const int t = threadIdx.x;
    if (t < 16) blk[kViewCamView + t] = view[t];
    else if (t < 32) blk[kViewCamProj + t - 16] = proj[t - 16];
    else if (t < 35) blk[kViewCamPos + t - 32] = campos[t - 32];
    else if (t == 35) {
        blk[kViewCamTanX] = tan_fovx;
        blk[kViewCamTanY] = tan_fovy;
        blk[kViewCamFocalX] = focal_x;
        blk[kViewCamFocalY] = focal_y;
        blk[kViewCamAA] = __uint_as_float((uint32_t)antialiasing);
        blk[kViewCamInvDepth] = __uint_as_float((uint32_t)have_invdepth);
    }
}

// ---- sparse view blocks (multi-GPU exchange) ------------------------------------------
// Only the Gaussians with a non-zero render gradient need to travel: behind saturated pixels
// most have none (about 14% of a 1M@1080p view do).  A packed block is the view block's header
// (64 floats, the entry count in float kViewPackCount) followed by count entries of 12 floats:
// Gaussian index (bits), sums.a (4), sums.b (4), sums.c (2), flag word (bits), in Gaussian
// order (a deterministic compaction: per-workgroup counts, one scan, an in-order scatter).
constexpr int kPackThreads = 256;

__device__ __forceinline__ bool view_entry_live(const float* body, uint32_t P, uint32_t g) {
    const float4 a = reinterpret_cast<const float4*>(body)[g];
    const float4 b = reinterpret_cast<const float4*>(body + 4 * (size_t)P)[g];
    const float2 c = reinterpret_cast<const float2*>(body + 8 * (size_t)P)[g];
    const uint32_t f = __float_as_uint(body[10 * (size_t)P + g]);
    return (f & 1u) && ((a.x != 0.f) | (a.y != 0.f) | (a.z != 0.f) | (a.w != 0.f) | (b.x != 0.f) | (b.y != 0.f) |
                        (b.z != 0.f) | (b.w != 0.f) | (c.x != 0.f) | (c.y != 0.f));
}

// rank of this thread among the live threads of its workgroup, and the workgroup's total
__device__ __forceinline__ uint32_t block_live_rank(bool live, uint32_t* s_w, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(live);
    const uint32_t in_wave = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < kPackThreads / 64; k++) {
        before += k < w ? s_w[k] : 0u;
        all += s_w[k];
    }
    *total = all;
    return before + in_wave;
}

// (range forms: only Gaussians [g0, g1) are packed, indexed, listed -- one chunk of a chunked exchange,
// distributed.py ViewExchange(chunks=K); entries keep their absolute Gaussian index)
__global__ void __launch_bounds__(kPackThreads) view_pack_count_kernel(uint32_t P, uint32_t g0, uint32_t g1,
                                                                       const float* __restrict__ block,
                                                                       uint32_t* __restrict__ wg_cnt) {
    __shared__ uint32_t s_w[kPackThreads / 64];
    const uint32_t g = g0 + blockIdx.x * kPackThreads + threadIdx.x;
    const bool live = g < g1 && view_entry_live(block + kViewBlockHeader, P, g);
    uint32_t total = 0;
    block_live_rank(live, s_w, &total);
    if (threadIdx.x == 0) wg_cnt[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the per-workgroup counts (in place), total into the packed header
__global__ void __launch_bounds__(1024) view_pack_scan_kernel(uint32_t nb, uint32_t* __restrict__ wg_cnt,
                                                              float* __restrict__ packed, uint32_t* __restrict__ count) {
    __shared__ uint32_t s_tot[1024 / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? wg_cnt[i] : 0u;
        const uint32_t incl = wave_incl_sum(v);
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        if (lane == 63) s_tot[w] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int k = 0; k < (int)(blockDim.x / 64); k++) {
            before += k < w ? s_tot[k] : 0u;
            all += s_tot[k];
        }
        if (i < nb) wg_cnt[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        packed[kViewPackCount] = __uint_as_float(carry);
        if (count) count[0] = carry;
    }
}

__global__ void __launch_bounds__(kPackThreads) view_pack_scatter_kernel(uint32_t P, uint32_t g0, uint32_t g1,
                                                                         const float* __restrict__ block,
                                                                         const uint32_t* __restrict__ wg_off,
                                                                         float* __restrict__ packed,
                                                                         unsigned long long cap) {
    __shared__ uint32_t s_w[kPackThreads / 64];
    if (blockIdx.x == 0 && threadIdx.x < kViewBlockHeader && threadIdx.x != kViewPackCount)
        packed[threadIdx.x] = block[threadIdx.x];
    const float* body = block + kViewBlockHeader;
    const uint32_t g = g0 + blockIdx.x * kPackThreads + threadIdx.x;
    const bool live = g < g1 && view_entry_live(body, P, g);
    uint32_t total = 0;
    const uint32_t pos = wg_off[blockIdx.x] + block_live_rank(live, s_w, &total);
    if (live && pos < cap) {
        const float4 a = reinterpret_cast<const float4*>(body)[g];
        const float4 b = reinterpret_cast<const float4*>(body + 4 * (size_t)P)[g];
        const float2 c = reinterpret_cast<const float2*>(body + 8 * (size_t)P)[g];
        const float f = body[10 * (size_t)P + g];
        float4* e = reinterpret_cast<float4*>(packed + kViewBlockHeader + (size_t)kViewPackEntry * pos);
        e[0] = make_float4(__uint_as_float(g), a.x, a.y, a.z);
        e[1] = make_float4(a.w, b.x, b.y, b.z);
        e[2] = make_float4(b.w, c.x, c.y, f);
    }
}

static hipError_t launch_view_pack(uint32_t P, uint32_t g0, uint32_t g1, const float* block, float* packed,
                            unsigned long long cap, uint32_t* scratch, uint32_t* count, hipStream_t stream) {
    const uint32_t nb = (g1 - g0 + kPackThreads - 1) / kPackThreads;
    if (nb == 0) {  // an empty range: a header with no entries
        hipLaunchKernelGGL(view_pack_scan_kernel, dim3(1), dim3(1024), 0, stream, 0u, scratch, packed, count);
        hipLaunchKernelGGL(view_pack_scatter_kernel, dim3(1), dim3(kPackThreads), 0, stream, P, g0, g0, block, scratch,
                           packed, cap);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(view_pack_count_kernel, dim3(nb), dim3(kPackThreads), 0, stream, P, g0, g1, block, scratch);
    hipLaunchKernelGGL(view_pack_scan_kernel, dim3(1), dim3(1024), 0, stream, nb, scratch, packed, count);
    hipLaunchKernelGGL(view_pack_scatter_kernel, dim3(nb), dim3(kPackThreads), 0, stream, P, g0, g1, block, scratch,
                       packed, cap);
    return hipGetLastError();
}

// The flag words of n_views dense view blocks zeroed: gauss_bwd_views_kernel reads a Gaussian's
// sums only when its flag has the visible bit, so after this and the scatter below the sums of
// the Gaussians left out of a packed block are never read, and need no zeroing (a 40-B-per-
// Gaussian memset per view, 320 MB at 8 views, reduced to 4 B).
__global__ void __launch_bounds__(kPackThreads) view_flags_zero_kernel(uint32_t P, float* __restrict__ blocks,
                                                                       unsigned long long block_floats) {
    uint32_t* f = reinterpret_cast<uint32_t*>(blocks + blockIdx.y * block_floats + kViewBlockHeader + 10 * (size_t)P);
    for (uint32_t g = blockIdx.x * kPackThreads + threadIdx.x; g < P; g += gridDim.x * kPackThreads) f[g] = 0u;
}

// packed [n_views][packed_floats] -> dense view blocks [n_views][view_block_floats(P)], whose
// flag words view_flags_zero_kernel cleared: header copy and one entry per thread.
__global__ void __launch_bounds__(kPackThreads) view_unpack_kernel(uint32_t P, const float* __restrict__ packed,
                                                                   unsigned long long packed_floats,
                                                                   float* __restrict__ blocks,
                                                                   unsigned long long block_floats,
                                                                   unsigned long long cap) {
    const uint32_t v = blockIdx.y;
    const float* pk = packed + v * packed_floats;
    float* blk = blocks + v * block_floats;
    if (blockIdx.x == 0 && threadIdx.x < kViewBlockHeader) blk[threadIdx.x] = threadIdx.x == kViewPackCount ? 0.f
                                                                                                       : pk[threadIdx.x];
    uint32_t n = __float_as_uint(pk[kViewPackCount]);
    n = n < cap ? n : (uint32_t)cap;
    float* body = blk + kViewBlockHeader;
    for (uint32_t i = blockIdx.x * kPackThreads + threadIdx.x; i < n; i += gridDim.x * kPackThreads) {
        const float4* e = reinterpret_cast<const float4*>(pk + kViewBlockHeader + (size_t)kViewPackEntry * i);
        const float4 e0 = e[0], e1 = e[1], e2 = e[2];
        const uint32_t g = __float_as_uint(e0.x);
        if (g >= P) continue;  // never for a block packed by view_pack_scatter_kernel
        reinterpret_cast<float4*>(body)[g] = make_float4(e0.y, e0.z, e0.w, e1.x);
        reinterpret_cast<float4*>(body + 4 * (size_t)P)[g] = make_float4(e1.y, e1.z, e1.w, e2.x);
        reinterpret_cast<float2*>(body + 8 * (size_t)P)[g] = make_float2(e2.y, e2.z);
        body[10 * (size_t)P + g] = e2.w;
    }
}

static hipError_t launch_view_unpack(uint32_t P, int n_views, const float* packed, unsigned long long packed_floats,
                              float* blocks, unsigned long long cap, hipStream_t stream) {
    if (n_views <= 0) return hipSuccess;
    const size_t bf = view_block_floats(P);
    const uint32_t gz = (P + kPackThreads - 1) / kPackThreads;
    hipLaunchKernelGGL(view_flags_zero_kernel, dim3(gz < 1024 ? (gz ? gz : 1) : 1024, n_views), dim3(kPackThreads), 0,
                       stream, P, blocks, (unsigned long long)bf);
    const uint32_t gx = (uint32_t)((cap + kPackThreads - 1) / kPackThreads);
    hipLaunchKernelGGL(view_unpack_kernel, dim3(gx < 1024 ? (gx ? gx : 1) : 1024, n_views), dim3(kPackThreads), 0,
                       stream, P, packed, packed_floats, blocks, (unsigned long long)bf, cap);
    return hipGetLastError();
}

// Packed mode of the multi-view backward: instead of rebuilding dense view blocks, each view's
// flag array [P] is cleared and, for every packed entry i, set to i << 4 | its flag bits -- one
// 4-byte store per entry instead of four scattered stores of 44 bytes.
__global__ void __launch_bounds__(kPackThreads) view_index_kernel(uint32_t P, const float* __restrict__ packed,
                                                                  unsigned long long packed_floats,
                                                                  uint32_t* __restrict__ flags,
                                                                  unsigned long long cap) {
    const uint32_t v = blockIdx.y;
    const float* pk = packed + v * packed_floats;
    uint32_t n = __float_as_uint(pk[kViewPackCount]);
    n = n < cap ? n : (uint32_t)cap;
    uint32_t* f = flags + (size_t)v * P;
    for (uint32_t i = blockIdx.x * kPackThreads + threadIdx.x; i < n; i += gridDim.x * kPackThreads) {
        const float* e = pk + kViewBlockHeader + (size_t)kViewPackEntry * i;
        const uint32_t g = __float_as_uint(e[0]);
        if (g < P) f[g] = (i << 4) | (__float_as_uint(e[11]) & 15u);
    }
}

__global__ void __launch_bounds__(kPackThreads) flags_zero_kernel(uint32_t P, uint32_t g0, uint32_t g1,
                                                                  uint32_t* __restrict__ flags) {
    uint32_t* f = flags + (size_t)blockIdx.y * P;
    for (uint32_t g = g0 + blockIdx.x * kPackThreads + threadIdx.x; g < g1; g += gridDim.x * kPackThreads) f[g] = 0u;
}

static hipError_t launch_view_index(uint32_t P, uint32_t g0, uint32_t g1, int n_views, const float* packed,
                             unsigned long long packed_floats, uint32_t* flags, unsigned long long cap,
                             hipStream_t stream) {
    if (n_views <= 0) return hipSuccess;
    const uint32_t gz = (g1 - g0 + kPackThreads - 1) / kPackThreads;
    hipLaunchKernelGGL(flags_zero_kernel, dim3(gz < 1024 ? (gz ? gz : 1) : 1024, n_views), dim3(kPackThreads), 0,
                       stream, P, g0, g1, flags);
    const uint32_t gx = (uint32_t)((cap + kPackThreads - 1) / kPackThreads);
    hipLaunchKernelGGL(view_index_kernel, dim3(gx < 1024 ? (gx ? gx : 1) : 1024, n_views), dim3(kPackThreads), 0,
                       stream, P, packed, packed_floats, flags, cap);
    return hipGetLastError();
}

// The Gaussians some view flags (visible with a gradient in a packed block), appended to the
// sharded live list (one atomic per wave, kLiveShards counters the caller zeroed).
__global__ void __launch_bounds__(64) views_live_kernel(uint32_t P, uint32_t g0, uint32_t g1, int n_views,
                                                        const uint32_t* __restrict__ flags,
                                                        uint32_t* __restrict__ live, uint32_t* __restrict__ live_count,
                                                        uint32_t live_cap) {
    const uint32_t g = g0 + blockIdx.x * 64 + threadIdx.x;
    bool lv = false;
    if (g < g1)
        for (int v = 0; v < n_views; v++) lv |= (flags[(size_t)v * P + g] & 1u) != 0;
    const unsigned long long m = __ballot(lv);
    if (!m) return;
    const uint32_t shard = blockIdx.x % kLiveShards;
    uint32_t base = 0;
    if (threadIdx.x == 0) base = atomicAdd(&live_count[shard * kLiveCntStride], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0);
    if (lv) live[(size_t)shard * live_cap + base + (uint32_t)__popcll(m & ((1ull << threadIdx.x) - 1ull))] = g;
}

static hipError_t launch_views_live(uint32_t P, uint32_t g0, uint32_t g1, int n_views, const uint32_t* flags, uint32_t* live,
                             uint32_t* live_count, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(live_count, 0, sizeof(uint32_t) * kLiveShards * kLiveCntStride, stream);
    if (e != hipSuccess || g1 <= g0) return e;
    // (a range's blocks are at most P's, so live_list_cap(P) bounds every shard)
    hipLaunchKernelGGL(views_live_kernel, dim3((g1 - g0 + 63) / 64), dim3(64), 0, stream, P, g0, g1, n_views, flags,
                       live, live_count, live_list_cap(P));
    return hipGetLastError();
}

hipError_t launch_view_header(float* blk, const float* view, const float* proj, const float* campos, float tan_fovx,
                              float tan_fovy, float focal_x, float focal_y, int antialiasing, int have_invdepth,
                              hipStream_t stream) {
    hipLaunchKernelGGL(view_header_kernel, dim3(1), dim3(64), 0, stream, blk, view, proj, campos, tan_fovx, tan_fovy,
                       focal_x, focal_y, antialiasing, have_invdepth);
    return hipGetLastError();
}

}  // namespace gsr

// ---- C entry points: the multi-GPU view exchange (include/gsr.h) -----------------------
using namespace gsr;

extern "C" {

unsigned long long gsr_view_block_floats(int P) { return P > 0 ? gsr::view_block_floats((size_t)P) : 0ull; }

unsigned long long gsr_view_pack_floats(long long entries) {
    return gsr::view_pack_floats(entries > 0 ? (size_t)entries : 0);
}

unsigned long long gsr_view_pack_scratch_bytes(int P) { return P > 0 ? 4ull * ((P + 255) / 256) : 4ull; }

int gsr_view_block_pack_range(int P, int g0, int g1, const float* view_block, float* packed, long long cap,
                              void* scratch, unsigned int* count, void* stream) {
    clear_error();
    if (P <= 0 || cap < 0) return fail(GSR_ERR_ARGUMENT, "view_block_pack: P=%d cap=%lld", P, cap);
    if (g0 < 0 || g1 < g0 || g1 > P) return fail(GSR_ERR_ARGUMENT, "view_block_pack: range [%d, %d) of P=%d", g0, g1, P);
    if (!view_block || !packed || !scratch) return fail(GSR_ERR_ARGUMENT, "view_block_pack: null pointer");
    if ((reinterpret_cast<uintptr_t>(view_block) & 15) || (reinterpret_cast<uintptr_t>(packed) & 15))
        return fail(GSR_ERR_ARGUMENT, "view_block_pack: blocks must be 16-byte aligned");
    HIP_TRY(gsr::launch_view_pack((uint32_t)P, (uint32_t)g0, (uint32_t)g1, view_block, packed, (unsigned long long)cap,
                                  reinterpret_cast<uint32_t*>(scratch), count, (hipStream_t)stream),
            "view_block_pack");
    return GSR_OK;
}

int gsr_view_block_pack(int P, const float* view_block, float* packed, long long cap, void* scratch,
                        unsigned int* count, void* stream) {
    return gsr_view_block_pack_range(P, 0, P, view_block, packed, cap, scratch, count, stream);
}

int gsr_view_block_unpack(int P, int n_views, const float* packed, long long packed_floats, float* blocks,
                          long long cap, void* stream) {
    clear_error();
    if (P <= 0 || n_views < 0 || cap < 0 || packed_floats < (long long)gsr::view_pack_floats(0))
        return fail(GSR_ERR_ARGUMENT, "view_block_unpack: P=%d views=%d packed_floats=%lld cap=%lld", P, n_views,
                    packed_floats, cap);
    if ((size_t)packed_floats < gsr::view_pack_floats((size_t)cap))
        return fail(GSR_ERR_ARGUMENT, "view_block_unpack: %lld floats per packed block cannot hold %lld entries",
                    packed_floats, cap);
    if (n_views > 0 && (!packed || !blocks)) return fail(GSR_ERR_ARGUMENT, "view_block_unpack: null pointer");
    if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(blocks) & 15) || (packed_floats & 3))
        return fail(GSR_ERR_ARGUMENT, "view_block_unpack: blocks must be 16-byte aligned");
    HIP_TRY(gsr::launch_view_unpack((uint32_t)P, n_views, packed, (unsigned long long)packed_floats, blocks,
                                    (unsigned long long)cap, (hipStream_t)stream),
            "view_block_unpack");
    return GSR_OK;
}

int gsr_view_block_index(int P, int n_views, const float* packed, long long packed_floats, unsigned int* flags,
                         long long cap, void* stream) {
    return gsr_view_block_index_range(P, 0, P, n_views, packed, packed_floats, flags, cap, stream);
}

int gsr_view_block_index_range(int P, int g0, int g1, int n_views, const float* packed, long long packed_floats,
                               unsigned int* flags, long long cap, void* stream) {
    clear_error();
    if (g0 < 0 || g1 < g0 || g1 > P) return fail(GSR_ERR_ARGUMENT, "view_block_index: range [%d, %d) of P=%d", g0, g1, P);
    if (P <= 0 || n_views < 0 || cap < 0 || packed_floats < (long long)gsr::view_pack_floats(0))
        return fail(GSR_ERR_ARGUMENT, "view_block_index: P=%d views=%d packed_floats=%lld cap=%lld", P, n_views,
                    packed_floats, cap);
    if ((size_t)packed_floats < gsr::view_pack_floats((size_t)cap))
        return fail(GSR_ERR_ARGUMENT, "view_block_index: %lld floats per packed block cannot hold %lld entries",
                    packed_floats, cap);
    if (cap >= (1ll << 28)) return fail(GSR_ERR_ARGUMENT, "view_block_index: %lld entries exceed 2^28", cap);
    if (n_views > 0 && (!packed || !flags)) return fail(GSR_ERR_ARGUMENT, "view_block_index: null pointer");
    if ((reinterpret_cast<uintptr_t>(packed) & 15) || (packed_floats & 3))
        return fail(GSR_ERR_ARGUMENT, "view_block_index: packed blocks must be 16-byte aligned");
    HIP_TRY(gsr::launch_view_index((uint32_t)P, (uint32_t)g0, (uint32_t)g1, n_views, packed,
                                   (unsigned long long)packed_floats, flags, (unsigned long long)cap, (hipStream_t)stream),
            "view_block_index");
    return GSR_OK;
}

}  // extern "C"

namespace {
int backward_views_impl(int P, int D, int M, const float* means3D, const float* dc, const float* shs,
                        const float* opacities, const float* scales, const float* rotations, float scale_modifier,
                        int n_views, const float* blocks, long long block_floats, const unsigned int* flags,
                        const unsigned int* live, const unsigned int* live_count, float* dL_dmean3D, float* dL_ddc,
                        float* dL_dsh, float* dL_dopacity, float* dL_dscale, float* dL_drot, void* stream) {
    using namespace gsr;
    clear_error();
    if (P < 0 || n_views < 0) return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: P=%d views=%d", P, n_views);
    if (P == 0) return GSR_OK;
    if (!flags && (size_t)block_floats != view_block_floats((size_t)P))
        return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: block of %lld floats, expected %zu", block_floats,
                    view_block_floats((size_t)P));
    if (flags && (block_floats < (long long)view_pack_floats(0) || (block_floats & 3) ||
                  (reinterpret_cast<uintptr_t>(blocks) & 15)))
        return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: packed blocks of %lld floats (16-byte aligned)",
                    block_floats);
    if (!means3D || !opacities || !scales || !rotations || (n_views > 0 && !blocks) || !dL_dmean3D || !dL_dopacity ||
        !dL_dscale || !dL_drot)
        return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: null pointer");
    if (D < 0 || D > 3) return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: SH degree %d", D);
    if (dc && M > 0 && !shs) return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: rest SH without shs");
    if ((shs && !dL_dsh) || (dc && !dL_ddc)) return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: missing SH outputs");
    if (!dc && !shs) return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: needs SH (precomputed colours are per view)");
    if ((D + 1) * (D + 1) > (dc ? M + 1 : M))  // as the forward (forward_impl): never read past a row
        return fail(GSR_ERR_ARGUMENT, "gauss_backward_views: SH degree %d needs %d coefficients, got %d", D,
                    (D + 1) * (D + 1), dc ? M + 1 : M);
    ViewsBwdArgs a{};
    a.P = P; a.D = D; a.M = dc ? M + 1 : M;
    a.means3D = means3D; a.shs = (dc && M == 0) ? nullptr : shs; a.dc = dc; a.opacities = opacities; a.scales = scales;
    a.rotations = rotations; a.scale_modifier = scale_modifier; a.n_views = n_views; a.blocks = blocks;
    a.block_floats = (size_t)block_floats;
    a.flags = flags;
    a.live = live;
    a.live_count = live_count;
    a.live_cap = live_list_cap((uint32_t)P);
    a.dL_dmean3D = dL_dmean3D; a.dL_dsh = a.shs ? dL_dsh : nullptr; a.dL_ddc = dc ? dL_ddc : nullptr;
    a.dL_dopacity = dL_dopacity; a.dL_dscale = dL_dscale; a.dL_drot = dL_drot;
    {
        StageScope sc(ST_GAUSS_BWD, (hipStream_t)stream);
        HIP_TRY(launch_gauss_bwd_views(a, (hipStream_t)stream), "gauss_backward_views");
    }
    return GSR_OK;
}
}  // namespace

extern "C" {

int gsr_gauss_backward_views(int P, int D, int M, const float* means3D, const float* dc, const float* shs,
                             const float* opacities, const float* scales, const float* rotations, float scale_modifier,
                             int n_views, const float* blocks, long long block_floats, float* dL_dmean3D,
                             float* dL_ddc, float* dL_dsh, float* dL_dopacity, float* dL_dscale, float* dL_drot,
                             void* stream) {
    return backward_views_impl(P, D, M, means3D, dc, shs, opacities, scales, rotations, scale_modifier, n_views,
                               blocks, block_floats, nullptr, nullptr, nullptr, dL_dmean3D, dL_ddc, dL_dsh, dL_dopacity,
                               dL_dscale, dL_drot, stream);
}

int gsr_gauss_backward_views_packed(int P, int D, int M, const float* means3D, const float* dc, const float* shs,
                                    const float* opacities, const float* scales, const float* rotations,
                                    float scale_modifier, int n_views, const float* packed, long long packed_floats,
                                    const unsigned int* flags, float* dL_dmean3D, float* dL_ddc, float* dL_dsh,
                                    float* dL_dopacity, float* dL_dscale, float* dL_drot, void* stream) {
    if (n_views > 0 && !flags) return fail(GSR_ERR_ARGUMENT, "gauss_backward_views_packed: null flags");
    return backward_views_impl(P, D, M, means3D, dc, shs, opacities, scales, rotations, scale_modifier, n_views,
                               packed, packed_floats, flags, nullptr, nullptr, dL_dmean3D, dL_ddc, dL_dsh, dL_dopacity,
                               dL_dscale, dL_drot, stream);
}

unsigned long long gsr_views_live_floats(int P) {
    return P > 0 ? (unsigned long long)gsr::kLiveShards * gsr::live_list_cap((uint32_t)P) +
                       (unsigned long long)gsr::kLiveShards * gsr::kLiveCntStride
                 : 0ull;
}

int gsr_views_live_list_range(int P, int g0, int g1, int n_views, const unsigned int* flags, unsigned int* live,
                              void* stream) {
    clear_error();
    if (P < 0 || n_views < 0) return fail(GSR_ERR_ARGUMENT, "views_live_list: P=%d views=%d", P, n_views);
    if (g0 < 0 || g1 < g0 || g1 > P) return fail(GSR_ERR_ARGUMENT, "views_live_list: range [%d, %d) of P=%d", g0, g1, P);
    if (P == 0) return GSR_OK;
    if (!live || (n_views > 0 && !flags)) return fail(GSR_ERR_ARGUMENT, "views_live_list: null pointer");
    unsigned int* count = live + (size_t)gsr::kLiveShards * gsr::live_list_cap((uint32_t)P);
    HIP_TRY(gsr::launch_views_live((uint32_t)P, (uint32_t)g0, (uint32_t)g1, n_views, flags, live, count,
                                   (hipStream_t)stream),
            "views_live_list");
    return GSR_OK;
}

int gsr_views_live_list(int P, int n_views, const unsigned int* flags, unsigned int* live, void* stream) {
    return gsr_views_live_list_range(P, 0, P, n_views, flags, live, stream);
}

int gsr_gauss_backward_views_live(int P, int D, int M, const float* means3D, const float* dc, const float* shs,
                                  const float* opacities, const float* scales, const float* rotations,
                                  float scale_modifier, int n_views, const float* packed, long long packed_floats,
                                  const unsigned int* flags, const unsigned int* live, float* dL_dmean3D,
                                  float* dL_ddc, float* dL_dsh, float* dL_dopacity, float* dL_dscale, float* dL_drot,
                                  void* stream) {
    if (n_views > 0 && (!flags || !live)) return fail(GSR_ERR_ARGUMENT, "gauss_backward_views_live: null list");
    const unsigned int* count = live ? live + (size_t)gsr::kLiveShards * gsr::live_list_cap((uint32_t)(P > 0 ? P : 0))
                                     : nullptr;
    return backward_views_impl(P, D, M, means3D, dc, shs, opacities, scales, rotations, scale_modifier, n_views,
                               packed, packed_floats, flags, live, count, dL_dmean3D, dL_ddc, dL_dsh, dL_dopacity,
                               dL_dscale, dL_drot, stream);
}

}  // extern "C"
