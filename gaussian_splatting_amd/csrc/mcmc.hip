// mcmc.hip -- 3DGS-MCMC density control (include/gsr_mcmc.h): position noise, relocation arithmetic, row surgery.
//
//   noise       (one thread per Gaussian, every iteration)  HBM-bound: 56 B read, 12 B written per Gaussian.  The
//               three [P][3] arrays (xyz, scaling, xi) cross HBM as 16-byte-per-lane accesses over the workgroup's
//               contiguous 3 KiB and are transposed through LDS (row stride 3 dwords: conflict-free); the [P][4]
//               quaternion is one 16-byte load per lane, the opacity one dword per lane.  float32 throughout.
//   count       (one thread per sample)  integer atomics into the zeroed per-Gaussian counts: deterministic
//   relocation  (one thread per sample)  float64: Pascal's triangle per workgroup in LDS, one alternating sum per
//               sample, rounded to float32 once on store
//   apply       (one thread per float of the sampled rows, one launch per parameter group)  bit copies
//               sampled -> dest, the relocation's opacity and scaling at both, zero Adam moments at the sources
//
// The C entry points (include/gsr_mcmc.h) are at the end of the file.
#include "../../include/gsr_mcmc.h"

#include <float.h>

#include "gsr_common.h"
#include "host.h"

namespace gsr {

constexpr int kNoiseThreads = 256;
constexpr int kNoiseVec = kNoiseThreads * 3 / 4;  // float4s of one [256][3] tile
constexpr int kRelocThreads = 256;
constexpr int kTri = GSR_MCMC_N_MAX + 1;  // rows and columns of the triangle: C(i, k), 0 <= i, k <= 51

// ---- noise --------------------------------------------------------------------------
// A workgroup's tile of a [P][3] array is the `nf` floats from `src` (16-byte aligned: the tile starts at a multiple
// of 768 floats).  Lane t moves floats 4t .. 4t + 3: one 16-byte access, or dword accesses where the array ends
// inside them.
__device__ __forceinline__ void tile_load(const float* __restrict__ src, float* dst, int t, int nf) {
    if (4 * t + 4 <= nf) {
        reinterpret_cast<float4*>(dst)[t] = reinterpret_cast<const float4*>(src)[t];
    } else {
        for (int e = 4 * t; e < nf; e++) dst[e] = src[e];
    }
}

__device__ __forceinline__ void tile_store(float* __restrict__ dst, const float* src, int t, int nf) {
    if (4 * t + 4 <= nf) {
        reinterpret_cast<float4*>(dst)[t] = reinterpret_cast<const float4*>(src)[t];
    } else {
        for (int e = 4 * t; e < nf; e++) dst[e] = src[e];
    }
}

__global__ void __launch_bounds__(kNoiseThreads) mcmc_noise_kernel(int P, float* __restrict__ xyz,
                                                                   const float* __restrict__ opacity,
                                                                   const float* __restrict__ scaling,
                                                                   const float* __restrict__ rotation,
                                                                   const float* __restrict__ xi, float noise_scale) {
    __shared__ float4 s_xyz4[kNoiseVec], s_scl4[kNoiseVec], s_xi4[kNoiseVec];
    float* s_xyz = reinterpret_cast<float*>(s_xyz4);
    float* s_scl = reinterpret_cast<float*>(s_scl4);
    float* s_xi = reinterpret_cast<float*>(s_xi4);
    const int t = threadIdx.x;
    const size_t g0 = (size_t)blockIdx.x * kNoiseThreads;  // the tile's first Gaussian (< P: the grid is ceil(P / 256))
    const int cnt = (size_t)P - g0 < (size_t)kNoiseThreads ? (int)((size_t)P - g0) : kNoiseThreads;
    const int nf = 3 * cnt;
    const size_t f0 = 3 * g0;
    if (t < kNoiseVec) {
        tile_load(xyz + f0, s_xyz, t, nf);
        tile_load(scaling + f0, s_scl, t, nf);
        tile_load(xi + f0, s_xi, t, nf);
    }
    const bool live = t < cnt;
    float4 q = make_float4(1.f, 0.f, 0.f, 0.f);
    float op = 0.f;
    if (live) {
        q = reinterpret_cast<const float4*>(rotation)[g0 + t];
        op = opacity[g0 + t];
    }
    __syncthreads();
    if (live) {
        const float o = 1.f / (1.f + expf(-op));
        // the paper's sigmoid(100 * ((1 - o) - 0.995)) without forming 1 - o; exp overflows to inf, the gate to 0
        const float gate = 1.f / (1.f + expf(GSR_MCMC_GATE_K * (o - GSR_MCMC_GATE_X0)));
        const float g = gate * noise_scale;
        const float v0 = s_xi[3 * t] * g, v1 = s_xi[3 * t + 1] * g, v2 = s_xi[3 * t + 2] * g;
        const float inv = 1.f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
        const float r = q.x * inv, x = q.y * inv, y = q.z * inv, z = q.w * inv;
        const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
        const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
        const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
        const float s0 = expf(s_scl[3 * t]), s1 = expf(s_scl[3 * t + 1]), s2 = expf(s_scl[3 * t + 2]);
        // Sigma v = R diag(s^2) R^T v
        const float u0 = (R00 * v0 + R10 * v1 + R20 * v2) * (s0 * s0);
        const float u1 = (R01 * v0 + R11 * v1 + R21 * v2) * (s1 * s1);
        const float u2 = (R02 * v0 + R12 * v1 + R22 * v2) * (s2 * s2);
        s_xyz[3 * t] += R00 * u0 + R01 * u1 + R02 * u2;
        s_xyz[3 * t + 1] += R10 * u0 + R11 * u1 + R12 * u2;
        s_xyz[3 * t + 2] += R20 * u0 + R21 * u1 + R22 * u2;
    }
    __syncthreads();
    if (t < kNoiseVec) tile_store(xyz + f0, s_xyz, t, nf);
}

// ---- relocation ---------------------------------------------------------------------
__global__ void __launch_bounds__(kRelocThreads) mcmc_count_kernel(int P, int n, const long long* __restrict__ sampled,
                                                                   int* __restrict__ count) {
    const int j = blockIdx.x * kRelocThreads + threadIdx.x;
    if (j >= n) return;
    const long long s = sampled[j];
    if (s >= 0 && s < P) atomicAdd(&count[s], 1);
}

__global__ void __launch_bounds__(kRelocThreads) mcmc_relocation_kernel(
    int P, int n, const float* __restrict__ opacity, const float* __restrict__ scaling,
    const long long* __restrict__ sampled, const int* __restrict__ count, int n_max, float min_opacity,
    float* __restrict__ new_opacity, float* __restrict__ new_scaling, int* __restrict__ ratio) {
    __shared__ double s_binom[kTri][kTri];  // Pascal's triangle: every entry an integer below 2^53, exact
    __shared__ double s_rsqrt[kTri];        // 1 / sqrt(k + 1)
    const int t = threadIdx.x;
    if (t < kTri) {
        s_binom[0][t] = t == 0 ? 1.0 : 0.0;
        s_rsqrt[t] = 1.0 / sqrt((double)(t + 1));
    }
    __syncthreads();
    for (int i = 1; i <= n_max; i++) {  // (n_max <= 51, the same in every thread)
        if (t < kTri) s_binom[i][t] = s_binom[i - 1][t] + (t > 0 ? s_binom[i - 1][t - 1] : 0.0);
        __syncthreads();
    }
    const int j = blockIdx.x * kRelocThreads + t;
    if (j >= n) return;
    const long long s = sampled[j];
    if (s < 0 || s >= P) return;
    int N = count[s] + 1;
    N = N < n_max ? N : n_max;
    ratio[j] = N;
    const double o = 1.0 / (1.0 + exp(-(double)opacity[s]));
    const double x = -expm1(log1p(-o) / (double)N);  // 1 - (1 - o)^(1/N)
    double den = 0.0, xp = x;                        // xp = x^(k+1)
    for (int k = 0; k < N; k++) {
        const double term = s_binom[N][k + 1] * xp * s_rsqrt[k];
        den += (k & 1) ? -term : term;
        xp *= x;
    }
    const double hi = 1.0 - (double)FLT_EPSILON;
    const double xc = fmin(fmax(x, (double)min_opacity), hi);
    new_opacity[j] = (float)log(xc / (1.0 - xc));
    const double shift = log(o / den);
#pragma unroll
    for (int c = 0; c < 3; c++) new_scaling[3 * (size_t)j + c] = (float)((double)scaling[3 * (size_t)s + c] + shift);
}

// ---- apply --------------------------------------------------------------------------
struct McmcApplyArgs {
    int P;
    uint32_t total;  // n * width
    uint32_t width;
    int role;
    const long long* sampled;
    const long long* dest;
    const uint32_t* new_opacity;
    const uint32_t* new_scaling;
    uint32_t* data;
    uint32_t* m;  // null: the group has no Adam state
    uint32_t* v;
};

__global__ void __launch_bounds__(kRelocThreads) mcmc_apply_kernel(McmcApplyArgs a) {
    const uint32_t t = blockIdx.x * kRelocThreads + threadIdx.x;
    if (t >= a.total) return;
    const uint32_t j = t / a.width, c = t - j * a.width;
    const long long s = a.sampled[j], d = a.dest[j];
    if (s < 0 || s >= a.P || d < 0 || d >= a.P) return;
    const size_t src = (size_t)s * a.width + c, dst = (size_t)d * a.width + c;
    if (a.role == GSR_MCMC_COPY) {
        a.data[dst] = a.data[src];  // rows `sampled` are never written: sampled and dest are disjoint
    } else {
        const uint32_t val = a.role == GSR_MCMC_OPACITY ? a.new_opacity[j] : a.new_scaling[3 * (size_t)j + c];
        a.data[dst] = val;
        a.data[src] = val;  // duplicates of a source write identical bits
    }
    if (a.m) {
        a.m[src] = 0u;
        a.v[src] = 0u;
    }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace gsr

// ---- C entry points (include/gsr_mcmc.h) -------------------------------------------
extern "C" {

int gsr_mcmc_noise(int P, float* xyz, const float* opacity, const float* scaling, const float* rotation,
                   const float* xi, float noise_scale, void* stream) {
    using namespace gsr;
    clear_error();
    if (P < 0) return fail(GSR_ERR_ARGUMENT, "mcmc_noise: P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!xyz || !opacity || !scaling || !rotation || !xi) return fail(GSR_ERR_ARGUMENT, "mcmc_noise: null pointer");
    if (!aligned16(xyz) || !aligned16(scaling) || !aligned16(rotation) || !aligned16(xi))
        return fail(GSR_ERR_ARGUMENT, "mcmc_noise: xyz, scaling, rotation and xi must be 16-byte aligned");
    const unsigned blocks = (unsigned)(((size_t)P + kNoiseThreads - 1) / kNoiseThreads);
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(blocks), dim3(kNoiseThreads), 0, (hipStream_t)stream, P, xyz, opacity,
                       scaling, rotation, xi, noise_scale);
    HIP_TRY(hipGetLastError(), "mcmc_noise");
    return GSR_OK;
}

unsigned long long gsr_mcmc_scratch_bytes(int P) { return P > 0 ? (unsigned long long)P * sizeof(int) : 0ull; }

int gsr_mcmc_relocation(int P, int n, const float* opacity, const float* scaling, const long long* sampled,
                        int n_max, float min_opacity, void* scratch, float* new_opacity, float* new_scaling,
                        int* ratio, void* stream) {
    using namespace gsr;
    clear_error();
    if (P < 0 || n < 0) return fail(GSR_ERR_ARGUMENT, "mcmc_relocation: P = %d, n = %d must be >= 0", P, n);
    if (n_max < 1 || n_max > GSR_MCMC_N_MAX)
        return fail(GSR_ERR_ARGUMENT, "mcmc_relocation: n_max = %d (1..%d)", n_max, GSR_MCMC_N_MAX);
    if (P == 0 || n == 0) return GSR_OK;
    if (!opacity || !scaling || !sampled || !scratch || !new_opacity || !new_scaling || !ratio)
        return fail(GSR_ERR_ARGUMENT, "mcmc_relocation: null pointer");
    const hipStream_t s = (hipStream_t)stream;
    int* count = (int*)scratch;
    HIP_TRY(hipMemsetAsync(count, 0, (size_t)P * sizeof(int), s), "mcmc_relocation counts");
    const unsigned blocks = (unsigned)((n + kRelocThreads - 1) / kRelocThreads);
    hipLaunchKernelGGL(mcmc_count_kernel, dim3(blocks), dim3(kRelocThreads), 0, s, P, n, sampled, count);
    hipLaunchKernelGGL(mcmc_relocation_kernel, dim3(blocks), dim3(kRelocThreads), 0, s, P, n, opacity, scaling, sampled,
                       count, n_max, min_opacity, new_opacity, new_scaling, ratio);
    HIP_TRY(hipGetLastError(), "mcmc_relocation");
    return GSR_OK;
}

int gsr_mcmc_apply(int P, int n, const long long* sampled, const long long* dest, const float* new_opacity,
                   const float* new_scaling, const gsr_mcmc_group* groups, int n_groups, void* stream) {
    using namespace gsr;
    clear_error();
    if (P < 0 || n < 0 || n_groups < 0 || n_groups > GSR_MCMC_MAX_GROUPS)
        return fail(GSR_ERR_ARGUMENT, "mcmc_apply: P = %d, n = %d, %d groups (0..%d)", P, n, n_groups,
                    GSR_MCMC_MAX_GROUPS);
    if (P == 0 || n == 0) return GSR_OK;
    if (!sampled || !dest || (n_groups > 0 && !groups)) return fail(GSR_ERR_ARGUMENT, "mcmc_apply: null pointer");
    for (int k = 0; k < n_groups; k++) {  // every group is checked before the first launch
        const gsr_mcmc_group& g = groups[k];
        if (!g.data) return fail(GSR_ERR_ARGUMENT, "mcmc_apply: group %d null array", k);
        if (g.width <= 0 || (unsigned long long)n * (unsigned long long)g.width > 0x7fffffffull)
            return fail(GSR_ERR_ARGUMENT, "mcmc_apply: group %d width %d with %d samples", k, g.width, n);
        if ((g.exp_avg == nullptr) != (g.exp_avg_sq == nullptr))
            return fail(GSR_ERR_ARGUMENT, "mcmc_apply: group %d Adam state pointers must both be given or both be null",
                        k);
        if (g.role < GSR_MCMC_COPY || g.role > GSR_MCMC_SCALING)
            return fail(GSR_ERR_ARGUMENT, "mcmc_apply: group %d role %d", k, g.role);
        if (g.role == GSR_MCMC_OPACITY && (g.width != 1 || !new_opacity))
            return fail(GSR_ERR_ARGUMENT, "mcmc_apply: the opacity group needs width 1 and new_opacity");
        if (g.role == GSR_MCMC_SCALING && (g.width != 3 || !new_scaling))
            return fail(GSR_ERR_ARGUMENT, "mcmc_apply: the scaling group needs width 3 and new_scaling");
    }
    for (int k = 0; k < n_groups; k++) {
        const gsr_mcmc_group& g = groups[k];
        McmcApplyArgs a{};
        a.P = P;
        a.total = (uint32_t)n * (uint32_t)g.width;
        a.width = (uint32_t)g.width;
        a.role = g.role;
        a.sampled = sampled; a.dest = dest;
        a.new_opacity = (const uint32_t*)new_opacity; a.new_scaling = (const uint32_t*)new_scaling;
        a.data = (uint32_t*)g.data; a.m = (uint32_t*)g.exp_avg; a.v = (uint32_t*)g.exp_avg_sq;
        hipLaunchKernelGGL(mcmc_apply_kernel, dim3((a.total + kRelocThreads - 1) / kRelocThreads), dim3(kRelocThreads),
                           0, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError(), "mcmc_apply");
    return GSR_OK;
}

}  // extern "C"
