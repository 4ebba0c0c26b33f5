// adam.hip -- the sparse Adam step of SparseGaussianAdam (include/gsr_adam.h).
//
// Semantics: the 3DGS-accel rasterizer's adamUpdate (not vendored by the reference;
// SURVEY.md section 8f row 3).  Per element i < N*M of a parameter tensor, if Gaussian
// i / M is visible: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g g; p += -lr m / (sqrt(v) + eps).
//
// MI355X structure: the step is a pure stream over param, grad, exp_avg and exp_avg_sq
// (16 B read + 12 B written per visible element, nothing for an invisible one), so it is
// HBM-bound and the kernel is organised for that alone:
//  * all parameter groups of one optimizer step (xyz, f_dc, f_rest, opacity, scaling,
//    rotation: scene/gaussian_model.py:235-242) in ONE launch -- each group owns a
//    contiguous range of workgroups, found by a wave-uniform scan of <= 8 bounds;
//  * 16-byte loads and stores of four consecutive elements; a float4 whose four
//    Gaussians are all invisible issues no memory access at all;
//  * element -> Gaussian by a multiply-shift division (exact for i < 2^31, magic number
//    from the host), so the per-element visibility lookup costs a v_mad_u64_u32.
// The C entry points (include/gsr_adam.h) are at the end of the file.
#include "../../include/gsr_adam.h"
#include "host.h"
#include "kernels.h"

namespace gsr {

constexpr int kAdamMaxGroups = 8;  // GSR_ADAM_MAX_GROUPS
struct AdamGroupDev {
    float* p;
    const float* g;
    float* m;
    float* v;
    uint32_t n;                // N * M
    uint32_t M;
    unsigned long long magic;  // i / M == (i * magic) >> shift for i < 2^31
    uint32_t shift;
    float lr, eps;
    uint32_t first_block;      // first workgroup of this group
    int vec;                   // all four arrays 16-byte aligned
};
struct AdamArgs {
    AdamGroupDev grp[kAdamMaxGroups];
    int n_groups;
    const uint8_t* vis;
    float b1, b2;
};
constexpr int kAdamThreads = 256;
constexpr int kAdamUnroll = 2;  // float4s per thread
constexpr uint32_t kAdamBlockElems = kAdamThreads * kAdamUnroll * 4;

__device__ __forceinline__ uint32_t gauss_of(uint32_t i, const AdamGroupDev& G) {
    return (uint32_t)(((unsigned long long)i * G.magic) >> G.shift);
}

// One element, in the reference's operation order, without contraction into FMAs.
__device__ __forceinline__ float adam_elem(float p, float g, float& m, float& v, float lr, float b1, float b2,
                                           float eps) {
#pragma clang fp contract(off)
    m = b1 * m + (1.0f - b1) * g;
    v = b2 * v + (1.0f - b2) * g * g;
    const float step = -lr * m / (sqrtf(v) + eps);
    return p + step;
}

__global__ void __launch_bounds__(kAdamThreads) adam_kernel(AdamArgs a) {
    int k = 0;
    while (k + 1 < a.n_groups && blockIdx.x >= a.grp[k + 1].first_block) k++;  // wave-uniform
    const AdamGroupDev& G = a.grp[k];
    const uint32_t base = (blockIdx.x - G.first_block) * kAdamBlockElems;
    if (G.vec) {
#pragma unroll
        for (int u = 0; u < kAdamUnroll; u++) {
            const uint32_t e = base + (u * kAdamThreads + threadIdx.x) * 4;
            if (e + 3 < G.n) {
                bool vis[4];
                bool any = false;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    vis[c] = a.vis[gauss_of(e + c, G)] != 0;
                    any |= vis[c];
                }
                if (!any) continue;
                float4 p = *reinterpret_cast<const float4*>(G.p + e);
                const float4 g = *reinterpret_cast<const float4*>(G.g + e);
                float4 m = *reinterpret_cast<const float4*>(G.m + e);
                float4 v = *reinterpret_cast<const float4*>(G.v + e);
                if (vis[0]) p.x = adam_elem(p.x, g.x, m.x, v.x, G.lr, a.b1, a.b2, G.eps);
                if (vis[1]) p.y = adam_elem(p.y, g.y, m.y, v.y, G.lr, a.b1, a.b2, G.eps);
                if (vis[2]) p.z = adam_elem(p.z, g.z, m.z, v.z, G.lr, a.b1, a.b2, G.eps);
                if (vis[3]) p.w = adam_elem(p.w, g.w, m.w, v.w, G.lr, a.b1, a.b2, G.eps);
                *reinterpret_cast<float4*>(G.p + e) = p;
                *reinterpret_cast<float4*>(G.m + e) = m;
                *reinterpret_cast<float4*>(G.v + e) = v;
            } else {
                for (uint32_t i = e; i < G.n && i < e + 4; i++) {  // the group's last 1-3 elements
                    if (!a.vis[gauss_of(i, G)]) continue;
                    float m = G.m[i], v = G.v[i];
                    G.p[i] = adam_elem(G.p[i], G.g[i], m, v, G.lr, a.b1, a.b2, G.eps);
                    G.m[i] = m;
                    G.v[i] = v;
                }
            }
        }
    } else {
        for (uint32_t j = threadIdx.x; j < kAdamBlockElems; j += kAdamThreads) {
            const uint32_t i = base + j;
            if (i >= G.n || !a.vis[gauss_of(i, G)]) continue;
            float m = G.m[i], v = G.v[i];
            G.p[i] = adam_elem(G.p[i], G.g[i], m, v, G.lr, a.b1, a.b2, G.eps);
            G.m[i] = m;
            G.v[i] = v;
        }
    }
}

static hipError_t launch_adam(const AdamArgs& a, uint32_t blocks, hipStream_t stream) {
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(kAdamThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace gsr

// ---- SparseGaussianAdam's step (include/gsr_adam.h) -------------------------------
static_assert(GSR_ADAM_MAX_GROUPS == gsr::kAdamMaxGroups, "group table size");

static int adam_launch(const gsr_adam_group* groups, int n_groups, const unsigned char* visible, int N, float b1,
                       float b2, void* stream) {
    using namespace gsr;
    clear_error();
    if (n_groups < 0 || n_groups > GSR_ADAM_MAX_GROUPS)
        return fail(GSR_ERR_ARGUMENT, "adam_update: %d parameter groups (0..%d)", n_groups, GSR_ADAM_MAX_GROUPS);
    if (N < 0) return fail(GSR_ERR_ARGUMENT, "adam_update: N must be >= 0");
    if (N == 0 || n_groups == 0) return GSR_OK;
    if (!visible || !groups) return fail(GSR_ERR_ARGUMENT, "adam_update: null pointer");
    AdamArgs a{};
    a.vis = visible;
    a.b1 = b1;
    a.b2 = b2;
    uint32_t blocks = 0;
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    for (int k = 0; k < n_groups; k++) {
        const gsr_adam_group& s = groups[k];
        if (s.M <= 0 || s.numel != (long long)N * s.M)
            return fail(GSR_ERR_ARGUMENT, "adam_update: group %d has %lld values, expected N*M = %d*%d", k, s.numel, N,
                        s.M);
        if (s.numel > 0x7fffffffLL)
            return fail(GSR_ERR_ARGUMENT, "adam_update: group %d has more than 2^31-1 values", k);
        if (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq)
            return fail(GSR_ERR_ARGUMENT, "adam_update: group %d has a null parameter/state pointer", k);
        AdamGroupDev& G = a.grp[a.n_groups++];
        G.p = s.param; G.g = s.grad; G.m = s.exp_avg; G.v = s.exp_avg_sq;
        G.n = (uint32_t)s.numel;
        G.M = (uint32_t)s.M;
        uint32_t l = 0;
        while ((1u << l) < G.M) l++;
        G.shift = 31 + l;
        G.magic = ((1ull << G.shift) + G.M - 1) / G.M;  // ceil(2^(31+l) / M): exact i / M for i < 2^31
        G.lr = s.lr;
        G.eps = s.eps;
        G.first_block = blocks;
        G.vec = al16(s.param) && al16(s.grad) && al16(s.exp_avg) && al16(s.exp_avg_sq);
        blocks += (G.n + kAdamBlockElems - 1) / kAdamBlockElems;
    }
    HIP_TRY(launch_adam(a, blocks, (hipStream_t)stream), "adam_update");
    return GSR_OK;
}

extern "C" {

int gsr_adam_update(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const unsigned char* visible,
                    float lr, float b1, float b2, float eps, int N, int M, void* stream) {
    const gsr_adam_group g{param, grad, exp_avg, exp_avg_sq, (long long)N * M, M, lr, eps};
    return adam_launch(&g, 1, visible, N, b1, b2, stream);
}

int gsr_adam_update_multi(const gsr_adam_group* groups, int n_groups, const unsigned char* visible, int N, float b1,
                          float b2, void* stream) {
    return adam_launch(groups, n_groups, visible, N, b1, b2, stream);
}

}  // extern "C"
