// densify.hip -- adaptive density control (include/gsr_densify.h).
//
// The reference does this in torch: boolean masks, a dozen index/cat/repeat ops per parameter
// group, fresh allocations for every intermediate, and a host sync per boolean index
// (scene/gaussian_model.py:400-654).  Here it is three passes over the Gaussians:
//
//   plan  (one thread per Gaussian)  decisions -> flag byte, per-block counts of the four
//                                    output sections (kept originals, clones, children, splits)
//   scan  (one workgroup)            exclusive scan of the block counts, section totals
//   index (one thread per Gaussian)  block-local ranks by wave ballots -> each Gaussian's rows
//                                    in the new arrays (int4: kept row, clone row, first child
//                                    row, split rank), or -1
//   apply (one thread per float of a group)  the copies: coalesced reads of the old rows, runs
//                                    of consecutive writes for kept rows; children's xyz and
//                                    scaling computed in flight; new rows' Adam moments zeroed
//
// plan, scan and index are HBM-light (24 B read, 17 B written per Gaussian); apply moves each
// parameter and moment once (HBM-bound).  No atomics: the output order is the reference's
// exactly and the result is bitwise reproducible.
// The C entry points (include/gsr_densify.h) are at the end of the file.
#include "../../include/gsr_densify.h"
#include "host.h"
#include "kernels.h"

namespace gsr {

struct DensifyArgs {
    int P;
    const float* accum;
    const float* denom;
    const float* opacity;
    const float* scaling;
    float grad_threshold, clone_extent, min_opacity, big_extent, split_div;
    int use_screen_size;
    uint8_t* split_mask;  // may be null
    // scratch (densify_carve)
    int4* rows;           // [P] kept row, clone row, first child row, split rank (-1: none)
    uint8_t* flags;       // [P]
    uint32_t* blk;        // [blocks][4] counts, then exclusive offsets
    uint32_t* totals;     // [4] kept, clones, children per copy, splits
};
struct DensifyApplyArgs {
    const uint32_t* src;
    uint32_t* dst;
    const uint32_t* src_m;
    const uint32_t* src_v;
    uint32_t* dst_m;  // null: the group has no Adam state
    uint32_t* dst_v;
    uint32_t n;       // P * width
    uint32_t width;
    unsigned long long magic;  // t / width == (t * magic) >> shift for t < 2^31
    uint32_t shift;
    int role;
    const int4* rows;
    const float* rotation;
    const float* samples;
    uint32_t n_split, n_children;
    int split_n;
    float split_div;
};

constexpr int kDenThreads = 256;
constexpr int kDenWaves = kDenThreads / 64;

enum : uint8_t { kKeepA = 1, kKeepB = 2, kKeepC = 4, kSplit = 8 };

__device__ __forceinline__ float sigmoidf_ref(float x) { return 1.f / (1.f + expf(-x)); }

// ---- train.py:212-215 ---------------------------------------------------------------
__global__ void __launch_bounds__(kDenThreads) densify_stats_kernel(int P, const float* __restrict__ vgrad,
                                                                    const int* __restrict__ radii,
                                                                    const uint8_t* __restrict__ visible,
                                                                    float* __restrict__ accum, float* __restrict__ denom,
                                                                    float* __restrict__ max_r) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kDenThreads + threadIdx.x;
    if (i >= P) return;
    const int r = radii ? radii[i] : 0;
    const bool vis = visible ? visible[i] != 0 : r > 0;
    if (!vis) return;
    if (vgrad) {
        const float gx = vgrad[3 * (size_t)i], gy = vgrad[3 * (size_t)i + 1];
        accum[i] += sqrtf(gx * gx + gy * gy);
        denom[i] += 1.f;
    }
    if (radii && max_r) max_r[i] = fmaxf(max_r[i], (float)r);
}

// ---- plan ---------------------------------------------------------------------------
// The four section flags of one Gaussian (gaussian_model.py:508-640).  A clone has its
// parent's opacity and scaling, and both children of a split share theirs, so one prune test
// each covers every copy.
__device__ __forceinline__ uint8_t densify_flags(float accum, float denom, float opacity, const float* s,
                                                 const DensifyArgs& a) {
#pragma clang fp contract(off)
    float g = accum / denom;
    if (g != g) g = 0.f;  // grads[grads.isnan()] = 0.0
    const float e0 = expf(s[0]), e1 = expf(s[1]), e2 = expf(s[2]);
    const float ms = fmaxf(fmaxf(e0, e1), e2);
    const bool sel = g >= a.grad_threshold;
    const bool clone = sel && ms <= a.clone_extent;
    const bool split = sel && ms > a.clone_extent;
    const bool low_op = sigmoidf_ref(opacity) < a.min_opacity;
    const bool prune_parent = low_op || (a.use_screen_size && ms > a.big_extent);
    bool prune_child = low_op;
    if (a.use_screen_size) {  // the child's scale as the reference re-reads it: exp(log(exp(s) / div))
        const float c0 = expf(logf(e0 / a.split_div)), c1 = expf(logf(e1 / a.split_div)),
                    c2 = expf(logf(e2 / a.split_div));
        prune_child = prune_child || fmaxf(fmaxf(c0, c1), c2) > a.big_extent;
    }
    uint8_t f = 0;
    if (!split && !prune_parent) f |= kKeepA;
    if (clone && !prune_parent) f |= kKeepB;
    if (split && !prune_child) f |= kKeepC;
    if (split) f |= kSplit;
    return f;
}

// Block-wide counts (and exclusive ranks) of the four flag bits: wave ballots, then a scan
// over the block's four waves in LDS.
struct BlockRanks {
    uint32_t rank[4];   // this thread's exclusive rank among the block's set bits
    uint32_t total[4];  // the block's counts
};

__device__ __forceinline__ BlockRanks block_ranks(uint8_t f) {
    __shared__ uint32_t s_cnt[kDenWaves][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    BlockRanks r;
    uint32_t in_wave[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long b = __ballot((f >> k) & 1);
        in_wave[k] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[w][k] = (uint32_t)__popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t before = 0, tot = 0;
        for (int v = 0; v < kDenWaves; v++) {
            const uint32_t c = s_cnt[v][k];
            before += v < w ? c : 0u;
            tot += c;
        }
        r.rank[k] = before + in_wave[k];
        r.total[k] = tot;
    }
    return r;
}

__global__ void __launch_bounds__(kDenThreads) densify_plan_kernel(DensifyArgs a) {
    const int i = blockIdx.x * kDenThreads + threadIdx.x;
    uint8_t f = 0;
    if (i < a.P) {
        f = densify_flags(a.accum[i], a.denom[i], a.opacity[i], a.scaling + 3 * (size_t)i, a);
        a.flags[i] = f;
        if (a.split_mask) a.split_mask[i] = (f & kSplit) ? 1 : 0;
    }
    const BlockRanks r = block_ranks(f);
    if (threadIdx.x < 4) a.blk[(size_t)blockIdx.x * 4 + threadIdx.x] = r.total[threadIdx.x];
}

// One workgroup: exclusive scan of the per-block counts (in place), then the section totals.
__global__ void __launch_bounds__(1024) densify_scan_kernel(uint32_t nblk, uint32_t* __restrict__ blk,
                                                            uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_w[16][4];
    __shared__ uint32_t s_carry[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x < 4) s_carry[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nblk; base += 1024) {
        const uint32_t b = base + threadIdx.x;
        uint32_t v[4], incl[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = b < nblk ? blk[(size_t)b * 4 + k] : 0u;
            incl[k] = v[k];
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t u = __shfl_up(incl[k], off);
                if (lane >= off) incl[k] += u;
            }
            if (lane == 63) s_w[w][k] = incl[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t before = s_carry[k];
            for (int x = 0; x < w; x++) before += s_w[x][k];
            if (b < nblk) blk[(size_t)b * 4 + k] = before + incl[k] - v[k];
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            uint32_t t = 0;
            for (int x = 0; x < 16; x++) t += s_w[x][threadIdx.x];
            s_carry[threadIdx.x] += t;
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) totals[threadIdx.x] = s_carry[threadIdx.x];
}

__global__ void __launch_bounds__(kDenThreads) densify_index_kernel(DensifyArgs a) {
    const int i = blockIdx.x * kDenThreads + threadIdx.x;
    const uint8_t f = i < a.P ? a.flags[i] : (uint8_t)0;
    const BlockRanks r = block_ranks(f);
    if (i >= a.P) return;
    const uint32_t* off = a.blk + (size_t)blockIdx.x * 4;
    const uint32_t nA = a.totals[0], nB = a.totals[1];
    int4 o;
    o.x = (f & kKeepA) ? (int)(off[0] + r.rank[0]) : -1;
    o.y = (f & kKeepB) ? (int)(nA + off[1] + r.rank[1]) : -1;
    o.z = (f & kKeepC) ? (int)(nA + nB + off[2] + r.rank[2]) : -1;  // first split copy; copy k adds k * nC
    o.w = (f & kSplit) ? (int)(off[3] + r.rank[3]) : -1;           // row of this parent's samples
    a.rows[i] = o;
}

// ---- apply --------------------------------------------------------------------------
// Row c of R(q) (utils/general_utils.py:78-99: q normalised, then the reference's element
// formulas) applied to the sample, plus the parent's coordinate: bmm(R, sample) + xyz
// (gaussian_model.py:530).
__device__ __forceinline__ float child_xyz(const float* q4, const float* smp, float xyz, int c) {
#pragma clang fp contract(off)
    const float nrm = sqrtf(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]);
    const float r = q4[0] / nrm, x = q4[1] / nrm, y = q4[2] / nrm, z = q4[3] / nrm;
    float R0, R1, R2;
    if (c == 0) {
        R0 = 1.f - 2.f * (y * y + z * z); R1 = 2.f * (x * y - r * z); R2 = 2.f * (x * z + r * y);
    } else if (c == 1) {
        R0 = 2.f * (x * y + r * z); R1 = 1.f - 2.f * (x * x + z * z); R2 = 2.f * (y * z - r * x);
    } else {
        R0 = 2.f * (x * z - r * y); R1 = 2.f * (y * z + r * x); R2 = 1.f - 2.f * (x * x + y * y);
    }
    const float d = fmaf(R2, smp[2], fmaf(R1, smp[1], R0 * smp[0]));
    return d + xyz;
}

__global__ void __launch_bounds__(kDenThreads) densify_apply_kernel(DensifyApplyArgs a) {
    const uint32_t t = blockIdx.x * kDenThreads + threadIdx.x;
    if (t >= a.n) return;
    const uint32_t i = (uint32_t)(((unsigned long long)t * a.magic) >> a.shift);  // t / width
    const uint32_t c = t - i * a.width;
    const int4 o = a.rows[i];
    const uint32_t v = a.src[t];  // bit copies: int tmp_radii move through here too
    if (o.x >= 0) {
        a.dst[(size_t)o.x * a.width + c] = v;
        if (a.dst_m) {
            a.dst_m[(size_t)o.x * a.width + c] = a.src_m[t];
            a.dst_v[(size_t)o.x * a.width + c] = a.src_v[t];
        }
    }
    if (o.y >= 0) {
        a.dst[(size_t)o.y * a.width + c] = v;
        if (a.dst_m) {
            a.dst_m[(size_t)o.y * a.width + c] = 0u;
            a.dst_v[(size_t)o.y * a.width + c] = 0u;
        }
    }
    if (o.z >= 0) {
        for (int k = 0; k < a.split_n; k++) {
            const size_t row = (size_t)o.z + (size_t)k * a.n_children;
            uint32_t out = v;
            if (a.role == GSR_DENSIFY_XYZ) {
                const float* smp = a.samples + 3 * ((size_t)k * a.n_split + (size_t)o.w);
                out = __float_as_uint(child_xyz(a.rotation + 4 * (size_t)i, smp, __uint_as_float(v), (int)c));
            } else if (a.role == GSR_DENSIFY_SCALING) {
#pragma clang fp contract(off)
                out = __float_as_uint(logf(expf(__uint_as_float(v)) / a.split_div));
            }
            a.dst[row * a.width + c] = out;
            if (a.dst_m) {
                a.dst_m[row * a.width + c] = 0u;
                a.dst_v[row * a.width + c] = 0u;
            }
        }
    }
}

// ---- launchers ----------------------------------------------------------------------
static size_t densify_scratch_bytes(int P) {
    const size_t nblk = ((size_t)P + kDenThreads - 1) / kDenThreads;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    return al((size_t)P * sizeof(int4)) + al((size_t)P) + al(nblk * 4 * sizeof(uint32_t)) + al(4 * sizeof(uint32_t));
}

static void densify_carve(void* scratch, int P, DensifyArgs& a) {
    const size_t nblk = ((size_t)P + kDenThreads - 1) / kDenThreads;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char* p = (char*)scratch;
    a.rows = (int4*)p;
    p += al((size_t)P * sizeof(int4));
    a.flags = (uint8_t*)p;
    p += al((size_t)P);
    a.blk = (uint32_t*)p;
    p += al(nblk * 4 * sizeof(uint32_t));
    a.totals = (uint32_t*)p;
}

static hipError_t launch_densify_stats(int P, const float* vgrad, const int* radii, const uint8_t* visible,
                                       float* accum, float* denom, float* max_r, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(densify_stats_kernel, dim3((P + kDenThreads - 1) / kDenThreads), dim3(kDenThreads), 0, stream,
                       P, vgrad, radii, visible, accum, denom, max_r);
    return hipGetLastError();
}

static hipError_t launch_densify_plan(const DensifyArgs& a, hipStream_t stream) {
    if (a.P <= 0) return hipSuccess;
    const uint32_t nblk = (uint32_t)((a.P + kDenThreads - 1) / kDenThreads);
    hipLaunchKernelGGL(densify_plan_kernel, dim3(nblk), dim3(kDenThreads), 0, stream, a);
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(1024), 0, stream, nblk, a.blk, a.totals);
    hipLaunchKernelGGL(densify_index_kernel, dim3(nblk), dim3(kDenThreads), 0, stream, a);
    return hipGetLastError();
}

static hipError_t launch_densify_apply(const DensifyApplyArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(densify_apply_kernel, dim3((a.n + kDenThreads - 1) / kDenThreads), dim3(kDenThreads), 0,
                       stream, a);
    return hipGetLastError();
}

}  // namespace gsr

// ---- C entry points (include/gsr_densify.h) ----------------------------------------
extern "C" {

int gsr_densify_stats(int P, const float* viewspace_grad, const int* radii, const unsigned char* visible,
                      float* grad_accum, float* denom, float* max_radii2D, void* stream) {
    using namespace gsr;
    clear_error();
    if (P < 0) return fail(GSR_ERR_ARGUMENT, "densify_stats: P must be >= 0");
    if (P == 0) return GSR_OK;
    if (viewspace_grad && (!grad_accum || !denom)) return fail(GSR_ERR_ARGUMENT, "densify_stats: null accumulator");
    if (!viewspace_grad && !(radii && max_radii2D))
        return fail(GSR_ERR_ARGUMENT, "densify_stats: nothing to update");
    if (!radii && !visible) return fail(GSR_ERR_ARGUMENT, "densify_stats: need radii or a visibility mask");
    HIP_TRY(launch_densify_stats(P, viewspace_grad, radii, visible, grad_accum, denom, max_radii2D,
                                 (hipStream_t)stream),
            "densify_stats");
    return GSR_OK;
}

unsigned long long gsr_densify_scratch_bytes(int P) { return P > 0 ? gsr::densify_scratch_bytes(P) : 0ull; }

int gsr_densify_plan(int P, const float* grad_accum, const float* denom, const float* opacity, const float* scaling,
                     const gsr_densify_params* prm, void* scratch, unsigned char* split_mask, long long* counts,
                     void* stream) {
    using namespace gsr;
    clear_error();
    if (!prm || !counts) return fail(GSR_ERR_ARGUMENT, "densify_plan: null params/counts");
    if (P < 0) return fail(GSR_ERR_ARGUMENT, "densify_plan: P must be >= 0");
    for (int k = 0; k < GSR_DENSIFY_NCOUNTS; k++) counts[k] = 0;
    if (P == 0) return GSR_OK;
    if (!grad_accum || !denom || !opacity || !scaling || !scratch)
        return fail(GSR_ERR_ARGUMENT, "densify_plan: null pointer");
    if (prm->split_n < 1 || prm->split_n > 64) return fail(GSR_ERR_ARGUMENT, "densify_plan: split N = %d", prm->split_n);
    DensifyArgs a{};
    a.P = P;
    a.accum = grad_accum; a.denom = denom; a.opacity = opacity; a.scaling = scaling;
    a.grad_threshold = prm->grad_threshold; a.clone_extent = prm->clone_extent; a.min_opacity = prm->min_opacity;
    a.big_extent = prm->big_extent; a.split_div = prm->split_div; a.use_screen_size = prm->use_screen_size;
    a.split_mask = split_mask;
    densify_carve(scratch, P, a);
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_densify_plan(a, s), "densify_plan");
    uint32_t tot[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, a.totals, sizeof(tot), hipMemcpyDeviceToHost, s), "densify_plan counts");
    HIP_TRY(hipStreamSynchronize(s), "densify_plan sync");
    counts[GSR_DENSIFY_KEPT] = tot[0];
    counts[GSR_DENSIFY_CLONES] = tot[1];
    counts[GSR_DENSIFY_CHILDREN] = tot[2];
    counts[GSR_DENSIFY_SPLIT] = tot[3];
    counts[GSR_DENSIFY_TOTAL] = (long long)tot[0] + tot[1] + (long long)prm->split_n * tot[2];
    if (counts[GSR_DENSIFY_TOTAL] > 0x7fffffffLL)
        return fail(GSR_ERR_OVERFLOW, "densify_plan: %lld Gaussians after densification", counts[GSR_DENSIFY_TOTAL]);
    return GSR_OK;
}

int gsr_densify_apply(int P, const void* scratch, const gsr_densify_group* groups, int n_groups,
                      const float* rotation, const float* samples, const int* tmp_radii_in, int* tmp_radii_out,
                      const gsr_densify_params* prm, void* stream) {
    using namespace gsr;
    clear_error();
    if (!prm) return fail(GSR_ERR_ARGUMENT, "densify_apply: null params");
    if (P < 0 || n_groups < 0 || n_groups > GSR_DENSIFY_MAX_GROUPS)
        return fail(GSR_ERR_ARGUMENT, "densify_apply: P = %d, %d groups (0..%d)", P, n_groups, GSR_DENSIFY_MAX_GROUPS);
    if (P == 0) return GSR_OK;
    if (!scratch || (n_groups > 0 && !groups)) return fail(GSR_ERR_ARGUMENT, "densify_apply: null pointer");
    if ((tmp_radii_in == nullptr) != (tmp_radii_out == nullptr))
        return fail(GSR_ERR_ARGUMENT, "densify_apply: tmp_radii in and out must both be given or both be null");
    DensifyArgs d{};
    densify_carve(const_cast<void*>(scratch), P, d);
    const hipStream_t s = (hipStream_t)stream;
    uint32_t tot[4] = {0, 0, 0, 0};  // the plan's totals (a tiny synchronous read; the plan already synchronised)
    HIP_TRY(hipMemcpyAsync(tot, d.totals, sizeof(tot), hipMemcpyDeviceToHost, s), "densify_apply counts");
    HIP_TRY(hipStreamSynchronize(s), "densify_apply sync");
    if ((unsigned long long)tot[0] + tot[1] + (unsigned long long)prm->split_n * tot[2] == 0)
        return GSR_OK;  // everything pruned: the new arrays are empty
    if (tot[3] > 0 && tot[2] > 0 && !samples)
        return fail(GSR_ERR_ARGUMENT, "densify_apply: %u split Gaussians but no samples", tot[3]);
    auto launch = [&](const void* src, void* dst, const void* sm, const void* sv, void* dm, void* dv, int width,
                      int role, const char* what) -> int {
        if (width <= 0) return fail(GSR_ERR_ARGUMENT, "densify_apply: %s width %d", what, width);
        if ((size_t)P * (size_t)width > 0x7fffffffull)
            return fail(GSR_ERR_ARGUMENT, "densify_apply: %s has more than 2^31-1 values", what);
        if (!src || !dst) return fail(GSR_ERR_ARGUMENT, "densify_apply: %s null array", what);
        if ((sm == nullptr) != (dm == nullptr) || (sv == nullptr) != (dv == nullptr) || (sm == nullptr) != (sv == nullptr))
            return fail(GSR_ERR_ARGUMENT, "densify_apply: %s Adam state pointers must all be given or all be null",
                        what);
        if (role == GSR_DENSIFY_XYZ && (width != 3 || !rotation))
            return fail(GSR_ERR_ARGUMENT, "densify_apply: the xyz group needs width 3 and the rotations");
        if (role == GSR_DENSIFY_SCALING && width != 3)
            return fail(GSR_ERR_ARGUMENT, "densify_apply: the scaling group needs width 3");
        if (role < GSR_DENSIFY_COPY || role > GSR_DENSIFY_SCALING)
            return fail(GSR_ERR_ARGUMENT, "densify_apply: %s role %d", what, role);
        DensifyApplyArgs a{};
        a.src = (const uint32_t*)src; a.dst = (uint32_t*)dst;
        a.src_m = (const uint32_t*)sm; a.src_v = (const uint32_t*)sv; a.dst_m = (uint32_t*)dm; a.dst_v = (uint32_t*)dv;
        a.n = (uint32_t)((size_t)P * width);
        a.width = (uint32_t)width;
        uint32_t l = 0;
        while ((1u << l) < a.width) l++;
        a.shift = 31 + l;
        a.magic = ((1ull << a.shift) + a.width - 1) / a.width;  // exact t / width for t < 2^31
        a.role = role;
        a.rows = d.rows;
        a.rotation = rotation;
        a.samples = samples;
        a.n_split = tot[3];
        a.n_children = tot[2];
        a.split_n = prm->split_n;
        a.split_div = prm->split_div;
        HIP_TRY(launch_densify_apply(a, s), "densify_apply");
        return GSR_OK;
    };
    for (int k = 0; k < n_groups; k++) {
        const gsr_densify_group& g = groups[k];
        if (int rc = launch(g.src, g.dst, g.src_exp_avg, g.src_exp_avg_sq, g.dst_exp_avg, g.dst_exp_avg_sq, g.width,
                            g.role, "group"))
            return rc;
    }
    if (tmp_radii_in)
        if (int rc = launch(tmp_radii_in, tmp_radii_out, nullptr, nullptr, nullptr, nullptr, 1, GSR_DENSIFY_COPY,
                            "tmp_radii"))
            return rc;
    return GSR_OK;
}

}  // extern "C"
