// backward.hip -- per-Gaussian backward.
//
//   gauss_reduce_kernel (one lane per Gaussian): sums each Gaussian's
//     per-(tile) gradient records.  They are contiguous per Gaussian and the
//     Gaussians' ranges follow each other, so consecutive lanes read
//     consecutive memory and the sum is deterministic -- no atomics.
//   gauss_bwd_kernel (one wave per 64 Gaussians):
//     - computeCov2DCUDA (CR/backward.cu:153-290) including the tail that the
//       vendored file truncates (dL/dcov3D and dL/dmean3D through the EWA
//       projection, the clamp masks and the inverse-depth term), derived in
//       DESIGN.md "Backward conventions";
//     - preprocessCUDA (CR/backward.cu:372-429): screen-space mean -> 3-D mean,
//       SH colour backward (:12-146) and scale/rotation backward (:296-365).
//     The 64 SH rows of the wave (64 x 192 B when M = 16) are staged through LDS
//     so both the global read of the coefficients and the write of dL/dSH are
//     fully coalesced 16-byte accesses; the SH backward streams one coefficient
//     at a time instead of holding 48 floats in registers.
// Every output row is written, zeros included, so the host never memsets the
// gradient tensors (the reference zero-fills all of them first,
// RI/rasterize_points.cu:186-195).
// The same math over several views' gathered sums (the multi-GPU view exchange) is views.hip.
#include "gauss_bwd_math.h"

namespace gsr {

// ---- 1. segmented sums of the per-instance records ------------------------------
// One wave per 64 consecutive Gaussians.  Their records form one contiguous range
// [E0, E1) (record index = rec_start[g] + k, k = the tile's row-major index in g's
// rectangle).  A record exists iff its content bit is set (render.hip writes records only for
// entries with a gradient term; the bits are zeroed by the forward's K3, binning.hip) -- 5M@4K:
// 7.6M records of 114.7M instances, the rest behind saturated pixels.  Per window of 1024
// positions the positions of the records are compacted into an LDS list (per-lane popcounts of
// the set bits, a wave prefix sum, each lane writing its own positions), and the list is reduced
// 64 RECORDS at a time: at 1M@1080p a wave's ~508 instance positions hold ~80 records, two
// groups.  A Gaussian's records are its slots [r0, r1) of the list (counted from the bits below
// its range start and end); each group is summed by a segmented scan over the wave (DPP row
// shifts and row broadcasts, the add masked where the source lane belongs to another Gaussian),
// which leaves each Gaussian's group total in the last lane of its run, handed to the owner lane
// through LDS.  A fixed order: the result does not depend on scheduling.  The records of a
// window's next group are requested before its current group is reduced, the radius is read at
// the start, and the LDS hand-offs are wave-local (the workgroup is one wave).
constexpr int kRecStride = 12;  // floats per Gaussian in the LDS hand-off of group totals (10 used), 48 B
__device__ __forceinline__ void reduce_sync() {
    wave_lds_sync();
}
__device__ __forceinline__ uint64_t byte_flags(uint64_t x) {  // each nonzero byte -> 0x01, zero -> 0x00
    x |= x >> 4;
    x |= x >> 2;
    x |= x >> 1;
    return x & 0x0101010101010101ull;
}
// ABS: the records' two pad floats hold the absolute screen-space terms (render_bwd ABSGRAD); they are summed
// as values 10 and 11 of the same scan into sd.  With ABS false the code is the one without them.
template <bool ABS>
__device__ __forceinline__ void reduce_records_compact(int P, int g0, const uint32_t* __restrict__ rec_start,
                                                       const uint32_t* __restrict__ tiles_touched,
                                                       const GradRecs& recs, float* s_rec, float4& sa, float4& sb,
                                                       float2& sc, float2& sd) {
    constexpr int NV = ABS ? 12 : 10;
    const int lane = threadIdx.x;
    const int g = g0 + lane;
    const bool valid = g < P;
    const int g_last = min(g0 + 63, P - 1);
    const uint32_t E0 = rec_start[g0];
    const uint32_t E1 = rec_start[g_last] + tiles_touched[g_last];
    const uint32_t n = valid ? tiles_touched[g] : 0u;
    const uint32_t my0 = valid ? rec_start[g] : E1;
    const uint32_t my1 = my0 + n;
    sa = make_float4(0.f, 0.f, 0.f, 0.f);
    sb = sa;
    sc = make_float2(0.f, 0.f);
    sd = sc;
    __shared__ uint16_t s_list[1024];  // the window's record positions, as offsets from its first byte
    __shared__ uint32_t s_mark[64];
    float4* part = reinterpret_cast<float4*>(s_rec);  // [64][3] float4: a Gaussian's group total
    for (uint32_t wa = E0 & ~15u; wa < E1; wa += 1024u) {  // uniform
        // content bytes [wa, wa + 1024): lane l holds wa + 16 l .. + 15, masked to [E0, E1)
        const uint32_t p = wa + 16u * (uint32_t)lane;
        // (flag bits: this lane's 16 positions are half of one 32-bit word, wa being a multiple of 16)
        uint32_t m16 = 0;
        if (p < E1) {
            m16 = (reinterpret_cast<const uint32_t*>(recs.flag)[p >> 5] >> (p & 16u)) & 0xffffu;
            const uint32_t k = E1 - p;  // positions of this lane below E1
            if (k < 16) m16 &= (1u << k) - 1u;
            if (p < E0) m16 &= 0xffffu << (E0 - p);  // (first window, lane 0 only) the previous wave's
        }
        const uint32_t c = (uint32_t)__popc(m16);
        const uint32_t incl = wave_incl_sum(c), off = incl - c;
        const uint32_t R = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);  // records in the window
        if (R == 0) continue;  // uniform
        wave_lds_sync();  // the previous window's readers are done (in-order LDS)
        {
            uint32_t k = off;
            for (uint32_t t = m16; t; t &= t - 1) s_list[k++] = (uint16_t)(16 * lane + __builtin_ctz(t));
        }
        wave_lds_sync();
        auto slots_below = [&](uint32_t q) -> uint32_t {
            const uint32_t d = q <= wa ? 0u : min(q - wa, 1024u);
            const int L = (int)min(d >> 4, 63u);
            const uint32_t offL = (uint32_t)__shfl((int)off, L), mL = (uint32_t)__shfl((int)m16, L);
            const uint32_t b = d - 16u * (uint32_t)L;  // positions of lane L below q (16: all of them)
            return offL + (uint32_t)__popc(mL & (b >= 16 ? 0xffffu : (1u << b) - 1u));
        };
        // (both calls on every lane: slots_below shuffles across lanes, so it must not sit in a branch)
        const uint32_t r0 = slots_below(my0), r1e = slots_below(my1), r1 = n ? r1e : r0;
        const bool mine = r1 > r0;
        // the next group's records are requested before this group is reduced (one latency per window
        // instead of one per group)
        float4 xn = make_float4(0.f, 0.f, 0.f, 0.f), yn = xn;
        float2 zn = make_float2(0.f, 0.f), wn = zn;  // (wn: ABS, the float2 behind c)
        if ((uint32_t)lane < R) {
            const uint32_t e = wa + (uint32_t)s_list[lane];
            xn = recs.a[(size_t)kRecAB * e];
            yn = recs.b[(size_t)kRecAB * e];
            zn = recs.c[(size_t)kRecC * e];
            if (ABS) wn = recs.c[(size_t)kRecC * e + 1];
        }
        for (uint32_t k0 = 0; k0 < R; k0 += 64) {  // uniform: 64 records at a time
            const uint32_t k = k0 + (uint32_t)lane;
            const bool has = k < R;
            const float4 x = xn, y = yn;
            const float2 z = zn, w2 = wn;
            if (k + 64 < R) {
                const uint32_t e = wa + (uint32_t)s_list[k + 64];
                xn = recs.a[(size_t)kRecAB * e];
                yn = recs.b[(size_t)kRecAB * e];
                zn = recs.c[(size_t)kRecC * e];
                if (ABS) wn = recs.c[(size_t)kRecC * e + 1];
            } else {  // (lanes past the window's records: zeros, as unloaded lanes always held)
                xn = yn = make_float4(0.f, 0.f, 0.f, 0.f);
                zn = make_float2(0.f, 0.f);
                wn = zn;
            }
            // owner of slot k: the largest lane with records whose first slot is <= k
            const unsigned long long st = __ballot(mine && r0 < k0);
            const uint32_t carry = st ? 64u - (uint32_t)__clzll((long long)st) : 0u;
            s_mark[lane] = 0u;
            wave_lds_sync();
            if (mine && r0 >= k0 && r0 < k0 + 64) s_mark[r0 - k0] = (uint32_t)lane + 1u;
            wave_lds_sync();
            const uint32_t m = max(wave_incl_max(s_mark[lane]), carry);
            wave_lds_sync();
            const int owner = has && m ? (int)m - 1 : -1;
            const uint32_t o0 = (uint32_t)__shfl((int)r0, owner < 0 ? 0 : owner);
            const int seg0 = has ? (o0 > k0 ? (int)(o0 - k0) : 0) : lane;
            const int r = lane & 15, row = lane >> 4;
            const float m1 = lane - 1 >= seg0 && r >= 1 ? 1.f : 0.f, m2 = lane - 2 >= seg0 && r >= 2 ? 1.f : 0.f,
                        m4 = lane - 4 >= seg0 && r >= 4 ? 1.f : 0.f, m8 = lane - 8 >= seg0 && r >= 8 ? 1.f : 0.f,
                        mb15 = (row & 1) && row * 16 - 1 >= seg0 ? 1.f : 0.f,
                        mb31 = row >= 2 && 31 >= seg0 ? 1.f : 0.f;
            float v[12] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w, z.x, z.y, w2.x, w2.y};
#pragma unroll
            for (int i = 0; i < NV; i++) {
                v[i] = fmaf(dpp_f32<0x111, 0xf, true>(v[i]), m1, v[i]);
                v[i] = fmaf(dpp_f32<0x112, 0xf, true>(v[i]), m2, v[i]);
                v[i] = fmaf(dpp_f32<0x114, 0xf, true>(v[i]), m4, v[i]);
                v[i] = fmaf(dpp_f32<0x118, 0xf, true>(v[i]), m8, v[i]);
                v[i] = fmaf(dpp_f32<0x142, 0xa, false>(v[i]), mb15, v[i]);
                v[i] = fmaf(dpp_f32<0x143, 0xc, false>(v[i]), mb31, v[i]);
            }
            const int next_owner = __shfl_down(owner, 1);
            if (owner >= 0 && (lane == 63 || next_owner != owner)) {  // the run's last lane hands it over
                part[owner * 3 + 0] = make_float4(v[0], v[1], v[2], v[3]);
                part[owner * 3 + 1] = make_float4(v[4], v[5], v[6], v[7]);
                part[owner * 3 + 2] = make_float4(v[8], v[9], ABS ? v[10] : 0.f, ABS ? v[11] : 0.f);
            }
            reduce_sync();
            if (max(r0, k0) < min(r1, k0 + 64)) {  // this Gaussian has records in the group
                const float4 pp = part[lane * 3 + 0], q = part[lane * 3 + 1], ww = part[lane * 3 + 2];
                sa.x += pp.x; sa.y += pp.y; sa.z += pp.z; sa.w += pp.w;
                sb.x += q.x; sb.y += q.y; sb.z += q.z; sb.w += q.w;
                sc.x += ww.x; sc.y += ww.y;
                if (ABS) { sd.x += ww.z; sd.y += ww.w; }
            }
            reduce_sync();
        }
    }
}

template <bool ABS>
__global__ void __launch_bounds__(64) gauss_reduce_kernel(int P, const uint32_t* __restrict__ rec_start,
                                                          const uint32_t* __restrict__ tiles_touched,
                                                          GradRecs recs, GradRecs sums, uint32_t* __restrict__ flags,
                                                          const int* __restrict__ radii,
                                                          const uint8_t* __restrict__ clamped,
                                                          uint32_t* __restrict__ live,
                                                          uint32_t* __restrict__ live_count, uint32_t live_cap,
                                                          float* __restrict__ abs_out) {
    __shared__ __attribute__((aligned(16))) float s_rec[64 * kRecStride];
    const int g = blockIdx.x * 64 + (int)threadIdx.x;
    const int rad = g < P ? radii[g] : 0;  // requested with the range loads, not after the reduction
    float4 sa, sb;
    float2 sc, sd;
    reduce_records_compact<ABS>(P, blockIdx.x * 64, rec_start, tiles_touched, recs, s_rec, sa, sb, sc, sd);
    // the absolute screen-space gradient [P,3]: every row written here (zeros for a Gaussian without records
    // or culled), so it needs no zero fill and gauss_bwd does not touch it on this path
    if (ABS && g < P) store3(abs_out, g, rad > 0 ? sd.x : 0.f, rad > 0 ? sd.y : 0.f, 0.f);
    // a Gaussian with a gradient (gauss_bwd's condition)
    const bool lv = g < P && rad > 0 &&
                    ((sa.x != 0.f) | (sa.y != 0.f) | (sa.z != 0.f) | (sa.w != 0.f) | (sb.x != 0.f) |
                     (sb.y != 0.f) | (sb.z != 0.f) | (sb.w != 0.f) | (sc.x != 0.f) | (sc.y != 0.f));
    // With a live list (single view) gauss_bwd reads the sums of the listed Gaussians only, so the
    // other ~87% (zeros) are not written; a view block (flags) or the dense backward reads every row.
    if (g < P && (!live || flags || lv)) {
        sums.a[g] = sa;
        sums.b[g] = sb;
        sums.c[g] = sc;
    }
    // view-block flag word (gauss_bwd_views_kernel): bit 0 visible, bits 1-3 the SH clamp mask
    if (g < P && flags) flags[g] = (rad > 0 ? 1u : 0u) | ((uint32_t)(clamped[g] & 7u) << 1);
    if (live) {
        // append them to the live list: one atomic per wave; the list order varies from run to run,
        // each entry's result does not
        const unsigned long long m = __ballot(lv);
        if (m) {  // uniform
            const int lane = threadIdx.x;
            const uint32_t shard = blockIdx.x % kLiveShards;
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&live_count[shard * kLiveCntStride], (uint32_t)__popcll(m));
            base = (uint32_t)__shfl((int)base, 0);
            if (lv) live[(size_t)shard * live_cap + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)g;
        }
    }
}

hipError_t launch_gauss_reduce(int P, const GeomState& g, const GradRecs& recs, const GradRecs& sums,
                               uint32_t* flags, const int* radii, uint32_t* live, uint32_t* live_count,
                               hipStream_t stream, float* dL_dmean2D_abs) {
    if (P == 0) return hipSuccess;
    if (dL_dmean2D_abs)
        hipLaunchKernelGGL(gauss_reduce_kernel<true>, dim3((P + 63) / 64), dim3(64), 0, stream, P, g.rec_start,
                           g.tiles_touched, recs, sums, flags, radii, g.clamped, live, live_count,
                           live_list_cap((uint32_t)P), dL_dmean2D_abs);
    else
        hipLaunchKernelGGL(gauss_reduce_kernel<false>, dim3((P + 63) / 64), dim3(64), 0, stream, P, g.rec_start,
                           g.tiles_touched, recs, sums, flags, radii, g.clamped, live, live_count,
                           live_list_cap((uint32_t)P), dL_dmean2D_abs);
    return hipGetLastError();
}

// ---- 1b. atomic backward ----------------------------------------------------------
// render_bwd ("bwd_atomic") added every instance's sums into its Gaussian's accumulator row and set
// the Gaussian's touched bit; gauss_bwd_touched_kernel (section 3) reads the rows of the touched
// Gaussians and restores them to zero, gauss_live_views (views.hip) fills a view block from them.

// ---- 2. the per-Gaussian, per-view gradient math: gauss_bwd_math.h (shared with views.hip) ----

// ---- 3. fused per-Gaussian backward ---------------------------------------------
// (Folding the record sums into this kernel was measured slower: the sums' dependent loads
// then run at this kernel's LDS-limited occupancy.)
// The SH rows go through LDS 32 at a time at the end of the kernel (lanes 0-31, then 32-63): 6.6 KiB
// of LDS per wave instead of 13, twice the waves per CU.
constexpr int kGbShRows = 32;
// Live-list entries per gauss_bwd wave (one per lane).
constexpr int kGbListE = 64;
// LIST: lane i of the grid takes entry i of the live list (the Gaussians with a gradient,
// gauss_reduce); the outputs were zero-filled, so no other row is touched.  At
// 1M@1080p that is ~2000 waves instead of 15625.
// The workgroup is one wave: the SH pass's LDS hand-offs need only the wave's own in-order LDS,
// not __syncthreads, whose fence also waits for every store the wave has issued.
__device__ __forceinline__ void gb_sync() {
    wave_lds_sync();
}
// The rows of one wave: Gaussians g0 + lane (dense), or each lane's idx (LIST; a.P: none).  TOUCHED (the
// atomic backward): the sums are the accumulator rows render_bwd added into, read and zeroed here.
constexpr int kGbShFloats = kGbShRows * kShStride;  // one wave's SH staging (LDS)
// ABS (TOUCHED only): floats 10, 11 of the row are the summed |dL/dmean2D| terms (render_bwd ABSGRAD) and go to
// GaussBwdArgs::dL_dmean2D_abs; a compile-time variant, so the kernels without it are the ones before it.
template <int SH_MODE, bool LIST, bool TOUCHED, bool ABS = false>
__device__ __forceinline__ void gauss_bwd_rows(const GaussBwdArgs& a, const int g0, const int idx, float* s_sh) {
    const int lane = threadIdx.x & 63;
    const int nvalid = min(64, a.P - g0);
    const int M = a.M;

    const ShAddr sh_src{a.shs, a.dc, M};
    const ShGradAddr sh_dst{a.dL_dsh, a.dL_ddc, M};
    constexpr bool kShLate = SH_MODE != kShGlobal;  // the SH backward deferred to the LDS pass at the end
    // deferred SH backward (kShLate): its inputs, and the 3-D mean gradient it adds to
    bool sh_late = false;
    float3 sh_v = make_float3(0.f, 0.f, 0.f), sh_g = sh_v, dmean_late = sh_v;

    const bool valid = idx < a.P;
    // The summed render gradients decide everything below: a Gaussian whose ten sums are all
    // zero -- culled, or visible but behind saturated pixels everywhere (about 86% of a 1M@1080p
    // frame) -- has all-zero parameter gradients, so it only writes zeros: none of its geometry
    // and none of its 192-byte SH row is read.
    float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = sa;
    float2 sc = make_float2(0.f, 0.f);
    int rad = 0;
    if (valid) {
        rad = a.radii[idx];
        if constexpr (TOUCHED) {
            const float4* row = a.acc + (size_t)idx * kAccRow4;
            sa = row[0];
            sb = row[1];
            const float4 c4 = row[2];
            sc = make_float2(c4.x, c4.y);
            // a touched row is a visible Gaussian's; the rows of the others were zero-filled with the dense outputs
            if constexpr (ABS) store3(a.dL_dmean2D_abs, idx, c4.z, c4.w, 0.f);
        } else {  // (record path: gauss_reduce's per-Gaussian sums)
            sa = a.sums.a[idx];
            sb = a.sums.b[idx];
            sc = a.sums.c[idx];
        }
    }
    const bool any_grad = (sa.x != 0.f) | (sa.y != 0.f) | (sa.z != 0.f) | (sa.w != 0.f) | (sb.x != 0.f) |
                          (sb.y != 0.f) | (sb.z != 0.f) | (sb.w != 0.f) | (sc.x != 0.f) | (sc.y != 0.f);
    if constexpr (TOUCHED) {  // the row back to zero for the next backward of the same forward (its sums are read)
        if (valid) {
            float4* row = a.acc + (size_t)idx * kAccRow4;
            row[0] = row[1] = row[2] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const bool visible = valid && rad > 0 && any_grad;
    if (valid && !visible) {
        if (!a.sparse) {  // (sparse: the outputs were zero-filled beforehand)
            store3(a.dL_dmean2D, idx, 0.f, 0.f, 0.f);
            if (a.dL_dconic) reinterpret_cast<float4*>(a.dL_dconic)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
            a.dL_dopacity[idx] = 0.f;
            store3(a.dL_dcolor, idx, 0.f, 0.f, 0.f);
            if (a.dL_dinvdepth) a.dL_dinvdepth[idx] = 0.f;
            store3(a.dL_dmean3D, idx, 0.f, 0.f, 0.f);
            for (int k = 0; k < 6; k++) a.dL_dcov3D[6 * idx + k] = 0.f;
            if (a.dL_dscale) store3(a.dL_dscale, idx, 0.f, 0.f, 0.f);
            if (a.dL_drot) reinterpret_cast<float4*>(a.dL_drot)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (a.dL_dsh || a.dL_ddc) {
            if constexpr (kShLate) {
                // rows zeroed in the SH pass below
            } else if (!a.sparse) {
                const ShGlobal acc{sh_src, sh_dst, idx};
                for (int k = 0; k < M; k++) acc.store(k, make_float3(0.f, 0.f, 0.f));
            }
        }
    }
    if (visible) {
        // ---- summed render gradients of this Gaussian (loaded above): colour, inverse depth,
        // mean2D, opacity, and dL/dconic in the reference's convention (CR/backward.cu:604-606)
        store3(a.dL_dmean2D, idx, sb.x, sb.y, 0.f);
        store3(a.dL_dcolor, idx, sa.x, sa.y, sa.z);
        if (a.dL_dconic) reinterpret_cast<float4*>(a.dL_dconic)[idx] = make_float4(sc.x, sb.w, 0.f, sc.y);
        if (a.dL_dinvdepth) a.dL_dinvdepth[idx] = sa.w;

        // ---- computeCov2DCUDA, the mean chain, SH and scale/rotation (view_backward, one view)
        const ViewCam cam{a.viewmatrix, a.projmatrix, a.campos, a.tan_fovx, a.tan_fovy,
                          a.focal_x,    a.focal_y,    a.antialiasing, a.have_invdepth};
        GaussIn gi;
        gi.have_scales = a.scales != nullptr;
        gi.mean = make_float3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
        gi.sc3 = make_float3(0.f, 0.f, 0.f);
        gi.q = make_float4(1.f, 0.f, 0.f, 0.f);
        if (a.scales) {
            gi.sc3 = make_float3(a.scales[3 * idx], a.scales[3 * idx + 1], a.scales[3 * idx + 2]);
            gi.q = reinterpret_cast<const float4*>(a.rotations)[idx];
        }
        gi.cov3D = a.cov3D_precomp ? a.cov3D_precomp + 6 * idx : nullptr;
        gi.scale_modifier = a.scale_modifier;
        gi.opacity = a.opacities + idx;
        // outputs stored as they are formed; dL/dmean3D waits for a deferred SH pass
        struct Sink {
            const GaussBwdArgs& a;
            int idx;
            bool& sh_late;
            float3 &sh_v, &sh_g, &dmean_late;
            __device__ __forceinline__ void dop(float v) const { a.dL_dopacity[idx] = v; }
            __device__ __forceinline__ void dcov(const float (&d)[6]) const {
                for (int k = 0; k < 6; k++) a.dL_dcov3D[6 * idx + k] = d[k];
            }
            __device__ __forceinline__ void sh_defer(float3 v, float3 g) const {
                sh_late = true;
                sh_v = v;
                sh_g = g;
            }
            // kept in a register and stored by the caller (after the SH pass adds the direction term, when
            // there is one): choosing here between the global store and the local made the compiler select
            // between a global and a private address, and dmean_late lived in scratch memory
            __device__ __forceinline__ void dmean(float3 m) const { dmean_late = m; }
            __device__ __forceinline__ void scale_rot(bool have, float3 ds, float4 dq) const {
                if (have || a.dL_dscale) store3(a.dL_dscale, idx, ds.x, ds.y, ds.z);
                if (have || a.dL_drot) reinterpret_cast<float4*>(a.dL_drot)[idx] = dq;
            }
        } sink{a, idx, sh_late, sh_v, sh_g, dmean_late};
        const bool do_sh = a.shs || a.dc;
        const uint8_t cm = do_sh ? a.geom.clamped[idx] : 0;
        if constexpr (kShLate)
            view_backward<kShDefer>(cam, gi, sa, sb, sc, cm, do_sh, a.D, M, ShLds{nullptr}, sink);
        else
            view_backward<kShNow>(cam, gi, sa, sb, sc, cm, do_sh, a.D, M, ShGlobal{sh_src, sh_dst, idx}, sink);
        if (!sh_late) store3(a.dL_dmean3D, idx, dmean_late.x, dmean_late.y, dmean_late.z);
        if (!do_sh && (a.dL_dsh || a.dL_ddc)) {  // colours precomputed: dL/dSH is zero
            const ShGlobal acc{sh_src, sh_dst, idx};
            for (int k = 0; k < M; k++) acc.store(k, make_float3(0.f, 0.f, 0.f));
        }
    }

    if constexpr (kShLate) {
        // SH backward, half a wave at a time through LDS: coalesced stage-in of 32 rows,
        // their lanes evaluate it in place, coalesced write-back of the 32 dL/dSH rows
        const unsigned long long need = __ballot(sh_late);  // rows whose SH is read at all
        for (int half = 0; half < 2; half++) {
            const int rows = LIST ? kGbShRows : min(kGbShRows, nvalid - half * kGbShRows);
            if (rows <= 0) break;  // wave-uniform
            if constexpr (LIST)  // the lanes' rows, wherever they are
                sh_gather_in<kGbShRows, 64, SH_MODE == kShLdsSplit>(sh_src, sh_late ? idx : -1, half * kGbShRows, s_sh,
                                                                   kShStride, lane);
            else
                sh_stage_in<kGbShRows, 64, SH_MODE == kShLdsSplit>(sh_src, g0 + half * kGbShRows, rows, s_sh,
                                                                  kShStride, lane, need >> (half * kGbShRows));
            gb_sync();
            if ((lane >> 5) == half && idx < a.P) {
                float* row = &s_sh[(lane & 31) * kShStride];
                if (sh_late) {
                    // split layout: pin the view vector here -- otherwise the compiler evaluates the SH
                    // basis ahead of the row gather and the barrier, and the values held across it push
                    // the list kernel to 1-3 waves per SIMD.  (The pin moves no arithmetic: with SLP
                    // vectorisation off and contraction per expression, build.py, both layouts round
                    // alike -- test_separate_sh.)
                    float3 v = sh_v;
                    if constexpr (SH_MODE == kShLdsSplit)
                        asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z));
                    float3 dm = dmean_late;
                    sh_dir_backward(ShLds{row}, a.D, M, v, sh_g, dm);
                    store3(a.dL_dmean3D, idx, dm.x, dm.y, dm.z);
                } else if (!a.sparse || SH_MODE == kShLdsSplit) {  // split: see sh_stage_out
                    for (int k = 0; k < kShRowF; k += 4)
                        *reinterpret_cast<float4*>(&row[k]) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            gb_sync();
            if constexpr (LIST) {
                if (a.dL_dsh || a.dL_ddc)
                    sh_gather_out<kGbShRows, 64, SH_MODE == kShLdsSplit>(sh_dst, sh_late ? idx : -1, half * kGbShRows,
                                                                        s_sh, kShStride, lane);
            } else if (a.dL_dsh || a.dL_ddc) {
                sh_stage_out<kGbShRows, 64, SH_MODE == kShLdsSplit>(sh_dst, g0 + half * kGbShRows, rows, s_sh,
                                                                   kShStride, lane,
                                                                   a.sparse ? need >> (half * kGbShRows) : ~0ull);
            }
            gb_sync();
        }
    }
}

// The live-list grid is sized for the worst case (every Gaussian listed: 64 shards x live_cap / E blocks, 15.7k
// at 1M@1080p, 78k at 5M@4K) while ~2000 blocks have entries; every surplus block is a wave launched to read a
// counter and exit (a grid-strided walk over the virtual blocks measured no better).
template <int SH_MODE, bool LIST = false>
__global__ void __launch_bounds__(64) gauss_bwd_kernel(GaussBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float s_sh[SH_MODE != kShGlobal ? kGbShFloats : 4];
    const int lane = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    if constexpr (LIST) {  // block b: entries [E (b / shards), +E) of shard b % shards, E = kGbListE
        const uint32_t shard = blk % kLiveShards, k0 = (blk / kLiveShards) * kGbListE;
        const uint32_t n = a.live_count[shard * kLiveCntStride];
        if (k0 >= n) return;  // uniform: past the shard's list (the grid is sized for the worst case)
        const int idx = lane < kGbListE && k0 + lane < n ? (int)a.live[(size_t)shard * a.live_cap + k0 + lane] : a.P;
        gauss_bwd_rows<SH_MODE, true, false>(a, (int)blk * 64, idx, s_sh);
    } else {
        gauss_bwd_rows<SH_MODE, false, false>(a, (int)blk * 64, (int)blk * 64 + lane, s_sh);
    }
}

// The atomic backward's per-Gaussian pass (bwd_atomic): a workgroup of kTouchedWaves waves per run of
// consecutive Gaussians reads the run's touched bits (render_bwd set them; cleared as read), lists the touched
// Gaussians in LDS, and wave w runs the live-list backward over list entries [64 w, 64 w + 64) -- the waves
// past the list skip -- with the sums read from, and the rows then zeroed in, the accumulator.  One kernel
// where a gauss_live pass listed the Gaussians into shards and moved their sums to list order for the list
// kernel (1M@1080p -6.8 us per step, 500k -9.3, r7e).  Two waves per workgroup: at 1M@1080p a run of 128
// holds ~17 touched Gaussians, so one wave works while the workgroup holds the LDS of its waves -- against
// four waves per run of 256, gauss_bwd -1.8 / -2.0 us at 1M (r7r, r7s), equal at 500k; one wave per run of
// 64: +6.5 us.
//   RUNS = false: runs of 128, one list of at most 128, no loop (the 1080p frames: ~13% of a 1M view touched).
//   RUNS = true: runs of 128 << touched_shift, sub-run by sub-run of 128 appended to a ring list and flushed
// 128 at a time (and the rest at the end), so the waves stay full where few Gaussians are touched: 5M@4K
// gauss_bwd 120 -> 56 us with runs of 2048 (r7g; 49 us with two waves, r7s).  The loop around the row
// backward costs registers (153 -> 197 VGPRs, combined SH layout) and 3-5 us at 1080p, hence two forms
// ("touched_run", api.hip).
constexpr int kTouchedWaves = 2;
constexpr int kTouchedSub = 64 * kTouchedWaves;  // Gaussians per sub-run (one bit per thread)
constexpr uint32_t kTouchedShiftMax = 5;         // at most 32 sub-runs per workgroup: a touched word per thread
constexpr uint32_t kTouchedRing = 2 * kTouchedSub;
static_assert((kTouchedSub << kTouchedShiftMax) / 32 == kTouchedSub, "one touched word per thread at most");
static_assert(kTouchedRing >= 2 * kTouchedSub, "the ring holds an unflushed rest plus one sub-run");
template <int SH_MODE, bool RUNS, bool ABS = false>
__global__ void __launch_bounds__(64 * kTouchedWaves) gauss_bwd_touched_kernel(GaussBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float s_sh[kTouchedWaves][SH_MODE != kShGlobal ? kGbShFloats : 4];
    __shared__ uint32_t s_list[RUNS ? kTouchedRing : kTouchedSub];
    __shared__ uint32_t s_words[RUNS ? kTouchedSub : 1];
    __shared__ uint32_t s_cnt[kTouchedWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if constexpr (!RUNS) {
        const uint32_t g = blockIdx.x * (uint32_t)kTouchedSub + threadIdx.x;
        const uint32_t w = g < (uint32_t)a.P ? a.touched[g >> 5] : 0u;  // (each word read by 32 lanes)
        const unsigned long long m = __ballot((w >> (lane & 31)) & 1u);
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kTouchedWaves; k++) {
            const uint32_t c = s_cnt[k];
            base += k < wave ? c : 0u;
            total += c;
        }
        if ((m >> lane) & 1ull) s_list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = g;
        if ((lane & 31) == 0 && w) a.touched[g >> 5] = 0u;  // (after the ballot read it)
        __syncthreads();
        const uint32_t k0 = 64u * (uint32_t)wave;
        if (k0 >= total) return;  // uniform per wave
        const int idx = k0 + (uint32_t)lane < total ? (int)s_list[k0 + lane] : a.P;
        gauss_bwd_rows<SH_MODE, true, true, ABS>(a, 0, idx, s_sh[wave]);
    } else {
        const int nsub = 1 << a.touched_shift;
        const uint32_t run0 = blockIdx.x * ((uint32_t)kTouchedSub << a.touched_shift);
        {
            const uint32_t nwords = (uint32_t)(kTouchedSub / 32) << a.touched_shift;
            const uint32_t wi = (run0 >> 5) + threadIdx.x;
            uint32_t w = 0;
            if (threadIdx.x < nwords && wi < ((uint32_t)a.P + 31u) >> 5) {
                w = a.touched[wi];
                if (w) a.touched[wi] = 0u;  // restored for the next backward of the same forward
            }
            s_words[threadIdx.x] = w;
        }
        __syncthreads();
        uint32_t head = 0, tail = 0;  // the ring's listed entries [head, tail) (uniform)
        for (int j = 0; j < nsub; j++) {
            const uint32_t g = run0 + (uint32_t)(j * kTouchedSub) + threadIdx.x;
            const uint32_t w = s_words[j * (kTouchedSub / 32) + (threadIdx.x >> 5)];
            const unsigned long long m = __ballot((w >> (lane & 31)) & 1u);
            if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
            __syncthreads();  // (also: every wave's reads of the ring's last flush are done)
            uint32_t base = 0, total = 0;
#pragma unroll
            for (int k = 0; k < kTouchedWaves; k++) {
                const uint32_t c = s_cnt[k];
                base += k < wave ? c : 0u;
                total += c;
            }
            if ((m >> lane) & 1ull)
                s_list[(tail + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))) % kTouchedRing] = g;
            tail += total;
            __syncthreads();
            // flush: kTouchedSub (128) at a time, and at the last sub-run the rest (tail - head < 2 kTouchedSub
            // here: under kTouchedSub were left, at most kTouchedSub appended -- the ring holds them)
            while (tail - head >= (uint32_t)kTouchedSub || (j == nsub - 1 && tail > head)) {  // uniform
                const uint32_t n = min(tail - head, (uint32_t)kTouchedSub);
                const uint32_t k0 = 64u * (uint32_t)wave;
                if (k0 < n) {  // uniform per wave
                    const int idx = k0 + (uint32_t)lane < n ? (int)s_list[(head + k0 + lane) % kTouchedRing] : a.P;
                    gauss_bwd_rows<SH_MODE, true, true, ABS>(a, 0, idx, s_sh[wave]);
                }
                head += n;
            }
        }
    }
}

// 16-byte stores (1 KiB per wave-instruction) over each range's aligned body, dwords for its
// unaligned head and tail.  A small grid (kFillBlocks workgroups of 256): beside render_bwd
// it should take few wave slots and only the HBM bandwidth render_bwd leaves idle.  The body
// stores are non-temporal (`nt`): 236 MB of zeros written through the caches evicted the
// records and pixel state render_bwd and gauss_reduce re-read (r2zv: render_bwd 298 -> 290 us,
// gauss_reduce 67 -> 63, preprocess 75.6 -> 72, step -19 us; 32 / 64 / 96 / 128 workgroups
// within noise once the stores stream, r2zw).
constexpr uint32_t kFillBlocks = 64;
__global__ void __launch_bounds__(256) zero_fill_kernel(FillArgs f) {
    zero_fill_part(f, (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x,
                   (unsigned long long)gridDim.x * blockDim.x);
}

hipError_t launch_zero_fill(const FillArgs& f, hipStream_t stream) {
    if (f.count == 0) return hipSuccess;
    hipLaunchKernelGGL(zero_fill_kernel, dim3(kFillBlocks), dim3(256), 0, stream, f);
    return hipGetLastError();
}

hipError_t launch_gauss_bwd(const GaussBwdArgs& a, hipStream_t stream) {
    if (a.P == 0) return hipSuccess;
    const dim3 grid((a.P + 63) / 64), block(64);
    const bool lds_ok = a.shs && a.dL_dsh && a.M == 16 && (!a.dc || a.dL_ddc) &&
                        ((reinterpret_cast<uintptr_t>(a.shs) & 15) == 0) &&
                        ((reinterpret_cast<uintptr_t>(a.dL_dsh) & 15) == 0);
    if (a.touched) {  // the atomic backward: runs of touched Gaussians (outputs zero-filled)
        if (a.touched_shift > kTouchedShiftMax) return hipErrorInvalidValue;
        const size_t run = (size_t)kTouchedSub << a.touched_shift;
        const dim3 tgrid((uint32_t)(((size_t)a.P + run - 1) / run)), tblock(64 * kTouchedWaves);
        const bool runs = a.touched_shift > 0;
        void (*k)(GaussBwdArgs);
        if (a.dL_dmean2D_abs) {
            if (lds_ok && a.dc)
                k = runs ? gauss_bwd_touched_kernel<kShLdsSplit, true, true>
                         : gauss_bwd_touched_kernel<kShLdsSplit, false, true>;
            else if (lds_ok)
                k = runs ? gauss_bwd_touched_kernel<kShLdsCombined, true, true>
                         : gauss_bwd_touched_kernel<kShLdsCombined, false, true>;
            else
                k = runs ? gauss_bwd_touched_kernel<kShGlobal, true, true> : gauss_bwd_touched_kernel<kShGlobal, false, true>;
        } else if (lds_ok && a.dc)
            k = runs ? gauss_bwd_touched_kernel<kShLdsSplit, true> : gauss_bwd_touched_kernel<kShLdsSplit, false>;
        else if (lds_ok)
            k = runs ? gauss_bwd_touched_kernel<kShLdsCombined, true> : gauss_bwd_touched_kernel<kShLdsCombined, false>;
        else
            k = runs ? gauss_bwd_touched_kernel<kShGlobal, true> : gauss_bwd_touched_kernel<kShGlobal, false>;
        hipLaunchKernelGGL(k, tgrid, tblock, 0, stream, a);
        return hipGetLastError();
    }
    if (a.live && a.sparse) {  // the live list: kLiveShards x live_cap entries at most
        const uint32_t worst = kLiveShards * ((a.live_cap + kGbListE - 1) / kGbListE);
        const dim3 lgrid(worst);
        if (lds_ok && a.dc)
            hipLaunchKernelGGL((gauss_bwd_kernel<kShLdsSplit, true>), lgrid, block, 0, stream, a);
        else if (lds_ok)
            hipLaunchKernelGGL((gauss_bwd_kernel<kShLdsCombined, true>), lgrid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((gauss_bwd_kernel<kShGlobal, true>), lgrid, block, 0, stream, a);
        return hipGetLastError();
    }
    const bool lds = a.shs && a.dL_dsh && a.M == 16 && (!a.dc || a.dL_ddc) &&
                     ((reinterpret_cast<uintptr_t>(a.shs) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(a.dL_dsh) & 15) == 0);
    if (lds && a.dc)
        hipLaunchKernelGGL(gauss_bwd_kernel<kShLdsSplit>, grid, block, 0, stream, a);
    else if (lds)
        hipLaunchKernelGGL(gauss_bwd_kernel<kShLdsCombined>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(gauss_bwd_kernel<kShGlobal>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace gsr
