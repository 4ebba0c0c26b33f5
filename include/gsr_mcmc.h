/*
 * gsr_mcmc.h -- C ABI of 3DGS-MCMC density control on MI355X (gfx950).
 *
 * "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024) keeps a fixed budget
 * of Gaussians: dead ones (opacity at or below a threshold) are relocated onto live ones, the set
 * grows a few percent at a time up to a cap, and opacity-gated noise is added to every position on
 * every iteration.  The reference has no such code; these entry points are specified here.  Below,
 * o = sigmoid(opacity_raw), s = exp(scaling_raw), q = the raw quaternion (normalised as the
 * children's rotation of gsr_densify_apply is).
 *
 *   gsr_mcmc_noise       <- every iteration, in place, one fused float32 kernel:
 *                             gate_i = 1 / (1 + exp(GATE_K * (o_i - GATE_X0)))
 *                             Sigma_i = R(q_i) diag(s_i^2) R(q_i)^T
 *                             xyz_i += Sigma_i * (xi_i * gate_i * noise_scale)
 *                           (the gate is the paper's sigmoid(100 * ((1 - o) - 0.995)) without 1 - o,
 *                           which float32 cannot form near o = 0).  68 B of traffic per Gaussian.
 *   gsr_mcmc_relocation  <- the opacity and scale n sampled sources and their n new copies share:
 *                             count[i] = how many j have sampled[j] == i       (integer atomics)
 *                             N_j      = min(count[sampled[j]] + 1, n_max)     (returned as ratio[j])
 *                             x_j      = 1 - (1 - o)^(1 / N_j)
 *                             den_j    = sum_{i=1..N_j} sum_{k=0..i-1} C(i-1,k) (-1)^k x_j^(k+1) / sqrt(k+1)
 *                             new_opacity_raw_j = logit(clamp(x_j, min_opacity, 1 - FLT_EPSILON))
 *                             new_scaling_raw_j = scaling_raw[sampled[j]] + log(o / den_j)   (three axes)
 *                           The float32 inputs are widened on load, everything is float64 and rounds once
 *                           on store; the double sum is evaluated as the equal single sum
 *                           sum_{k=0..N-1} C(N,k+1) (-1)^k x^(k+1) / sqrt(k+1) (hockey-stick identity).
 *   gsr_mcmc_apply       <- the row surgery, in place, per parameter group: row dest[j] becomes a bit
 *                           copy of row sampled[j]; the OPACITY and SCALING groups take the relocation's
 *                           values at both dest[j] and sampled[j]; exp_avg and exp_avg_sq become zero at
 *                           sampled[j]; rows dest[j] keep the moments they hold.  No value is both read
 *                           and written: sampled and dest must be disjoint, dest distinct.
 *
 * Growth is the same surgery on arrays the caller has already extended by n rows (old rows copied,
 * the new rows' moments zeroed), with dest = P .. P + n - 1.
 *
 * The random draws (xi, the multinomial samples) are the caller's.  All pointers are device pointers
 * to contiguous arrays; work is enqueued on `stream` (hipStream_t) and nothing synchronises.  P == 0
 * or n == 0 returns 0 without a launch.  Returns 0 or a GSR_ERR_* code (include/gsr.h).
 */
#ifndef GSR_MCMC_H_INCLUDED
#define GSR_MCMC_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_MCMC_MAX_GROUPS 8
#define GSR_MCMC_N_MAX 51       /* largest n_max: C(51, k) is exact in double */
#define GSR_MCMC_GATE_K 100.0f
#define GSR_MCMC_GATE_X0 0.005f

/* what a parameter group's rows at dest[j] (and, for the last two, at sampled[j]) become */
#define GSR_MCMC_COPY 0    /* row sampled[j] (xyz, f_dc, f_rest, rotation) */
#define GSR_MCMC_OPACITY 1 /* new_opacity_raw[j]; width 1 */
#define GSR_MCMC_SCALING 2 /* new_scaling_raw[j]; width 3 */

typedef struct gsr_mcmc_group {
    float* data;       /* [P][width], edited in place */
    float* exp_avg;    /* Adam moments [P][width], or NULL when the group has no state yet */
    float* exp_avg_sq; /* NULL iff exp_avg is NULL */
    int width;         /* floats per Gaussian */
    int role;          /* GSR_MCMC_COPY / _OPACITY / _SCALING */
} gsr_mcmc_group;

/* xyz [P][3] in/out; opacity [P] raw; scaling [P][3] raw; rotation [P][4] raw; xi [P][3] standard
   normal draws; noise_scale = noise_lr * xyz_lr.  xyz, scaling, rotation and xi must be 16-byte
   aligned (whole allocations are). */
int gsr_mcmc_noise(int P, float* xyz, const float* opacity, const float* scaling, const float* rotation,
                   const float* xi, float noise_scale, void* stream);

/* device scratch of gsr_mcmc_relocation (the per-Gaussian counts) */
unsigned long long gsr_mcmc_scratch_bytes(int P);

/* opacity [P] raw, scaling [P][3] raw; sampled [n] int64 in [0, P), duplicates expected (an index
   outside the range is skipped and leaves its outputs unwritten); 1 <= n_max <= GSR_MCMC_N_MAX;
   out: new_opacity [n], new_scaling [n][3], ratio [n] int. */
int gsr_mcmc_relocation(int P, int n, const float* opacity, const float* scaling, const long long* sampled,
                        int n_max, float min_opacity, void* scratch, float* new_opacity, float* new_scaling,
                        int* ratio, void* stream);

/* sampled, dest [n] int64 in [0, P), disjoint, dest distinct (the caller checks; an index outside the
   range is skipped); new_opacity [n] and new_scaling [n][3] as gsr_mcmc_relocation wrote them. */
int gsr_mcmc_apply(int P, int n, const long long* sampled, const long long* dest, const float* new_opacity,
                   const float* new_scaling, const gsr_mcmc_group* groups, int n_groups, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_MCMC_H_INCLUDED */
