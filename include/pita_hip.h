/*
 * pita_hip.h -- C ABI of libpita_hip.so: MI355X (gfx950) kernels for the inference-time
 * annealed reverse-SDE sampling path of PITA (taraak/pita).
 *
 * The reference has no FFI (it is 100% Python); its "plugin API" is the Python classes
 * WeightedSDEIntegrator / VEReverseSDE / ScoreNet / EGNN_dynamics / MyMLP /
 * LennardJonesEnergy / GMM / Prior.  pita_amd/ mirrors those classes and binds the entry
 * points below through ctypes (INTEGRATION.md shows the binding).  Each entry point cites
 * the reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer named x/out/logp/force/... is a DEVICE pointer owned by the caller
 *     (torch tensors); the library never allocates per call and never synchronises;
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it;
 *   - walker-major row-major layout [B, D] with D = n_particles * n_dim, fp32, exactly the
 *     reference's tensor layout (no transposes at the boundary);
 *   - every function returns 0 on success or a negative PITA_E* code; pita_last_error()
 *     gives the message.  Nothing throws, nothing aborts;
 *   - handles (pita_egnn_t, pita_mlp_t, pita_ff_t) live on the device that was current when they were
 *     created; calls that take an EGNN handle make that device current for their duration (its scratch
 *     buffers -- reverse-mode checkpoints, the f16 path's walker backup, divergence marks, the primal
 *     cache -- grow on demand on THAT device) and restore the caller's.  A handle's scratch is shared by
 *     its launches: use one handle from ONE stream at a time (one handle per stream for concurrency).
 */
#ifndef PITA_HIP_H
#define PITA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PITA_ABI_VERSION 13

enum {
  PITA_OK = 0,
  PITA_EINVAL = -1,      /* bad argument (null pointer, unsupported shape ...) */
  PITA_EUNSUPPORTED = -2,/* configuration the HIP path does not implement */
  PITA_EHIP = -3,        /* a HIP runtime call failed */
  PITA_ENOMEM = -4
};

int pita_abi_version(void);
/* copies the calling thread's last error message into buf (NUL terminated); returns its length */
int pita_last_error(char* buf, size_t buflen);
/* number of visible HIP devices, or a negative error */
int pita_device_count(void);

/* ---------------------------------------------------------------- target energies (K1-K3)
 * All return log-density = -E/T (the reference convention, base_energy_function.py:149) and,
 * when force != NULL, force = d logp / dx.
 * Accepted shapes of the pair targets and their fused descents: 2 <= n_particles <= 256, n_dim 1, 2 or 3 (else
 * PITA_EINVAL); every one of them is served (LJ13, LJ55 and DW4 by kernels of their own).  B = 0 returns PITA_OK and
 * touches nothing.
 */

/* Lennard-Jones cluster + harmonic oscillator.
 * replaces LennardJonesEnergy.__call__ (pita/src/energies/lennardjones_energy.py:213-227),
 * LennardJonesPotential._energy/_log_prob (:121-155) and bgflow's distance_vectors /
 * distances_from_vectors (r = sqrt(|dx|^2 + dist_eps)); ordered pairs (each pair twice). */
int pita_lj_logp_force(const float* x, float* logp, float* force /*nullable*/, int64_t B,
                       int n_particles, int n_dim, float temperature, float energy_factor,
                       float dist_eps, float eps, float rm, float osc_scale, void* stream);

/* The same target with the reference's smooth core (LennardJonesEnergy(smooth=True),
 * pita/src/energies/lennardjones_energy.py:39-54,114-119,131-133): for r < range_min the pair energy is the first
 * interval of the cubic spline fitted to the LJ curve on [range_min, range_max] -- coef4 = its four coefficients
 * (host memory; scipy CubicSpline(...).c[:, 0] as the reference computes them), evaluated as
 * c0 u^3 + c1 u^2 + c2 u + c3 with u = r - range_min.  The force is the analytic derivative of that expression. */
int pita_lj_smooth_logp_force(const float* x, float* logp, float* force /*nullable*/, int64_t B,
                              int n_particles, int n_dim, float temperature, float energy_factor,
                              float dist_eps, float eps, float rm, float osc_scale, float range_min,
                              const float* coef4, void* stream);

/* DW4-style multi double well  E = sum_{i<j} a (d-d0)^4 + b (d-d0)^2 + c.
 * Not present in the reference tree (only a dead import, base_datamodule.py:13); formula of
 * bgflow.MultiDoubleWellPotential. */
int pita_dw_logp_force(const float* x, float* logp, float* force /*nullable*/, int64_t B,
                       int n_particles, int n_dim, float temperature, float a, float b, float c,
                       float d0, void* stream);

/* Fused descent on the target: nsteps of  x <- remove_mean(x + F(x) dt + (noise_scale xi) sqrt_dt)  in one launch,
 * walkers resident in LDS throughout.  replaces WeightedSDEIntegrator.negative_time_descent
 * (pita/src/models/components/sde_integration.py:353-360): dt = dt_negative_time, noise_scale = 1 and
 * sqrt_dt = sqrt(2 dt) when do_langevin, else noise_scale = 0.  Bit-identical to pita_*_logp_force followed by
 * pita_em_step, step after step.  noise: nullable device [nsteps, B, n*d]; NULL -> Philox keyed
 * (seed, walker_offset + walker, step0 + s, particle). */
int pita_lj_descent(float* x, const float* noise, int64_t B, int n_particles, int n_dim, float temperature,
                    float energy_factor, float dist_eps, float eps, float rm, float osc_scale, int nsteps, float dt,
                    float noise_scale, float sqrt_dt, uint64_t seed, uint64_t walker_offset, int64_t step0,
                    int remove_mean, void* stream);
int pita_dw_descent(float* x, const float* noise, int64_t B, int n_particles, int n_dim, float temperature, float a,
                    float b, float c, float d0, int nsteps, float dt, float noise_scale, float sqrt_dt, uint64_t seed,
                    uint64_t walker_offset, int64_t step0, int remove_mean, void* stream);

/* Fused MALA chain on a pair target: all nsteps of metropolis_hastings_mala / _adaptive
 * (pita/src/models/components/sde_integration.py:28-45,362-470) in fused launches, walkers resident on chip; bit-identical
 * to pita_*_logp_force + pita_mala_propose + pita_*_logp_force + pita_mala_accept + pita_mala_adapt step after step.
 * pita_lj_mala: LJ13 and LJ55; pita_dw_mala: DW4.  x [B, n*d] and logp [B] (log-density of x on entry) are updated in
 * place; dt_dev holds the step size (adapted in place when adaptive != 0, against the acceptance rate over `total` walkers
 * -- this rank's B: with several ranks the global rate needs the launch-per-kernel path); rates_out [nsteps] receives the
 * acceptance rates.  noise [nsteps, B, n*d] / uniforms [nsteps, B] nullable -> Philox keyed (seed, walker key, step0 + s,
 * particle / 0xFFFFF), walker key = walker_ids[w] or walker_offset + w.  workspace: 8-byte aligned device scratch of
 * pita_lj_mala_workspace_bytes(nsteps) bytes.
 * A non-adaptive chain is ONE launch with the walkers resident on chip over all steps.  An adaptive chain is one launch
 * per step: the order of the stream is what lets a step see the acceptance count of the step before, and every launch
 * derives its step size on the device from dt_dev[0] and the counts so far (no host synchronisation).  There is no
 * grid-wide barrier and no wait inside the kernels, so these entry points cannot time out: they have no NaN result and
 * no rerun protocol, and the device need not be idle. */
size_t pita_lj_mala_workspace_bytes(int nsteps);
int pita_lj_mala(float* x, float* logp, const float* noise /*nullable*/, const float* uniforms /*nullable*/, int64_t B,
                 int n_particles, int n_dim, float temperature, float energy_factor, float dist_eps, float eps, float rm,
                 float osc_scale, int nsteps, double* dt_dev, int adaptive, int64_t total, uint64_t seed,
                 uint64_t walker_offset, const int64_t* walker_ids /*nullable*/, int64_t step0, int remove_mean,
                 float* rates_out /*nullable*/, void* workspace, void* stream);
int pita_dw_mala(float* x, float* logp, const float* noise /*nullable*/, const float* uniforms /*nullable*/, int64_t B,
                 int n_particles, int n_dim, float temperature, float a, float b, float c, float d0, int nsteps,
                 double* dt_dev, int adaptive, int64_t total, uint64_t seed, uint64_t walker_offset,
                 const int64_t* walker_ids /*nullable*/, int64_t step0, int remove_mean, float* rates_out /*nullable*/,
                 void* workspace, void* stream);

/* The same chains with one step size, one acceptance count and one adaptation PER POPULATION, for batches that are n_pop
 * independent populations of pop_size consecutive Philox walker keys (WeightedSDEIntegrator(populations=P,
 * mcmc_per_population=True)).  Population of row w: (key - pop_base) / pop_size with key = walker_ids[w] or
 * walker_offset + w and pop_base the key of the first row of the call's first population; the caller guarantees
 * 0 <= population < n_pop (device ids cannot be checked without a host read).  In place of `total`: totals (device
 * int64 [n_pop]: the walkers each population's rates are taken over, i.e. its rows in this call).  dt_dev is fp64 [n_pop]
 * (in: step sizes, out: final step sizes), rates_out fp32 [nsteps, n_pop], workspace 8-byte aligned device scratch of
 * pita_mala_pop_workspace_bytes(nsteps, n_pop) bytes (one size function for the pair targets and the force field).
 * A population's walkers, rates and final step size are bit-identical to pita_*_mala on that population's rows alone
 * (total = its row count); a population with totals[p] == 0 keeps dt_dev[p] and gets NaN rates.  Launches as above: one
 * for a non-adaptive chain, one per step for an adaptive one, no grid-wide barrier, no wait; every walker replays the
 * adaptation of its own population, and a block's count is split by population before it reaches memory (integer adds).
 * dt_dev, totals, workspace non-null, B >= 0, nsteps >= 0, n_pop >= 1, pop_size >= 1 and the workspace alignment are
 * checked before any device call (PITA_EINVAL); geometries without a fused chain answer PITA_EUNSUPPORTED as above. */
size_t pita_mala_pop_workspace_bytes(int nsteps, int n_pop);
int pita_lj_mala_pop(float* x, float* logp, const float* noise /*nullable*/, const float* uniforms /*nullable*/, int64_t B,
                     int n_particles, int n_dim, float temperature, float energy_factor, float dist_eps, float eps,
                     float rm, float osc_scale, int nsteps, double* dt_dev, int adaptive, const int64_t* totals, int n_pop,
                     int64_t pop_size, uint64_t pop_base, uint64_t seed, uint64_t walker_offset,
                     const int64_t* walker_ids /*nullable*/, int64_t step0, int remove_mean,
                     float* rates_out /*nullable*/, void* workspace, void* stream);
int pita_dw_mala_pop(float* x, float* logp, const float* noise /*nullable*/, const float* uniforms /*nullable*/, int64_t B,
                     int n_particles, int n_dim, float temperature, float a, float b, float c, float d0, int nsteps,
                     double* dt_dev, int adaptive, const int64_t* totals, int n_pop, int64_t pop_size, uint64_t pop_base,
                     uint64_t seed, uint64_t walker_offset, const int64_t* walker_ids /*nullable*/, int64_t step0,
                     int remove_mean, float* rates_out /*nullable*/, void* workspace, void* stream);

/* ---------------------------------------------------------------- wide EGNN backbone (hidden_nf <= 64, static node features)
 * replaces EGNN_dynamics_AD2_cat.forward (pita/src/models/components/egnn_dynamics_ad2_cat.py:157-203; the
 * alanine-dipeptide backbone of configs/model/net/egnn_dynamics_ad2_cat.yaml: hidden 64 x 5 layers, one-hot atom-type
 * node features concatenated with t and beta) over EGNN / E_GCL of egnn.py:108-346, and ScoreNet's EDM preconditioning
 * (score_net.py:13-43).  Two kernels serve the handle: a matrix-pipe kernel (csrc/egnn_wide_mfma_kernel.hip: 64 x 64 dense
 * layers as 2 x 2 blocks of 32 x 32 x 16 f16 MFMAs on the fp32-equivalent two-piece split) for the particle systems it is
 * instantiated for (22, 33, 42, 13, 55 particles x 3), and a vector-pipe kernel (csrc/egnn_wide_kernel.hip: lane = hidden feature, fp32 FMA
 * chains) for every other shape -- which also recomputes, behind the matrix-pipe launch, exactly those walkers whose
 * result came out non-finite (an activation beyond the f16 range).
 * weights: the module's state_dict flattened in registration order (embedding, embedding_out, gcl_0 .. gcl_{L-1}, like
 * pita_egnn_create); h_initial: host [n_particles, n_static] static node features (the reference's get_h_initial()). */
typedef struct pita_egnn_wide pita_egnn_wide_t;
typedef struct {
  int n_particles, n_dim, hidden_nf, n_layers;
  int n_static;       /* static features per node; in_node_nf = n_static + 1 (t) + condition_beta */
  int condition_beta;
  int attention, tanh;
  float coords_range; /* 15.0 in the reference; per-layer range = coords_range / n_layers */
} pita_egnn_wide_config;
int64_t pita_egnn_wide_num_weights(const pita_egnn_wide_config* cfg);
int pita_egnn_wide_create(pita_egnn_wide_t** out, const pita_egnn_wide_config* cfg, const float* weights,
                          int64_t n_weights, const float* h_initial /* host; nullable when n_static == 0 */);
int pita_egnn_wide_destroy(pita_egnn_wide_t* net);
/* 1 when pita_egnn_wide_eval runs this handle on the matrix-pipe kernel, 0 when on the vector-pipe kernel alone */
int pita_egnn_wide_uses_matrix_pipe(const pita_egnn_wide_t* net);
/* 1 when pita_egnn_wide_jvp / pita_egnn_wide_jacobian_trace run this handle's forward-mode launches on the matrix-pipe
 * kernel (csrc/egnn_wide_mfma_jvp_kernel.hip: instantiated for 22, 33, 42 particles x 3, LDS need within a workgroup's
 * 160 KB, PITA_WIDE_NO_MFMA unset), 0 when on the vector-pipe kernel alone (13, 55 particles and every shape
 * pita_egnn_wide_uses_matrix_pipe is 0 for) */
int pita_egnn_wide_jvp_uses_matrix_pipe(const pita_egnn_wide_t* net);
/* 1 when pita_egnn_wide_vjp runs this handle's reverse-mode sweep on the matrix-pipe kernel
 * (csrc/egnn_wide_mfma_vjp_kernel.hip: instantiated for 22, 33, 42 particles x 3, LDS need within a workgroup's 160 KB,
 * PITA_WIDE_NO_MFMA unset), 0 when on the vector-pipe kernel alone */
int pita_egnn_wide_vjp_uses_matrix_pipe(const pita_egnn_wide_t* net);
/* what = 0: vel[B, n*d] = backbone(t[B], x[B, n*d], beta[B]) (mean-free); 1: denoiser D_theta(h = t, x); 2: score */
int pita_egnn_wide_eval(pita_egnn_wide_t* net, int what, const float* t, const float* x, const float* beta /*nullable*/,
                        float* out, int64_t B, void* stream);

/* Fused sampler on this backbone: n_steps Euler-Maruyama steps of the NOT-debiased reverse VE-SDE in ONE launch, walkers
 * on chip between the steps -- pita_egnn_sampler_run for EGNN_dynamics_AD2_cat (same step table PITA_ST_*, same Philox
 * keying by (seed, walker_offset + walker, step0 + step, particle), same stats_out moments; replaces, per step,
 * sdes.py:117-128,245-251 + sde_integration.py:299-351,148).  Matrix-pipe kernel where the particle system has one,
 * then the fp32 vector-pipe kernel on exactly the walkers it left non-finite (an activation beyond the f16 range),
 * restarted from a handle-owned backup. */
int pita_egnn_wide_sampler_run(pita_egnn_wide_t* net, float* x, int64_t B, const float* step_tab, int n_steps,
                               const float* noise /*nullable*/, uint64_t seed, uint64_t walker_offset, int64_t step0,
                               int remove_mean, double* stats_out /*nullable*/, void* stream);

/* Forward-mode derivative of the EDM denoiser D(h, x) = c_s x + c_out F(c_noise(h), c_in(h) x, beta) around this
 * backbone, one tangent direction per launch (arguments as pita_egnn_jvp):  dout = J_x D . vx + dD/dh . vh, out = D
 * (nullable), dot_out[b * dot_stride + dot_off] = <x_b, dD_b>, diag_acc[b] += dD[b, dir].  What the debiased
 * Feynman-Kac regime (pita/src/models/components/sdes.py:151-239 with utils.py:30-51, energy_net.py:51-62) needs of
 * EGNN_dynamics_AD2_cat: trace J_x D, J_x D^T x and <x, dD/dh> are sums over such directions; the reference takes them
 * from vmap(jacrev) and autograd.  Matrix-pipe kernel (csrc/egnn_wide_mfma_jvp_kernel.hip) for 22, 33 and 42 particles
 * (pita_egnn_wide_jvp_uses_matrix_pipe), then the fp32 vector-pipe kernel (csrc/egnn_wide_kernel.hip:
 * egnn_wide_jvp_kernel) on exactly the walkers whose primal or tangent left the f16 range; the vector-pipe kernel alone
 * for every other shape. */
int pita_egnn_wide_jvp(pita_egnn_wide_t* net, const float* h, const float* x, const float* beta /*nullable*/,
                       const float* vx /*nullable*/, int dir, const float* vh /*nullable*/, float* out /*nullable*/,
                       float* dout /*nullable*/, float* dot_out /*nullable*/, int64_t dot_stride, int64_t dot_off,
                       float* diag_acc /*nullable*/, int64_t B, void* stream);

/* Reverse-mode derivative of the same denoiser (arguments as pita_egnn_vjp): vjp = J_x D(h, x)^T cot for a per-walker
 * cotangent (null: x itself -- grad_x E_theta = ((1 + c_s) x - D - J_x D^T x)/h, which the reference takes from autograd,
 * pita/src/models/components/energy_net.py:51-62), out = D (nullable), dot_h (nullable) = <cot, dD/dh> (the h-derivative
 * term of dE_theta/dt, sdes.py:218) -- ONE sweep instead of dim + 1 forward-mode launches, with per-layer checkpoints
 * in a handle-owned scratch.  Matrix-pipe kernel (csrc/egnn_wide_mfma_vjp_kernel.hip: f16 two-piece primal, exact
 * bf16 x 3 adjoint products) for 22, 33 and 42 particles (pita_egnn_wide_vjp_uses_matrix_pipe), then the fp32 vector-pipe
 * kernel (csrc/egnn_wide_kernel.hip: egnn_wide_vjp_kernel) on exactly the walkers whose primal left the f16 range -- they
 * get out, vjp and dot_h from it; the vector-pipe kernel alone for every other shape.  A walker's bits do not depend on
 * B, on its place in the batch or on the run. */
int pita_egnn_wide_vjp(pita_egnn_wide_t* net, const float* h, const float* x, const float* beta /*nullable*/,
                       const float* cot /*nullable*/, float* out /*nullable*/, float* vjp, float* dot_h /*nullable*/,
                       int64_t B, void* stream);

/* pita_egnn_wide_vjp (which forwards here with dot_parts = NULL) with the split of dot_h that pita_egnn_vjp offers:
 * dot_parts (nullable, device [B, 2], needs dot_h): the same derivative split the way the reference's energy is written
 * (energy_net.py:33-41, E = |x|^2 (1 - c_s)/(2h) - c_out/(c_in h) <F, c_in x>):
 *   dot_parts[b][0] = c_out <cot, F>,   dot_parts[b][1] = <cot, d(c_out F)/dh> = dot_h[b] - c_s'(h) <cot, x>.
 * pita_fk_assemble builds E_theta and dE_theta/dh (sdes.py:218) from these without the |x|^2/h^2-sized cancellation that
 * the forms through <D, x> and <x, dD/dh> carry at small h.  Both kernels add the three shares over the walker in a fixed
 * order (no atomics); a walker the matrix-pipe kernel marks gets dot_parts, like out, vjp and dot_h, from the vector-pipe
 * kernel.  dot_parts == NULL: out, vjp and dot_h have the bits of pita_egnn_wide_vjp.  dot_parts != NULL: out and vjp keep
 * those bits; dot_h[b] is the fp32 sum dot_parts[b][1] + (the kernel's own c_s'(h) <cot, x>), which may differ from the
 * plain call's dot_h by rounding.  dot_parts without dot_h, or a null net, is PITA_EINVAL before any device call; B = 0
 * is PITA_OK and touches nothing. */
int pita_egnn_wide_vjp_parts(pita_egnn_wide_t* net, const float* h, const float* x, const float* beta /*nullable*/,
                             const float* cot /*nullable*/, float* out /*nullable*/, float* vjp, float* dot_h /*nullable*/,
                             float* dot_parts /*nullable [B,2], needs dot_h*/, int64_t B, void* stream);

/* trace(J_x D)(h, x) of the EDM denoiser around the wide backbone and, optionally, D itself: ONE call
 * (replaces n*d pita_egnn_wide_jvp launches, utils.py:30-51); bit-identical to them.  One launch whose work items are
 * (walker, unit direction) pairs -- the matrix-pipe kernel where pita_egnn_wide_jvp_uses_matrix_pipe (22, 33, 42
 * particles), the vector-pipe kernel on exactly the items it flagged (and on all items of every other shape, or under
 * PITA_WIDE_NO_MFMA) -- writes the diagonal entries
 * dD[b, dir] to a handle-owned scratch; a reduction adds them per walker in direction order. */
int pita_egnn_wide_jacobian_trace(pita_egnn_wide_t* net, const float* h, const float* x,
                                  const float* beta /*nullable*/, float* trace /*[B]*/,
                                  float* denoiser_out /*nullable [B, n*d]*/, int64_t B, void* stream);

/* Hutchinson estimate of trace(J_x D)(h, x) from n_probes = K probes and, optionally, D itself: ONE call (the
 * estimator the reference's utils.py ships beside compute_divergence_exact, :30-51; what VEReverseSDE's cdf= slot is
 * for).  estimate[b] = (sum_k q[k, b], added in probe order from +0) / (float)K with q[k, b] = <v_k, J_x D v_k>;
 * per_probe (nullable) receives q.  One launch whose work items are (walker, probe) pairs, each computed exactly as
 * pita_egnn_wide_jvp(vx = v_k, vh = NULL) computes its tangent -- the matrix-pipe kernel where
 * pita_egnn_wide_jvp_uses_matrix_pipe, the vector-pipe kernel on exactly the items it flagged (and on all items of every
 * other shape, or under PITA_WIDE_NO_MFMA) -- writes q to a handle-owned scratch; no atomics, every sum in a fixed
 * order, so a walker's bits depend on neither B nor its row.  denoiser_out has the bits of
 * pita_egnn_wide_jacobian_trace's.
 * probes != NULL: v_k = probes[k, b, :], arbitrary floats (parity hook).  probes == NULL: Rademacher signs from the
 * library's Philox4x32-10 keyed (seed, walker_offset + b, step) like the samplers' noise, counter tag
 * 0x80000 | (k << 10) | particle (disjoint from the noise tags, particle < 1 024, and from the MALA uniform's 0xFFFFF);
 * coordinate c of the particle is +1 where bit c of the first output word is set, else -1: what pita_rademacher_probes
 * writes out for the same key.  The drawn path needs K <= 256 and n_particles <= 1 023.
 * The estimate is unbiased with variance (1 / 2K) sum_{i != j} (J_ij + J_ji)^2 per walker.
 * B = 0 is PITA_OK and touches nothing; a null net / h / x / estimate, n_probes < 1, K > 256 on the drawn path or a
 * missing beta on a condition_beta handle is PITA_EINVAL before any device call. */
int pita_egnn_wide_trace_probes(pita_egnn_wide_t* net, const float* h, const float* x, const float* beta /*nullable*/,
                                int n_probes, const float* probes /*nullable [K,B,n*d]*/, uint64_t seed,
                                uint64_t walker_offset, int64_t step, float* estimate /*[B]*/,
                                float* per_probe /*nullable [K,B]*/, float* denoiser_out /*nullable [B,n*d]*/,
                                int64_t B, void* stream);
/* The Rademacher probes (+1 / -1) that pita_egnn_wide_trace_probes draws in its kernels for (seed, walker_offset, step),
 * from the same device function: out[k, b, :] is probe k of walker walker_offset + b, so the drawn path can be replayed
 * through the injected one, and backbones without a probe kernel draw theirs here.  1 <= n_probes <= 256,
 * 1 <= n_particles <= 1 023, 1 <= n_dim <= 32; B = 0 is PITA_OK and touches nothing. */
int pita_rademacher_probes(float* out /*[K,B,n*d]*/, int64_t B, int n_particles, int n_dim, int n_probes, uint64_t seed,
                           uint64_t walker_offset, int64_t step, void* stream);

/* Diagonal Gaussian mixture with equal weights.
 * replaces GMM.__call__ (pita/src/energies/gmm_energy.py:87-90) ->
 * fab GMM.log_prob (fab/fab/target_distributions/gmm.py:71-79,104).
 * means, scales: device [K, dim].  1 <= dim <= 4 (else PITA_EUNSUPPORTED), 1 <= K <= 2048 (else PITA_EINVAL); the
 * table lives in 4 (2 K dim + K) bytes of dynamic LDS -- 73 728 at K = 2048, dim = 4, which gfx950 launches as it is
 * (tests/test_pair_shapes_gpu.py calls it).  */
int pita_gmm_logp_force(const float* x, float* logp, float* force /*nullable*/, int64_t B, int dim,
                        const float* means, const float* scales, int K, float temperature,
                        void* stream);

/* Table-driven classical force field (K4): bonds, angles, periodic torsions, LJ + Coulomb over all atom pairs with
 * exceptions and the optional CutoffNonPeriodic reaction field, and the GB-OBC1 implicit solvent with its ACE
 * surface-area term -- the functional forms of OpenMM's HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce,
 * NonbondedForce and GBSAOBCForce.  Stands in for the arithmetic ALPEnergy.__call__
 * (pita/src/energies/alp_energy.py:93-149) delegates to OpenMM (amber14-all.xml + implicit/obc1.xml); the real
 * amber14 parameters are outside the reference tree (parity unpinned).  All table pointers are HOST pointers copied
 * at creation.  Units: nm, kJ/mol, elementary charges; x_model * length_scale = nm; logp = -E/kT. */
typedef struct pita_ff pita_ff_t;
typedef struct {
  int n_atoms;
  int n_bonds;      const int* bond_idx;  /* [n_bonds][2] */      const float* bond_par;  /* [n_bonds][2]: r0, k */
  int n_angles;     const int* angle_idx; /* [n_angles][3] */     const float* angle_par; /* [n_angles][2]: theta0, k */
  int n_torsions;   const int* tors_idx;  /* [n_torsions][4] */   const float* tors_par;  /* [n_torsions][3]: periodicity, phase, k */
  const float* charge; const float* sigma; const float* epsilon;  /* per atom; Lorentz-Berthelot mixing */
  int n_exceptions; const int* exc_idx;   /* [n_exceptions][2] */ const float* exc_par;   /* [n][3]: chargeProd, sigma, epsilon */
  int use_cutoff; float cutoff; float rf_dielectric;              /* CutoffNonPeriodic reaction field (78.3 in OpenMM) */
  float length_scale;                                              /* 0.1640 for the reference's normalised ALDP (energy/aldp.yaml:11) */
  float kT;                                                        /* kJ/mol */
  /* GBSAOBCForce, OBC1 (amber implicit/obc1.xml): NULL gb_radius = no implicit solvent */
  const float* gb_radius;                                          /* [n] nm */
  const float* gb_scale;                                           /* [n] HCT overlap scale factors */
  float gb_solute_dielectric, gb_solvent_dielectric;               /* OpenMM defaults 1.0, 78.5 */
  float gb_surface_area_factor;                                    /* 4 pi x 2.25936 kJ/mol/nm^2 = 28.3919551; 0 = no SA term */
} pita_ff_config;
/* Capacity: 2 <= n_atoms <= 256 (one thread per (walker, atom) in a 256-thread block), else PITA_EINVAL before any
 * device call.  The handle carries one launch plan for both entry points: floor(256 / n_atoms) walkers per block, or
 * fewer where the device's per-block LDS cannot hold the interaction tables (bonded terms, the dense pair table,
 * per-atom lists) plus that many walkers' working set; where not even one walker fits, PITA_EUNSUPPORTED with the bytes
 * needed and available.  A handle that exists is therefore taken by pita_ff_logp_force, pita_ff_descent and
 * pita_ff_mala (which lives in the descent's footprint), and a walker's result does not depend on the plan.
 * Measured capacity: 256 is the bound of the thread mapping, not what the LDS holds.  The dense pair table grows as
 * n_atoms^2 (24 B per pair: 100 KB at 92 atoms), so with amber-shaped tables (about one bond, 1.7 angles and 4.8 torsion
 * terms per atom, GB on) and the 163 840 B per block of gfx950 the largest peptide chain accepted is
 * ACE-(ALA)7-GLY-NME, 89 atoms (159 868 B for one walker per block), and the first one refused is ACE-(ALA)8-NME,
 * 92 atoms (169 104 B): PITA_EUNSUPPORTED.  Walkers per block at that limit: 11 at 22 atoms, 3 at 64 and 65, 2 at 73,
 * 1 from 85 on (tests/_ff_shapes.py restates the accounting; tests/test_ff_shapes_gpu.py runs every step of it).
 * Systems with fewer bonded terms reach further, none past 113 atoms: the pair table and one walker's arrays alone
 * exceed that limit from 114 atoms on. */
int pita_ff_create(pita_ff_t** out, const pita_ff_config* cfg);
int pita_ff_destroy(pita_ff_t* ff);
int pita_ff_logp_force(pita_ff_t* ff, const float* x, float* logp, float* force /*nullable*/, int64_t B, void* stream);

/* Negative-time / Langevin descent on the force-field target (sde_integration.py:353-360 with the target of
 * alp_energy.py:122-149): n_steps of x <- remove_mean(x + F dt + noise_scale sqrt_dt xi) in ONE launch, walkers LDS-resident,
 * in place on x [B, 3 n_atoms]; bit-identical to n_steps x (pita_ff_logp_force + pita_em_step).  noise: [n_steps, B, 3 n]
 * injected normals or NULL (Philox keyed by seed, walker_offset + walker, step0 + step, atom). */
int pita_ff_descent(pita_ff_t* ff, float* x, const float* noise /*nullable*/, int64_t B, int n_steps, float dt,
                    float noise_scale, float sqrt_dt, uint64_t seed, uint64_t walker_offset, int64_t step0,
                    int remove_mean, void* stream);

/* Fused MALA chain on the force-field target: metropolis_hastings_mala / _adaptive
 * (pita/src/models/components/sde_integration.py:28-45,362-470) with the target of alp_energy.py:122-149; bit-identical
 * to pita_ff_logp_force + pita_mala_propose + pita_ff_logp_force + pita_mala_accept + pita_mala_adapt step after step.
 * Contract and argument meaning of pita_lj_mala: x [B, 3 n_atoms] and logp [B] (log-density of x on entry) are updated in
 * place; dt_dev holds the step size (adapted in place when adaptive != 0, against the acceptance rate over `total`
 * walkers -- this rank's B); rates_out [n_steps] receives the acceptance rates.  noise [n_steps, B, 3 n] / uniforms
 * [n_steps, B] nullable -> Philox keyed (seed, walker key, step0 + s, atom / 0xFFFFF), walker key = walker_ids[w] or
 * walker_offset + w.  workspace: 8-byte aligned device scratch of pita_ff_mala_workspace_bytes(n_steps) bytes.
 * A non-adaptive chain is ONE launch with the walkers resident on chip over all steps.  An adaptive chain is one launch
 * per step: the order of the stream is what lets a step see the acceptance count of the step before, and every launch
 * derives its step size on the device from dt_dev[0] and the counts so far (no host synchronisation).  There is no
 * grid-wide barrier and no wait inside the kernel, so this entry point cannot time out: it has no NaN result and no
 * rerun protocol.  The chain runs in the launch plan of pita_ff_descent, so a handle
 * that exists is taken; PITA_EUNSUPPORTED is reserved for a handle whose plan cannot hold the chain.
 * ff, dt_dev, workspace non-null, B >= 0, n_steps >= 0, total > 0 and the workspace alignment are checked before any
 * device call (PITA_EINVAL); B == 0 or n_steps == 0 is PITA_OK and leaves dt_dev as it is. */
size_t pita_ff_mala_workspace_bytes(int n_steps);
int pita_ff_mala(pita_ff_t* ff, float* x, float* logp, const float* noise /*nullable [n_steps,B,3n]*/,
                 const float* uniforms /*nullable [n_steps,B]*/, int64_t B, int n_steps, double* dt_dev, int adaptive,
                 int64_t total, uint64_t seed, uint64_t walker_offset, const int64_t* walker_ids /*nullable*/,
                 int64_t step0, int remove_mean, float* rates_out /*nullable*/, void* workspace, void* stream);

/* pita_ff_mala with one step size, count and adaptation per population: contract and arguments of pita_lj_mala_pop
 * (totals / n_pop / pop_size / pop_base in place of total, dt_dev [n_pop], rates_out [n_steps, n_pop], workspace of
 * pita_mala_pop_workspace_bytes(n_steps, n_pop) bytes), bit-identical per population to pita_ff_mala on its rows alone.
 * ff, dt_dev, totals, workspace non-null, B >= 0, n_steps >= 0, n_pop >= 1, pop_size >= 1 and the workspace alignment are
 * checked before any device call (PITA_EINVAL); B == 0 or n_steps == 0 is PITA_OK and leaves dt_dev as it is. */
int pita_ff_mala_pop(pita_ff_t* ff, float* x, float* logp, const float* noise /*nullable [n_steps,B,3n]*/,
                     const float* uniforms /*nullable [n_steps,B]*/, int64_t B, int n_steps, double* dt_dev, int adaptive,
                     const int64_t* totals, int n_pop, int64_t pop_size, uint64_t pop_base, uint64_t seed,
                     uint64_t walker_offset, const int64_t* walker_ids /*nullable*/, int64_t step0, int remove_mean,
                     float* rates_out /*nullable*/, void* workspace, void* stream);

/* ---------------------------------------------------------------- EGNN backbone (K5, K7)
 * replaces EGNN_dynamics.forward (pita/src/models/components/egnn_temp_conditioned.py:56-93,
 * egnn.py:50-80), EGNN.forward (:172-194), E_GCL (:197-356) and the EDM wrappers
 * ScoreNet.denoiser / ScoreNet.forward (score_net.py:13-43).
 */
typedef struct pita_egnn pita_egnn_t;

typedef struct {
  int n_particles;
  int n_dim;
  int hidden_nf;        /* only 32 is implemented in HIP */
  int n_layers;
  int in_node_nf;       /* 1 = time only (egnn.py), 2 = time + temperature */
  int attention;        /* att_mlp sigmoid gate present */
  int tanh;             /* tanh on the coordinate head (* coords_range / n_layers) */
  float coords_range;   /* 15.0 in the reference */
  int feature_layout;   /* 0 = "pita": the reference's t/beta interleave quirk
                           (egnn_temp_conditioned.py:68-78); 1 = per-node (t, beta) */
  int precision;        /* arithmetic of the dense layers, all fp32-accurate:
                           0 = v_mfma_f32_32x32x2_f32 (bit-exact fp32 fmaf chains),
                           1 = bf16 matrix pipe with an exact 3-way operand split (6 products,
                               error <= 2^-24 |w||x|: fp32-equivalent, not bit-identical to 0),
                           2 = f16 matrix pipe with a 2-way round-to-nearest operand split (3 products,
                               each operand within 2^-24 relative; operands travel scaled by 16, so
                               |activations| must stay below 4094; forward / fused sampler only -- the
                               derivative kernels of the same handle run mode 1) */
} pita_egnn_config;

/* `weights` is a HOST pointer to the reference state_dict flattened in its own key order:
 * embedding.{weight,bias}, embedding_out.{weight,bias}, then per layer l:
 * edge_mlp.0.{weight[H,2H+2],bias}, edge_mlp.2.{weight,bias}, node_mlp.0.{weight[H,2H],bias},
 * node_mlp.2.{weight,bias}, coord_mlp.0.{weight,bias}, coord_mlp.2.weight[1,H],
 * (att_mlp.0.{weight[1,H],bias[1]} if attention).  n_weights is checked. */
int pita_egnn_create(pita_egnn_t** out, const pita_egnn_config* cfg, const float* weights,
                     int64_t n_weights);
int pita_egnn_destroy(pita_egnn_t* net);
int64_t pita_egnn_num_weights(const pita_egnn_config* cfg);

/* backbone forward: out[B,D] = F(t[B], x[B,D], beta[B]) (beta nullable when in_node_nf==1) */
int pita_egnn_forward(pita_egnn_t* net, const float* t, const float* x, const float* beta,
                      float* out, int64_t B, void* stream);
/* EDM-preconditioned outputs, h = sigma^2 per walker (score_net.py:21-43):
 *   what = 1: denoiser D = c_s x + c_out F(c_noise, c_in x, beta)
 *   what = 2: score (D - x)/h */
int pita_egnn_edm(pita_egnn_t* net, int what, const float* h, const float* x, const float* beta,
                  float* out, int64_t B, void* stream);

/* Forward-mode derivative of the denoiser D(h, x) = c_s x + c_out F(c_noise(h), c_in(h) x, beta), one tangent
 * direction per launch:  dout = J_x D . vx + dD/dh . vh   (and out = D when out != NULL).
 * vx: device [B, D] or NULL; when NULL the direction is the unit vector e_dir of every walker (0 <= dir < D) or
 * zero (dir = -1).  vh: device [B] or NULL (= 0).
 * Building block of the debiased Feynman-Kac regime (sdes.py:151-239): div_x s_theta (utils.py:30-51),
 * grad_x E_theta (energy_net.py:51-62) and dE_theta/dt (sdes.py:218) are linear in these JVPs -- the reference
 * gets them from torch.func.jacrev / autograd. */
int pita_egnn_jvp(pita_egnn_t* net, const float* h, const float* x, const float* beta, const float* vx,
                  int dir, const float* vh, float* out /*nullable*/, float* dout /*nullable*/,
                  float* dot_out /*nullable: dot_out[b*dot_stride + dot_off] = <x_b, dD_b>*/, int64_t dot_stride,
                  int64_t dot_off, float* diag_acc /*nullable: diag_acc[b] += dD[b, dir]*/, int64_t B, void* stream);

/* Reverse-mode derivative of the denoiser:  vjp = J_x D(h, x)^T cot  (and out = D when out != NULL), one launch for
 * all walkers.  cot: device [B, D] or NULL (= x).  With cot = x this is the only derivative grad_x E_theta needs
 * (energy_net.py:33-62: E = (1+c_s)|x|^2/(2h) - <D, x>/h, so grad E = ((1+c_s) x - D - J^T x)/h), replacing the
 * reference's torch.autograd.grad through the network.  Checkpoint scratch is owned by the handle.
 * dot_h (nullable, device [B]): <cot, dD/dh> from the same reverse sweep (it also reaches the h-dependent inputs of the
 * backbone -- time feature ln(h)/8, the scaling c_in(h) -- and the explicit c_s(h), c_out(h)): with cot = x this is the
 * term of dE_theta/dt (sdes.py:218) that otherwise takes a forward-mode launch in the h direction.
 * dot_parts (nullable, device [B, 2], needs dot_h): the same derivative split the way the reference's energy is written
 * (energy_net.py:33-41, E = |x|^2 (1 - c_s)/(2h) - c_out/(c_in h) <F, c_in x>):
 *   dot_parts[b][0] = c_out <cot, F>,   dot_parts[b][1] = <cot, d(c_out F)/dh> = dot_h[b] - c_s'(h) <cot, x>.
 * pita_fk_assemble builds E_theta and dE_theta/dh from these without the |x|^2/h^2-sized cancellation that the forms
 * through <D, x> and <x, dD/dh> carry at small h. */
int pita_egnn_vjp(pita_egnn_t* net, const float* h, const float* x, const float* beta, const float* cot /*nullable*/,
                  float* out /*nullable*/, float* vjp, float* dot_h /*nullable*/, float* dot_parts /*nullable*/, int64_t B,
                  void* stream);

/* Exact trace of the denoiser Jacobian, K unit directions per launch sharing one primal evaluation:
 *   diag_acc[b] += sum_{k < ndir} (J_x D(h, x) e_{dir0+k})_{dir0+k},   1 <= ndir <= pita_egnn_div_directions(net).
 * Looping dir0 over 0, K, 2K, ... < D accumulates trace(J_x D), from which div_x s_theta = (trace - D)/h: the exact
 * divergence the reference computes with vmap(jacrev) (pita/src/models/components/utils.py:30-51). */
int pita_egnn_div_directions(const pita_egnn_t* net);
int pita_egnn_div_accumulate(pita_egnn_t* net, const float* h, const float* x, const float* beta, int dir0, int ndir,
                             float* diag_acc, float* denoiser_out /*nullable: D(h, x) of the shared primal*/, int64_t B,
                             void* stream);

/* The whole trace in one call: trace[b] = trace(J_x D(h_b, x_b)) (overwritten), optionally D itself.  Handles of
 * precision 2 compute the primal network ONCE: the first launch stores the per-edge primal factors the tangent chains
 * consume in a handle-owned cache (about 180 KB per LJ13 walker; batches beyond PITA_DIV_CACHE_GB, default 24, go in chunks
 * of walkers) and the remaining directions run as tangent-only launches, four directions each, streaming that cache. */
int pita_egnn_jacobian_trace(pita_egnn_t* net, const float* h, const float* x, const float* beta, float* trace,
                             float* denoiser_out /*nullable*/, int64_t B, void* stream);

/* Hutchinson estimate of trace(J_x D)(h, x) from n_probes = K probes and, optionally, D itself, on the hidden-32 EGNN:
 * ONE call (arguments and contract of pita_egnn_wide_trace_probes).  estimate[b] = (sum_k q[k, b], added in probe order
 * from +0) / (float)K with q[k, b] = <v_k, J_x D v_k>; per_probe (nullable) receives q.  The probes go through the
 * multi-direction kernels of pita_egnn_div_accumulate with probes in the place of unit vectors, K_launch =
 * pita_egnn_div_directions(net) of them per launch sharing ONE primal evaluation: ceil(K / K_launch) launches (the last
 * one may be short) and one small reduction, against K pita_egnn_jvp launches that each recompute the primal.
 * Precision-2 handles run the f16 kernel, which leaves the probes of a walker with a non-finite term unwritten and marks
 * it, then the bf16x3 kernel on exactly the marked walkers; other precisions run the bf16x3 kernel.  Per (walker, probe)
 * q = sum_{i,c} v_ic [c_s v_ic + c_out (dF_ic - (1/N) sum_j dF_jc)] is summed by one lane in (particle, coordinate) order
 * and stored once: no atomics, so a walker's q, estimate and D bits depend on neither B, its row, walker_offset beyond
 * its own global index, the number of probes in the call nor the launch slot a probe lands in.  denoiser_out comes from
 * the first launch and has the bits of pita_egnn_jacobian_trace's on the same handle.  q lives in per_probe when given,
 * else in a handle-owned [K, B] buffer.
 * probes != NULL: v_k = probes[k, b, :], arbitrary floats (parity hook).  probes == NULL: Rademacher signs drawn in the
 * kernels with the key, tag and bit convention of pita_egnn_wide_trace_probes -- what pita_rademacher_probes writes out
 * for the same (seed, walker_offset, step); needs K <= 256.
 * B = 0 is PITA_OK and touches nothing; a null net / h / x / estimate, n_probes < 1, K > 256 on the drawn path or a
 * missing beta with in_node_nf == 2 is PITA_EINVAL before any device call; a particle system without a multi-direction
 * kernel (pita_egnn_div_directions < 0) is PITA_EUNSUPPORTED. */
int pita_egnn_trace_probes(pita_egnn_t* net, const float* h, const float* x, const float* beta /*nullable*/,
                           int n_probes, const float* probes /*nullable [K,B,n*d]*/, uint64_t seed,
                           uint64_t walker_offset, int64_t step, float* estimate /*[B]*/,
                           float* per_probe /*nullable [K,B]*/, float* denoiser_out /*nullable [B,n*d]*/, int64_t B,
                           void* stream);

/* Work accounting for the roofline of the debiased leg (bench.py): matrix-core wave-instructions per walker for one full
 * trace (all n_particles * n_dim directions) on the path this handle takes; units as pita_egnn_sampler_work. */
int pita_egnn_div_work(const pita_egnn_t* net, double* mfma16_per_walker, double* mfma32_per_walker);

/* Feynman-Kac drift assembly per walker from those reductions (replaces the torch/autograd expressions of
 * sdes.py:157-227): with E = be [(1+c_s)|x|^2/(2h) - <D_E,x>/h],
 *   grad E = be ((1+c_s) x - D_E - jtx_E)/h,  s = bs (D_S - x)/h,  b = s g2/2,
 *   U = E, or with pin_energy (energy_net.py:43-48)  U = w U0 + (1-w) E,  U0 = clamp(-logp_target, +-1e3),
 *   grad U = (1-w) grad E  (the reference's energy classes return log p detached: no target force enters),
 *   dU/dt = dw/dt (U0 - E) + (1-w) dE/dh dh/dt   (dh/dt from the schedule, not assumed equal to g^2),
 *   drift_X = gamma (-grad U) g2/2 + gamma b,
 *   drift_A = gamma^2 <-grad U, b> + gamma bs (trace_S - D)/h g2/2 + gamma dU/dt + dgamma U   (NOT yet clamped).
 * be / bs: per-walker inverse temperatures when the energy / score net was built with precondition_beta
 * (score_net.py:36-38, energy_net.py:40-41), NULL = 1.  pin_w = (1-t)^3 and pin_dw = -3 (1-t)^2 with logp_target [B];
 * logp_target NULL = no pinning.  All arrays are device pointers: x, D_E, jtx_E, D_S, drift_X [B,D]; the rest [B].
 * dot_parts ([B, 2] from pita_egnn_vjp, nullable): when given, E = be [|x|^2/(2(1+h)) - s1/h] and
 * dE/dh = be [-|x|^2/(2(1+h)^2) + s1/h^2 - s2/h] with (s1, s2) = dot_parts[b] -- the same quantities in the
 * reference's own well-conditioned form; NULL keeps the forms through <D_E, x> and dot_h.
 * The clamp of U0 is torch.clamp's: +-inf become -+1e3, and a NaN logp_target stays NaN -- that walker's Ut, dUt_dt and
 * drift_A are NaN (its drift_X, divergence_score and cross_term do not read logp_target), no other walker is touched.
 * B = 0 returns PITA_OK without a launch; B < 0, D < 1, a null required pointer with B > 0 and non-zero pin weights
 * without logp_target are PITA_EINVAL. */
int pita_fk_assemble(const float* x, const float* h, const float* g2, const float* dhdt, const float* D_E,
                     const float* jtx_E, const float* dot_h, const float* dot_parts /*nullable*/, const float* D_S,
                     const float* trace_S, float gamma, float dgamma, const float* beta_e /*nullable*/, const float* beta_s /*nullable*/, float pin_w,
                     float pin_dw, const float* logp_target /*nullable*/, float* drift_X, float* drift_A, float* div_bt,
                     float* cross, float* dUdt, float* Ut, int64_t B, int D, void* stream);
/* K11: in place a[c] = min(a[c], quantile_q(a over its chunk)), chunks of `chunk` consecutive walkers, linear
 * interpolation like torch.quantile (sdes.py:230; sde_integration.py:179).
 * NaN entries -- a departure from torch, which turns the whole chunk into NaN: a NaN keeps its place and its value; in
 * the order statistics it sorts above +inf (by its bit pattern: a NaN with the sign bit set sorts below -inf); the other
 * entries are clamped by the quantile of those keys; a chunk whose quantile itself comes out NaN is left unchanged
 * (fminf returns the entry). */
int pita_quantile_clamp(float* a, int64_t B, int64_t chunk, float q, void* stream);

/* ---------------------------------------------------------------- fused sampler (K5+K7+K8)
 * Runs n_steps Euler-Maruyama steps of the NOT-debiased reverse VE-SDE in ONE launch, walkers
 * resident on chip for the whole trajectory.  replaces, per step,
 * VEReverseSDE.f_not_debiased + .diffusion (sdes.py:117-128,245-251),
 * WeightedSDEIntegrator.euler_maruyama_step (sde_integration.py:299-351) and the
 * remove_mean of integrate_sde (:148).
 *
 * step_tab: device [n_steps][PITA_STEP_STRIDE] floats computed by the host in the
 * reference's fp32 op order (see pita_amd/sde_integration.py):
 */
#define PITA_STEP_STRIDE 16
enum {
  PITA_ST_CS = 0, PITA_ST_CIN = 1, PITA_ST_COUT = 2, PITA_ST_CNOISE = 3, PITA_ST_H = 4,
  PITA_ST_G2 = 5, PITA_ST_GAMMA = 6, PITA_ST_DT = 7, PITA_ST_NOISE_SCALE = 8 /* scale*g(t) */,
  PITA_ST_SQRT_DT = 9, PITA_ST_BETA = 10
};
/* noise: nullable device [n_steps, B, D] standard normals (parity mode).  When NULL the kernel
 * draws Philox4x32-10 normals keyed by (seed, walker_offset + walker, step0 + step, particle)
 * so results do not depend on how walkers are sharded over GPUs.
 * drift_out: nullable device [B, D]; receives drift_X of the LAST step of the launch.
 * stats_out: nullable device double [n_steps][4]; step s ADDS (sum drift_X, sum drift_X^2, sum diffusion,
 * sum diffusion^2) over this call's B*D elements, diffusion = noise_scale * xi (sdes.py:250).  These are the moments
 * behind the per-step SDETerms the reference returns and only ever reduces to .mean()/.std()
 * (sde_integration.py:150,289; energytemp_module.py:1132-1143). */
int pita_egnn_sampler_run(pita_egnn_t* net, float* x, int64_t B, const float* step_tab,
                          int n_steps, const float* noise, uint64_t seed, uint64_t walker_offset,
                          int64_t step0, int remove_mean, float* drift_out, double* stats_out, void* stream);

/* Work accounting for the roofline of pita_egnn_sampler_run (bench.py): matrix-core wave-instructions executed per
 * walker-step at batch B, counted on the kernel's own loop structure -- mfma16: v_mfma_f32_32x32x16_{bf16,f16}
 * (32 768 flop each), mfma32: v_mfma_f32_32x32x2_f32 (4 096 flop each). */
int pita_egnn_sampler_work(const pita_egnn_t* net, int64_t B, double* mfma16_per_walker_step,
                           double* mfma32_per_walker_step);

/* How pita_egnn_sampler_run maps a batch of B walkers onto the device (bench.py `small_batch`: the reference generates
 * num_eval_samples = 2 048 walkers in inference chunks of 512, configs/experiment/lj13.yaml:27,32 -- far fewer than the
 * chip holds): walkers_per_group = walkers packed into one wavefront's column tiles (the small-group mapping is chosen
 * when the regular one would leave SIMDs with a single wave), waves = wavefronts the launch starts, wave_slots = wavefronts
 * of this kernel the device can hold at once (CUs x resident blocks x waves per block). */
int pita_egnn_sampler_mapping(const pita_egnn_t* net, int64_t B, int* walkers_per_group, int64_t* waves,
                              int64_t* wave_slots);

/* ---------------------------------------------------------------- MLP backbone (K6)
 * replaces MyMLP.forward (mlp.py:244-267) / MyMLPTemperature.forward (:501-524) incl. the
 * sinusoidal embeddings (:11-24) and residual GELU blocks (:100-118). */
typedef struct pita_mlp pita_mlp_t;
typedef struct {
  int input_dim;       /* number of coordinates (each embedded with scale 25) */
  int out_dim;
  int hidden_size;     /* multiple of 32; == emb_size in every reference config */
  int hidden_layers;
  int emb_size;        /* sinusoidal embedding size (even) */
  int temperature_conditioned; /* MyMLPTemperature: extra beta embedding */
} pita_mlp_config;
/* weights: HOST pointer, reference state_dict order: joint_mlp.0.{weight,bias},
 * joint_mlp.{1..L}.ff.{weight,bias}, joint_mlp.{L+1}.{weight,bias}.
 * freqs: HOST pointer to the emb_size/2 sinusoidal frequencies exp(-ln(1e4)/(half-1) * k) as the
 * caller's framework computes them in fp32 (mlp.py:20-21) -- passed in rather than recomputed so
 * that the angles are bit-identical to the reference's. */
int pita_mlp_create(pita_mlp_t** out, const pita_mlp_config* cfg, const float* weights,
                    int64_t n_weights, const float* freqs);
int pita_mlp_destroy(pita_mlp_t* net);
int64_t pita_mlp_num_weights(const pita_mlp_config* cfg);
int pita_mlp_forward(pita_mlp_t* net, const float* t, const float* x, const float* beta /*nullable*/,
                     float* out, int64_t B, void* stream);
/* Fused not-debiased sampler for the MLP backbone: the counterpart of pita_egnn_sampler_run (same step table, noise and
 * Philox conventions; sde_integration.py:299-351 + sdes.py:117-128 + score_net.py:13-43) with the walkers LDS-resident
 * for all n_steps.  Requires out_dim == input_dim == n_particles * n_dim, 1 <= input_dim <= 64 and n_dim <= 4 (GMM:
 * n_particles = 1, n_dim = 2); anything else is refused with an error code before a launch.  The walkers take
 * 1 024 * input_dim bytes of dynamic LDS (64 KB at input_dim = 64) next to 12 KB of static LDS for the weight stream;
 * the launcher does not raise the kernel's dynamic-LDS limit.  Observed with ROCm 7.2.0 on gfx950: the whole range
 * launches and computes correctly (tests/test_mlp_shapes_gpu.py runs input_dim = 52, 53 and 64).  B = 0 or n_steps = 0
 * returns without a launch (as do pita_mlp_forward, pita_mlp_jacobian and pita_mlp_jvp at B = 0). */
int pita_mlp_sampler_run(pita_mlp_t* net, float* x, int64_t B, const float* step_tab, int n_steps,
                         const float* noise /*nullable*/, uint64_t seed, uint64_t walker_offset, int64_t step0,
                         int remove_mean, int n_particles, int n_dim, double* stats_out /*nullable, as above*/,
                         void* stream);
/* Derivatives of the MLP's EDM denoiser D(h, x) = c_s x + c_out F(c_noise, c_in x, beta), c_noise = ln(h)/8 (score_net.py:
 * 13-43 around mlp.py:11-24, 100-118, 244-267, 501-524), for the debiased Feynman-Kac regime (sdes.py:151-239).  They
 * replace the reference's vmap(jacrev) (utils.py:30-51), autograd of E_theta (energy_net.py:51-62) and its
 * h-derivative (sdes.py:218).  Forward mode: the primal tile and up to K tangent tiles share one weight stream (K = 4, 2,
 * 1 for hidden 32, 64, 128; more directions run in passes).  h and x are the unscaled per-walker noise level and
 * coordinates; c_in, c_noise, c_s, c_out are computed in-kernel.  beta (device [B]) is read for
 * MyMLPTemperature only and not differentiated.  Requires out_dim == input_dim <= 64, else PITA_EUNSUPPORTED.
 * Every output is nullable and work that no requested output needs is skipped:
 *   out_D[b]      = D(h_b, x_b)                                          [B, D]
 *   trace[b]      = tr(J_x D)                                            [B]  (overwritten)
 *   vjp[b]        = J_x D^T cot, (J^T cot)_k = <cot, J e_k> from the same unit tangents   [B, D]
 *   dot_h[b]      = <cot, dD/dh>                                         [B]
 *   dot_parts[b]  = (c_out <cot, F>, <cot, d(c_out F)/dh>) as pita_egnn_vjp defines it    [B, 2]
 * cot: device [B, D] or NULL (= x). */
int pita_mlp_jacobian(pita_mlp_t* net, const float* h, const float* x, const float* beta /*nullable*/,
                      const float* cot /*nullable*/, float* out_D, float* trace, float* vjp, float* dot_h,
                      float* dot_parts, int64_t B, void* stream);
/* One forward-mode tangent of the same denoiser; parameter list and semantics of pita_egnn_jvp:
 * dout = J_x D . vx + dD/dh . vh (vx NULL: unit direction dir, -1 = none; vh NULL = 0), out = D,
 * dot_out[b*dot_stride + dot_off] = <x_b, dD_b>, diag_acc[b] += dD[b, dir]. */
int pita_mlp_jvp(pita_mlp_t* net, const float* h, const float* x, const float* beta, const float* vx, int dir,
                 const float* vh, float* out /*nullable*/, float* dout /*nullable*/, float* dot_out /*nullable*/,
                 int64_t dot_stride, int64_t dot_off, float* diag_acc /*nullable*/, int64_t B, void* stream);

/* ---------------------------------------------------------------- elementwise sampler pieces
 * K8: x <- x + drift*dt + (noise_scale*xi)*sqrt_dt, then optional per-walker mean removal
 * (sde_integration.py:347-349,148; data_utils.py:4-26).  noise nullable -> Philox as above.
 * stats_out: nullable device double [4], += the same four moments as pita_egnn_sampler_run for this one step. */
int pita_em_step(float* x, const float* drift, const float* noise, int64_t B, int n_particles,
                 int n_dim, float dt, float noise_scale, float sqrt_dt, uint64_t seed,
                 uint64_t walker_offset, int64_t step, int remove_mean, double* stats_out, void* stream);
/* out[0] += sum v, out[1] += sum v^2 (device double[2]): moments of one SDETerms field (divergence_score, cross_term,
 * dUt_dt; sdes.py:34-41), so the integrator returns statistics instead of N x [B] host copies (sde_integration.py:289) */
int pita_moments(const float* v, int64_t n, double* out, void* stream);
/* The same for up to four vectors of one length in one launch (null pointers are skipped): out[2 q], out[2 q + 1] += the sum /
 * sum of squares of v_q -- the four per-step SDETerms statistics of the debiased regime (drift_A, divergence_score,
 * cross_term, dUt_dt; sde_integration.py:150,289). */
int pita_moments4(const float* v0, const float* v1, const float* v2, const float* v3, int64_t n, double* out /*[8]*/,
                  void* stream);
/* Histogram of n device floats over nbins + 1 ascending device bin edges, as numpy.histogram / matplotlib's `hist` count
 * them (bin i = [edges[i], edges[i+1]), the last bin closed; values outside the edges and NaNs are not counted):
 * counts[nbins] (device, overwritten).  The two 100-bin density arrays under the reference's sample figure
 * (src/energies/base_molecule_energy_function.py:160-254: bins from the test set, energy range (min - 10, max + 10)) are
 * these counts divided by (their sum x the bin widths): pita_amd.metrics.sample_histograms.  1 <= nbins <= 1024. */
int pita_histogram(const float* v, int64_t n, const float* edges, int nbins, unsigned long long* counts, void* stream);
/* K9: MeanFreePrior.sample (base_prior.py:77-83): x = scale * N(0,1) minus particle mean.
 * noise nullable -> Philox keyed (seed, walker_offset + walker, step = -1). */
int pita_prior_sample(float* x, const float* noise, int64_t B, int n_particles, int n_dim,
                      float scale, uint64_t seed, uint64_t walker_offset, int mean_free,
                      void* stream);
/* data_utils.remove_mean in place */
int pita_remove_mean(float* x, int64_t B, int n_particles, int n_dim, void* stream);
/* standard normals [B, D] from the library's Philox stream (the generator used when noise==NULL) */
int pita_fill_normal(float* out, int64_t B, int n_particles, int n_dim, uint64_t seed,
                     uint64_t walker_offset, int64_t step, void* stream);

/* EDM preconditioning around a backbone that is NOT one of the fused kernels (ScoreNet.denoiser / forward,
 * pita/src/models/components/score_net.py:13-43): scale gives the backbone inputs x_in = c_in x and c_noise = ln(h)/8;
 * combine gives D = c_s x + c_out F (times beta + (1-beta) x when beta != NULL, :36-38) and score = (D - x)/h
 * (times beta).  D_out / score_out nullable. */
int pita_edm_scale_input(const float* h, const float* x, float* x_scaled, float* c_noise, int64_t B, int D,
                         void* stream);
int pita_edm_combine(const float* h, const float* x, const float* F, const float* beta /*nullable*/, float* D_out,
                     float* score_out, int64_t B, int D, void* stream);

/* E_theta(h, x) = (1 - c_s)/(2h) |x|^2 - c_out/(c_in h) <F, c_in x> from the backbone output F = F(c_noise, c_in x, beta)
 * (EnergyNet.forward_energy, pita/src/models/components/energy_net.py:14-41; times beta when beta != NULL). */
int pita_energy_theta(const float* h, const float* x, const float* F, const float* beta /*nullable*/, float* E,
                      int64_t B, int D, void* stream);

/* ---------------------------------------------------------------- MALA (K12)
 * sde_integration.py:28-45 mala_proposal; :362-470 accept/reject and step-size adaptation.
 * dt_dev: device double holding the step size (adapted in place by pita_mala_adapt, no host round trip).
 *   propose: x_prop = (x + dt/2 * force) + sqrt(dt) * xi    (noise nullable -> Philox (seed, walker, step, particle))
 *   accept : log q_f = -|x_prop - (x + dt/2 F)|^2 / 2dt, log q_b = -|x - (x_prop + dt/2 F_prop)|^2 / 2dt,
 *            accept iff log u < (logp_prop - logp) + (log q_b - log q_f); x and logp are updated in place with the
 *            reference's float blend a*new + (1-a)*old; optional mean removal (is_molecule); *acc_count += #accepted.
 *            uniforms nullable -> Philox.
 *   adapt  : rate = acc_count / total -> rate_out (nullable); adaptive: dt *= 1.1 if rate > 0.55 else dt /= 1.1;
 *            acc_count is reset.  With several ranks all-reduce acc_count first and pass the global total.
 *   walker_ids (device int64[B], nullable): the Philox walker key of row w; NULL = walker_offset + w.  The chain runs on
 *            the walkers with a finite log-density only (quirk Q7), i.e. on a compacted batch: keying by the original
 *            global index keeps the noise of a walker independent of how many were set aside before it / on other ranks. */
int pita_mala_propose(const float* x, const float* force, float* x_prop, const float* noise, int64_t B,
                      int n_particles, int n_dim, const double* dt_dev, uint64_t seed, uint64_t walker_offset,
                      const int64_t* walker_ids /*nullable*/, int64_t step, void* stream);
int pita_mala_accept(float* x, float* logp, const float* force, const float* x_prop, const float* logp_prop,
                     const float* force_prop, const float* uniforms, int64_t B, int n_particles, int n_dim,
                     const double* dt_dev, uint64_t seed, uint64_t walker_offset, const int64_t* walker_ids /*nullable*/,
                     int64_t step, int remove_mean, int* acc_count, void* stream);
int pita_mala_adapt(double* dt_dev, int* acc_count, int64_t total, int adaptive, float* rate_out, void* stream);
/* The three steps per population (see pita_lj_mala_pop for the population of a row): dt_dev fp64 [n_pop] and acc_count
 * int [n_pop]; propose and accept read dt_dev[population of the row], accept adds into acc_count[population]; adapt runs
 * the rule above, in the same arithmetic, for every population against totals (device int64 [n_pop]) -> rate_out [n_pop]
 * (nullable) and zeroes acc_count.  A population with totals[p] == 0 keeps its dt and gets a NaN rate.  Null dt_dev /
 * acc_count / totals, n_pop < 1, pop_size < 1 and B < 0 are PITA_EINVAL before any device call. */
int pita_mala_propose_pop(const float* x, const float* force, float* x_prop, const float* noise, int64_t B,
                          int n_particles, int n_dim, const double* dt_dev, int n_pop, int64_t pop_size, uint64_t pop_base,
                          uint64_t seed, uint64_t walker_offset, const int64_t* walker_ids /*nullable*/, int64_t step,
                          void* stream);
int pita_mala_accept_pop(float* x, float* logp, const float* force, const float* x_prop, const float* logp_prop,
                         const float* force_prop, const float* uniforms, int64_t B, int n_particles, int n_dim,
                         const double* dt_dev, int n_pop, int64_t pop_size, uint64_t pop_base, uint64_t seed,
                         uint64_t walker_offset, const int64_t* walker_ids /*nullable*/, int64_t step, int remove_mean,
                         int* acc_count, void* stream);
int pita_mala_adapt_pop(double* dt_dev, int* acc_count, const int64_t* totals, int n_pop, int adaptive, float* rate_out,
                        void* stream);

/* ---------------------------------------------------------------- resampling (K10, K11)
 * K10 systematic resampling, replaces sample_cat_sys (utils.py:111-120): weights =
 * clip(softmax(logits),1e-6,1) (not renormalised), inclusive fp32 cumsum, u_k = (u0 + k/B) mod 1
 * in fp64, ids = digitize(u, bins, right=True) clamped to B-1.
 * Five short multi-block passes (block maxima, block sums, clipped-weight block sums, bins, binary search), fixed
 * summation order; exp evaluated in double and rounded once.
 * workspace: 8-byte aligned device scratch of at least pita_resample_workspace_bytes(B) bytes. */
size_t pita_resample_workspace_bytes(int64_t B);
int pita_systematic_resample(const float* logits, int64_t B, double u0, int64_t* ids,
                             void* workspace, void* stream);
/* out[k, :] = src[ids[k], :] */
int pita_gather_rows(const float* src, const int64_t* ids, float* out, int64_t B, int D,
                     void* stream);

/* Number of distinct parents of one resampling event, max(1, #{i : ids[i] != ids[(i - 1) mod B]}), written to the device
 * word `out` (no host synchronisation): the ids of a systematic resampling are non-decreasing up to the cyclic rotation by
 * the event's uniform (utils.py:111-120), so every distinct parent is one cyclic run.  Replaces
 * len(np.unique(choice)) of sde_integration.py:295. */
int pita_count_runs(const int64_t* ids, int64_t B, int64_t* out, void* stream);

/* ---------------------------------------------------------------- adaptive (ESS-triggered) resampling
 * An extension: the reference resamples on a fixed schedule and computes no weight diagnostics.
 *
 * stats (device double[6]) of B log-weights a:
 *  [0] m    = max over the finite entries (0 when there is none)
 *  [1] lmw  = m + log( (1/B) * sum_i exp(a_i - m) )      log of the mean weight; -inf entries contribute 0
 *  [2] ess  = (sum w)^2 / sum w^2,  w_i = exp(a_i - m)    0 when sum w is not a positive finite number
 *  [3] ess / B
 *  [4] number of NaN or +inf entries (excluded from every sum)
 *  [5] number of -inf entries
 * exp, the differences a_i - m and all sums in double; fixed summation order (bitwise run to run): one block of 1 024
 * threads, thread t takes a_t, a_{t+1024}, ..., xor-shuffle wave reduction, the 16 wave partials added in index order.
 * The block needs no scratch: pita_logweight_stats_workspace_bytes is 0 and `workspace` may then be null. */
size_t pita_logweight_stats_workspace_bytes(int64_t B);
int pita_logweight_stats(const float* a, int64_t B, double* stats, void* workspace, void* stream);

/* One resampling event decided on the device.  resampled = (theta >= 1) || (stats[4] > 0) || (ess <= theta * B).
 *  resampled == 1: ids = exactly what pita_systematic_resample(logits, B, u0) writes, bit for bit, for ANY input;
 *                  *n_unique = what pita_count_runs gives on them
 *  resampled == 0: ids[k] = k, *n_unique = B
 * stats as above (the same bits as pita_logweight_stats), always written.  n_unique nullable.  No host synchronisation,
 * no host-visible branch.  B >= 1, theta in [0, 1], u0 in [0, 1).
 * B <= 2 048 (pita_adaptive_resample_single_launch(B) == 1): ONE launch, one block that holds the log-weights in LDS
 * and walks the virtual blocks of the five passes in their order -- the threshold is where that launch was measured
 * faster than the multi-pass sequence (0.93 of its time at 2 048 walkers, 3.2 times it at 16 384).  Larger B: the stats
 * pass writes `resampled`, the five passes and the run count follow and return on entry when it is clear (the search
 * pass then writes the identity).
 * workspace: 8-byte aligned device scratch of at least pita_adaptive_resample_workspace_bytes(B) bytes. */
size_t pita_adaptive_resample_workspace_bytes(int64_t B);
int pita_adaptive_resample(const float* logits, int64_t B, double u0, double theta, int64_t* ids, int64_t* n_unique,
                           double* stats, int* resampled, void* workspace, void* stream);
/* 1 when B takes the one-launch path, 0 for the gated multi-pass path */
int pita_adaptive_resample_single_launch(int64_t B);

/* n_pop independent populations of pop_size walkers each, one event per population, in ONE launch: block p owns rows
 * [p * pop_size, (p + 1) * pop_size) of every array and does exactly what
 *   pita_adaptive_resample(logits + p * pop_size, pop_size, u0_dev[p], theta, ...)
 * does: stats row p (device double[n_pop, 6]), resampled[p] and n_unique[p] (nullable) are that call's bits, and
 * ids[p * pop_size + k] = p * pop_size + (that call's ids[k]) -- GLOBAL rows, so pita_gather_rows takes the vector as it
 * is.  theta >= 1 is the fixed schedule (every population resamples).  logw_next (nullable, device [n_pop * pop_size]):
 * 0 where population p resampled, logits where it did not; it may be `logits` itself (a block reads its slice into LDS
 * before it writes anything).  Blocks share nothing and there are no atomics: a population's bits depend neither on n_pop
 * nor on p.  u0_dev: DEVICE double[n_pop], each in [0, 1) (not checked: the host never reads it).  theta in [0, 1].
 * 1 <= pop_size <= 2 048, what one block holds in LDS (pita_adaptive_resample_single_launch); a larger pop_size is
 * PITA_EUNSUPPORTED.  All argument checks run before any device call.  workspace: 8-byte aligned, at least
 * pita_population_resample_workspace_bytes bytes (the event needs no scratch; the size is never 0). */
size_t pita_population_resample_workspace_bytes(int64_t n_pop, int64_t pop_size);
int pita_population_resample(const float* logits, int64_t n_pop, int64_t pop_size, const double* u0_dev, double theta,
                             int64_t* ids, int64_t* n_unique, double* stats, int* resampled, float* logw_next,
                             void* workspace, void* stream);

/* The same events for populations of ANY size (pop_size >= 1, no PITA_EUNSUPPORTED case): arguments, outputs and
 * argument checks of pita_population_resample, and the same contract -- population p's stats row, resampled[p],
 * n_unique[p], ids (global rows) and logw_next are, bit for bit, those of
 *   pita_adaptive_resample(logits + p * pop_size, pop_size, u0_dev[p], theta, ...)
 * on its slice, whatever n_pop and p are (systematic resampling of utils.py:111-120 per population).  Always the
 * multi-block route, also for pop_size <= 2 048: one statistics block per population (the single-block summation order of
 * pita_adaptive_resample, so the ESS bits and the decisions are its own) writes resampled[p]; the five passes of
 * pita_systematic_resample follow over a (virtual block of 1 024 walkers, population) grid, every block testing its
 * population's flag; the search pass writes global rows, the identity where the flag is clear, and logw_next; one block
 * per population counts the runs (n_unique[p] = pop_size where it did not resample).  At most seven launches whatever
 * n_pop is (six when n_unique is null), stream order only: no grid barrier, no atomics, no host read; blocks of different
 * populations share nothing.  logw_next may be `logits`: every pass that reads logits for the bins precedes the search
 * pass in stream order, which copies an element only onto its own index.
 * workspace: 8-byte aligned device scratch of at least pita_population_resample_blocks_workspace_bytes bytes = n_pop
 * copies of pita_systematic_resample's layout (n_pop * pita_resample_workspace_bytes(pop_size)). */
size_t pita_population_resample_blocks_workspace_bytes(int64_t n_pop, int64_t pop_size);
int pita_population_resample_blocks(const float* logits, int64_t n_pop, int64_t pop_size, const double* u0_dev, double theta,
                                    int64_t* ids, int64_t* n_unique, double* stats, int* resampled, float* logw_next,
                                    void* workspace, void* stream);

/* ---------------------------------------------------------------- weighted per-population observables
 * An extension: the reference's evaluation counts every walker once and treats the batch as one population.
 *
 * The batch is n_pop populations of pop_size walkers, population p in rows [p * pop_size, (p + 1) * pop_size) (the
 * integrator's layout).  logw: device float [n_pop * pop_size], nullable = unit weights.  Per population p:
 *  m_p = max over the finite entries of its logw (0 when there is none; pita_logweight_stats' convention),
 *  relative weight of walker i: w_i = exp((double)logw_i - m_p), in double;
 *  a walker whose logw is NaN or +inf is left out of every sum and counted in n_bad, one whose logw is -inf has
 *  weight 0 and is counted in n_neg_inf (and in `counts`).
 * The weighted bin sums are FIXED-POINT integers: with shift = min(40, 62 - ceil(log2(pop_size * values per walker)))
 * every value adds q_i = (uint64) rint(w_i * 2^shift) to its bin with integer adds only (LDS-privatised bins per block,
 * a block works on one population, one 64-bit integer add per non-empty bin and block), so a population's total stays
 * below 2^63 and its output bits depend neither on n_pop, nor on p, nor on the ORDER of the walkers inside the
 * population, nor on the run.  shift < 20 (more than 2^42 values per population) is PITA_EUNSUPPORTED.  All argument
 * checks run before any device call.  Outputs are overwritten.
 *
 * pita_weighted_histogram: v float [n_pop * pop_size * per_walker], value k belongs to walker k / per_walker; bins as
 * pita_histogram counts them (the same device function), 1 <= nbins <= 1024.
 *  wsum   uint64 [n_pop, nbins]  the fixed-point sums; the weighted histogram is wsum * 2^-shift
 *  counts uint64 [n_pop, nbins]  the plain counts over the walkers that were not left out; with n_pop = 1,
 *                                per_walker = 1 and logw = NULL exactly what pita_histogram writes
 *  info   double [n_pop, 4]      {m_p, n_bad, n_neg_inf, shift} */
int pita_weighted_histogram(const float* v, const float* logw /*nullable*/, int64_t n_pop, int64_t pop_size,
                            int64_t per_walker, const float* edges, int nbins, unsigned long long* wsum,
                            unsigned long long* counts, double* info, void* stream);
/* The same histogram over the n (n - 1) / 2 upper-triangle pair distances of every walker, from the coordinates x
 * (float [n_pop * pop_size, n_particles * n_dim]) with no distance array in memory: a block stages a chunk of its
 * population's walkers in LDS and its threads stride over the (walker, pair) items; every pair carries its walker's
 * weight.  2 <= n_particles <= 256, 1 <= n_dim <= 3.  Arithmetic, in fp32 without contraction, so that a numpy float32
 * restatement is bit-identical: per dimension delta = x_j - x_i (i < j); s = delta_0 * delta_0, then s = s + delta_1 *
 * delta_1, then s = s + delta_2 * delta_2; r = sqrt(s) correctly rounded.  wsum, counts and info are bit for bit those
 * of pita_weighted_histogram(per_walker = n (n - 1) / 2) on these distances. */
int pita_pair_distance_histogram(const float* x, const float* logw /*nullable*/, int64_t n_pop, int64_t pop_size,
                                 int n_particles, int n_dim, const float* edges, int nbins, unsigned long long* wsum,
                                 unsigned long long* counts, double* info, void* stream);
/* Weighted moments of one value per walker: out double [n_pop, 6] = {m_p, sum w, sum w v, sum w v^2, n_bad, n_neg_inf}
 * (v float [n_pop * pop_size]).  Here a walker is ALSO left out, and counted in n_bad, when its value is not finite;
 * n_neg_inf counts the walkers with logw = -inf among the others; m_p is over all finite logw of the population.
 * fp64 sums in a fixed order: one block of 1 024 threads per population, thread t takes rows t, t + 1024, ...,
 * xor-shuffle wave reduction, the 16 wave partials added in index order (pita_logweight_stats' order).  The bits of a
 * population therefore depend on the ORDER of its rows (unlike the two histograms), but neither on n_pop nor on p. */
int pita_weighted_moments(const float* v, const float* logw /*nullable*/, int64_t n_pop, int64_t pop_size, double* out,
                          void* stream);

/* ---------------------------------------------------------------- dihedral angles and weighted Ramachandran maps
 * An extension: the reference takes (phi, psi) from mdtraj on the host, unweighted, the batch as one population.
 *
 * x: device float [B, n_atoms * 3], 3-D coordinates, 4 <= n_atoms <= 256 (the force field's limit).  A quad is four
 * atoms (i, j, k, l); its angle is the torsion of pita_ff_logp_force, formula and sign, in fp32 without contraction, every
 * operation rounded on its own, so that a numpy float32 restatement differs only by atan2f's last ulps:
 *   b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k;  n1 = b1 x b2, n2 = b2 x b3 (a_y b_z - a_z b_y, ...);
 *   y = (b1 . n2) * sqrt(b2 . b2), the root correctly rounded;  xv = n1 . n2;  dots as ((p0 + p1) + p2);
 *   theta = atan2f(y, xv) in [-pi, pi].
 * Collinear atoms give atan2f of two zeros, which is 0 (pi where xv is -0): a value like any other, counted like any
 * other.  Where y or xv is not finite -- a non-finite coordinate among the four atoms, or products beyond the fp32
 * range -- the angle is NaN.
 * quads live on the DEVICE (int32), so the entry points cannot check them without a copy: the CALLER guarantees
 * 0 <= index < n_atoms (four distinct atoms for a meaningful angle); pita_amd.metrics checks before it uploads.
 * All argument checks run before any device call.  Both kernels stage chunks of walker rows in LDS with coalesced reads.
 *
 * pita_dihedral_angles: out float [B, n_dih], out[b, k] = angle of quad k (quads int32 [n_dih, 4]) of walker b;
 * 1 <= n_dih <= 1024; B = 0 is a no-op. */
int pita_dihedral_angles(const float* x, int64_t B, int n_atoms, const int32_t* quads, int n_dih, float* out, void* stream);
/* Importance-weighted 2-D histograms of angle pairs per population, from the coordinates, no angle in memory.
 * quads int32 [n_pair, 2, 4]: the a-quad and the b-quad of every pair (phi and psi of a residue), 1 <= n_pair <= 64.
 * Each angle is binned on its own axis by the rule of pita_histogram (the same device function): edges_a / edges_b
 * device float [nbins_a + 1] / [nbins_b + 1], ascending, the last bin closed -- +pi falls into the last bin, there is
 * no wrap-around.  A walker is left out of a pair's cells when either angle is NaN or outside its edges.
 * Populations, logw, m_p, the left-out walkers and the fixed-point sums are those of pita_weighted_histogram with
 * shift = min(40, 62 - ceil(log2(pop_size))) (one value per walker and cell array); a block works on one (population,
 * pair) with LDS-privatised 64-bit cells and ends with one 64-bit integer add per non-empty cell, so the output bits
 * depend neither on the order of the walkers, nor on n_pop, nor on p, nor on the run.
 *  wsum   uint64 [n_pop, n_pair, nbins_a, nbins_b]  the fixed-point sums; the weighted histogram is wsum * 2^-shift
 *  counts uint64 [n_pop, n_pair, nbins_a, nbins_b]  plain counts over the walkers that were not left out
 *  info   double [n_pop, 4]                         {m_p, n_bad, n_neg_inf, shift}
 * nbins_a, nbins_b >= 1; nbins_a * nbins_b <= 4096 (64 x 64: the sums and counts of a block are then 64 KB of the
 * 160 KB of LDS), a larger product is PITA_EUNSUPPORTED, as is shift < 20.  Outputs are overwritten. */
int pita_dihedral_histogram2d(const float* x, const float* logw /*nullable*/, int64_t n_pop, int64_t pop_size, int n_atoms,
                              const int32_t* quads, int n_pair, const float* edges_a, int nbins_a, const float* edges_b,
                              int nbins_b, unsigned long long* wsum, unsigned long long* counts, double* info,
                              void* stream);

/* ---------------------------------------------------------------- weighted per-population mix-RBF Gram sums (MMD)
 * The sample-space member of the family above.  The reference's mmd.py (mix_rbf_mmd2, called with the bandwidths 0.01,
 * 0.1, 1, 10, 100) was never restated in oracle/: THIS definition is the specification -- unpinned by construction, like
 * DW4 and the POT W2.  Mix-RBF kernel k(x, y) = sum_s exp(-gamma_s |x - y|^2), gamma_s = 1 / (2 sigma_s^2).
 *
 * a: device float [n_pop * pop_size, dim], population p in rows [p * pop_size, (p + 1) * pop_size) (the integrator's
 * layout), relative row weights w_i from logw_a.  b: device float [n_b, dim], ONE set shared by every population, row
 * weights v_j from logw_b.  logw_*: device float, nullable = unit weights.  The call writes
 *  sums   double [n_pop, n_gamma]  S[p, s] = sum_i sum_j w_i v_j exp(-gamma_s |a_i - b_j|^2), i over population p
 *  info_a double [n_pop, 5]        {m_p, sum w, sum w^2, n_bad, n_neg_inf}
 *  info_b double [5]               the same for b (nullable: not wanted)
 * With b == NULL (self mode) population p is summed against itself, every ordered pair and the diagonal included; then
 * logw_b must be NULL and n_b 0, and info_b is ignored.  1 <= dim <= 768 (the force field's 256 atoms x 3), 1 <= n_gamma
 * <= 16, every gamma finite and >= 0; gammas is a HOST array, read in the call, and travels as kernel arguments.  All
 * argument checks run before any device call (PITA_EINVAL); sizes whose block or element counts overflow are
 * PITA_EUNSUPPORTED.  workspace: 8-byte aligned device scratch of at least pita_rbf_gram_workspace_bytes(n_pop, pop_size,
 * n_b) bytes (n_b = 0: self mode; 0 is returned for sizes the call refuses).  Outputs are overwritten.
 *
 * Weights, the family's convention: m_p = max over the finite log-weights of the population (0 when there is none), w =
 * exp((double)logw - m_p) rounded to fp32 ONCE; a row whose logw is NaN or +inf, or which holds a coordinate that is
 * not finite (as pita_weighted_moments does for values), is left out and counted in n_bad; a row with logw = -inf among
 * the others has weight 0 and is counted in n_neg_inf.  A weights pass writes the fp32 row weights (0 for a row left
 * out) to the workspace; sum w and sum w^2 are sums of those fp32 weights, in double, in pita_weighted_moments' fixed
 * order.  A row of weight 0 contributes exactly 0 by SELECTION: its squared distance is replaced by 0 before the
 * exponential, so that NaN coordinates never meet a product.
 *
 * Pair arithmetic, fp32, vector pipe, no contraction beyond the fmaf named here: d_k = a_k - b_k first, then s =
 * fmaf(d_k, d_k, s) over k in index order from s = 0; s = min(s, FLT_MAX) (finite rows whose distance overflows: gamma =
 * 0 still gives 1, every other gamma 0); e = exp2(c_s * s) by the hardware's exp2 (about 1 ulp), c_s = (float)(-gamma_s *
 * log2 e) computed in double on the host; term = (w_i * v_j) * e.  Two bit-identical rows therefore give s = 0 and e = 1
 * EXACTLY for every gamma -- the reason the distance does not go through |a|^2 + |b|^2 - 2 a.b or the matrix pipe: after
 * a resampling event many walkers are copies, and the rounding noise of the expanded form would be multiplied by gamma
 * (5 000 at sigma = 0.01).  fp32 accumulation is confined to the 16 terms a thread holds of one 64 x 64 tile pair (its 4
 * x 4 sub-tile, a-row outer, b-row inner); everything above is double.
 *
 * Reduction: no floating-point atomics.  A block takes one (population, a-tile of 64 rows) and every nbg-th b-tile,
 * nbg a function of (pop_size, n_b) alone; threads add their tiles in double, xor-shuffle wave reduction, the four
 * wave partials in index order, one partial per block; a second kernel adds a population's partials in a fixed order.
 * Self mode visits only the tile pairs jb >= ia and counts an off-diagonal tile twice (a multiplication by 2 in double).
 * The bits of population p are the same from run to run and depend neither on n_pop nor on p (a call on its slice alone
 * gives the same bits); they DO depend on the order of the rows, as pita_weighted_moments' do. */
size_t pita_rbf_gram_workspace_bytes(int64_t n_pop, int64_t pop_size, int64_t n_b);
int pita_rbf_gram_sums(const float* a, const float* logw_a /*nullable*/, int64_t n_pop, int64_t pop_size,
                       const float* b /*nullable = self mode*/, const float* logw_b /*nullable*/, int64_t n_b, int dim,
                       const double* gammas /*HOST, n_gamma entries*/, int n_gamma, double* sums, double* info_a,
                       double* info_b /*nullable*/, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PITA_HIP_H */
