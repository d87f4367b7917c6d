// Elementwise pieces of the sampler and systematic resampling for gfx950.
//
// Replaces (paths relative to /root/reference/pita/src/):
//   models/components/sde_integration.py:347-349   x += drift*dt + diffusion*sqrt(dt)
//   models/components/sdes.py:245-251              diffusion = scale * g(t) * randn_like(x)
//   utils/data_utils.py:4-26                       remove_mean
//   energies/base_prior.py:77-83                   MeanFreePrior.sample
//   models/components/utils.py:111-120             sample_cat_sys (systematic resampling)
//   models/components/sde_integration.py:293       x = x[choice]
//   models/components/sde_integration.py:28-45     mala_proposal
//   models/components/sde_integration.py:379-398, 430-461   MALA accept/reject, step-size adaptation
#include "common.h"
#include "hist_common.h"

namespace pita {

// One thread per (walker, particle); WB = floor(256/n) walkers per block staged in LDS so the
// per-walker mean is a broadcast read and every global access is one coalesced span.
enum { OP_EM = 0, OP_PRIOR = 1, OP_RMEAN = 2, OP_NORMAL = 3 };

struct ElemParams {
  float dt, noise_scale, sqrt_dt, scale;
  unsigned long long seed, walker_offset;
  long long step;
  int remove_mean;
  const long long* walker_ids;  // optional: Philox walker key of row w is walker_ids[w] instead of walker_offset + w
  double* stats_out;            // OP_EM, nullable [4]: += sum / sum of squares of drift and of noise_scale * xi
};

template <int DIM, int OP>
__global__ void __launch_bounds__(256) elem_kernel(float* __restrict__ x, const float* __restrict__ drift,
                                                   const float* __restrict__ noise, long long B, int n, int WB,
                                                   ElemParams p) {
  extern __shared__ float sm[];  // [WB*n*DIM]
  __shared__ double red[4][4];   // OP_EM moments: one commit per BLOCK at the end of its grid-stride loop (an atomic per
                                 // wave and batch of WB walkers -- 55 000 double atomics on four addresses at 65 536 LJ13
                                 // walkers -- made this the slowest small kernel of a debiased step: 0.67 ms)
  const int tid = threadIdx.x;
  const long long nblk = (B + WB - 1) / WB;
  double momd[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const long long w0 = blk * WB;
    const int nw = (int)((B - w0) < WB ? (B - w0) : WB);
    const int w = tid / n, i = tid - w * n;
    const bool act = w < nw;
    float v[DIM];
    float mom[4] = {0.f, 0.f, 0.f, 0.f};
    if (act) {
      const long long base = ((w0 + w) * n + i) * DIM;
      float xi[4] = {0.f, 0.f, 0.f, 0.f};
      if (OP == OP_EM || OP == OP_PRIOR || OP == OP_NORMAL) {
        if (noise) {
#pragma unroll
          for (int k = 0; k < DIM; ++k) xi[k] = noise[base + k];
        } else {
          philox_normal4(p.seed, p.walker_offset + (unsigned long long)(w0 + w), p.step, (uint32_t)i, xi);
        }
      }
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        if (OP == OP_EM) {
          const float dr = drift[base + k], dif = p.noise_scale * xi[k];
          v[k] = x[base + k] + (dr * p.dt + (dif * p.sqrt_dt));
          if (p.stats_out) {
            mom[0] += dr; mom[1] = fmaf(dr, dr, mom[1]);
            mom[2] += dif; mom[3] = fmaf(dif, dif, mom[3]);
          }
        }
        if (OP == OP_PRIOR) v[k] = xi[k] * p.scale;
        if (OP == OP_RMEAN) v[k] = x[base + k];
        if (OP == OP_NORMAL) v[k] = xi[k];
        sm[(w * n + i) * DIM + k] = v[k];
      }
    }
    if (OP == OP_EM && p.stats_out) {
#pragma unroll
      for (int q = 0; q < 4; ++q) momd[q] += (double)mom[q];
    }
    __syncthreads();
    if (act) {
      const long long base = ((w0 + w) * n + i) * DIM;
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        if (p.remove_mean) {
          float s = 0.f;
          for (int q = 0; q < n; ++q) s += sm[(w * n + q) * DIM + k];
          v[k] -= s / (float)n;
        }
        x[base + k] = v[k];
      }
    }
    __syncthreads();
  }
  if (OP == OP_EM && p.stats_out) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double vq = momd[q];
      for (int o = 32; o > 0; o >>= 1) vq += __shfl_xor(vq, o, 64);
      if ((tid & 63) == 0) red[tid >> 6][q] = vq;
    }
    __syncthreads();
    if (tid < 4) atomicAdd(p.stats_out + tid, (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]));
  }
}

template <int OP>
static int launch_elem(float* x, const float* drift, const float* noise, int64_t B, int n, int d, const ElemParams& p,
                       void* stream) {
  PITA_REQUIRE(B >= 0, "elementwise: negative batch");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(x, "elementwise: null argument");
  PITA_REQUIRE(n >= 1 && n <= 256, "elementwise: n_particles must be in [1,256]");
  PITA_REQUIRE(d >= 1 && d <= 3, "elementwise: n_dim must be 1, 2 or 3");
  if (B == 0) return PITA_OK;
  const int WB = 256 / n;
  const long long nblk = (B + WB - 1) / WB;
  // with moments: a grid-stride loop over fewer blocks (one set of four atomics per block)
  const long long cap = (OP == OP_EM && p.stats_out) ? 256LL * 4 : 256LL * 16;
  const unsigned grid = (unsigned)(nblk < cap ? nblk : cap);
  const size_t lds = sizeof(float) * (size_t)(WB * n * d);
  hipStream_t s = (hipStream_t)stream;
  switch (d) {
    case 1: hipLaunchKernelGGL((elem_kernel<1, OP>), dim3(grid), dim3(256), lds, s, x, drift, noise, B, n, WB, p); break;
    case 2: hipLaunchKernelGGL((elem_kernel<2, OP>), dim3(grid), dim3(256), lds, s, x, drift, noise, B, n, WB, p); break;
    default: hipLaunchKernelGGL((elem_kernel<3, OP>), dim3(grid), dim3(256), lds, s, x, drift, noise, B, n, WB, p); break;
  }
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

// sum and sum of squares of a device vector (per-step statistics of SDETerms fields, sde_integration.py:150)
__global__ void __launch_bounds__(256) moments_kernel(const float* __restrict__ v, long long n, double* __restrict__ out) {
  double s = 0.0, s2 = 0.0;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const double a = (double)v[e];
    s += a;
    s2 += a * a;
  }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); s2 += __shfl_xor(s2, o, 64); }
  if ((threadIdx.x & 63) == 0) { atomicAdd(out, s); atomicAdd(out + 1, s2); }
}

// ---------------------------------------------------------------------------- EDM preconditioning around a foreign backbone
// score_net.py:13-43 for backbones that are not fused HIP kernels (any module with forward(t, x, beta)):
//   scale : x_in = c_in x, t_in = c_noise = ln(h)/8                       (inputs of the backbone)
//   combine: D = c_s x + c_out F; optional beta preconditioning (:36-38); score = (D - x)/h
__global__ void __launch_bounds__(256) edm_scale_kernel(const float* __restrict__ h, const float* __restrict__ x,
                                                        float* __restrict__ xs, float* __restrict__ cn, long long B, int D) {
  const long long total = B * D;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long b = e / D;
    const float hv = h[b];
    xs[e] = (1.0f / sqrtf(1.0f + hv)) * x[e];
    if (e - b * D == 0) cn[b] = 0.125f * logf(hv);
  }
}

__global__ void __launch_bounds__(256) edm_combine_kernel(const float* __restrict__ h, const float* __restrict__ x,
                                                          const float* __restrict__ F, const float* __restrict__ beta,
                                                          float* __restrict__ Dout, float* __restrict__ score, long long B,
                                                          int D) {
  const long long total = B * D;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long b = e / D;
    const float hv = h[b], xv = x[e];
    const float c_s = 1.0f / (1.0f + hv), c_in = 1.0f / sqrtf(1.0f + hv), c_out = sqrtf(hv) * c_in;
    float Dv = c_s * xv + c_out * F[e];
    float sc = (Dv - xv) / hv;
    if (beta) {
      const float bt = beta[b];
      Dv = Dv * bt + (1.0f - bt) * xv;
      sc = sc * bt;
    }
    if (Dout) Dout[e] = Dv;
    if (score) score[e] = sc;
  }
}

// ---------------------------------------------------------------------------- MALA
// The step size lives on the device (double, like the Python float it replaces) so the adaptive chain
// runs without a host round trip per step; the kernels round it to fp32 where torch would.
// The per-population chain (pita_mala_*_pop) instantiates the kernels with one trailing PopKeys argument: dt_dev and
// acc_count are then [n_pop] and every walker reads and counts in the entry of its own population.
struct PopKeys {
  unsigned long long base;  // population of the walker with Philox key k: (k - base) / size
  long long size;
  __device__ __forceinline__ int of(unsigned long long key) const { return (int)((key - base) / (unsigned long long)size); }
};
template <class T>
__device__ __forceinline__ const T& only(const T& t) { return t; }

template <int DIM, class... Pop>
__global__ void __launch_bounds__(256) mala_propose_kernel(const float* __restrict__ x, const float* __restrict__ force,
                                                           float* __restrict__ x_prop, const float* __restrict__ noise,
                                                           long long B, int n, const double* __restrict__ dt_dev,
                                                           ElemParams p, Pop... pk) {
  constexpr bool POP = sizeof...(Pop) != 0;
  float hdt = 0.f, sdt = 0.f;
  if constexpr (!POP) { hdt = (float)(0.5 * dt_dev[0]); sdt = (float)sqrt(dt_dev[0]); }
  const long long total = B * n;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long w = t / n;
    const int i = (int)(t - w * n);
    const long long base = t * DIM;
    if constexpr (POP) {
      const double dt = dt_dev[only(pk...).of(p.walker_ids ? (unsigned long long)p.walker_ids[w]
                                                           : p.walker_offset + (unsigned long long)w)];
      hdt = (float)(0.5 * dt); sdt = (float)sqrt(dt);
    }
    float xi[4] = {0.f, 0.f, 0.f, 0.f};
    if (noise) {
#pragma unroll
      for (int k = 0; k < DIM; ++k) xi[k] = noise[base + k];
    } else {
      philox_normal4(p.seed, p.walker_ids ? (unsigned long long)p.walker_ids[w] : p.walker_offset + (unsigned long long)w,
                     p.step, (uint32_t)i, xi);
    }
#pragma unroll
    for (int k = 0; k < DIM; ++k) x_prop[base + k] = (x[base + k] + hdt * force[base + k]) + sdt * xi[k];
  }
}

template <int DIM, class... Pop>
__global__ void __launch_bounds__(256) mala_accept_kernel(float* __restrict__ x, float* __restrict__ logp,
                                                          const float* __restrict__ force, const float* __restrict__ x_prop,
                                                          const float* __restrict__ logp_prop,
                                                          const float* __restrict__ force_prop,
                                                          const float* __restrict__ uniforms, long long B, int n, int WB,
                                                          const double* __restrict__ dt_dev, int* __restrict__ acc_count,
                                                          ElemParams p, Pop... pk) {
  constexpr bool POP = sizeof...(Pop) != 0;
  extern __shared__ float sm[];
  float* xsel = sm;                      // [WB*n*DIM] accepted/kept coordinates
  float* qf = sm + WB * n * DIM;         // [WB*n] partial |x' - fwd_mean|^2
  float* qb = qf + WB * n;               // [WB*n] partial |x - bwd_mean|^2
  float* flag = qb + WB * n;             // [WB]   1.0 = accepted
  int* popl = reinterpret_cast<int*>(flag + WB);  // POP: [WB] population of the block's walkers
  float hdt = 0.f, tdt = 0.f;
  if constexpr (!POP) { hdt = (float)(0.5 * dt_dev[0]); tdt = (float)(2.0 * dt_dev[0]); }
  const int tid = threadIdx.x;
  const long long nblk = (B + WB - 1) / WB;
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const long long w0 = blk * WB;
    const int nw = (int)((B - w0) < WB ? (B - w0) : WB);
    const int w = tid / n, i = tid - w * n;
    const bool act = w < nw;
    const long long base = ((w0 + w) * n + i) * DIM;
    float xo[DIM], xp[DIM];
    if constexpr (POP) {
      if (act) {
        const int pop = only(pk...).of(p.walker_ids ? (unsigned long long)p.walker_ids[w0 + w]
                                                    : p.walker_offset + (unsigned long long)(w0 + w));
        const double dt = dt_dev[pop];
        hdt = (float)(0.5 * dt); tdt = (float)(2.0 * dt);
        if (i == 0) popl[w] = pop;
      }
    }
    if (act) {
      float sf = 0.f, sb = 0.f;
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        xo[k] = x[base + k];
        xp[k] = x_prop[base + k];
        const float df = xp[k] - (xo[k] + hdt * force[base + k]);
        const float db = xo[k] - (xp[k] + hdt * force_prop[base + k]);
        sf += df * df;
        sb += db * db;
      }
      qf[w * n + i] = sf;
      qb[w * n + i] = sb;
    }
    __syncthreads();
    if (act && i == 0) {
      float sf = 0.f, sb = 0.f;
      for (int j = 0; j < n; ++j) { sf += qf[w * n + j]; sb += qb[w * n + j]; }
      const float lqf = -sf / tdt, lqb = -sb / tdt;
      const float lp = logp[w0 + w], lpp = logp_prop[w0 + w];
      const float ratio = (lpp - lp) + (lqb - lqf);
      const float u = uniforms ? uniforms[w0 + w]
                               : philox_uniform(p.seed, p.walker_ids ? (unsigned long long)p.walker_ids[w0 + w]
                                                                     : p.walker_offset + (unsigned long long)(w0 + w),
                                                p.step, 0xFFFFFu);
      const float af = (logf(u) < ratio) ? 1.0f : 0.0f;
      logp[w0 + w] = af * lpp + (1.0f - af) * lp;
      flag[w] = af;
    }
    __syncthreads();
    float v[DIM];
    if (act) {
      const float af = flag[w];
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        v[k] = af * xp[k] + (1.0f - af) * xo[k];
        xsel[(w * n + i) * DIM + k] = v[k];
      }
    }
    if (tid == 0) {
      int c = 0;
      if constexpr (POP) {  // a block's walkers can straddle populations: one add per run of equal populations
        for (int j = 0; j < nw; ++j) {
          c += flag[j] != 0.f;
          if (c && (j + 1 == nw || popl[j + 1] != popl[j])) {
            atomicAdd(&acc_count[popl[j]], c);
            c = 0;
          }
        }
      } else {
        for (int j = 0; j < nw; ++j) c += flag[j] != 0.f;
        if (c) atomicAdd(acc_count, c);
      }
    }
    __syncthreads();
    if (act) {
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        if (p.remove_mean) {
          float s = 0.f;
          for (int j = 0; j < n; ++j) s += xsel[(w * n + j) * DIM + k];
          v[k] -= s / (float)n;
        }
        x[base + k] = v[k];
      }
    }
    __syncthreads();
  }
}

__global__ void mala_adapt_kernel(double* dt_dev, int* acc_count, long long total, int adaptive, float* rate_out) {
  const float rate = (float)acc_count[0] / (float)total;
  if (rate_out) rate_out[0] = rate;
  if (adaptive) dt_dev[0] = ((double)rate > 0.55) ? dt_dev[0] * 1.1 : dt_dev[0] / 1.1;  // sde_integration.py:439-443
  acc_count[0] = 0;
}

// the rule of mala_adapt_kernel for every population, one thread each; a population without walkers keeps its step size
__global__ void __launch_bounds__(64) mala_adapt_pop_kernel(double* dt_dev, int* acc_count, const long long* totals,
                                                            int n_pop, int adaptive, float* rate_out) {
  const int pop = blockIdx.x * 64 + threadIdx.x;
  if (pop >= n_pop) return;
  const long long total = totals[pop];
  const float rate = total > 0 ? (float)acc_count[pop] / (float)total : NAN;
  if (rate_out) rate_out[pop] = rate;
  if (adaptive && total > 0) dt_dev[pop] = ((double)rate > 0.55) ? dt_dev[pop] * 1.1 : dt_dev[pop] / 1.1;
  acc_count[pop] = 0;
}

// ---------------------------------------------------------------------------- resampling
// Systematic resampling (utils.py:111-120) as five short multi-block passes over the logits, all in a fixed
// summation order (bitwise reproducible), 1 024 walkers per block:
//   A  block maxima                      B  block sums of exp(l - max) in double
//   C  block sums of the clipped weights clip(exp(l - max) / sum, 1e-6, 1) in double
//   D  bins = inclusive cumsum: blocks' prefix (sequential over the block totals) + in-block scan, accumulated in
//      double and rounded to fp32 per prefix -- torch's CPU cumsum semantics (float input, double accumulator)
//   E  ids[k] = #bins < u_k (digitize right=True), one thread per k, binary search
// exp is evaluated in double and rounded once: the correctly rounded fp32 exponential, which is what torch-CPU's
// (SLEEF, <= 1 ulp) expf returns in all but a vanishing fraction of arguments; the ocml expf differs from it far
// more often and each difference can move an id whose uniform lies within an ulp of a bin edge.
constexpr int RS_T = 256, RS_E = 1024;  // threads and elements per block

__device__ __forceinline__ float rs_exp(float v) { return (float)exp((double)v); }

// The arithmetic of the passes lives in the rs_pass_* device functions of (virtual block vb of RS_E elements, thread t of
// RS_T): the multi-block kernels run one virtual block per block (vb = blockIdx.x, t = threadIdx.x), the one-launch kernel
// of the adaptive event (adaptive_resample_block_kernel) runs all of them in ONE block of four groups of RS_T threads.  The
// summation order -- and with it every bit of the ids -- is theirs alone.  Functions with a barrier are called by every
// thread of the block (a virtual block past the end loads nothing and contributes nothing).
__device__ __forceinline__ double block_sum_d(double v, double* red, int t) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  double r = 0.0;
  for (int k = 0; k < RS_T / 64; ++k) r += red[k];
  return r;
}

// pass A: the maximum of virtual block vb (valid in t == 0); red: RS_T / 64 slots of the virtual block
__device__ __forceinline__ float rs_pass_max(const float* logits, long long B, long long vb, int t, float* red) {
  const long long lo = vb * RS_E;
  float mx = -INFINITY;
  for (int i = t; i < RS_E; i += RS_T)
    if (lo + i < B) mx = fmaxf(mx, logits[lo + i]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((t & 63) == 0) red[t >> 6] = mx;
  __syncthreads();
  if (t == 0)
    for (int k = 1; k < RS_T / 64; ++k) mx = fmaxf(mx, red[k]);
  return mx;
}

// the global maximum and the softmax denominator (rounded to fp32 once) from the blocks' partials, in index order
__device__ __forceinline__ float rs_fold_max(const float* bmax, int nblk) {
  float mx = -INFINITY;
  for (int k = 0; k < nblk; ++k) mx = fmaxf(mx, bmax[k]);
  return mx;
}
__device__ __forceinline__ double rs_fold_sum(const double* v, int nblk) {
  double t = 0.0;
  for (int k = 0; k < nblk; ++k) t += v[k];
  return t;
}

// passes B (phase 0: exp(l - max)) and C (phase 1: the clipped weights): the sum over virtual block vb, in every thread
__device__ __forceinline__ double rs_pass_sum(const float* logits, long long B, long long vb, int t, float mx, float sm,
                                              int phase, double* red) {
  const long long lo = vb * RS_E;
  double acc = 0.0;
  for (int i = t; i < RS_E; i += RS_T)
    if (lo + i < B) {
      float w = rs_exp(logits[lo + i] - mx);
      if (phase == 1) w = fminf(fmaxf(w / sm, 1e-6f), 1.0f);
      acc += (double)w;
    }
  return block_sum_d(acc, red, t);
}

// pass D: the bins of virtual block vb on top of `base`, the sum of the earlier blocks' totals; part: RS_T slots.  Every
// thread reads its own elements before it writes them: `bins` may be `logits` (the one-launch kernel scans in place).
__device__ __forceinline__ void rs_pass_bins(const float* logits, long long B, long long vb, int t, float mx, float sm,
                                             double base, double* part, float* bins) {
  constexpr int PER = RS_E / RS_T;  // contiguous elements per thread
  const long long lo = vb * RS_E + (long long)t * PER;
  float w[PER];
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    w[q] = (lo + q < B) ? fminf(fmaxf(rs_exp(logits[lo + q] - mx) / sm, 1e-6f), 1.0f) : 0.0f;
    acc += (double)w[q];
  }
  part[t] = acc;
  __syncthreads();
  if (t == 0) {
    double run = 0.0;
    for (int k = 0; k < RS_T; ++k) { const double v = part[k]; part[k] = run; run += v; }
  }
  __syncthreads();
  acc = base + part[t];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    acc += (double)w[q];
    if (lo + q < B) bins[lo + q] = (float)acc;
  }
}

// pass E for walker k: u_k = (u0 + fp32(k * fp32(1/B))) mod 1 in double; id = #bins < u  (digitize right=True), clamp
__device__ __forceinline__ long long rs_search(const float* bins, long long B, double u0, float invB, long long k) {
  const double u = fmod(u0 + (double)((float)k * invB), 1.0);
  long long a = 0, b = B;  // first index with bins[idx] >= u
  while (a < b) {
    const long long m = (a + b) >> 1;
    if ((double)bins[m] < u) a = m + 1; else b = m;
  }
  return (a >= B) ? B - 1 : a;
}

// one block's share of each multi-block pass: the body of the plain kernel and, behind the device flag, of the gated one
__device__ __forceinline__ void rs_max_block(const float* logits, long long B, float* bmax) {
  __shared__ float red[RS_T / 64];
  const float mx = rs_pass_max(logits, B, blockIdx.x, threadIdx.x, red);
  if (threadIdx.x == 0) bmax[blockIdx.x] = mx;
}
__device__ __forceinline__ void rs_sum_block(const float* logits, long long B, int nblk, const float* bmax,
                                             const double* bsum, double* out, int phase) {
  __shared__ double red[RS_T / 64];
  const float mx = rs_fold_max(bmax, nblk);
  const float sm = phase == 1 ? (float)rs_fold_sum(bsum, nblk) : 1.0f;
  const double acc = rs_pass_sum(logits, B, blockIdx.x, threadIdx.x, mx, sm, phase, red);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}
__device__ __forceinline__ void rs_bins_block(const float* logits, long long B, int nblk, const float* bmax,
                                              const double* bsum, const double* bw, float* bins) {
  __shared__ double part[RS_T];
  const float mx = rs_fold_max(bmax, nblk);
  const float sm = (float)rs_fold_sum(bsum, nblk);
  const double base = rs_fold_sum(bw, (int)blockIdx.x);
  rs_pass_bins(logits, B, blockIdx.x, threadIdx.x, mx, sm, base, part, bins);
}
__device__ __forceinline__ void rs_search_grid(const float* bins, long long B, double u0, long long* ids) {
  const float invB = (float)(1.0 / (double)B);
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < B; k += (long long)gridDim.x * 256)
    ids[k] = rs_search(bins, B, u0, invB, k);
}

__global__ void __launch_bounds__(RS_T) rs_max_kernel(const float* __restrict__ logits, long long B, float* __restrict__ bmax) {
  rs_max_block(logits, B, bmax);
}

// phase 0: sums of exp(l - max);  phase 1: sums of the clipped weights
__global__ void __launch_bounds__(RS_T) rs_sum_kernel(const float* __restrict__ logits, long long B, int nblk,
                                                      const float* __restrict__ bmax, const double* __restrict__ bsum,
                                                      double* __restrict__ out, int phase) {
  rs_sum_block(logits, B, nblk, bmax, bsum, out, phase);
}

__global__ void __launch_bounds__(RS_T) rs_bins_kernel(const float* __restrict__ logits, long long B, int nblk,
                                                       const float* __restrict__ bmax, const double* __restrict__ bsum,
                                                       const double* __restrict__ bw, float* __restrict__ bins) {
  rs_bins_block(logits, B, nblk, bmax, bsum, bw, bins);
}

__global__ void __launch_bounds__(256) rs_search_kernel(const float* __restrict__ bins, long long B, double u0,
                                                        long long* __restrict__ ids) {
  rs_search_grid(bins, B, u0, ids);
}

__global__ void __launch_bounds__(256) gather_rows_kernel(const float* __restrict__ src, const long long* __restrict__ ids,
                                                          float* __restrict__ out, long long B, int D) {
  const long long total = B * D;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long r = e / D;
    out[e] = src[ids[r] * D + (e - r * D)];
  }
}

// distinct parents of a systematic resampling = cyclic runs of the id vector (ids are non-decreasing up to the rotation by the
// event's uniform): one block, integer sums -- replaces roll + != + cast + sum + clamp (five launches) behind every event
template <class Id>
__device__ __forceinline__ void count_runs_block(const Id* ids, long long B, long long* out) {
  __shared__ unsigned part[16];
  unsigned c = 0;
  for (long long i = threadIdx.x; i < B; i += 1024) c += ids[i] != ids[i == 0 ? B - 1 : i - 1] ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < 16; ++w) t += part[w];
    *out = t < 1u ? 1 : (long long)t;
  }
}

__global__ void __launch_bounds__(1024) count_runs_kernel(const long long* __restrict__ ids, long long B,
                                                          long long* __restrict__ out) {
  count_runs_block(ids, B, out);
}

// ---------------------------------------------------------------------------- adaptive resampling event
// Statistics of B log-weights a (pita_hip.h: pita_logweight_stats) by ONE block of AR_T threads, and the decision of an
// adaptive event from them.  Fixed order: thread t takes a[t], a[t + AR_T], ... in double, xor-shuffle wave reduction,
// the sixteen wave partials added in index order -- the same in the stats kernel (a in global memory) and in the
// one-launch event (a in LDS), so both write the same bits.  Two sweeps: the maximum of the finite entries and the
// counts, then sum w and sum w^2 of w = exp(a - max), differences and exp in double.  NaN and +inf entries are counted
// and left out of every sum (and force the event); -inf entries are counted and contribute 0.
constexpr int AR_T = 1024, AR_W = AR_T / 64;

struct StatsLds {
  double s1[AR_W], s2[AR_W];
  float mx[AR_W];
  unsigned bad[AR_W], ninf[AR_W];
};

// returns the decision (identical in every thread); thread 0 writes stats[6].  Called by all AR_T threads.
__device__ __forceinline__ int logweight_stats_block(const float* a, long long B, double theta, double* stats,
                                                     StatsLds& L) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float mx = -INFINITY;
  unsigned bad = 0, ninf = 0;
  for (long long i = t; i < B; i += AR_T) {
    const float v = a[i];
    if (v != v || v == INFINITY) ++bad;
    else if (v == -INFINITY) ++ninf;
    else mx = fmaxf(mx, v);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    bad += __shfl_xor(bad, o, 64);
    ninf += __shfl_xor(ninf, o, 64);
  }
  if (lane == 0) { L.mx[wv] = mx; L.bad[wv] = bad; L.ninf[wv] = ninf; }
  __syncthreads();
  mx = -INFINITY; bad = 0; ninf = 0;
  for (int k = 0; k < AR_W; ++k) { mx = fmaxf(mx, L.mx[k]); bad += L.bad[k]; ninf += L.ninf[k]; }
  const double m = mx > -INFINITY ? (double)mx : 0.0;  // no finite entry: 0

  double s1 = 0.0, s2 = 0.0;
  for (long long i = t; i < B; i += AR_T) {
    const float v = a[i];
    if (v == v && fabsf(v) != INFINITY) {
      const double w = exp((double)v - m);
      s1 += w;
      s2 = fma(w, w, s2);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  if (lane == 0) { L.s1[wv] = s1; L.s2[wv] = s2; }
  __syncthreads();
  s1 = 0.0; s2 = 0.0;
  for (int k = 0; k < AR_W; ++k) { s1 += L.s1[k]; s2 += L.s2[k]; }
  const double ess = (s1 > 0.0 && s1 < (double)INFINITY) ? s1 * s1 / s2 : 0.0;
  if (t == 0) {
    stats[0] = m;
    stats[1] = m + log(s1 / (double)B);
    stats[2] = ess;
    stats[3] = ess / (double)B;
    stats[4] = (double)bad;
    stats[5] = (double)ninf;
  }
  return (theta >= 1.0 || bad > 0u || ess <= theta * (double)B) ? 1 : 0;
}

// the statistics as a pass of their own: pita_logweight_stats (resampled == nullptr) and the first pass of the gated event
__global__ void __launch_bounds__(AR_T) logweight_stats_kernel(const float* __restrict__ a, long long B, double theta,
                                                               double* __restrict__ stats, int* __restrict__ resampled) {
  __shared__ StatsLds L;
  const int flag = logweight_stats_block(a, B, theta, stats, L);
  if (threadIdx.x == 0 && resampled) *resampled = flag;
}

// One adaptive event of B <= AR_MAX_B walkers in ONE launch: the log-weights are read once into LDS, the block takes
// the statistics and the decision, and, where the event resamples, the five passes of pita_systematic_resample and the
// run count without leaving the block.  The four groups of RS_T threads each take one virtual block of RS_E walkers per
// round through the rs_pass_* functions, so every sum has the order of the multi-block kernels and the ids are theirs bit
// for bit.  The bins overwrite the log-weights in place; the parents are kept as 16-bit words (ids < 65 536) for the run
// count.  Dynamic LDS: float val[B] | unsigned short par[B].
// AR_MAX_B is where the launch still wins: measured against the seven launches of the fixed sequence it takes 0.93 of
// their time at 2 048 walkers and 3.2 times it at 16 384 (profiles/r14_adaptive_resample.txt) -- one compute unit then
// walks sixteen virtual blocks, serial scans included, that the multi-block passes spread over sixteen.
constexpr int AR_G = AR_T / RS_T, AR_MAX_B = 2048, AR_MAX_VB = AR_MAX_B / RS_E;
static_assert(AR_MAX_B % RS_E == 0 && AR_MAX_B <= 65536 && AR_MAX_B * 6 + 16384 <= 65536, "ids as 16-bit words, static LDS limit");

__host__ __device__ inline size_t ar_val_bytes(long long B) { return ((size_t)B * 4 + 7) & ~(size_t)7; }

// The event of one block: the body of adaptive_resample_block_kernel (one population: id_base 0, no logw_next) and of
// population_resample_kernel (block p: its slice of every array, id_base = p * B).  ids are written as parent + id_base;
// logw_next (nullable) gets 0 where the event resamples and the log-weights where not, from the LDS copy -- every read of
// `logits` precedes the first barrier and every write follows it, so logw_next may be logits.  Called by all AR_T threads.
__device__ __forceinline__ void adaptive_resample_block(const float* logits, int B, double u0, double theta, long long* ids,
                                                        long long id_base, long long* n_unique, double* stats,
                                                        int* resampled, float* logw_next) {
  extern __shared__ double ar_lds[];
  __shared__ StatsLds L;
  __shared__ double part[AR_G][RS_T], red[AR_G][RS_T / 64], bsum[AR_MAX_VB], bw[AR_MAX_VB];
  __shared__ float redf[AR_G][RS_T / 64], bmax[AR_MAX_VB];
  float* val = reinterpret_cast<float*>(ar_lds);
  unsigned short* par = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(ar_lds) + ar_val_bytes(B));
  const int tid = threadIdx.x, g = tid / RS_T, t = tid % RS_T;
  for (int i = tid; i < B; i += AR_T) val[i] = logits[i];
  __syncthreads();
  const int flag = logweight_stats_block(val, B, theta, stats, L);
  if (tid == 0) *resampled = flag;
  if (!flag) {  // uniform: every thread folded the same partials
    for (int i = tid; i < B; i += AR_T) ids[i] = id_base + i;
    if (logw_next)
      for (int i = tid; i < B; i += AR_T) logw_next[i] = val[i];
    if (tid == 0 && n_unique) *n_unique = B;
    return;
  }
  if (logw_next)
    for (int i = tid; i < B; i += AR_T) logw_next[i] = 0.0f;
  const int nb = (B + RS_E - 1) / RS_E;
  for (int v0 = 0; v0 < nb; v0 += AR_G) {  // A
    const float m = rs_pass_max(val, B, v0 + g, t, redf[g]);
    if (t == 0 && v0 + g < nb) bmax[v0 + g] = m;
    __syncthreads();  // redf is read by t == 0 after the pass's own barrier
  }
  const float mx = rs_fold_max(bmax, nb);
  for (int v0 = 0; v0 < nb; v0 += AR_G) {  // B
    const double s = rs_pass_sum(val, B, v0 + g, t, mx, 1.0f, 0, red[g]);
    if (t == 0 && v0 + g < nb) bsum[v0 + g] = s;
  }
  __syncthreads();
  const float sm = (float)rs_fold_sum(bsum, nb);
  for (int v0 = 0; v0 < nb; v0 += AR_G) {  // C
    const double s = rs_pass_sum(val, B, v0 + g, t, mx, sm, 1, red[g]);
    if (t == 0 && v0 + g < nb) bw[v0 + g] = s;
  }
  __syncthreads();
  for (int v0 = 0; v0 < nb; v0 += AR_G) {  // D, in place
    const int vb = v0 + g;
    rs_pass_bins(val, B, vb, t, mx, sm, rs_fold_sum(bw, vb < nb ? vb : nb), part[g], val);
  }
  __syncthreads();
  const float invB = (float)(1.0 / (double)B);
  for (int k = tid; k < B; k += AR_T) {  // E
    const long long id = rs_search(val, B, u0, invB, k);
    ids[k] = id_base + id;
    par[k] = (unsigned short)id;
  }
  __syncthreads();
  long long runs = 0;
  count_runs_block(par, B, &runs);  // thread 0 holds the count
  if (tid == 0 && n_unique) *n_unique = runs;
}

__global__ void __launch_bounds__(AR_T) adaptive_resample_block_kernel(const float* __restrict__ logits, int B, double u0,
                                                                       double theta, long long* __restrict__ ids,
                                                                       long long* __restrict__ n_unique,
                                                                       double* __restrict__ stats,
                                                                       int* __restrict__ resampled) {
  adaptive_resample_block(logits, B, u0, theta, ids, 0, n_unique, stats, resampled, nullptr);
}

// P independent populations of S <= AR_MAX_B walkers, one event each, in ONE launch: block p owns rows [p S, (p + 1) S) and
// runs the one-population body on them with its own uniform u0[p].  Blocks share nothing (no atomics, no scratch), so a
// population's bits depend neither on n_pop nor on p; the ids are global rows (p S + parent), ready for gather_rows_kernel.
// No __restrict__: logw_next may be logits.
__global__ void __launch_bounds__(AR_T) population_resample_kernel(const float* logits, int S, const double* __restrict__ u0,
                                                                   double theta, long long* ids, long long* n_unique,
                                                                   double* stats, int* resampled, float* logw_next) {
  const long long p = blockIdx.x, base = p * S;
  adaptive_resample_block(logits + base, S, u0[p], theta, ids + base, base, n_unique ? n_unique + p : nullptr,
                          stats + 6 * p, resampled + p, logw_next ? logw_next + base : nullptr);
}

// ---- the gated multi-pass event (B > AR_MAX_B): logweight_stats_kernel writes the flag, the passes of
// pita_systematic_resample and the run count follow and test it on entry.  Flag clear: they return at once and the
// search pass writes the identity; flag set: exactly the arithmetic of the plain kernels.
__global__ void __launch_bounds__(RS_T) rs_max_gated_kernel(const int* __restrict__ gate, const float* __restrict__ logits,
                                                            long long B, float* __restrict__ bmax) {
  if (*gate) rs_max_block(logits, B, bmax);
}
__global__ void __launch_bounds__(RS_T) rs_sum_gated_kernel(const int* __restrict__ gate, const float* __restrict__ logits,
                                                            long long B, int nblk, const float* __restrict__ bmax,
                                                            const double* __restrict__ bsum, double* __restrict__ out,
                                                            int phase) {
  if (*gate) rs_sum_block(logits, B, nblk, bmax, bsum, out, phase);
}
__global__ void __launch_bounds__(RS_T) rs_bins_gated_kernel(const int* __restrict__ gate, const float* __restrict__ logits,
                                                             long long B, int nblk, const float* __restrict__ bmax,
                                                             const double* __restrict__ bsum, const double* __restrict__ bw,
                                                             float* __restrict__ bins) {
  if (*gate) rs_bins_block(logits, B, nblk, bmax, bsum, bw, bins);
}
__global__ void __launch_bounds__(256) rs_search_gated_kernel(const int* __restrict__ gate, const float* __restrict__ bins,
                                                              long long B, double u0, long long* __restrict__ ids) {
  if (*gate) {
    rs_search_grid(bins, B, u0, ids);
  } else {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < B; k += (long long)gridDim.x * 256) ids[k] = k;
  }
}
__global__ void __launch_bounds__(1024) count_runs_gated_kernel(const int* __restrict__ gate, const long long* __restrict__ ids,
                                                                long long B, long long* __restrict__ out) {
  if (*gate) {
    count_runs_block(ids, B, out);
  } else if (threadIdx.x == 0) {
    *out = B;
  }
}

// ---- populations of any size: P independent events of S walkers each through the SAME passes, over a (virtual block,
// population) grid.  pop_stats_kernel (one block per population: the single-block summation order of the one-population
// event, hence its ESS bits and decision) writes the P flags; every later block tests the flag of its population and runs
// rs_*_block on the population's slice of the logits and its own copy of the scratch, so population p's bits are those of
// pita_adaptive_resample on its slice, whatever P and p are.  Blocks of different populations share nothing; stream order
// is the only synchronisation.  Populations beyond gridDim.y are reached by striding; the barrier that ends a round keeps
// the next population's pass off the LDS the last one is still reading.
struct RsScratch {
  float *bins, *bmax;
  double *bsum, *bw;
};
__host__ __device__ inline size_t rs_scratch_bytes(long long B, long long nb) {
  return (((size_t)B * 4 + 7) & ~(size_t)7) + (((size_t)nb * 4 + 7) & ~(size_t)7) + 2 * (size_t)nb * 8;
}
// float bins[B] | float bmax[nb] | double bsum[nb] | double bw[nb]   (8-byte aligned sections)
__host__ __device__ inline RsScratch rs_scratch(void* workspace, long long B, long long nb) {
  char* w = static_cast<char*>(workspace);
  RsScratch r;
  r.bins = reinterpret_cast<float*>(w);
  w += ((size_t)B * 4 + 7) & ~(size_t)7;
  r.bmax = reinterpret_cast<float*>(w);
  w += ((size_t)nb * 4 + 7) & ~(size_t)7;
  r.bsum = reinterpret_cast<double*>(w);
  r.bw = r.bsum + nb;
  return r;
}

__global__ void __launch_bounds__(AR_T) pop_stats_kernel(const float* __restrict__ logits, long long S, double theta,
                                                         double* __restrict__ stats, int* __restrict__ resampled) {
  __shared__ StatsLds L;
  const long long p = blockIdx.x;
  const int flag = logweight_stats_block(logits + p * S, S, theta, stats + 6 * p, L);
  if (threadIdx.x == 0) resampled[p] = flag;
}
__global__ void __launch_bounds__(RS_T) pop_rs_max_kernel(const int* __restrict__ gate, const float* __restrict__ logits,
                                                          long long S, int nblk, long long P, char* ws, size_t stride) {
  for (long long p = blockIdx.y; p < P; p += gridDim.y) {
    if (gate[p]) rs_max_block(logits + p * S, S, rs_scratch(ws + p * stride, S, nblk).bmax);
    __syncthreads();
  }
}
__global__ void __launch_bounds__(RS_T) pop_rs_sum_kernel(const int* __restrict__ gate, const float* __restrict__ logits,
                                                          long long S, int nblk, long long P, char* ws, size_t stride,
                                                          int phase) {
  for (long long p = blockIdx.y; p < P; p += gridDim.y) {
    if (gate[p]) {
      const RsScratch w = rs_scratch(ws + p * stride, S, nblk);
      rs_sum_block(logits + p * S, S, nblk, w.bmax, w.bsum, phase == 1 ? w.bw : w.bsum, phase);
    }
    __syncthreads();
  }
}
__global__ void __launch_bounds__(RS_T) pop_rs_bins_kernel(const int* __restrict__ gate, const float* __restrict__ logits,
                                                           long long S, int nblk, long long P, char* ws, size_t stride) {
  for (long long p = blockIdx.y; p < P; p += gridDim.y) {
    if (gate[p]) {
      const RsScratch w = rs_scratch(ws + p * stride, S, nblk);
      rs_bins_block(logits + p * S, S, nblk, w.bmax, w.bsum, w.bw, w.bins);
    }
    __syncthreads();
  }
}
// pass E per population, as GLOBAL rows (p S + parent); the identity where the flag is clear.  logw_next (nullable): 0
// where the population resampled, its log-weights where not.  This is the last pass, the bins were made from `logits` by
// earlier launches and element k is copied only onto index k, so logw_next may be logits (no __restrict__ on either).
__global__ void __launch_bounds__(256) pop_rs_search_kernel(const int* __restrict__ gate, const float* logits, long long S,
                                                            int nblk, long long P, const double* __restrict__ u0, char* ws,
                                                            size_t stride, long long* __restrict__ ids, float* logw_next) {
  const float invS = (float)(1.0 / (double)S);
  for (long long p = blockIdx.y; p < P; p += gridDim.y) {
    const long long base = p * S;
    const int flag = gate[p];
    const float* bins = rs_scratch(ws + p * stride, S, nblk).bins;
    const double u = u0[p];
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < S; k += (long long)gridDim.x * 256) {
      ids[base + k] = base + (flag ? rs_search(bins, S, u, invS, k) : k);
      if (logw_next) logw_next[base + k] = flag ? 0.0f : logits[base + k];
    }
  }
}
__global__ void __launch_bounds__(1024) pop_count_runs_kernel(const int* __restrict__ gate, const long long* __restrict__ ids,
                                                              long long S, long long* __restrict__ n_unique) {
  const long long p = blockIdx.x;
  if (gate[p]) {
    count_runs_block(ids + p * S, S, n_unique + p);  // a common offset does not change where the runs break
  } else if (threadIdx.x == 0) {
    n_unique[p] = S;
  }
}

}  // namespace pita

using namespace pita;

extern "C" int pita_count_runs(const int64_t* ids, int64_t B, int64_t* out, void* stream) {
  PITA_REQUIRE(ids && out && B >= 1, "pita_count_runs: bad argument");
  hipLaunchKernelGGL(count_runs_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const long long*)ids, (long long)B,
                     (long long*)out);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_em_step(float* x, const float* drift, const float* noise, int64_t B, int n, int d, float dt,
                            float noise_scale, float sqrt_dt, uint64_t seed, uint64_t walker_offset, int64_t step,
                            int remove_mean, double* stats_out, void* stream) {
  PITA_REQUIRE(drift, "pita_em_step: drift is null");
  ElemParams p{};
  p.dt = dt; p.noise_scale = noise_scale; p.sqrt_dt = sqrt_dt; p.seed = seed; p.walker_offset = walker_offset;
  p.step = step; p.remove_mean = remove_mean; p.stats_out = stats_out;
  return launch_elem<OP_EM>(x, drift, noise, B, n, d, p, stream);
}

// the same for up to four vectors of one length in ONE launch: out[2 q], out[2 q + 1] += sum / sum of squares of v_q
// (the four per-step statistics of the debiased regime were four launches of ~27 us)
__global__ void __launch_bounds__(256) moments4_kernel(const float* __restrict__ v0, const float* __restrict__ v1,
                                                       const float* __restrict__ v2, const float* __restrict__ v3,
                                                       long long n, double* __restrict__ out) {
  const float* vs[4] = {v0, v1, v2, v3};
  __shared__ double red[4][8];
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (vs[q]) {
        const double a = (double)vs[q][e];
        acc[2 * q] += a;
        acc[2 * q + 1] += a * a;
      }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    double t = acc[q];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = t;
  }
  __syncthreads();
  if (threadIdx.x < 8 && vs[threadIdx.x >> 1])
    atomicAdd(out + threadIdx.x, (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]));
}

extern "C" int pita_moments4(const float* v0, const float* v1, const float* v2, const float* v3, int64_t n, double* out,
                             void* stream) {
  PITA_REQUIRE(n >= 0 && out, "pita_moments4: bad argument");
  if (n == 0 || !(v0 || v1 || v2 || v3)) return PITA_OK;
  const long long nb = (n + 255) / 256;
  hipLaunchKernelGGL(moments4_kernel, dim3((unsigned)(nb < 256 ? nb : 256)), dim3(256), 0, (hipStream_t)stream, v0, v1, v2, v3,
                     (long long)n, out);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

// ---- histogram of a sample over given bin edges (the reference's evaluation figure: base_molecule_energy_function.py:160-254,
// matplotlib `hist` = numpy.histogram): counts[i] = #{ edges[i] <= v < edges[i+1] }, the last bin closed on the right,
// values outside [edges[0], edges[nbins]] and NaNs not counted.  One pass over the sample: bins privatised in LDS per
// block (one copy per wave: the four waves of a block do not contend), a guessed bin from the uniform spacing corrected
// against the edges (numpy's own rule, so that counts agree with numpy.histogram bin for bin), one 64-bit add per bin
// and block at the end.  The bin rule is hist_bin (hist_common.h), shared with the weighted histograms.
__global__ void __launch_bounds__(256) histogram_kernel(const float* __restrict__ v, long long n, const float* __restrict__ edges,
                                                        int nbins, unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned hist_lds[];  // [4 waves][nbins] counters, then [nbins + 1] edges
  unsigned* bins = hist_lds + (threadIdx.x >> 6) * nbins;
  float* e = reinterpret_cast<float*>(hist_lds + 4 * nbins);
  for (int i = threadIdx.x; i < 4 * nbins; i += 256) hist_lds[i] = 0u;
  for (int i = threadIdx.x; i <= nbins; i += 256) e[i] = edges[i];
  __syncthreads();
  const float lo = e[0], hi = e[nbins];
  const float inv = (float)nbins / (hi - lo);
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long long)gridDim.x * 256) {
    const int i = hist_bin(v[k], e, nbins, lo, hi, inv);
    if (i >= 0) atomicAdd(&bins[i], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += 256) {
    const unsigned long long t = (unsigned long long)hist_lds[i] + hist_lds[nbins + i] + hist_lds[2 * nbins + i] + hist_lds[3 * nbins + i];
    if (t) atomicAdd(counts + i, t);
  }
}

extern "C" int pita_histogram(const float* v, int64_t n, const float* edges, int nbins, unsigned long long* counts, void* stream) {
  PITA_REQUIRE(n >= 0 && edges && counts && nbins >= 1 && nbins <= HIST_MAX_BINS, "pita_histogram: bad argument (1 <= nbins <= %d)",
               HIST_MAX_BINS);
  PITA_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * (size_t)nbins, (hipStream_t)stream));
  if (n == 0) return PITA_OK;
  PITA_REQUIRE(v, "pita_histogram: null input");
  const long long nb = (n + 255) / 256;
  const size_t lds = sizeof(unsigned) * 4 * (size_t)nbins + sizeof(float) * ((size_t)nbins + 1);
  hipLaunchKernelGGL(histogram_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), lds, (hipStream_t)stream, v,
                     (long long)n, edges, nbins, counts);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_moments(const float* v, int64_t n, double* out, void* stream) {
  PITA_REQUIRE(n >= 0 && out, "pita_moments: bad argument");
  if (n == 0) return PITA_OK;
  PITA_REQUIRE(v, "pita_moments: null input");
  const long long nb = (n + 255) / 256;
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, (hipStream_t)stream, v,
                     (long long)n, out);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_prior_sample(float* x, const float* noise, int64_t B, int n, int d, float scale, uint64_t seed,
                                 uint64_t walker_offset, int mean_free, void* stream) {
  ElemParams p{};
  p.scale = scale; p.seed = seed; p.walker_offset = walker_offset; p.step = -1; p.remove_mean = mean_free;
  return launch_elem<OP_PRIOR>(x, nullptr, noise, B, n, d, p, stream);
}

extern "C" int pita_remove_mean(float* x, int64_t B, int n, int d, void* stream) {
  ElemParams p{};
  p.remove_mean = 1;
  return launch_elem<OP_RMEAN>(x, nullptr, nullptr, B, n, d, p, stream);
}

extern "C" int pita_fill_normal(float* out, int64_t B, int n, int d, uint64_t seed, uint64_t walker_offset,
                                int64_t step, void* stream) {
  ElemParams p{};
  p.seed = seed; p.walker_offset = walker_offset; p.step = step; p.remove_mean = 0;
  return launch_elem<OP_NORMAL>(out, nullptr, nullptr, B, n, d, p, stream);
}

static inline long long rs_nblk(int64_t B) { return (B + RS_E - 1) / RS_E; }

// workspace: float bins[B] | float bmax[nblk] | double bsum[nblk] | double bw[nblk]   (8-byte aligned sections)
extern "C" size_t pita_resample_workspace_bytes(int64_t B) {
  const long long n = B > 0 ? B : 1;
  return rs_scratch_bytes(n, rs_nblk(n));
}

extern "C" int pita_systematic_resample(const float* logits, int64_t B, double u0, int64_t* ids, void* workspace,
                                        void* stream) {
  PITA_REQUIRE(logits && ids && workspace && B >= 0, "pita_systematic_resample: null argument");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(((uintptr_t)workspace & 7) == 0, "pita_systematic_resample: workspace must be 8-byte aligned");
  const long long nb = rs_nblk(B);
  const RsScratch w = rs_scratch(workspace, B, nb);
  float *bins = w.bins, *bmax = w.bmax;
  double *bsum = w.bsum, *bw = w.bw;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rs_max_kernel, dim3((unsigned)nb), dim3(RS_T), 0, s, logits, (long long)B, bmax);
  hipLaunchKernelGGL(rs_sum_kernel, dim3((unsigned)nb), dim3(RS_T), 0, s, logits, (long long)B, (int)nb, bmax, bsum, bsum, 0);
  hipLaunchKernelGGL(rs_sum_kernel, dim3((unsigned)nb), dim3(RS_T), 0, s, logits, (long long)B, (int)nb, bmax, bsum, bw, 1);
  hipLaunchKernelGGL(rs_bins_kernel, dim3((unsigned)nb), dim3(RS_T), 0, s, logits, (long long)B, (int)nb, bmax, bsum, bw, bins);
  const long long sb = (B + 255) / 256;
  hipLaunchKernelGGL(rs_search_kernel, dim3((unsigned)(sb < 8192 ? sb : 8192)), dim3(256), 0, s, bins, (long long)B, u0,
                     (long long*)ids);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

// one block of AR_T threads sweeps the vector: no scratch
extern "C" size_t pita_logweight_stats_workspace_bytes(int64_t) { return 0; }

extern "C" int pita_logweight_stats(const float* a, int64_t B, double* stats, void* /*workspace*/, void* stream) {
  PITA_REQUIRE(a && stats && B >= 1, "pita_logweight_stats: bad argument (B >= 1, non-null a and stats)");
  hipLaunchKernelGGL(logweight_stats_kernel, dim3(1), dim3(AR_T), 0, (hipStream_t)stream, a, (long long)B, 0.0, stats,
                     (int*)nullptr);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_adaptive_resample_single_launch(int64_t B) { return B >= 1 && B <= AR_MAX_B ? 1 : 0; }

// the gated path's scratch is pita_systematic_resample's; the one-launch path needs none (8 bytes so that it is never null)
extern "C" size_t pita_adaptive_resample_workspace_bytes(int64_t B) {
  return pita_adaptive_resample_single_launch(B) ? 8 : pita_resample_workspace_bytes(B);
}

extern "C" int pita_adaptive_resample(const float* logits, int64_t B, double u0, double theta, int64_t* ids,
                                      int64_t* n_unique, double* stats, int* resampled, void* workspace, void* stream) {
  PITA_REQUIRE(B >= 1, "pita_adaptive_resample: B must be at least 1 (got %lld)", (long long)B);
  PITA_REQUIRE(logits && ids && stats && resampled && workspace, "pita_adaptive_resample: null argument");
  PITA_REQUIRE(theta >= 0.0 && theta <= 1.0, "pita_adaptive_resample: theta must be in [0, 1] (got %g)", theta);
  PITA_REQUIRE(u0 >= 0.0 && u0 < 1.0, "pita_adaptive_resample: u0 must be in [0, 1) (got %g)", u0);
  PITA_REQUIRE(((uintptr_t)workspace & 7) == 0, "pita_adaptive_resample: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (pita_adaptive_resample_single_launch(B)) {
    hipLaunchKernelGGL(adaptive_resample_block_kernel, dim3(1), dim3(AR_T), ar_val_bytes(B) + 2 * (size_t)B, s, logits,
                       (int)B, u0, theta, (long long*)ids, (long long*)n_unique, stats, resampled);
    PITA_LAUNCH_CHECK();
    return PITA_OK;
  }
  const long long nb = rs_nblk(B);
  const RsScratch w = rs_scratch(workspace, B, nb);
  float *bins = w.bins, *bmax = w.bmax;
  double *bsum = w.bsum, *bw = w.bw;
  const int* gate = resampled;
  hipLaunchKernelGGL(logweight_stats_kernel, dim3(1), dim3(AR_T), 0, s, logits, (long long)B, theta, stats, resampled);
  hipLaunchKernelGGL(rs_max_gated_kernel, dim3((unsigned)nb), dim3(RS_T), 0, s, gate, logits, (long long)B, bmax);
  hipLaunchKernelGGL(rs_sum_gated_kernel, dim3((unsigned)nb), dim3(RS_T), 0, s, gate, logits, (long long)B, (int)nb, bmax,
                     bsum, bsum, 0);
  hipLaunchKernelGGL(rs_sum_gated_kernel, dim3((unsigned)nb), dim3(RS_T), 0, s, gate, logits, (long long)B, (int)nb, bmax,
                     bsum, bw, 1);
  hipLaunchKernelGGL(rs_bins_gated_kernel, dim3((unsigned)nb), dim3(RS_T), 0, s, gate, logits, (long long)B, (int)nb, bmax,
                     bsum, bw, bins);
  const long long sb = (B + 255) / 256;
  hipLaunchKernelGGL(rs_search_gated_kernel, dim3((unsigned)(sb < 8192 ? sb : 8192)), dim3(256), 0, s, gate, bins,
                     (long long)B, u0, (long long*)ids);
  if (n_unique)
    hipLaunchKernelGGL(count_runs_gated_kernel, dim3(1), dim3(1024), 0, s, gate, (const long long*)ids, (long long)B,
                       (long long*)n_unique);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

// every population is the one-launch event of its block: no scratch (8 bytes so that the pointer is never null)
extern "C" size_t pita_population_resample_workspace_bytes(int64_t, int64_t) { return 8; }

extern "C" int pita_population_resample(const float* logits, int64_t n_pop, int64_t pop_size, const double* u0_dev,
                                        double theta, int64_t* ids, int64_t* n_unique, double* stats, int* resampled,
                                        float* logw_next, void* workspace, void* stream) {
  PITA_REQUIRE(n_pop >= 1 && n_pop <= 0x7fffffffLL, "pita_population_resample: n_pop must be in [1, 2^31) (got %lld)",
               (long long)n_pop);
  PITA_REQUIRE(pop_size >= 1, "pita_population_resample: pop_size must be at least 1 (got %lld)", (long long)pop_size);
  if (pop_size > AR_MAX_B)
    return fail(PITA_EUNSUPPORTED, "pita_population_resample: pop_size %lld exceeds the %d walkers one block holds in LDS",
                (long long)pop_size, AR_MAX_B);
  PITA_REQUIRE(logits && u0_dev && ids && stats && resampled && workspace, "pita_population_resample: null argument");
  PITA_REQUIRE(theta >= 0.0 && theta <= 1.0, "pita_population_resample: theta must be in [0, 1] (got %g)", theta);
  PITA_REQUIRE(((uintptr_t)workspace & 7) == 0, "pita_population_resample: workspace must be 8-byte aligned");
  hipLaunchKernelGGL(population_resample_kernel, dim3((unsigned)n_pop), dim3(AR_T),
                     ar_val_bytes(pop_size) + 2 * (size_t)pop_size, (hipStream_t)stream, logits, (int)pop_size, u0_dev, theta,
                     (long long*)ids, (long long*)n_unique, stats, resampled, logw_next);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

// P copies of pita_systematic_resample's scratch, one per population (each a multiple of 8 bytes)
extern "C" size_t pita_population_resample_blocks_workspace_bytes(int64_t n_pop, int64_t pop_size) {
  return (size_t)(n_pop > 0 ? n_pop : 1) * pita_resample_workspace_bytes(pop_size);
}

extern "C" int pita_population_resample_blocks(const float* logits, int64_t n_pop, int64_t pop_size, const double* u0_dev,
                                               double theta, int64_t* ids, int64_t* n_unique, double* stats, int* resampled,
                                               float* logw_next, void* workspace, void* stream) {
  PITA_REQUIRE(n_pop >= 1 && n_pop <= 0x7fffffffLL, "pita_population_resample_blocks: n_pop must be in [1, 2^31) (got %lld)",
               (long long)n_pop);
  PITA_REQUIRE(pop_size >= 1, "pita_population_resample_blocks: pop_size must be at least 1 (got %lld)",
               (long long)pop_size);
  PITA_REQUIRE(logits && u0_dev && ids && stats && resampled && workspace, "pita_population_resample_blocks: null argument");
  PITA_REQUIRE(theta >= 0.0 && theta <= 1.0, "pita_population_resample_blocks: theta must be in [0, 1] (got %g)", theta);
  PITA_REQUIRE(((uintptr_t)workspace & 7) == 0, "pita_population_resample_blocks: workspace must be 8-byte aligned");
  const long long P = n_pop, S = pop_size, nb = rs_nblk(S), sb = (S + 255) / 256;
  const size_t stride = pita_resample_workspace_bytes(S);
  char* ws = static_cast<char*>(workspace);
  const int* gate = resampled;
  const unsigned gy = (unsigned)(P < 65535 ? P : 65535);
  const dim3 pass((unsigned)nb, gy), search((unsigned)(sb < 8192 ? sb : 8192), gy);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pop_stats_kernel, dim3((unsigned)P), dim3(AR_T), 0, s, logits, S, theta, stats, resampled);
  hipLaunchKernelGGL(pop_rs_max_kernel, pass, dim3(RS_T), 0, s, gate, logits, S, (int)nb, P, ws, stride);
  hipLaunchKernelGGL(pop_rs_sum_kernel, pass, dim3(RS_T), 0, s, gate, logits, S, (int)nb, P, ws, stride, 0);
  hipLaunchKernelGGL(pop_rs_sum_kernel, pass, dim3(RS_T), 0, s, gate, logits, S, (int)nb, P, ws, stride, 1);
  hipLaunchKernelGGL(pop_rs_bins_kernel, pass, dim3(RS_T), 0, s, gate, logits, S, (int)nb, P, ws, stride);
  hipLaunchKernelGGL(pop_rs_search_kernel, search, dim3(256), 0, s, gate, logits, S, (int)nb, P, u0_dev, ws, stride,
                     (long long*)ids, logw_next);
  if (n_unique)
    hipLaunchKernelGGL(pop_count_runs_kernel, dim3((unsigned)P), dim3(1024), 0, s, gate, (const long long*)ids, S,
                       (long long*)n_unique);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_gather_rows(const float* src, const int64_t* ids, float* out, int64_t B, int D, void* stream) {
  PITA_REQUIRE(src && ids && out && B >= 0 && D >= 1, "pita_gather_rows: bad argument");
  PITA_REQUIRE(src != out, "pita_gather_rows: in-place gather is not supported");
  if (B == 0) return PITA_OK;
  const long long nb = (B * D + 255) / 256;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, (hipStream_t)stream, src,
                     (const long long*)ids, out, (long long)B, D);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

// the launches of pita_mala_propose (no pk) and pita_mala_propose_pop (pk: one PopKeys)
template <class... Pop>
static int launch_mala_propose(const float* x, const float* force, float* x_prop, const float* noise, int64_t B, int n, int d,
                               const double* dt_dev, const ElemParams& p, void* stream, Pop... pk) {
  const long long nb = (B * n + 255) / 256;
  const unsigned grid = (unsigned)(nb < 8192 ? nb : 8192);
  hipStream_t s = (hipStream_t)stream;
  switch (d) {
    case 1: hipLaunchKernelGGL((mala_propose_kernel<1, Pop...>), dim3(grid), dim3(256), 0, s, x, force, x_prop, noise, B, n, dt_dev, p, pk...); break;
    case 2: hipLaunchKernelGGL((mala_propose_kernel<2, Pop...>), dim3(grid), dim3(256), 0, s, x, force, x_prop, noise, B, n, dt_dev, p, pk...); break;
    default: hipLaunchKernelGGL((mala_propose_kernel<3, Pop...>), dim3(grid), dim3(256), 0, s, x, force, x_prop, noise, B, n, dt_dev, p, pk...); break;
  }
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_mala_propose(const float* x, const float* force, float* x_prop, const float* noise, int64_t B, int n,
                                 int d, const double* dt_dev, uint64_t seed, uint64_t walker_offset,
                                 const int64_t* walker_ids, int64_t step, void* stream) {
  PITA_REQUIRE(B >= 0, "pita_mala_propose: negative batch");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(x && force && x_prop && dt_dev, "pita_mala_propose: null argument");
  PITA_REQUIRE(n >= 1 && n <= 256 && d >= 1 && d <= 3, "pita_mala_propose: n_particles in [1,256], n_dim in [1,3]");
  ElemParams p{};
  p.seed = seed; p.walker_offset = walker_offset; p.step = step; p.walker_ids = (const long long*)walker_ids;
  return launch_mala_propose(x, force, x_prop, noise, B, n, d, dt_dev, p, stream);
}

extern "C" int pita_mala_propose_pop(const float* x, const float* force, float* x_prop, const float* noise, int64_t B, int n,
                                     int d, const double* dt_dev, int n_pop, int64_t pop_size, uint64_t pop_base,
                                     uint64_t seed, uint64_t walker_offset, const int64_t* walker_ids, int64_t step,
                                     void* stream) {
  PITA_REQUIRE(B >= 0, "pita_mala_propose_pop: negative batch");
  PITA_REQUIRE(dt_dev, "pita_mala_propose_pop: null argument (dt_dev)");
  PITA_REQUIRE(n_pop >= 1 && pop_size >= 1, "pita_mala_propose_pop: bad argument (n_pop >= 1, pop_size >= 1)");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(x && force && x_prop, "pita_mala_propose_pop: null argument");
  PITA_REQUIRE(n >= 1 && n <= 256 && d >= 1 && d <= 3, "pita_mala_propose_pop: n_particles in [1,256], n_dim in [1,3]");
  ElemParams p{};
  p.seed = seed; p.walker_offset = walker_offset; p.step = step; p.walker_ids = (const long long*)walker_ids;
  return launch_mala_propose(x, force, x_prop, noise, B, n, d, dt_dev, p, stream, PopKeys{pop_base, (long long)pop_size});
}

// the launches of pita_mala_accept (no pk) and pita_mala_accept_pop (pk: one PopKeys, and WB more LDS words for popl)
template <class... Pop>
static int launch_mala_accept(float* x, float* logp, const float* force, const float* x_prop, const float* logp_prop,
                              const float* force_prop, const float* uniforms, int64_t B, int n, int d, const double* dt_dev,
                              int* acc_count, const ElemParams& p, void* stream, Pop... pk) {
  const int WB = 256 / n;
  const long long nblk = (B + WB - 1) / WB;
  const unsigned grid = (unsigned)(nblk < 256LL * 16 ? nblk : 256LL * 16);
  const size_t lds = sizeof(float) * (size_t)(WB * n * d + 2 * WB * n + WB + (sizeof...(Pop) ? WB : 0));
  hipStream_t s = (hipStream_t)stream;
  switch (d) {
    case 1: hipLaunchKernelGGL((mala_accept_kernel<1, Pop...>), dim3(grid), dim3(256), lds, s, x, logp, force, x_prop, logp_prop, force_prop, uniforms, B, n, WB, dt_dev, acc_count, p, pk...); break;
    case 2: hipLaunchKernelGGL((mala_accept_kernel<2, Pop...>), dim3(grid), dim3(256), lds, s, x, logp, force, x_prop, logp_prop, force_prop, uniforms, B, n, WB, dt_dev, acc_count, p, pk...); break;
    default: hipLaunchKernelGGL((mala_accept_kernel<3, Pop...>), dim3(grid), dim3(256), lds, s, x, logp, force, x_prop, logp_prop, force_prop, uniforms, B, n, WB, dt_dev, acc_count, p, pk...); break;
  }
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_mala_accept(float* x, float* logp, const float* force, const float* x_prop, const float* logp_prop,
                                const float* force_prop, const float* uniforms, int64_t B, int n, int d,
                                const double* dt_dev, uint64_t seed, uint64_t walker_offset, const int64_t* walker_ids,
                                int64_t step, int remove_mean, int* acc_count, void* stream) {
  PITA_REQUIRE(B >= 0, "pita_mala_accept: negative batch");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(x && logp && force && x_prop && logp_prop && force_prop && dt_dev && acc_count,
               "pita_mala_accept: null argument");
  PITA_REQUIRE(n >= 1 && n <= 256 && d >= 1 && d <= 3, "pita_mala_accept: n_particles in [1,256], n_dim in [1,3]");
  ElemParams p{};
  p.seed = seed; p.walker_offset = walker_offset; p.step = step; p.remove_mean = remove_mean;
  p.walker_ids = (const long long*)walker_ids;
  return launch_mala_accept(x, logp, force, x_prop, logp_prop, force_prop, uniforms, B, n, d, dt_dev, acc_count, p, stream);
}

extern "C" int pita_mala_accept_pop(float* x, float* logp, const float* force, const float* x_prop, const float* logp_prop,
                                    const float* force_prop, const float* uniforms, int64_t B, int n, int d,
                                    const double* dt_dev, int n_pop, int64_t pop_size, uint64_t pop_base, uint64_t seed,
                                    uint64_t walker_offset, const int64_t* walker_ids, int64_t step, int remove_mean,
                                    int* acc_count, void* stream) {
  PITA_REQUIRE(B >= 0, "pita_mala_accept_pop: negative batch");
  PITA_REQUIRE(dt_dev && acc_count, "pita_mala_accept_pop: null argument (dt_dev, acc_count)");
  PITA_REQUIRE(n_pop >= 1 && pop_size >= 1, "pita_mala_accept_pop: bad argument (n_pop >= 1, pop_size >= 1)");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(x && logp && force && x_prop && logp_prop && force_prop, "pita_mala_accept_pop: null argument");
  PITA_REQUIRE(n >= 1 && n <= 256 && d >= 1 && d <= 3, "pita_mala_accept_pop: n_particles in [1,256], n_dim in [1,3]");
  ElemParams p{};
  p.seed = seed; p.walker_offset = walker_offset; p.step = step; p.remove_mean = remove_mean;
  p.walker_ids = (const long long*)walker_ids;
  return launch_mala_accept(x, logp, force, x_prop, logp_prop, force_prop, uniforms, B, n, d, dt_dev, acc_count, p, stream,
                            PopKeys{pop_base, (long long)pop_size});
}

extern "C" int pita_mala_adapt(double* dt_dev, int* acc_count, int64_t total, int adaptive, float* rate_out, void* stream) {
  PITA_REQUIRE(dt_dev && acc_count && total > 0, "pita_mala_adapt: bad argument");
  hipLaunchKernelGGL(mala_adapt_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, dt_dev, acc_count, (long long)total,
                     adaptive, rate_out);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_mala_adapt_pop(double* dt_dev, int* acc_count, const int64_t* totals, int n_pop, int adaptive,
                                   float* rate_out, void* stream) {
  PITA_REQUIRE(dt_dev && acc_count && totals, "pita_mala_adapt_pop: null argument (dt_dev, acc_count, totals)");
  PITA_REQUIRE(n_pop >= 1, "pita_mala_adapt_pop: bad argument (n_pop >= 1)");
  hipLaunchKernelGGL(mala_adapt_pop_kernel, dim3((unsigned)((n_pop + 63) / 64)), dim3(64), 0, (hipStream_t)stream, dt_dev,
                     acc_count, (const long long*)totals, n_pop, adaptive, rate_out);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_edm_scale_input(const float* h, const float* x, float* x_scaled, float* c_noise, int64_t B, int D,
                                    void* stream) {
  PITA_REQUIRE(B >= 0 && D >= 1, "pita_edm_scale_input: bad shape");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(h && x && x_scaled && c_noise, "pita_edm_scale_input: null argument");
  const long long nb = (B * D + 255) / 256;
  hipLaunchKernelGGL(edm_scale_kernel, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, (hipStream_t)stream, h, x,
                     x_scaled, c_noise, (long long)B, D);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_edm_combine(const float* h, const float* x, const float* F, const float* beta, float* D_out,
                                float* score_out, int64_t B, int D, void* stream) {
  PITA_REQUIRE(B >= 0 && D >= 1, "pita_edm_combine: bad shape");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(h && x && F && (D_out || score_out), "pita_edm_combine: null argument");
  const long long nb = (B * D + 255) / 256;
  hipLaunchKernelGGL(edm_combine_kernel, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, (hipStream_t)stream, h, x, F,
                     beta, D_out, score_out, (long long)B, D);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}
