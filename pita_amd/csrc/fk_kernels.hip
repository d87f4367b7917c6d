// Feynman-Kac weight-drift assembly and the per-chunk quantile clamp (K11) for gfx950.
//
// Replaces (paths relative to /root/reference/pita/src/models/components/):
//   sdes.py:157-227   nabla_Ut, s_t, b_t, drift_X, <-nabla U, b>, div b, dU/dt, drift_A   (torch ops + autograd)
//   sdes.py:230       drift_A = clamp(drift_A, max = quantile(drift_A, 0.9))   (per inference chunk)
// Inputs are the reductions produced by pita_egnn_jvp (csrc/egnn_jvp_kernel.hip).
#include "common.h"

namespace pita {

struct FkParams {
  const float *x, *h, *g2, *dhdt;    // [B,D], [B], [B], [B]
  const float *beta_e, *beta_s;      // nullable [B]: precondition_beta of the energy net / of the score net
  float pin_w, pin_dw;               // pin_energy: w = (1 - t)^3 and dw/dt (0, 0 = off)
  const float* logp_target;          // pin_energy: log p_target(x) [B]
  const float *D_E, *jtx_E, *dot_h;  // energy net: denoiser, J^T x, <x, dD/dh>
  const float* dot_parts;            // nullable [B, 2]: { c_out <x, F>, <x, d(c_out F)/dh> } (pita_egnn_vjp): E and dE/dh
                                     // without the 1/h^2-sized cancellation of the forms through <D, x> and <x, dD/dh>
  const float *D_S, *trace_S;        // score net: denoiser, trace of J_x D
  float gamma, dgamma;
  float *drift_X, *drift_A, *div_bt, *cross, *dUdt, *Ut;
  long long B;
  int D;
};

// One wavefront per walker: lane k takes components k, k + 64, ... of the walker's row, so every array is read as
// one contiguous 4*D-byte span (a thread-per-walker mapping measured 25x the algorithmic HBM traffic: 64 lanes x 156 B
// strides); the three per-walker sums are wave butterflies.
__global__ void __launch_bounds__(256) fk_assemble_kernel(FkParams p) {
  const int lane = threadIdx.x & 63;
  const long long nwaves = (long long)gridDim.x * 4;
  for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < p.B; b += nwaves) {
    const float h = p.h[b], g2 = p.g2[b];
    const float c_s = 1.0f / (1.0f + h);
    // precondition_beta (score_net.py:36-38, energy_net.py:40-41): E, grad E, dE/dt scale with beta_e; s and div s with
    // beta_s.  pin_energy (energy_net.py:43-48): U = w U0 + (1 - w) E with U0 = clamp(-log p_target, +-1e3); the
    // reference's energy classes return log p DETACHED, so grad_x U = (1 - w) grad_x E (no target force)
    const float be = p.beta_e ? p.beta_e[b] : 1.0f, bs = p.beta_s ? p.beta_s[b] : 1.0f;
    const float keep = (1.0f - p.pin_w) * be;
    const float* x = p.x + b * p.D;
    const float* DE = p.D_E + b * p.D;
    const float* JE = p.jtx_E + b * p.D;
    const float* DS = p.D_S + b * p.D;
    float* dX = p.drift_X + b * p.D;
    float x2 = 0.f, DEx = 0.f, inner = 0.f;
    for (int k = lane; k < p.D; k += 64) {
      const float xv = x[k];
      x2 = fmaf(xv, xv, x2);
      DEx = fmaf(DE[k], xv, DEx);
      const float nab = keep * ((fmaf(1.0f + c_s, xv, -DE[k]) - JE[k]) / h);   // grad_x U_t
      const float bt = (bs * ((DS[k] - xv) / h)) * g2 * 0.5f;                   // b_t = s_theta g^2 / 2
      dX[k] = p.gamma * (-nab) * g2 * 0.5f + p.gamma * bt;             // sdes.py:172-174 (gamma_score = gamma_energy)
      inner = fmaf(-nab, bt, inner);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      x2 += __shfl_xor(x2, o, 64);
      DEx += __shfl_xor(DEx, o, 64);
      inner += __shfl_xor(inner, o, 64);
    }
    if (lane == 0) {
      // dE/dt = dE/dh dh/dt, dh/dt supplied by the schedule (== g^2 for the variance-exploding schedules, but a
      // plug-in schedule need not satisfy that identity exactly: sdes.py:218 differentiates through h(t))
      float Et, dEdt;
      if (p.dot_parts) {
        // With D = c_s x + c_out F:  E = |x|^2 / (2 (1 + h)) - s1 / h,  s1 = c_out <x, F>  -- the reference's own form
        // (energy_net.py:33-41) -- and dE/dh = -|x|^2 / (2 (1 + h)^2) + s1 / h^2 - s2 / h,  s2 = <x, d(c_out F)/dh>.
        // The forms below through <D, x> and <x, dD/dh> are the same numbers, but there |x|^2 / h^2-sized terms cancel
        // to O(|x|^2): at h = 0.03 that costs three digits, measured as 2 - 8 x the fp32 reference's error in dU/dt.
        const float s1 = p.dot_parts[2 * b], s2 = p.dot_parts[2 * b + 1];
        const float op = 1.0f + h;
        Et = be * (x2 / (2.0f * op) - s1 / h);
        dEdt = be * (-x2 / (2.0f * op * op) + s1 / (h * h) - s2 / h) * p.dhdt[b];
      } else {
        Et = be * ((1.0f + c_s) / (2.0f * h) * x2 - DEx / h);
        const float den = 2.0f * h + 2.0f * h * h;
        const float dq = (-2.0f * h * h - 8.0f * h - 4.0f) / (den * den);  // d/dh [(1 + c_s)/(2h)]
        dEdt = be * (dq * x2 + DEx / (h * h) - p.dot_h[b] / h) * p.dhdt[b];
      }
      float Ut = Et, dUdt = dEdt;
      if (p.logp_target) {
        // torch.clamp keeps a NaN (energy_net.py:44); fmaxf / fminf return their OTHER operand for one, which made a NaN
        // target log-density U0 = -1000 and the walker's Ut, dUt_dt and drift_A finite
        const float nlp = -p.logp_target[b];
        const float U0 = (nlp != nlp) ? nlp : fminf(fmaxf(nlp, -1e3f), 1e3f);
        Ut = p.pin_w * U0 + (1.0f - p.pin_w) * Et;
        dUdt = p.pin_dw * (U0 - Et) + (1.0f - p.pin_w) * dEdt;
      }
      const float div_bt = (bs * ((p.trace_S[b] - (float)p.D) / h)) * g2 * 0.5f;
      p.drift_A[b] = p.gamma * p.gamma * inner + p.gamma * div_bt + p.gamma * dUdt + p.dgamma * Ut;  // :222-227
      p.div_bt[b] = div_bt;
      p.cross[b] = inner;
      p.dUdt[b] = dUdt;
      p.Ut[b] = Ut;
    }
  }
}

// E_theta(h, x) from the backbone output F = F_theta(c_noise, c_in x, beta)  (energy_net.py:33-41):
//   E = (1 - c_s)/(2h) |x|^2 - c_out/(c_in h) <F, c_in x>   (times beta when beta != NULL: precondition_beta).
// One wavefront per walker, like fk_assemble_kernel.
__global__ void __launch_bounds__(256) energy_theta_kernel(const float* __restrict__ h, const float* __restrict__ x,
                                                           const float* __restrict__ F, const float* __restrict__ beta,
                                                           float* __restrict__ E, long long B, int D) {
  const int lane = threadIdx.x & 63;
  const long long nwaves = (long long)gridDim.x * 4;
  for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += nwaves) {
    const float hv = h[b];
    const float c_s = 1.0f / (1.0f + hv), c_in = 1.0f / sqrtf(1.0f + hv), c_out = sqrtf(hv) * c_in;
    float x2 = 0.f, U = 0.f;
    for (int k = lane; k < D; k += 64) {
      const float xv = x[b * D + k];
      x2 = fmaf(xv, xv, x2);
      U = fmaf(F[b * D + k], c_in * xv, U);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      x2 += __shfl_xor(x2, o, 64);
      U += __shfl_xor(U, o, 64);
    }
    if (lane == 0) {
      float e = (1.0f - c_s) / (2.0f * hv) * x2 - c_out / (c_in * hv) * U;
      if (beta) e *= beta[b];
      E[b] = e;
    }
  }
}

// ---- K11: per-chunk quantile (linear interpolation, torch.quantile semantics) + clamp, one block per chunk.
// The two order statistics come from an exact 4-pass radix select over order-preserving integer keys.
constexpr int QT = 1024;
__device__ __forceinline__ unsigned f2key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ float radix_select(const float* __restrict__ a, long long n, long long k, unsigned* hist, unsigned* sh) {
  unsigned prefix = 0, mask = 0;
  for (int pass = 3; pass >= 0; --pass) {
    for (int i = threadIdx.x; i < 256; i += QT) hist[i] = 0;
    __syncthreads();
    const int shift = pass * 8;
    for (long long i = threadIdx.x; i < n; i += QT) {
      const unsigned key = f2key(a[i]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long cum = 0;
      unsigned bin = 0;
      for (; bin < 256; ++bin) {
        if (cum + hist[bin] > (unsigned long long)k) break;
        cum += hist[bin];
      }
      sh[0] = bin;
      sh[1] = (unsigned)cum;
    }
    __syncthreads();
    prefix |= sh[0] << shift;
    mask |= 255u << shift;
    k -= sh[1];
    __syncthreads();
  }
  return key2f(prefix);
}

__global__ void __launch_bounds__(QT) quantile_clamp_kernel(float* __restrict__ a, long long B, long long chunk, float q) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh[2];
  const long long lo = (long long)blockIdx.x * chunk;
  const long long n = (B - lo) < chunk ? (B - lo) : chunk;
  if (n <= 0) return;
  float* ac = a + lo;
  const float rank = q * (float)(n - 1);
  const long long klo = (long long)floorf(rank);
  const long long khi = (klo + 1 < n) ? (long long)ceilf(rank) : klo;
  const float w = rank - (float)klo;
  float vlo, vhi;
  if (n <= QT) {
    // chunks of up to 1 024 walkers (the reference's inference chunks: 512 for LJ13): both order statistics by rank
    // counting -- thread i counts the elements that sort before its own (ties broken by index, so ranks are a
    // permutation), all threads reading the same key from LDS at a time (broadcast reads).  ~2 n instructions per
    // thread instead of the radix select's eight serial 256-bin scans (65 536 values: 17 us in chunks of 512, 43 us in
    // chunks of 1 024; the radix select takes 81 us in chunks of 2 048 and 163 us as one chunk: tools/time_clamp.py).
    __shared__ unsigned keys[QT];
    __shared__ float picked[2];
    const int t = threadIdx.x;
    const unsigned mine = t < n ? f2key(ac[t]) : 0xFFFFFFFFu;
    keys[t] = mine;
    __syncthreads();
    if (t < n) {
      int rank = 0;
      for (int j = 0; j < (int)n; ++j) {
        const unsigned kj = keys[j];
        rank += (kj < mine || (kj == mine && j < t)) ? 1 : 0;
      }
      if (rank == (int)klo) picked[0] = key2f(mine);
      if (rank == (int)khi) picked[1] = key2f(mine);
    }
    __syncthreads();
    vlo = picked[0];
    vhi = picked[1];
  } else {
    vlo = radix_select(ac, n, klo, hist, sh);
    vhi = (khi == klo) ? vlo : radix_select(ac, n, khi, hist, sh);
  }
  const float diff = vhi - vlo;
  const float quant = (w < 0.5f) ? fmaf(w, diff, vlo) : vhi - diff * (1.0f - w);  // at::lerp
  // a NaN entry keeps its value (fminf alone would hand it the quantile); a NaN quantile leaves the chunk as it is
  for (long long i = threadIdx.x; i < n; i += QT) {
    const float v = ac[i];
    ac[i] = (v != v) ? v : fminf(v, quant);
  }
}

}  // namespace pita

using namespace pita;

extern "C" int pita_fk_assemble(const float* x, const float* h, const float* g2, const float* dhdt, const float* D_E,
                                const float* jtx_E, const float* dot_h, const float* dot_parts, const float* D_S,
                                const float* trace_S, float gamma, float dgamma, const float* beta_e, const float* beta_s, float pin_w,
                                float pin_dw, const float* logp_target, float* drift_X, float* drift_A, float* div_bt,
                                float* cross, float* dUdt, float* Ut, int64_t B, int D, void* stream) {
  PITA_REQUIRE(B >= 0 && D >= 1, "pita_fk_assemble: bad shape");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(x && h && g2 && dhdt && D_E && jtx_E && dot_h && D_S && trace_S && drift_X && drift_A && div_bt && cross &&
               dUdt && Ut, "pita_fk_assemble: null argument");
  PITA_REQUIRE(logp_target || (pin_w == 0.f && pin_dw == 0.f), "pita_fk_assemble: pin weights without logp_target");
  FkParams p{};
  p.x = x; p.h = h; p.g2 = g2; p.dhdt = dhdt; p.beta_e = beta_e; p.beta_s = beta_s;
  p.pin_w = logp_target ? pin_w : 0.f; p.pin_dw = logp_target ? pin_dw : 0.f; p.logp_target = logp_target;
  p.D_E = D_E; p.jtx_E = jtx_E; p.dot_h = dot_h; p.dot_parts = dot_parts; p.D_S = D_S; p.trace_S = trace_S; p.gamma = gamma; p.dgamma = dgamma;
  p.drift_X = drift_X; p.drift_A = drift_A; p.div_bt = div_bt; p.cross = cross; p.dUdt = dUdt; p.Ut = Ut; p.B = B; p.D = D;
  const long long nb = (B + 3) / 4;  // one wave per walker, four waves per block
  hipLaunchKernelGGL(fk_assemble_kernel, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, (hipStream_t)stream, p);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_quantile_clamp(float* a, int64_t B, int64_t chunk, float q, void* stream) {
  PITA_REQUIRE(B >= 0 && chunk >= 1 && q >= 0.f && q <= 1.f, "pita_quantile_clamp: bad argument");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(a, "pita_quantile_clamp: null argument");
  const long long nchunk = (B + chunk - 1) / chunk;
  hipLaunchKernelGGL(quantile_clamp_kernel, dim3((unsigned)nchunk), dim3(QT), 0, (hipStream_t)stream, a, (long long)B,
                     (long long)chunk, q);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_energy_theta(const float* h, const float* x, const float* F, const float* beta, float* E, int64_t B,
                                 int D, void* stream) {
  PITA_REQUIRE(B >= 0 && D >= 1, "pita_energy_theta: bad shape");
  if (B == 0) return PITA_OK;
  PITA_REQUIRE(h && x && F && E, "pita_energy_theta: null argument");
  const long long nb = (B + 3) / 4;
  hipLaunchKernelGGL(energy_theta_kernel, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, (hipStream_t)stream, h, x, F,
                     beta, E, (long long)B, D);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}
