// Forward-mode derivatives of the EDM denoiser around the MLP backbone (MyMLP / MyMLPTemperature), for the debiased
// Feynman-Kac regime:  D(h, x) = c_s x + c_out F(c_noise, c_in x, beta),  c_noise = ln(h)/8.
//
// Replaces the reference's autograd / vmap(jacrev) through the network (paths relative to the reference's
// src/models/components/): score_net.py:13-43 around mlp.py:11-24, 100-118, 244-267, 501-524,
// differentiated by utils.py:30-51 (div s_theta), energy_net.py:51-62 (grad_x E_theta) and sdes.py:218 (dE_theta/dt).
//
// Mapping: mlp_tile's (mlp_kernel.hip) -- one wave = 32 walkers = the columns of a 32x32 tile, bf16 three-piece split,
// weights streamed once per workgroup -- plus K tangent tiles of the SAME 32 walkers, one direction each: every
// weight block fetched is applied to the primal tile and to the K tangent tiles.  GELU'(v) = Phi(v) + v phi(v) is taken
// from the primal pre-activation in the same lane and register.  The layer-0 tangent of an embedding chunk of variable
// v is [cos, -sin] * scale * f_k * dv, with dv = c_in dx_v + c_in' dh x_v for a coordinate and dh / (8h) for time; a
// tangent that does not touch a chunk's variable (a unit direction of another coordinate) skips its products.  When
// the directions exceed K they run in passes of K, each recomputing the primal (cheaper than keeping the per-layer
// GELU' anywhere: the register file holds the primal and K tangents).  All per-walker
// reductions (trace, <cot, J e_k>, <cot, dD/dh>, ...) happen in-kernel; only [B] and [B, D] results reach memory.
#include "mlp_common.h"

namespace pita {

struct MlpJacParams {
  MlpParams m;
  const float* h;
  const float* x;
  const float* beta;
  const float* cot;  // null: x
  // pita_mlp_jvp (jvp = 1): ONE tangent, dense vx or the unit direction dir (-1: none), plus vh
  const float* vx;
  const float* vh;
  int dir, jvp;
  // pita_mlp_jacobian (jvp = 0): unit directions 0 .. nx-1, then the h direction if with_h
  int nx, with_h;
  float *out_D, *trace, *vjp, *dot_h, *dot_parts;
  float *dout, *dot_out, *diag_acc;
  long long dot_stride, dot_off;
};

// d/dv of gelu_erf: Phi(v) + v phi(v), the normal cdf through the same erf as the primal
__device__ __forceinline__ float gelu_erf_deriv(float v) {
  const float Phi = 0.5f * (1.0f + erf_as(v * 0.70710678118654752f));
  const float phi = 0.39894228040143268f * __builtin_amdgcn_exp2f(-0.72134752044448170f * (v * v));  // e^{-v^2/2}/sqrt(2pi)
  return fmaf(v, phi, Phi);
}

// One pass over a 32-walker tile: the primal network and the K tangents of directions pass*K .. pass*K+K-1.
// tr accumulates this lane's walker's trace over the passes.
template <int NB, int K, typename Weights>
__device__ __forceinline__ void mlp_jac_tile(const MlpJacParams& q, Weights& W, int hh, long long wid, bool valid,
                                             int pass, float& tr) {
  const MlpParams& p = q.m;
  const int D = p.input_dim, half = p.emb >> 1;
  const long long wl = valid ? wid : p.B - 1;
  const float* xrow = q.x + wl * D;
  const float hv = q.h[wl];
  const float bv = p.temp ? q.beta[wl] : 0.f;
  // score_net.py:26-29 as pita_edm_scale_input / pita_edm_combine evaluate them, and their h-derivatives
  const float c_s = 1.0f / (1.0f + hv), c_in = 1.0f / sqrtf(1.0f + hv), sh = sqrtf(hv);
  const float c_out = sh * c_in, tv = 0.125f * logf(hv);
  const float dc_s = -c_s * c_s, dc_in = -0.5f * c_in * c_s, dc_out = 0.5f * c_in / sh + sh * dc_in;
  // tangent slots (wave-uniform except the per-walker h tangent sdh)
  int sdir[K];
  bool slive[K], sdense[K], shc[K];
  float sdh[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (q.jvp) {
      slive[k] = k == 0; sdir[k] = q.dir; sdense[k] = q.vx != nullptr; shc[k] = q.vh != nullptr;
      sdh[k] = shc[k] ? q.vh[wl] : 0.f;
    } else {
      const int g = pass * K + k;
      slive[k] = g < q.nx + q.with_h; sdir[k] = g < q.nx ? g : -1; sdense[k] = false; shc[k] = g == q.nx && q.with_h;
      sdh[k] = shc[k] ? 1.0f : 0.f;
    }
  }
  // tangent of backbone input `var` (coordinate, time, beta) along slot k, and whether it can be non-zero
  auto dinput = [&](int k, int var) -> float {
    if (var < D) {
      const float dx = sdense[k] ? q.vx[wl * D + var] : (var == sdir[k] ? 1.0f : 0.0f);
      return fmaf(c_in, dx, (sdh[k] * dc_in) * xrow[var]);
    }
    return var == D ? sdh[k] * (0.125f / hv) : 0.f;
  };
  auto touches = [&](int k, int var) -> bool {
    return slive[k] && (var < D ? (sdense[k] || shc[k] || var == sdir[k]) : (var == D && shc[k]));
  };
  auto input_of = [&](int var, float& v, float& scale) {
    if (var < D) { v = xrow[var] * c_in; scale = 25.0f; }
    else if (var == D) { v = tv; scale = 1.0f; }
    else { v = bv; scale = 1.0f; }
  };

  // ---- layer 0
  f32x16 z[NB], dz[K][NB];
#pragma unroll
  for (int ob = 0; ob < NB; ++ob) {
    z[ob] = mlp_bias(p.b0 + ob * 32, hh);
#pragma unroll
    for (int k = 0; k < K; ++k) dz[k][ob] = f32x16{0};
  }
  auto feed = [&](const f32x16& e, const f32x16 (&de)[K], const bool (&on)[K], int kc) {
    u32x4 es[3][2], ds[K][3][2];
    WFrag<1>::split(e, es);
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (on[k]) WFrag<1>::split(de[k], ds[k]);
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {
      const WFrag<1> w = W.fetch(p.w0, ob * p.KC + kc);
      z[ob] = w.mul_split(es, z[ob]);
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (on[k]) dz[k][ob] = w.mul_split(ds[k], dz[k][ob]);
      W.done();
    }
  };
  if ((half & 31) == 0) {  // the block order of StreamWeights: each sine chunk, then its cosine chunk
    const int hc = half >> 5, per_var = 2 * hc;
    for (int kc = 0; kc < p.KC; ++kc) {
      const int var = kc / per_var, c = kc - var * per_var;
      if (c >= hc) continue;
      float v, scale;
      input_of(var, v, scale);
      bool on[K];
      float dv[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        on[k] = touches(k, var);
        dv[k] = on[k] ? dinput(k, var) * scale : 0.f;
      }
      f32x16 es_, ec_, des[K], dec[K];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float fr = p.freqs[c * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh];
        float sn, cs;
        sincos_rev((v * scale) * fr, sn, cs);
        es_[r] = sn;
        ec_[r] = cs;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float da = dv[k] * fr;
          des[k][r] = cs * da;
          dec[k][r] = -(sn * da);
        }
      }
      feed(es_, des, on, kc);
      feed(ec_, dec, on, kc + hc);
    }
  } else {
    for (int kc = 0; kc < p.KC; ++kc) {
      f32x16 e, de[K];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = kc * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        const int var = f / p.emb, idx = f - var * p.emb;
        float v, scale;
        input_of(var, v, scale);
        const float fr = p.freqs[idx < half ? idx : idx - half];
        float sn, cs;
        sincos_rev((v * scale) * fr, sn, cs);
        e[r] = idx < half ? sn : cs;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float da = slive[k] ? (dinput(k, var) * scale) * fr : 0.f;
          de[k][r] = idx < half ? cs * da : -(sn * da);
        }
      }
      feed(e, de, slive, kc);
    }
  }
#pragma unroll
  for (int ob = 0; ob < NB; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = z[ob][r], gd = gelu_erf_deriv(v);
      z[ob][r] = gelu_erf(v);
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (slive[k]) dz[k][ob][r] *= gd;
    }
  // ---- residual blocks: z += GELU(W_l z + b_l),  dz += GELU'(W_l z + b_l) W_l dz
  for (int l = 0; l < p.n_layers; ++l) {
    f32x16 nz[NB], dnz[K][NB];
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {
      nz[ob] = mlp_bias(p.bl + ((size_t)l * NB + ob) * 32, hh);
#pragma unroll
      for (int k = 0; k < K; ++k) dnz[k][ob] = f32x16{0};
    }
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      u32x4 zs[3][2], ds[K][3][2];
      WFrag<1>::split(z[kb], zs);
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (slive[k]) WFrag<1>::split(dz[k][kb], ds[k]);
#pragma unroll
      for (int ob = 0; ob < NB; ++ob) {
        const WFrag<1> w = W.fetch(p.wl, (l * NB + ob) * NB + kb);
        nz[ob] = w.mul_split(zs, nz[ob]);
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (slive[k]) dnz[k][ob] = w.mul_split(ds[k], dnz[k][ob]);
        W.done();
      }
    }
#pragma unroll
    for (int ob = 0; ob < NB; ++ob)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = nz[ob][r], gd = gelu_erf_deriv(v);
        z[ob][r] += gelu_erf(v);
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (slive[k]) dz[k][ob][r] = fmaf(gd, dnz[k][ob][r], dz[k][ob][r]);
      }
  }
  // ---- output head, D and dD row by row, per-walker reductions
  float pF = 0.f, pp = 0.f, ptr = 0.f, pv[K];
#pragma unroll
  for (int k = 0; k < K; ++k) pv[k] = 0.f;
  for (int ob = 0; ob < p.NBO; ++ob) {
    f32x16 o = mlp_bias(p.bf + ob * 32, hh), dO[K];
#pragma unroll
    for (int k = 0; k < K; ++k) dO[k] = f32x16{0};
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      const WFrag<1> w = W.fetch(p.wf, ob * NB + kb);
      o = w.mul(z[kb], o);
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (slive[k]) dO[k] = w.mul(dz[k][kb], dO[k]);
      W.done();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (row >= D) continue;
      const float xv = xrow[row], F = o[r];
      const float cv = q.cot ? q.cot[wl * D + row] : xv;
      if (pass == 0) {
        if (q.out_D && valid) q.out_D[wid * D + row] = c_s * xv + c_out * F;
        pF = fmaf(cv, F, pF);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (!slive[k]) continue;
        const float dx = sdense[k] ? q.vx[wl * D + row] : (row == sdir[k] ? 1.0f : 0.0f);
        const float dcF = fmaf(c_out, dO[k][r], (sdh[k] * dc_out) * F);  // d(c_out F)
        const float dD = fmaf(c_s, dx, fmaf(sdh[k] * dc_s, xv, dcF));
        pv[k] = fmaf(cv, dD, pv[k]);
        if (shc[k]) pp = fmaf(cv, dcF, pp);
        if (row == sdir[k]) ptr += dD;
        if (q.jvp && q.dout && valid) q.dout[wid * D + row] = dD;
      }
    }
  }
  // the two lanes of a walker (hh = 0, 1) hold complementary rows
  pF += __shfl_xor(pF, 32, 64);
  pp += __shfl_xor(pp, 32, 64);
  ptr += __shfl_xor(ptr, 32, 64);
#pragma unroll
  for (int k = 0; k < K; ++k) pv[k] += __shfl_xor(pv[k], 32, 64);
  tr += ptr;
  if (!valid || hh != 0) return;
  if (q.jvp) {
    if (q.dot_out) q.dot_out[wid * q.dot_stride + q.dot_off] = pv[0];
    if (q.diag_acc && q.dir >= 0) q.diag_acc[wid] += ptr;
    return;
  }
  if (pass == 0 && q.dot_parts) q.dot_parts[wid * 2] = c_out * pF;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (!slive[k]) continue;
    if (sdir[k] >= 0 && q.vjp) q.vjp[wid * D + sdir[k]] = pv[k];
    if (shc[k]) {
      if (q.dot_h) q.dot_h[wid] = pv[k];
      if (q.dot_parts) q.dot_parts[wid * 2 + 1] = pp;
    }
  }
}

template <int NB, int K, bool STREAM>
__global__ void __launch_bounds__(256, 1) mlp_jac_kernel(MlpJacParams q) {
  __shared__ __attribute__((aligned(16))) unsigned wbuf[STREAM ? 2 * MAT_W : 4];
  const MlpParams& p = q.m;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, cl = lane & 31, hh = lane >> 5;
  const long long ntile = (p.B + 31) / 32, ngroup = (ntile + 3) / 4;
  const int ndir = q.jvp ? 1 : q.nx + q.with_h;
  const int npass = ndir == 0 ? 1 : (ndir + K - 1) / K;
  StreamWeights SW{p.stream, wbuf, p.S, 0, 0, (int)threadIdx.x, lane, {}};
  GlobalWeights GW{p, lane};
  if (STREAM) SW.prime();
  for (long long grp = blockIdx.x; grp < ngroup; grp += gridDim.x) {  // block-uniform trip counts (barriers inside)
    const long long wid = (grp * 4 + wave) * 32 + cl;
    const bool valid = wid < p.B;
    float tr = 0.f;
    for (int pass = 0; pass < npass; ++pass) {
      if (STREAM) mlp_jac_tile<NB, K>(q, SW, hh, wid, valid, pass, tr);
      else mlp_jac_tile<NB, K>(q, GW, hh, wid, valid, pass, tr);
    }
    if (q.trace && valid && hh == 0) q.trace[wid] = tr;
  }
}

// tangent tiles per pass of pita_mlp_jacobian, by hidden blocks NB: what fits the 512 registers of one wave per SIMD
// next to the primal without scratch (the residual layer holds z, W z and their K tangents: 32 NB (1 + K) registers,
// plus the bf16 splits of one input block for the primal and each tangent)
constexpr int mlp_jac_k(int nb) { return nb == 1 ? 4 : (nb == 2 ? 2 : 1); }

}  // namespace pita

using namespace pita;

static int mlp_jac_check(const pita_mlp* net, const float* h, const float* x, const float* beta, int64_t B,
                         const char* who) {
  PITA_REQUIRE(net && B >= 0, "%s: bad argument", who);
  // an empty batch has null data pointers: the callers return before any launch
  PITA_REQUIRE(B == 0 || (h && x), "%s: null argument", who);
  PITA_REQUIRE(B == 0 || beta || !net->cfg.temperature_conditioned, "%s: beta required (temperature_conditioned)", who);
  const int D = net->cfg.input_dim;
  if (net->cfg.out_dim != D)
    return fail(PITA_EUNSUPPORTED, "%s: the denoiser's Jacobian needs out_dim == input_dim (got %d, %d)", who,
                net->cfg.out_dim, D);
  if (D > 64) return fail(PITA_EUNSUPPORTED, "%s: input_dim=%d (<= 64 implemented)", who, D);
  return PITA_OK;
}

template <int NB, int K>
static void mlp_jac_launch_nb(const MlpJacParams& q, unsigned grid, hipStream_t s) {
  if (q.m.stream) hipLaunchKernelGGL((mlp_jac_kernel<NB, K, true>), dim3(grid), dim3(256), 0, s, q);
  else hipLaunchKernelGGL((mlp_jac_kernel<NB, K, false>), dim3(grid), dim3(256), 0, s, q);
}

static int mlp_jac_launch(const pita_mlp* net, MlpJacParams& q, int64_t B, void* stream) {
  q.m = net->p;
  q.m.B = B;
  const long long nblk = ((B + 31) / 32 + 3) / 4;
  const unsigned grid = (unsigned)(nblk < 4096 ? nblk : 4096);
  hipStream_t s = (hipStream_t)stream;
  // the jvp carries one tangent, the Jacobian mlp_jac_k(NB) per pass
  switch (net->cfg.hidden_size / 32) {
    case 1: q.jvp ? mlp_jac_launch_nb<1, 1>(q, grid, s) : mlp_jac_launch_nb<1, mlp_jac_k(1)>(q, grid, s); break;
    case 2: q.jvp ? mlp_jac_launch_nb<2, 1>(q, grid, s) : mlp_jac_launch_nb<2, mlp_jac_k(2)>(q, grid, s); break;
    default: mlp_jac_launch_nb<4, mlp_jac_k(4)>(q, grid, s); break;
  }
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_mlp_jacobian(pita_mlp_t* net, const float* h, const float* x, const float* beta, const float* cot,
                                 float* out_D, float* trace, float* vjp, float* dot_h, float* dot_parts, int64_t B,
                                 void* stream) {
  const int rc = mlp_jac_check(net, h, x, beta, B, "pita_mlp_jacobian");
  if (rc != PITA_OK) return rc;
  if (B == 0 || !(out_D || trace || vjp || dot_h || dot_parts)) return PITA_OK;
  MlpJacParams q{};
  q.h = h; q.x = x; q.beta = beta; q.cot = cot;
  q.jvp = 0; q.dir = -1;
  q.nx = (trace || vjp) ? net->cfg.input_dim : 0;
  q.with_h = (dot_h || dot_parts) ? 1 : 0;
  q.out_D = out_D; q.trace = trace; q.vjp = vjp; q.dot_h = dot_h; q.dot_parts = dot_parts;
  return mlp_jac_launch(net, q, B, stream);
}

extern "C" int pita_mlp_jvp(pita_mlp_t* net, const float* h, const float* x, const float* beta, const float* vx, int dir,
                            const float* vh, float* out, float* dout, float* dot_out, int64_t dot_stride, int64_t dot_off,
                            float* diag_acc, int64_t B, void* stream) {
  const int rc = mlp_jac_check(net, h, x, beta, B, "pita_mlp_jvp");
  if (rc != PITA_OK) return rc;
  const int D = net->cfg.input_dim;
  PITA_REQUIRE(dir >= -1 && dir < D, "pita_mlp_jvp: dir=%d outside [-1, %d)", dir, D);
  PITA_REQUIRE(!dot_out || (dot_stride >= 1 && dot_off >= 0 && dot_off < dot_stride),
               "pita_mlp_jvp: dot_out needs 0 <= dot_off < dot_stride");
  if (B == 0 || !(out || dout || dot_out || diag_acc)) return PITA_OK;
  MlpJacParams q{};
  q.h = h; q.x = x; q.beta = beta; q.cot = nullptr;
  q.vx = vx; q.vh = vh; q.dir = dir; q.jvp = 1;
  q.out_D = out; q.dout = dout; q.dot_out = dot_out; q.dot_stride = dot_stride; q.dot_off = dot_off;
  q.diag_acc = diag_acc;
  return mlp_jac_launch(net, q, B, stream);
}
