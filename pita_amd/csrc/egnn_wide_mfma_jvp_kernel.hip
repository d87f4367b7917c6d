// Forward-mode derivative of the EDM denoiser around the wide EGNN backbone on the MATRIX pipe of gfx950 (MI355X).
//
// Replaces, for EGNN_dynamics_AD2_cat / egnn_aldp.EGNN_dynamics (paths relative to /root/reference/pita/src/models/components/):
//   utils.py:30-51          compute_divergence_exact (vmap(jacrev) of the score net)
//   energy_net.py:51-62     grad_x E_theta by autograd
//   sdes.py:218             dE_theta/dt by autograd through h(t)
// all of which are sums of directional derivatives  dD = J_x D(h, x) . vx + dD/dh . vh  of
// D(h, x) = c_s x + c_out F(c_noise(h), c_in(h) x, beta)  (score_net.py:13-43 around egnn_dynamics_ad2_cat.py:157-203).
//
// Mapping: egnn_wide64_kernel's one-walker-per-wave instantiation (one column tile: lane = (column, half of the 64 hidden
// features), dense layers as 2 x 2 blocks of the f16 two-piece MFMA tile); particle systems of more than 32 atoms take
// NT = 2 waves per item, one per 32-column tile, that share the item's LDS tables and meet at a block barrier wherever
// a table is published (each wave keeps the one-tile register footprint).  ONE tangent direction is carried beside the
// primal: every linear map is applied to the tangent with the same weight fragments (the tangent of a GEMM is the GEMM of
// the tangent), every SiLU passes its derivative sigma + y (1 - sigma) / kS on from the primal's own sigmoid (no further
// transcendental), tangents travel in the scaled units of their primals (egnn_common.h: kS, F16_SX, F16_SW), partner
// terms Wb dh_j and tangent positions in LDS tables beside the primal ones.  A walker whose primal or tangent leaves
// the f16 range is flagged and left to the fp32 vector-pipe kernel (egnn_wide_kernel.hip: egnn_wide_jvp_kernel).
#include "egnn_wide_mfma_common.h"

namespace pita {

struct Wide64JvpParams {
  const unsigned* m16h;
  const float* vecs;
  const float* est;
  int L, has_beta;
  float coord_scale;
  long long B;
  const float* x;
  const float* h;
  const float* beta;
  const float* vx;   // nullable [B, N*DIM]
  const float* vh;   // nullable [B]
  int dir;           // unit direction when vx is null (-1: none)
  float* out;        // nullable: D
  float* dout;       // nullable: dD
  float* dot_out;    // nullable: dot_out[b * dot_stride + dot_off] = <x_b, dD_b>
  long long dot_stride, dot_off;
  float* diag_acc;   // nullable: diag_acc[b] += dD[b, dir]; MULTI: [N*DIM, B], diag_acc[dir * B + b] = dD[b, dir]
  int* bad;          // [B] (MULTI: [B * N*DIM], PROBE: [B * n_probes], one per item), zeroed by the launch wrapper: 1 = left
                     // to the vector-pipe kernel
  // PROBE items, as WideJvpParams
  int n_probes;
  const float* probes;
  unsigned long long seed, walker_offset;
  long long step;
};

template <int N, int DIM, int WAVES>
struct Wide64JvpCfg {
  static constexpr int NCOLP = 32 * ((N + 31) / 32);
  static constexpr int NT = NCOLP / 32;
  static constexpr int PB_F = NCOLP * W64_PBS;
  static constexpr int POS_F = NCOLP * DIM;
  static constexpr int IPB = WAVES / NT;               // items per block: NT waves (one per column tile) share an item
  static constexpr int WAVE_F = 2 * PB_F + 6 * POS_F;  // per item: partner table + its tangent, pos[2], pos0 + their tangents
  static __host__ __device__ constexpr int vec_f(int L) { return ((W64_HEAD_F + L * W64_LAYER_F) + 3) & ~3; }
  static __host__ __device__ constexpr size_t lds_bytes(int L) {
    return sizeof(float) * (size_t)(vec_f(L) + N * 64 + IPB * WAVE_F);
  }
};

// MULTI: the work items are (walker, unit direction) pairs, item = walker * N*DIM + direction (adjacent items share a
// walker's inputs), each computed exactly as the single-direction launch with vx = vh = null computes it; the item's
// diagonal entry dD[dir] goes to its own slot (plain store), the item of direction 0 writes the denoiser row; vx, vh, dir,
// dout and dot_out are ignored.
// PROBE: the work items are (walker, probe) pairs, item = walker * n_probes + probe, each computed exactly as the
// single-direction launch with vx = v_probe, vh = null computes it -- v_probe row [probe, walker] of `probes`, or, without
// it, Rademacher signs drawn here (common.h: philox_rademacher_word; bit k of the column's word is coordinate k) --; the
// item's quadratic form <v_probe, dD>, summed on the path of dot_out's <x, dD> (within a column over the coordinates,
// then over columns 0 .. N-1), goes to its own slot diag_acc[probe * B + walker] (plain store), the item of probe 0 writes
// the denoiser row; vx, vh, dir, dout and dot_out are ignored.
template <int N, int DIM, int WAVES, bool ATT, bool TANH, int KIND = WIDE_JVP_ONE>
__global__ void __launch_bounds__(WAVES * 64, 1) egnn_wide64_jvp_kernel(Wide64JvpParams p) {
  using C = Wide64JvpCfg<N, DIM, WAVES>;
  constexpr bool MULTI = KIND == WIDE_JVP_UNIT, PROBE = KIND == WIDE_JVP_PROBE;
  static_assert(C::NT * C::IPB == WAVES && C::NT <= 2, "NT waves per item, one per column tile");
  constexpr int NT = C::NT;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int L = p.L;
  const int vec_f = C::vec_f(L);
  for (int i = threadIdx.x; i < W64_HEAD_F + L * W64_LAYER_F; i += WAVES * 64) lds[i] = p.vecs[i];
  float* est = lds + vec_f;
  for (int i = threadIdx.x; i < N * 64; i += WAVES * 64) est[i] = p.est[i];
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, cl = lane & 31, hh = lane >> 5;
  const int slot = wave / NT, tile = wave % NT;  // the item's place in the block, this wave's column tile
  float* PB = est + N * 64 + slot * C::WAVE_F;
  float* dPB = PB + C::PB_F;
  float* posbuf0 = dPB + C::PB_F;
  float* posbuf1 = posbuf0 + C::POS_F;
  float* pos0 = posbuf1 + C::POS_F;
  float* dposbuf0 = pos0 + C::POS_F;
  float* dposbuf1 = dposbuf0 + C::POS_F;
  float* dpos0 = dposbuf1 + C::POS_F;
  const f32x16 zero16 = {0};
  const int col = tile * 32 + cl, nodei = col < N ? col : 0;
  const bool valid = col < N;
  const int live = valid ? 1 : 0;

  constexpr int NDIR = N * DIM;
  const long long items = MULTI ? p.B * NDIR : PROBE ? p.B * p.n_probes : p.B;
  // block-uniform trip count (the NT == 2 body holds block barriers): a slot past the last item computes that item again
  // in its own tables and writes nothing (at most one wasted item per block and launch, in the block's last trip); with
  // one wave per item such a wave has no barrier to keep and leaves
  for (long long base = (long long)blockIdx.x * C::IPB; base < items; base += (long long)gridDim.x * C::IPB) {
    const bool active = base + slot < items;
    if (NT == 1 && !active) break;
    const long long item = active ? base + slot : items - 1;
    const long long w = MULTI ? item / NDIR : PROBE ? item / p.n_probes : item;
    const int dir = MULTI ? (int)(item - w * NDIR) : PROBE ? -1 : p.dir;
    const int probe = PROBE ? (int)(item - w * p.n_probes) : 0;
    const float* const vxp = MULTI ? nullptr : PROBE ? (p.probes ? p.probes + (long long)probe * p.B * NDIR : nullptr) : p.vx;
    const float hv = p.h[w];
    const float bet = p.has_beta ? p.beta[w] : 0.f;
    const float vh = (!MULTI && !PROBE && p.vh) ? p.vh[w] : 0.f;
    uint32_t signs = 0;
    if constexpr (PROBE)
      if (!vxp) signs = philox_rademacher_word(p.seed, p.walker_offset + (unsigned long long)w, p.step, (uint32_t)probe, (uint32_t)nodei);
    // score_net.py:26-29 and their h-derivatives
    const float c_s = 1.0f / (1.0f + hv), c_in = 1.0f / sqrtf(1.0f + hv), sh = sqrtf(hv);
    const float c_out = sh * c_in, tfeat = 0.125f * logf(hv);
    const float dc_s = -c_s * c_s, dc_in = -0.5f * c_in * c_s, dc_out = 0.5f * c_in / sh + sh * dc_in;
    const float dtf = vh * (0.125f / hv);
    float xin[DIM], dxin[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const long long e = (w * N + col) * DIM + k;
      xin[k] = valid ? p.x[e] : 0.f;
      if constexpr (PROBE) dxin[k] = valid ? (vxp ? vxp[e] : rademacher_sign(signs, k)) : 0.f;
      else dxin[k] = valid ? (vxp ? vxp[e] : ((col * DIM + k) == dir ? 1.0f : 0.0f)) : 0.f;
      const float ps = c_in * xin[k], dps = fmaf(c_in, dxin[k], (vh * dc_in) * xin[k]);
      if (hh == 0) {
        pos0[col * DIM + k] = ps; posbuf0[col * DIM + k] = ps;
        dpos0[col * DIM + k] = dps; dposbuf0[col * DIM + k] = dps;
      }
    }
    f32x16 hfeat[2], dhfeat[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const f32x16 wt = lds_vec16(lds + b * 32 + hh * 16), wb = lds_vec16(lds + 64 + b * 32 + hh * 16);
      const f32x16 es = lds_vec16(est + nodei * 64 + b * 32 + hh * 16);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        hfeat[b][r] = fmaf(wt[r], tfeat, fmaf(wb[r], bet, es[r]));
        dhfeat[b][r] = wt[r] * dtf;
      }
    }
    item_fence<NT>();

    float* poscur = posbuf0; float* posnext = posbuf1;
    float* dposcur = dposbuf0; float* dposnext = dposbuf1;
    for (int l = 0; l < L; ++l) {
      const unsigned* ml = p.m16h + (size_t)l * WM_COUNT * W64_MAT_W;
      const float* vbase = lds + W64_HEAD_F + l * W64_LAYER_F;
      const float* vl = vbase + hh * 16;
      const bool last = (l == L - 1);
      const float aggw = last ? 0.0f : 1.0f;
      {  // partner tables Wb h_col, Wb dh_col
        f32x16 pb[2] = {zero16, zero16}, dpb[2] = {zero16, zero16};
        w64_mul_stream(ml, WM_WB, lane, hfeat, pb);
        w64_mul_stream(ml, WM_WB, lane, dhfeat, dpb);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          pb[b] *= F16_UNSCALE; dpb[b] *= F16_UNSCALE;
          lds_store16(PB + col * W64_PBS + b * 32 + hh * 16, pb[b]);
          lds_store16(dPB + col * W64_PBS + b * 32 + hh * 16, dpb[b]);
        }
      }
      item_fence<NT>();

      W64Mat w2f, wc1f;
      w2f.load(ml, WM_W2, lane);
      wc1f.load(ml, WM_WC1, lane);
      w2f.to_agpr();
      wc1f.to_agpr();
      const float a_re0 = vbase[WV_WRE * 64 + lane], a_re1 = vbase[WV_WRE * 64 + 64 + lane];
      const float b_att = vbase[WV_COUNT * 64];

      f32x16 Ai[2] = {lds_vec16(vl + WV_B1 * 64), lds_vec16(vl + WV_B1 * 64 + 32)}, dAi[2] = {zero16, zero16};
      w64_mul_stream(ml, WM_WA, lane, hfeat, Ai);
      w64_mul_stream(ml, WM_WA, lane, dhfeat, dAi);
      Ai[0] *= F16_UNSCALE; Ai[1] *= F16_UNSCALE; dAi[0] *= F16_UNSCALE; dAi[1] *= F16_UNSCALE;
      f32x16 agg[2] = {zero16, zero16}, dagg[2] = {zero16, zero16};
      float xacc[DIM], dxacc[DIM], pown[DIM], p0own[DIM], dpown[DIM], dp0own[DIM];
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        xacc[k] = 0.f; dxacc[k] = 0.f;
        pown[k] = poscur[col * DIM + k]; p0own[k] = pos0[col * DIM + k];
        dpown[k] = dposcur[col * DIM + k]; dp0own[k] = dpos0[col * DIM + k];
      }
      for (int dd = 1; dd < N; ++dd) {
        asm volatile("" ::: "memory");
        int j = nodei + dd * live;
        j = (j >= N) ? j - N : j;
        const int cj = valid ? j : col;
        float df[DIM], ddf[DIM], radial = 0.f, ea = 0.f, dradial = 0.f, dea = 0.f;
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
          df[k] = pown[k] - poscur[cj * DIM + k];
          ddf[k] = dpown[k] - dposcur[cj * DIM + k];
          radial = fmaf(df[k], df[k], radial);
          dradial = fmaf(df[k], ddf[k], dradial);
          const float e0 = p0own[k] - pos0[cj * DIM + k];
          ea = fmaf(e0, e0, ea);
          dea = fmaf(e0, dp0own[k] - dpos0[cj * DIM + k], dea);
        }
        dradial *= 2.0f; dea *= 2.0f;
        const float geo = hh ? ea : radial, dgeo = hh ? dea : dradial;
        f32x16 m[2], dm[2], g[2];
        m[0] = Ai[0] + lds_vec16(PB + cj * W64_PBS + hh * 16);
        m[1] = Ai[1] + lds_vec16(PB + cj * W64_PBS + 32 + hh * 16);
        dm[0] = dAi[0] + lds_vec16(dPB + cj * W64_PBS + hh * 16);
        dm[1] = dAi[1] + lds_vec16(dPB + cj * W64_PBS + 32 + hh * 16);
        m[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re0, geo, m[0], 0, 0, 0);
        m[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re1, geo, m[1], 0, 0, 0);
        dm[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re0, dgeo, dm[0], 0, 0, 0);
        dm[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re1, dgeo, dm[1], 0, 0, 0);
        silu16_d<false>(m[0], g[0]);
        silu16_d<false>(m[1], g[1]);
        dm[0] *= g[0]; dm[1] *= g[1];
        f32x16 z[2] = {lds_vec16(vl + WV_B2 * 64), lds_vec16(vl + WV_B2 * 64 + 32)}, dz[2] = {zero16, zero16};
        w2f.mul(m, z);
        w2f.mul(dm, dz);
        silu16_d<true>(z[0], g[0]);
        silu16_d<true>(z[1], g[1]);
        dz[0] *= g[0] * F16_UNSCALE; dz[1] *= g[1] * F16_UNSCALE;
        if (ATT) {
          const f32x16 wa0 = lds_vec16(vl + WV_WATT * 64), wa1 = lds_vec16(vl + WV_WATT * 64 + 32);
          const float s = xhalf_sum(dot16(wa0, z[0]) + dot16(wa1, z[1])) + b_att;
          const float ds = xhalf_sum(dot16(wa0, dz[0]) + dot16(wa1, dz[1]));
          const float att = fast_sigmoid(s);
          const float datt = att * (1.0f - att) * ds;
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              dz[b][r] = fmaf(dz[b][r], att, z[b][r] * datt);
              z[b][r] *= att;
            }
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            agg[b][r] = fmaf(z[b][r], aggw, agg[b][r]);
            dagg[b][r] = fmaf(dz[b][r], aggw, dagg[b][r]);
          }
        f32x16 c1[2] = {lds_vec16(vl + WV_BC1 * 64), lds_vec16(vl + WV_BC1 * 64 + 32)}, dc1[2] = {zero16, zero16};
        wc1f.mul(z, c1);
        wc1f.mul(dz, dc1);
        silu16_d<true>(c1[0], g[0]);
        silu16_d<true>(c1[1], g[1]);
        dc1[0] *= g[0] * F16_UNSCALE; dc1[1] *= g[1] * F16_UNSCALE;
        const f32x16 wc0 = lds_vec16(vl + WV_WC2 * 64), wc1v = lds_vec16(vl + WV_WC2 * 64 + 32);
        float cs = xhalf_sum(dot16(wc0, c1[0]) + dot16(wc1v, c1[1]));
        float dcs = xhalf_sum(dot16(wc0, dc1[0]) + dot16(wc1v, dc1[1]));
        if (TANH) {
          const float th = tanh_select(cs);
          dcs = (1.0f - th * th) * p.coord_scale * dcs;
          cs = th * p.coord_scale;
        }
        const float sq = __builtin_amdgcn_sqrtf(radial + 1e-8f);
        const float inrm = __builtin_amdgcn_rcpf(sq + 1.0f);
        const float dinrm = -inrm * inrm * (0.5f * dradial * __builtin_amdgcn_rcpf(sq));
        const float dsc = fmaf(dinrm, cs, inrm * dcs);
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
          xacc[k] = fmaf(df[k] * inrm, cs, xacc[k]);
          dxacc[k] = fmaf(ddf[k], inrm * cs, fmaf(df[k], dsc, dxacc[k]));
        }
      }
#pragma unroll
      for (int k = 0; k < DIM; ++k)
        if (hh == 0) {
          posnext[col * DIM + k] = pown[k] + xacc[k];
          dposnext[col * DIM + k] = dpown[k] + dxacc[k];
        }
      if (!last) {  // node model, recurrent
        f32x16 n1[2] = {lds_vec16(vl + WV_BN1 * 64), lds_vec16(vl + WV_BN1 * 64 + 32)}, dn1[2] = {zero16, zero16}, g[2];
        w64_mul_stream(ml, WM_WN1A, lane, hfeat, n1);
        w64_mul_stream(ml, WM_WN1B, lane, agg, n1);
        w64_mul_stream(ml, WM_WN1A, lane, dhfeat, dn1);
        w64_mul_stream(ml, WM_WN1B, lane, dagg, dn1);
        silu16_d<true>(n1[0], g[0]);
        silu16_d<true>(n1[1], g[1]);
        dn1[0] *= g[0] * F16_UNSCALE; dn1[1] *= g[1] * F16_UNSCALE;
        f32x16 o[2] = {lds_vec16(vl + WV_BN2 * 64), lds_vec16(vl + WV_BN2 * 64 + 32)}, d_o[2] = {zero16, zero16};
        w64_mul_stream(ml, WM_WN2, lane, n1, o);
        w64_mul_stream(ml, WM_WN2, lane, dn1, d_o);
        hfeat[0] += o[0] * F16_UNSCALE; hfeat[1] += o[1] * F16_UNSCALE;
        dhfeat[0] += d_o[0] * F16_UNSCALE; dhfeat[1] += d_o[1] * F16_UNSCALE;
      }
      item_fence<NT>();
      float* tmp = poscur; poscur = posnext; posnext = tmp;
      tmp = dposcur; dposcur = dposnext; dposnext = tmp;
    }

    // ---- F = x_final - x (mean-free), D = c_s x + c_out F and their tangents; reductions over the walker
    float* scr = PB;        // [NCOLP][DIM] F, then per-column <x, dD> and the non-finite flags
    float* dscr = dPB;      // [NCOLP][DIM] dF
    float F[DIM], dF[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      F[k] = poscur[col * DIM + k] - pos0[col * DIM + k];
      dF[k] = dposcur[col * DIM + k] - dpos0[col * DIM + k];
      if (hh == 0) { scr[col * DIM + k] = F[k]; dscr[col * DIM + k] = dF[k]; }
    }
    item_fence<NT>();
    float Dv[DIM], dD[DIM], part = 0.f;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      float s = 0.f, ds = 0.f;
      for (int q = 0; q < N; ++q) { s += scr[q * DIM + k]; ds += dscr[q * DIM + k]; }
      F[k] -= s / (float)N;
      dF[k] -= ds / (float)N;
      Dv[k] = fmaf(c_s, xin[k], c_out * F[k]);
      dD[k] = fmaf(c_s, dxin[k], fmaf(c_out, dF[k], vh * fmaf(dc_s, xin[k], dc_out * F[k])));
      part = fmaf(PROBE ? dxin[k] : xin[k], dD[k], part);
      ok = ok && __builtin_isfinite(Dv[k]) && __builtin_isfinite(dD[k]);
    }
    item_fence<NT>();
    float* red = scr;       // [NCOLP][2]: <x, dD> (PROBE: <v, dD>) of the column, its non-finite flag
    if (hh == 0) { red[col * 2] = valid ? part : 0.f; red[col * 2 + 1] = (valid && !ok) ? 1.0f : 0.0f; }
    item_fence<NT>();
    float dot = 0.f, nbad = 0.f;
    for (int q = 0; q < N; ++q) { dot += red[q * 2]; nbad += red[q * 2 + 1]; }
    if (!active) {  // a slot past the last item: its recomputed copy writes nothing
    } else if (nbad != 0.f) {  // uniform over the item's waves: all read the same flags
      if (lane == 0 && tile == 0) p.bad[item] = 1;
    } else if (valid && hh == 0) {
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        const long long e = (w * N + col) * DIM + k;
        if (MULTI) {
          if (p.out && dir == 0) p.out[e] = Dv[k];
          if ((col * DIM + k) == dir) p.diag_acc[(long long)dir * p.B + w] = dD[k];
        } else if (PROBE) {
          if (p.out && probe == 0) p.out[e] = Dv[k];
        } else {
          if (p.out) p.out[e] = Dv[k];
          if (p.dout) p.dout[e] = dD[k];
          if (p.diag_acc && !p.vx && (col * DIM + k) == p.dir) p.diag_acc[w] += dD[k];
        }
      }
      if (PROBE && col == 0) p.diag_acc[(long long)probe * p.B + w] = dot;
      if (!MULTI && !PROBE && p.dot_out && col == 0) p.dot_out[w * p.dot_stride + p.dot_off] = dot;
    }
    item_fence<NT>();
  }
}

// alanine dipeptide (22 atoms: one wave per item), tri-alanine (33) and ACE-(ALA)3-NME (42: two waves per item, one per
// column tile: 4 or 2 items per block); other particle counts take the vector-pipe kernel
template <int N, int DIM, int WAVES>
static Wide64Row<Wide64JvpParams> wide64_jvp_row_of() {
  using C = Wide64JvpCfg<N, DIM, WAVES>;
#define PITA_K(A, T) egnn_wide64_jvp_kernel<N, DIM, WAVES, A, T>
#define PITA_KM(A, T) egnn_wide64_jvp_kernel<N, DIM, WAVES, A, T, WIDE_JVP_UNIT>
#define PITA_KP(A, T) egnn_wide64_jvp_kernel<N, DIM, WAVES, A, T, WIDE_JVP_PROBE>
  return {N, DIM, {PITA_WIDE64_FNS(PITA_K), wide64_lds_of<C>, 1, WAVES, C::NT},
          {PITA_WIDE64_FNS(PITA_KM), wide64_lds_of<C>, 1, WAVES, C::NT}, nullptr,
          {PITA_WIDE64_FNS(PITA_KP), wide64_lds_of<C>, 1, WAVES, C::NT}};
#undef PITA_K
#undef PITA_KM
#undef PITA_KP
}
static const Wide64Row<Wide64JvpParams> kWide64JvpRows[] = {wide64_jvp_row_of<22, 3, 4>(), wide64_jvp_row_of<33, 3, 4>(),
                                                            wide64_jvp_row_of<42, 3, 4>()};

const Wide64Row<Wide64JvpParams>* wide64_jvp_row(const pita_egnn_wide_config& cfg) { return wide64_find(kWide64JvpRows, cfg); }

int wide64_jvp(pita_egnn_wide* net, const WideJvpParams& v, int kind, int* bad, hipStream_t stream) {
  Wide64JvpParams p = wide64_params<Wide64JvpParams>(net, v.base.B);
  p.x = v.base.x; p.h = v.base.t; p.beta = v.base.beta; p.out = v.base.out;
  p.vx = v.vx; p.vh = v.vh; p.dir = v.dir; p.dout = v.dout; p.dot_out = v.dot_out; p.dot_stride = v.dot_stride;
  p.dot_off = v.dot_off; p.diag_acc = v.diag_acc; p.bad = bad;
  p.n_probes = v.n_probes; p.probes = v.probes; p.seed = v.seed; p.walker_offset = v.walker_offset; p.step = v.step;
  const Wide64Kernel<Wide64JvpParams>& k =
      kind == WIDE_JVP_UNIT ? net->jvp64->alt : kind == WIDE_JVP_PROBE ? net->jvp64->probes : net->jvp64->k;
  const long long items =
      kind == WIDE_JVP_UNIT ? p.B * net->cfg.n_particles * net->cfg.n_dim : kind == WIDE_JVP_PROBE ? p.B * v.n_probes : p.B;
  return wide64_launch(net, k, wide64_grid(net, k, items), p, stream);
}

}  // namespace pita
