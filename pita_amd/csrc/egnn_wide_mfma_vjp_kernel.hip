// Reverse-mode sweep of the EDM denoiser around the wide EGNN backbone on the MATRIX pipe of gfx950 (MI355X).
//
// Same results as egnn_wide_vjp_kernel (egnn_wide_kernel.hip) for EGNN_dynamics_AD2_cat / egnn_aldp.EGNN_dynamics:
//   vjp = J_x D(h, x)^T cot  (cot null: x -- grad_x E_theta, energy_net.py:51-62),  out = D (optional),
//   dot_h = <cot, dD/dh> (optional; the h-derivative term of dE_theta/dt, sdes.py:218)
// from ONE sweep per walker.
//
// Mapping: egnn_wide64_jvp_kernel's (one walker per item; lane = (column = atom, half of the 64 hidden features); a
// 64 x 64 dense layer is 2 x 2 blocks of a 32x32x16 MFMA tile; edges j = (i + dd) mod N, all columns of a trip at once;
// NT = 1 wave per item up to 32 atoms, NT = 2 above, one per 32-column tile, sharing the item's LDS tables).
// Structure: egnn_vjp_kernel.hip's.  The forward sweep (f16 two-piece fragments, as the forward-mode kernel's primal)
// checkpoints, per layer, the entering features and positions and the node model's pre-activation in a global scratch
// sized by resident item slots.  The backward sweep runs the layers in reverse: every edge is recomputed with its SiLU
// derivatives; a node's own sums over its edges (S = sum of the pre-activation adjoints, the position adjoints) stay in
// registers; what an edge sends to its partner j (the W_b path, position and edge-attribute adjoints) is added into the
// item's LDS tables; W_a^T and W_b^T are applied once per node to the summed adjoints.
//
// Adjoint GEMMs take route (a) of the two the design weighed: the EXACT bf16 x 3 split (WFrag<1>) on fragments of the
// unscaled transposes, packed by wide64_prepare.  Adjoints have no fixed range -- a fresh coordinate head makes the
// feature adjoints ~1e-4 of the position adjoints, a trained one need not -- and bf16 pieces keep the fp32 exponent, so
// there is no per-walker scale to choose and no adjoint range to police; only the primal (f16) can leave its range.
// Registers: W2 and W_c1 (f16, 128 registers) stay resident in AGPRs as in the forward-mode kernel; their bf16 x 3
// transposes (192 registers) would not fit beside them, so the block stages W2^T and W_c1^T of the current layer in LDS
// (48 KB, shared by its waves) and the per-node transposes stream from memory like the per-node forward matrices.
//
// Determinism: no floating-point atomics.  For a fixed dd the map i -> j is a permutation of the item's columns, so the
// scatter of one trip is conflict-free over all of the item's waves; an item fence closes every trip, so row j receives
// its contributions in dd order whatever the batch, the walker's place in it or the run.
// A walker whose primal or recompute leaves the f16 range comes out non-finite: it is marked, nothing is written for
// it, and pita_egnn_wide_vjp recomputes exactly the marked walkers with the vector-pipe kernel.
#include "egnn_wide_mfma_common.h"

namespace pita {

struct Wide64VjpParams {
  const unsigned* m16h;   // forward fragments (f16 two-piece), as the other matrix-pipe kernels
  const unsigned* m16t;   // [L][7][2 x 2 blocks] bf16 x 3 fragments of the unscaled transposes
  const float* vecs;
  const float* vecst;     // [L][w_r 64 | w_e 64] unscaled, fragment order
  const float* est;
  int L, has_beta;
  float coord_scale;
  long long B;
  const float* x;
  const float* h;
  const float* beta;
  const float* cot;  // nullable [B, N*DIM] (null: x)
  float* out;        // nullable: D
  float* vjp;        // [B, N*DIM]
  float* dot_h;      // nullable [B]
  float* dot_parts;  // nullable [B, 2] (needs dot_h), see WideVjpParams
  float* ws;         // checkpoints, one region per resident item slot
  int* mark;         // [B] zeroed by the launch wrapper: 1 = left to the vector-pipe kernel
  int* flag;         // one word, zeroed by the launch wrapper: 1 = some walker is marked
};

template <int N, int DIM, int WAVES>
struct Wide64VjpCfg {
  static constexpr int NCOLP = 32 * ((N + 31) / 32);
  static constexpr int NT = NCOLP / 32;
  static constexpr int PB_F = NCOLP * W64_PBS;
  static constexpr int POS_F = NCOLP * DIM;
  static constexpr int IPB = WAVES / NT;
  // per item: partner table, its adjoint table, pos[2], pos0, adjoints of the positions leaving / entering the layer and
  // of the input geometry, reduction scratch [NCOLP][4]
  static constexpr int ITEM_F = 2 * PB_F + 6 * POS_F + 4 * NCOLP;
  static constexpr int WT_W = 2 * W64T_MAT_W;  // W2^T, W_c1^T of the current layer
  static constexpr int CK_Q = 16;              // checkpointed f32x4 per lane and layer: features 8, node pre-activation 8
  static constexpr int PARK_Q = 16;            // parked across the backward edge loop: the node's hb and aggb, 8 each
  static __host__ __device__ constexpr int vec_f(int L) {
    return ((W64_HEAD_F + L * (W64_LAYER_F + W64T_VEC_F)) + 3) & ~3;
  }
  static __host__ __device__ constexpr size_t lds_bytes(int L) {
    return sizeof(float) * (size_t)(vec_f(L) + N * 64 + WT_W + IPB * ITEM_F);
  }
  static __host__ __device__ constexpr size_t ck_item_f(int L) {  // floats of checkpoint scratch per resident item
    return (size_t)L * ((size_t)CK_Q * NT * 64 * 4 + (size_t)NCOLP * 4) + (size_t)PARK_Q * NT * 64 * 4;
  }
};

// acc += W^T in with the four bf16 x 3 blocks of the transposed matrix read one at a time from `mat` (LDS or memory)
__device__ __forceinline__ void w64t_mul(const unsigned* __restrict__ mat, int lane, const f32x16 (&in)[2],
                                         f32x16 (&acc)[2]) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {  // one input block's pieces at a time: 24 registers of operand pieces, not 48
    u32x4 xs[3][2];
    WFrag<1>::split(in[kb], xs);
#pragma unroll
    for (int ob = 0; ob < 2; ++ob) {
      WFrag<1> w;
      w.load(nullptr, mat, ob * 2 + kb, lane);
      acc[ob] = w.mul_split(xs, acc[ob]);
    }
  }
}

template <int N, int DIM, int WAVES, bool ATT, bool TANH>
__global__ void __launch_bounds__(WAVES * 64, 1) egnn_wide64_vjp_kernel(Wide64VjpParams p) {
  using C = Wide64VjpCfg<N, DIM, WAVES>;
  static_assert(C::NT * C::IPB == WAVES && C::NT <= 2, "NT waves per item, one per column tile");
  constexpr int NT = C::NT;
  static_assert(F16_SX == 1.0f, "the gate / head vectors are read back as w / kS");
  constexpr float kS = SILU_PRESCALE;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int L = p.L;
  const int nvec = W64_HEAD_F + L * W64_LAYER_F;
  for (int i = threadIdx.x; i < nvec; i += WAVES * 64) lds[i] = p.vecs[i];
  for (int i = threadIdx.x; i < L * W64T_VEC_F; i += WAVES * 64) lds[nvec + i] = p.vecst[i];
  float* est = lds + C::vec_f(L);
  for (int i = threadIdx.x; i < N * 64; i += WAVES * 64) est[i] = p.est[i];
  unsigned* wt = reinterpret_cast<unsigned*>(est + N * 64);
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, cl = lane & 31, hh = lane >> 5;
  const int slot = wave / NT, tile = wave % NT;
  float* PB = est + N * 64 + C::WT_W + slot * C::ITEM_F;
  float* TB = PB + C::PB_F;          // adjoint of PB, summed over the edges that read row j
  float* posbuf0 = TB + C::PB_F;
  float* posbuf1 = posbuf0 + C::POS_F;
  float* pos0 = posbuf1 + C::POS_F;
  float* pb = pos0 + C::POS_F;       // adjoint of the positions leaving the layer
  float* pbn = pb + C::POS_F;        // adjoint of the positions entering it (being summed)
  float* p0b = pbn + C::POS_F;       // adjoint of the input geometry (edge attribute of every layer, and -u)
  float* red = p0b + C::POS_F;       // [NCOLP][4] reductions over the walker
  const f32x16 zero16 = {0};
  const int col = tile * 32 + cl, nodei = col < N ? col : 0;
  const bool valid = col < N;
  const int live = valid ? 1 : 0;
  const bool want_h = p.dot_h != nullptr;
  const bool want_p = p.dot_parts != nullptr;  // wave-uniform: without it the h-sum is accumulated exactly as ever

  // this item slot's checkpoints: [L][CK_Q][NT * 64 lanes] f32x4, then [L][NCOLP][4] positions, then the parked values
  // (addressed as checkpoint layer L: [PARK_Q][NT * 64 lanes] f32x4 behind the positions)
  float* ws = p.ws + (size_t)((size_t)blockIdx.x * C::IPB + slot) * C::ck_item_f(L);
  f32x4* ck4 = reinterpret_cast<f32x4*>(ws);
  const int lit = tile * 64 + lane;
  float* ckpos = ws + (size_t)L * C::CK_Q * NT * 64 * 4;
  f32x4* park4 = reinterpret_cast<f32x4*>(ckpos + (size_t)L * C::NCOLP * 4);
  auto park_put = [&](int q0, const f32x16 (&v)[2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        park4[(size_t)(q0 + b * 4 + q) * (NT * 64) + lit] = f32x4{v[b][4 * q], v[b][4 * q + 1], v[b][4 * q + 2], v[b][4 * q + 3]};
  };
  auto park_get = [&](int q0, int b) {
    f32x16 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 t = park4[(size_t)(q0 + b * 4 + q) * (NT * 64) + lit];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    return v;
  };
  auto ck_put = [&](int l, int q0, const f32x16 (&v)[2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        ck4[(size_t)(l * C::CK_Q + q0 + b * 4 + q) * (NT * 64) + lit] =
            f32x4{v[b][4 * q], v[b][4 * q + 1], v[b][4 * q + 2], v[b][4 * q + 3]};
  };
  auto ck_get = [&](int l, int q0, f32x16 (&v)[2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 t = ck4[(size_t)(l * C::CK_Q + q0 + b * 4 + q) * (NT * 64) + lit];
        v[b][4 * q] = t.x; v[b][4 * q + 1] = t.y; v[b][4 * q + 2] = t.z; v[b][4 * q + 3] = t.w;
      }
  };

  // block-uniform trip count (the body holds block barriers): a slot past the last walker computes that walker again in
  // its own tables and writes nothing
  for (long long base = (long long)blockIdx.x * C::IPB; base < p.B; base += (long long)gridDim.x * C::IPB) {
    const bool active = base + slot < p.B;
    const long long w = active ? base + slot : p.B - 1;
    const float hv = p.h[w];
    const float bet = p.has_beta ? p.beta[w] : 0.f;
    // score_net.py:26-29 and their h-derivatives
    const float c_s = 1.0f / (1.0f + hv), c_in = 1.0f / sqrtf(1.0f + hv), sh = sqrtf(hv);
    const float c_out = sh * c_in, tfeat = 0.125f * logf(hv);
    const float dc_s = -c_s * c_s, dc_in = -0.5f * c_in * c_s, dc_out = 0.5f * c_in / sh + sh * dc_in;
    float xin[DIM], ct[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const long long e = (w * N + col) * DIM + k;
      xin[k] = valid ? p.x[e] : 0.f;
      ct[k] = valid ? (p.cot ? p.cot[e] : xin[k]) : 0.f;
      const float ps = c_in * xin[k];
      if (hh == 0) { pos0[col * DIM + k] = ps; posbuf0[col * DIM + k] = ps; }
    }
    f32x16 hfeat[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const f32x16 wtm = lds_vec16(lds + b * 32 + hh * 16), wbt = lds_vec16(lds + 64 + b * 32 + hh * 16);
      const f32x16 es = lds_vec16(est + nodei * 64 + b * 32 + hh * 16);
#pragma unroll
      for (int r = 0; r < 16; ++r) hfeat[b][r] = fmaf(wtm[r], tfeat, fmaf(wbt[r], bet, es[r]));
    }
    item_fence<NT>();

    // ------------------------------------------------------------------ forward sweep, checkpoints
    float* poscur = posbuf0; float* posnext = posbuf1;
    for (int l = 0; l < L; ++l) {
      const unsigned* ml = p.m16h + (size_t)l * WM_COUNT * W64_MAT_W;
      const float* vbase = lds + W64_HEAD_F + l * W64_LAYER_F;
      const float* vl = vbase + hh * 16;
      const bool last = (l == L - 1);
      const float aggw = last ? 0.0f : 1.0f;
      ck_put(l, 0, hfeat);
      {
        f32x16 pbv[2] = {zero16, zero16};
        w64_mul_stream(ml, WM_WB, lane, hfeat, pbv);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          pbv[b] *= F16_UNSCALE;
          lds_store16(PB + col * W64_PBS + b * 32 + hh * 16, pbv[b]);
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

      f32x16 Ai[2] = {lds_vec16(vl + WV_B1 * 64), lds_vec16(vl + WV_B1 * 64 + 32)};
      w64_mul_stream(ml, WM_WA, lane, hfeat, Ai);
      Ai[0] *= F16_UNSCALE; Ai[1] *= F16_UNSCALE;
      f32x16 agg[2] = {zero16, zero16};
      float xacc[DIM], pown[DIM], p0own[DIM];
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        xacc[k] = 0.f;
        pown[k] = poscur[col * DIM + k]; p0own[k] = pos0[col * DIM + k];
        if (hh == 0) ckpos[((size_t)l * C::NCOLP + col) * 4 + k] = pown[k];
      }
      for (int dd = 1; dd < N; ++dd) {
        asm volatile("" ::: "memory");
        int j = nodei + dd * live;
        j = (j >= N) ? j - N : j;
        const int cj = valid ? j : col;
        float df[DIM], radial = 0.f, ea = 0.f;
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
          df[k] = pown[k] - poscur[cj * DIM + k];
          radial = fmaf(df[k], df[k], radial);
          const float e0 = p0own[k] - pos0[cj * DIM + k];
          ea = fmaf(e0, e0, ea);
        }
        const float geo = hh ? ea : radial;
        f32x16 m[2];
        m[0] = Ai[0] + lds_vec16(PB + cj * W64_PBS + hh * 16);
        m[1] = Ai[1] + lds_vec16(PB + cj * W64_PBS + 32 + hh * 16);
        m[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re0, geo, m[0], 0, 0, 0);
        m[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re1, geo, m[1], 0, 0, 0);
        silu16_out(m[0]);
        silu16_out(m[1]);
        f32x16 z[2] = {lds_vec16(vl + WV_B2 * 64), lds_vec16(vl + WV_B2 * 64 + 32)};
        w2f.mul(m, z);
        silu16_acc(z[0]);
        silu16_acc(z[1]);
        if (ATT) {
          const f32x16 wa0 = lds_vec16(vl + WV_WATT * 64), wa1 = lds_vec16(vl + WV_WATT * 64 + 32);
          const float att = fast_sigmoid(xhalf_sum(dot16(wa0, z[0]) + dot16(wa1, z[1])) + b_att);
          z[0] *= att; z[1] *= att;
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) agg[b][r] = fmaf(z[b][r], aggw, agg[b][r]);
        f32x16 c1[2] = {lds_vec16(vl + WV_BC1 * 64), lds_vec16(vl + WV_BC1 * 64 + 32)};
        wc1f.mul(z, c1);
        silu16_acc(c1[0]);
        silu16_acc(c1[1]);
        const f32x16 wc0 = lds_vec16(vl + WV_WC2 * 64), wc1v = lds_vec16(vl + WV_WC2 * 64 + 32);
        float cs = xhalf_sum(dot16(wc0, c1[0]) + dot16(wc1v, c1[1]));
        if (TANH) cs = tanh_select(cs) * p.coord_scale;
        const float inrm = __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(radial + 1e-8f) + 1.0f);
#pragma unroll
        for (int k = 0; k < DIM; ++k) xacc[k] = fmaf(df[k] * inrm, cs, xacc[k]);
      }
#pragma unroll
      for (int k = 0; k < DIM; ++k)
        if (hh == 0) posnext[col * DIM + k] = pown[k] + xacc[k];
      if (!last) {  // node model; its pre-activation (the accumulator: F16_SX F16_SW kS zn) is checkpointed
        f32x16 n1[2] = {lds_vec16(vl + WV_BN1 * 64), lds_vec16(vl + WV_BN1 * 64 + 32)};
        w64_mul_stream(ml, WM_WN1A, lane, hfeat, n1);
        w64_mul_stream(ml, WM_WN1B, lane, agg, n1);
        ck_put(l, 8, n1);
        silu16_acc(n1[0]);
        silu16_acc(n1[1]);
        f32x16 o[2] = {lds_vec16(vl + WV_BN2 * 64), lds_vec16(vl + WV_BN2 * 64 + 32)};
        w64_mul_stream(ml, WM_WN2, lane, n1, o);
        hfeat[0] += o[0] * F16_UNSCALE; hfeat[1] += o[1] * F16_UNSCALE;
      }
      item_fence<NT>();
      float* tmp = poscur; poscur = posnext; posnext = tmp;
    }

    // ---- F = (pos^L - pos0) - mean, D = c_s x + c_out F; adjoint of u = pos^L - pos0: c_out (cot - mean_i cot)
    float F[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      F[k] = poscur[col * DIM + k] - pos0[col * DIM + k];
      if (hh == 0) { red[col * 4 + k] = F[k]; pbn[col * DIM + k] = ct[k]; }
    }
    item_fence<NT>();
    // hpart: this column's share of <cot, dD/dh>; with dot_parts, of <cot, d(c_out F)/dh> alone, and the shares of
    // c_out <cot, F> and c_s'(h) <cot, x> (fpart, xpart) wait in the free slots 2 and 3 of `red` for the final reduction
    float Dv[DIM], u[DIM], hpart = 0.f, fpart = 0.f, xpart = 0.f;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      float s = 0.f, sc = 0.f;
      for (int q = 0; q < N; ++q) { s += red[q * 4 + k]; sc += pbn[q * DIM + k]; }
      F[k] -= s / (float)N;
      Dv[k] = fmaf(c_s, xin[k], c_out * F[k]);
      if (want_p) {
        hpart = fmaf(ct[k], dc_out * F[k], hpart);
        fpart = fmaf(ct[k], c_out * F[k], fpart);
        xpart = fmaf(ct[k], dc_s * xin[k], xpart);
      } else {
        hpart = fmaf(ct[k], fmaf(dc_s, xin[k], dc_out * F[k]), hpart);
      }
      u[k] = valid ? c_out * (ct[k] - sc / (float)N) : 0.f;
    }
    item_fence<NT>();
#pragma unroll
    for (int k = 0; k < DIM; ++k)
      if (hh == 0) { pb[col * DIM + k] = u[k]; p0b[col * DIM + k] = -u[k]; }
    if (want_p && hh == 0) { red[col * 4 + 2] = valid ? fpart : 0.f; red[col * 4 + 3] = valid ? xpart : 0.f; }
    f32x16 hb[2] = {zero16, zero16};  // adjoint of the node's features leaving the layer (then: entering it)
    item_fence<NT>();

    // ------------------------------------------------------------------ backward sweep
    float* posl = posbuf0;  // positions entering the layer, from the checkpoint
    for (int l = L - 1; l >= 0; --l) {
      const unsigned* ml = p.m16h + (size_t)l * WM_COUNT * W64_MAT_W;
      const unsigned* mt = p.m16t + (size_t)l * WM_COUNT * W64T_MAT_W;
      const float* vbase = lds + W64_HEAD_F + l * W64_LAYER_F;
      const float* vl = vbase + hh * 16;
      const float* vt = lds + nvec + l * W64T_VEC_F + hh * 16;
      const bool last = (l == L - 1);
      const bool need_h = (l > 0) || want_h;  // h^0 does not depend on x (but on h, through the time feature)
      __syncthreads();  // every wave of the block is done with the previous layer's staged transposes
      {
        const u32x4* s2 = reinterpret_cast<const u32x4*>(mt + (size_t)WM_W2 * W64T_MAT_W);
        const u32x4* sc = reinterpret_cast<const u32x4*>(mt + (size_t)WM_WC1 * W64T_MAT_W);
        u32x4* d = reinterpret_cast<u32x4*>(wt);
        for (int i = threadIdx.x; i < W64T_MAT_W / 4; i += WAVES * 64) {
          d[i] = s2[i];
          d[W64T_MAT_W / 4 + i] = sc[i];
        }
      }
      ck_get(l, 0, hfeat);
#pragma unroll
      for (int k = 0; k < DIM; ++k)
        if (hh == 0) {
          posl[col * DIM + k] = ckpos[((size_t)l * C::NCOLP + col) * 4 + k];
          pbn[col * DIM + k] = 0.f;
        }
      {
        f32x16 pbv[2] = {zero16, zero16};
        w64_mul_stream(ml, WM_WB, lane, hfeat, pbv);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          pbv[b] *= F16_UNSCALE;
          lds_store16(PB + col * W64_PBS + b * 32 + hh * 16, pbv[b]);
          lds_store16(TB + col * W64_PBS + b * 32 + hh * 16, zero16);
        }
      }
      __syncthreads();  // staged transposes and the item's tables are published

      W64Mat w2f, wc1f;
      w2f.load(ml, WM_W2, lane);
      wc1f.load(ml, WM_WC1, lane);
      w2f.to_agpr();
      wc1f.to_agpr();
      const float a_re0 = vbase[WV_WRE * 64 + lane], a_re1 = vbase[WV_WRE * 64 + 64 + lane];
      const float b_att = vbase[WV_COUNT * 64];

      f32x16 Ai[2] = {lds_vec16(vl + WV_B1 * 64), lds_vec16(vl + WV_B1 * 64 + 32)};
      w64_mul_stream(ml, WM_WA, lane, hfeat, Ai);
      Ai[0] *= F16_UNSCALE; Ai[1] *= F16_UNSCALE;

      // node model backward: h' = h + Wn2 silu(zn) + bn2, zn = Wn1a h + Wn1b agg + bn1
      f32x16 aggb[2] = {zero16, zero16};
      if (!last) {
        f32x16 zn[2], gz[2], t1[2] = {zero16, zero16};
        ck_get(l, 8, zn);
        silu16_d<true>(zn[0], gz[0]);
        silu16_d<true>(zn[1], gz[1]);
        w64t_mul(mt + (size_t)WM_WN2 * W64T_MAT_W, lane, hb, t1);
        t1[0] *= gz[0]; t1[1] *= gz[1];
        w64t_mul(mt + (size_t)WM_WN1B * W64T_MAT_W, lane, t1, aggb);
        if (need_h) w64t_mul(mt + (size_t)WM_WN1A * W64T_MAT_W, lane, t1, hb);
      }
      // hb and aggb are parked in this lane's own words of the scratch across the edge loop (aggb is read back once per
      // trip): with them resident the loop's live set is past the register file
      park_put(0, hb);
      park_put(8, aggb);
      float X[DIM], pown[DIM], p0own[DIM], pacc[DIM], p0acc[DIM];
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        X[k] = pb[col * DIM + k];
        pown[k] = posl[col * DIM + k]; p0own[k] = pos0[col * DIM + k];
        pacc[k] = 0.f; p0acc[k] = 0.f;
      }
      f32x16 S[2] = {zero16, zero16};
      for (int dd = 1; dd < N; ++dd) {
        asm volatile("" ::: "memory");
        int j = nodei + dd * live;
        j = (j >= N) ? j - N : j;
        const int cj = valid ? j : col;
        float df[DIM], e0[DIM], radial = 0.f, ea = 0.f, t = 0.f;
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
          df[k] = pown[k] - posl[cj * DIM + k];
          radial = fmaf(df[k], df[k], radial);
          e0[k] = p0own[k] - pos0[cj * DIM + k];
          ea = fmaf(e0[k], e0[k], ea);
          t = fmaf(df[k], X[k], t);
        }
        // the edge again, with derivative factors
        const float geo = hh ? ea : radial;
        f32x16 m[2], g1[2], g2[2], gc[2];
        m[0] = Ai[0] + lds_vec16(PB + cj * W64_PBS + hh * 16);
        m[1] = Ai[1] + lds_vec16(PB + cj * W64_PBS + 32 + hh * 16);
        m[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re0, geo, m[0], 0, 0, 0);
        m[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re1, geo, m[1], 0, 0, 0);
        silu16_d<false>(m[0], g1[0]);
        silu16_d<false>(m[1], g1[1]);
        f32x16 z[2] = {lds_vec16(vl + WV_B2 * 64), lds_vec16(vl + WV_B2 * 64 + 32)};  // -> kS m2 (before the gate)
        w2f.mul(m, z);
        silu16_d<true>(z[0], g2[0]);
        silu16_d<true>(z[1], g2[1]);
        float att = 1.0f;
        f32x16 zg[2] = {z[0], z[1]};  // -> kS m (gated message)
        if (ATT) {
          const f32x16 wa0 = lds_vec16(vl + WV_WATT * 64), wa1 = lds_vec16(vl + WV_WATT * 64 + 32);
          att = fast_sigmoid(xhalf_sum(dot16(wa0, z[0]) + dot16(wa1, z[1])) + b_att);
          zg[0] *= att; zg[1] *= att;
        }
        f32x16 c1[2] = {lds_vec16(vl + WV_BC1 * 64), lds_vec16(vl + WV_BC1 * 64 + 32)};
        wc1f.mul(zg, c1);
        silu16_d<true>(c1[0], gc[0]);
        silu16_d<true>(c1[1], gc[1]);
        const f32x16 wc0 = lds_vec16(vl + WV_WC2 * 64), wc1v = lds_vec16(vl + WV_WC2 * 64 + 32);  // w_c2 / kS
        float cs = xhalf_sum(dot16(wc0, c1[0]) + dot16(wc1v, c1[1])), dcs = 1.0f;
        if (TANH) {
          const float th = tanh_select(cs);
          dcs = p.coord_scale * fmaf(-th, th, 1.0f);
          cs = th * p.coord_scale;
        }
        const float sq = __builtin_amdgcn_sqrtf(radial + 1e-8f);
        const float inv = __builtin_amdgcn_rcpf(sq + 1.0f);
        // backward: pos'_i += df inv cs
        const float csb = (inv * t) * dcs, invb = cs * t;
        const float csk = csb * kS;  // w_c2 = kS x the packed vector
        f32x16 zcb[2];
        zcb[0] = gc[0] * wc0 * csk;
        zcb[1] = gc[1] * wc1v * csk;
        f32x16 mb[2] = {park_get(8, 0), park_get(8, 1)};  // aggb: adjoint of the gated message
        w64t_mul(wt + W64T_MAT_W, lane, zcb, mb);
        if (ATT) {
          const f32x16 wa0 = lds_vec16(vl + WV_WATT * 64), wa1 = lds_vec16(vl + WV_WATT * 64 + 32);  // w_att / kS
          // <mb, m2> with m2 = z / kS, times the packed gate vector's kS: the two factors cancel
          const float sb = (att * (1.0f - att)) * xhalf_sum(dot16(mb[0], z[0]) + dot16(mb[1], z[1]));
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) mb[b][r] = fmaf(mb[b][r], att, (b ? wa1[r] : wa0[r]) * sb);
        }
        mb[0] *= g2[0]; mb[1] *= g2[1];
        f32x16 z1b[2] = {zero16, zero16};
        w64t_mul(wt, lane, mb, z1b);
        z1b[0] *= g1[0]; z1b[1] *= g1[1];
        if (need_h) {
          S[0] += z1b[0]; S[1] += z1b[1];
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            float* row = TB + cj * W64_PBS + b * 32 + hh * 16;
            lds_store16(row, lds_vec16(row) + z1b[b]);
          }
        }
        const f32x16 wr0 = lds_vec16(vt), wr1 = lds_vec16(vt + 32), we0 = lds_vec16(vt + 64), we1 = lds_vec16(vt + 96);
        const float radb = fmaf(invb, -(inv * inv) * (0.5f * __builtin_amdgcn_rcpf(sq)),
                                xhalf_sum(dot16(wr0, z1b[0]) + dot16(wr1, z1b[1])));
        const float eab = xhalf_sum(dot16(we0, z1b[0]) + dot16(we1, z1b[1]));
        const float ic = inv * cs;
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
          const float dfb = fmaf(ic, X[k], 2.0f * radb * df[k]);
          const float e0b = 2.0f * eab * e0[k];
          pacc[k] += dfb;
          p0acc[k] += e0b;
          if (hh == 0) {
            pbn[cj * DIM + k] -= dfb;
            p0b[cj * DIM + k] -= e0b;
          }
        }
        item_fence<NT>();  // closes the trip: the next one adds into other rows of the same tables
      }
      hb[0] = park_get(0, 0); hb[1] = park_get(0, 1);
      if (need_h) w64t_mul(mt + (size_t)WM_WA * W64T_MAT_W, lane, S, hb);
#pragma unroll
      for (int k = 0; k < DIM; ++k)
        if (hh == 0) {
          pbn[col * DIM + k] += X[k] + pacc[k];
          p0b[col * DIM + k] += p0acc[k];
        }
      if (need_h) {
        const f32x16 tb[2] = {lds_vec16(TB + col * W64_PBS + hh * 16), lds_vec16(TB + col * W64_PBS + 32 + hh * 16)};
        w64t_mul(mt + (size_t)WM_WB * W64T_MAT_W, lane, tb, hb);
      }
      item_fence<NT>();
#pragma unroll
      for (int k = 0; k < DIM; ++k)
        if (hh == 0) pb[col * DIM + k] = pbn[col * DIM + k];
      item_fence<NT>();
    }

    // ---- pos^0 = pos0 = c_in x
    float vj[DIM];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const float yb = pb[col * DIM + k] + p0b[col * DIM + k];
      vj[k] = fmaf(c_s, ct[k], c_in * yb);
      hpart = fmaf(dc_in * yb, xin[k], hpart);
      ok = ok && __builtin_isfinite(Dv[k]) && __builtin_isfinite(vj[k]);
    }
    if (want_h) {  // through the time feature ln(h)/8 of every node's embedding
      const f32x16 et0 = lds_vec16(lds + hh * 16), et1 = lds_vec16(lds + 32 + hh * 16);
      hpart = fmaf(xhalf_sum(dot16(hb[0], et0) + dot16(hb[1], et1)), 0.125f / hv, hpart);
      ok = ok && __builtin_isfinite(hpart);
      if (want_p) ok = ok && __builtin_isfinite(red[col * 4 + 2]) && __builtin_isfinite(red[col * 4 + 3]);
    }
    if (hh == 0) { red[col * 4] = valid ? hpart : 0.f; red[col * 4 + 1] = (valid && !ok) ? 1.0f : 0.0f; }
    item_fence<NT>();
    float dot = 0.f, nbad = 0.f, dot_f = 0.f, dot_x = 0.f;
    for (int q = 0; q < N; ++q) { dot += red[q * 4]; nbad += red[q * 4 + 1]; }
    if (want_p)
      for (int q = 0; q < N; ++q) { dot_f += red[q * 4 + 2]; dot_x += red[q * 4 + 3]; }
    if (!active) {  // a slot past the last walker: its recomputed copy writes nothing
    } else if (nbad != 0.f) {  // uniform over the item's waves: all read the same flags
      if (lane == 0 && tile == 0) { p.mark[w] = 1; *p.flag = 1; }
    } else if (valid && hh == 0) {
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        const long long e = (w * N + col) * DIM + k;
        if (p.out) p.out[e] = Dv[k];
        p.vjp[e] = vj[k];
      }
      if (want_h && col == 0) {
        p.dot_h[w] = want_p ? dot + dot_x : dot;
        if (want_p) { p.dot_parts[2 * w] = dot_f; p.dot_parts[2 * w + 1] = dot; }
      }
    }
    item_fence<NT>();
  }
}

// alanine dipeptide (22 atoms: one wave per item), tri-alanine (33) and ACE-(ALA)3-NME (42: two waves per item: 4 or 2
// resident items per block); other particle counts take the vector-pipe kernel
template <int N, int DIM, int WAVES>
static size_t wide64_vjp_ck_of(int L) { return Wide64VjpCfg<N, DIM, WAVES>::ck_item_f(L); }
template <int N, int DIM, int WAVES>
static Wide64Row<Wide64VjpParams> wide64_vjp_row_of() {
  using C = Wide64VjpCfg<N, DIM, WAVES>;
#define PITA_K(A, T) egnn_wide64_vjp_kernel<N, DIM, WAVES, A, T>
  return {N, DIM, {PITA_WIDE64_FNS(PITA_K), wide64_lds_of<C>, 1, WAVES, C::NT}, {}, wide64_vjp_ck_of<N, DIM, WAVES>};
#undef PITA_K
}
static const Wide64Row<Wide64VjpParams> kWide64VjpRows[] = {wide64_vjp_row_of<22, 3, 4>(), wide64_vjp_row_of<33, 3, 4>(),
                                                            wide64_vjp_row_of<42, 3, 4>()};

const Wide64Row<Wide64VjpParams>* wide64_vjp_row(const pita_egnn_wide_config& cfg) { return wide64_find(kWide64VjpRows, cfg); }

int wide64_vjp(pita_egnn_wide* net, const WideVjpParams& v, int* mark, int* flag, hipStream_t stream) {
  const Wide64Row<Wide64VjpParams>& r = *net->vjp64;
  Wide64VjpParams p = wide64_params<Wide64VjpParams>(net, v.base.B);
  const unsigned grid = wide64_grid(net, r.k, p.B);
  PITA_HIP_CHECK(net->vjp_ck.grow(sizeof(float) * (size_t)grid * (r.k.waves / r.k.item_waves) * r.ck_item_f(p.L), stream));
  p.m16t = net->m16t.as<unsigned>(); p.vecst = net->vecs64t.as<float>();
  p.x = v.base.x; p.h = v.base.t; p.beta = v.base.beta; p.cot = v.cot; p.out = v.base.out; p.vjp = v.vjp; p.dot_h = v.dot_h;
  p.dot_parts = v.dot_parts;
  p.ws = net->vjp_ck.as<float>(); p.mark = mark; p.flag = flag;
  return wide64_launch(net, r.k, grid, p, stream);
}

}  // namespace pita
