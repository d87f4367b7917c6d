// Shared pieces of the matrix-pipe kernels of the wide EGNN backbone (egnn_wide_mfma_kernel.hip: forward / sampler;
// egnn_wide_mfma_jvp_kernel.hip: forward-mode derivative; egnn_wide_mfma_vjp_kernel.hip: reverse-mode sweep): LDS / fragment
// layout constants, the parameter block, the 64 x 64 dense layer as 2 x 2 blocks of the f16 two-piece MFMA tile, the item
// fence and the SiLU with its derivative of the two derivative kernels.
#pragma once
#include "egnn_common.h"
#include "egnn_wide_common.h"

namespace pita {

constexpr int W64_PBS = 68;  // LDS row stride (floats) of the partner table: 64 + 4, conflict-free ds_read_b128
enum { WM_WA = 0, WM_WB, WM_W2, WM_WC1, WM_WN1A, WM_WN1B, WM_WN2, WM_COUNT };
constexpr int W64_MAT_W = 4 * MAT_WH;  // words per 64 x 64 matrix: blocks [out block][in block], each a WFrag<2> fragment
// per-layer vectors, 64 floats each in fragment order [block][hh][r] unless noted
enum { WV_WRE = 0 /* 128 floats: [block][w_r 32 | w_e 32], natural order (A operand of the f32 k-step) */, WV_B1 = 2, WV_B2,
       WV_WATT, WV_BC1, WV_WC2, WV_BN1, WV_BN2, WV_COUNT };
// reverse-mode kernel: bf16 x 3 fragments (WFrag<1>) of the UNSCALED transposes, same [out block][in block] order, and per
// layer the unscaled w_r | w_e in fragment order
constexpr int W64T_MAT_W = 4 * MAT_W;
constexpr int W64T_VEC_F = 128;
constexpr int W64_HEAD_F = 128;                     // emb_t, emb_beta (fragment order)
constexpr int W64_LAYER_F = WV_COUNT * 64 + 4;      // + b_att

struct Wide64Params {
  const unsigned* m16h;
  const float* vecs;
  const float* est;
  int L, attention, tanh_on, has_beta;
  float coord_scale;
  long long B;
  int mode;  // 0 backbone forward (t = its time input), 1 denoiser, 2 score (t = h = sigma^2)
  const float* x;
  const float* t;
  const float* beta;
  float* out;
  // mode 3: n_steps Euler-Maruyama steps of the not-debiased reverse SDE in one launch (pita_egnn_wide_sampler_run)
  float* xs;               // [B, N*DIM] walkers, in place
  const float* step_tab;   // [n_steps][PITA_STEP_STRIDE]
  int n_steps;
  const float* noise;      // nullable [n_steps, B, N*DIM]
  unsigned long long seed, walker_offset;
  long long step0;
  int remove_mean;
  double* stats_out;       // nullable [n_steps][4]
  int* bad_from;           // [B*N]: first step whose moments this launch left out for the particle (INT_MAX: none)
  int* flag;               // nullable: set to 1 when a result of this launch is not finite (the repair pass has work)
};

template <int N, int DIM, int G, int WAVES>
struct Wide64Cfg {
  static constexpr int NCOL = G * N;
  static constexpr int NT = (NCOL + 31) / 32;
  static constexpr int NCOLP = NT * 32;
  static constexpr int PB_F = NCOLP * W64_PBS;
  static constexpr int POS_F = NCOLP * DIM;
  static constexpr int WAVE_F = PB_F + 4 * POS_F;  // partner table, pos[2], pos0, the walkers' unscaled coordinates
  static __host__ __device__ constexpr int vec_f(int L) { return ((W64_HEAD_F + L * W64_LAYER_F) + 3) & ~3; }
  static __host__ __device__ constexpr size_t lds_bytes(int L) {
    return sizeof(float) * (size_t)(vec_f(L) + N * 64 + WAVES * WAVE_F);
  }
};

// ---- host side, shared by the three files' tables (P: the kernel's parameter block)
// One kernel of a row, its four [attention][tanh] instantiations: an item is G walkers (forward kernel) or one walker /
// (walker, direction) pair on item_waves waves (derivative kernels); `waves` waves per block, one block per CU
template <class P>
struct Wide64Kernel {
  void (*fn[2][2])(P);
  size_t (*lds_bytes)(int);
  int G, waves, item_waves;
};
template <class P>
struct Wide64Row {
  int n, dim;
  Wide64Kernel<P> k;
  Wide64Kernel<P> alt;        // forward: the small-batch mapping (fn null: none); forward mode: (walker, direction) items
  size_t (*ck_item_f)(int);   // reverse mode: floats of checkpoint scratch per resident item
  Wide64Kernel<P> probes;     // forward mode: (walker, probe) items
};
template <class C>
static size_t wide64_lds_of(int L) { return C::lds_bytes(L); }
// K(ATT, TANH): a function-like macro that names one instantiation
#define PITA_WIDE64_FNS(K) {{K(false, false), K(false, true)}, {K(true, false), K(true, true)}}

// the row of the handle's particle system, when the LDS of its kernel holds the handle's depth
template <class P, size_t K>
static const Wide64Row<P>* wide64_find(const Wide64Row<P> (&rows)[K], const pita_egnn_wide_config& c) {
  for (const auto& r : rows)
    if (r.n == c.n_particles && r.dim == c.n_dim && r.k.lds_bytes(c.n_layers) <= kWideLdsBlock) return &r;
  return nullptr;
}
template <class P>
static unsigned wide64_grid(const pita_egnn_wide* net, const Wide64Kernel<P>& k, long long count) {
  const long long items = (count + k.G - 1) / k.G, per_block = k.waves / k.item_waves;
  const long long want = (items + per_block - 1) / per_block, cap = net->n_cu;
  return (unsigned)(want < cap ? want : cap);
}
template <class P>
static int wide64_launch(const pita_egnn_wide* net, const Wide64Kernel<P>& k, unsigned grid, const P& p, hipStream_t st) {
  const auto fn = k.fn[net->cfg.attention ? 1 : 0][net->cfg.tanh ? 1 : 0];
  const size_t lds = k.lds_bytes(net->cfg.n_layers);
  PITA_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void*>(fn), lds));
  hipLaunchKernelGGL(fn, dim3(grid), dim3(k.waves * 64), lds, st, p);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}
// the fields the three parameter blocks share
template <class P>
static P wide64_params(const pita_egnn_wide* net, long long B) {
  P p{};
  p.m16h = net->m16h.as<unsigned>(); p.vecs = net->vecs64.as<float>(); p.est = net->est64.as<float>();
  p.L = net->cfg.n_layers; p.has_beta = net->cfg.condition_beta;
  p.coord_scale = net->cfg.coords_range / (float)net->cfg.n_layers;
  p.B = B;
  return p;
}

#ifndef PITA_WIDE64_AGPR_WEIGHTS
#define PITA_WIDE64_AGPR_WEIGHTS 1
#endif
// the four 32 x 32 blocks of a 64 x 64 matrix, resident
struct W64Mat {
  WFrag<2> b[2][2];
  __device__ __forceinline__ void load(const unsigned* __restrict__ layer, int mat, int lane) {
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) b[ob][kb].load(nullptr, layer, mat * 4 + ob * 2 + kb, lane);
  }
  // park the fragments in accumulation registers: the MFMA reads its A operand from there directly, so the resident
  // matrices cost no VALU-visible registers (left to itself the allocator keeps them in VGPRs and spills around them)
  __device__ __forceinline__ void to_agpr() {
#if PITA_WIDE64_AGPR_WEIGHTS
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc)
#pragma unroll
          for (int st = 0; st < 2; ++st) asm volatile("" : "+a"(b[ob][kb].w[pc][st]));
#endif
  }
  __device__ __forceinline__ void mul(const f32x16 (&in)[2], f32x16 (&acc)[2]) const {
    u32x4 xs[2][2][2];
    WFrag<2>::split(in[0], xs[0]);
    WFrag<2>::split(in[1], xs[1]);
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) acc[ob] = b[ob][kb].mul_split(xs[kb], acc[ob]);
  }
};
// the same product with the blocks streamed from memory one at a time (per-node layers: used once per tile and layer)
__device__ __forceinline__ void w64_mul_stream(const unsigned* __restrict__ layer, int mat, int lane, const f32x16 (&in)[2],
                                               f32x16 (&acc)[2]) {
  u32x4 xs[2][2][2];
  WFrag<2>::split(in[0], xs[0]);
  WFrag<2>::split(in[1], xs[1]);
#pragma unroll
  for (int ob = 0; ob < 2; ++ob)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      WFrag<2> w;
      w.load(nullptr, layer, mat * 4 + ob * 2 + kb, lane);
      acc[ob] = w.mul_split(xs[kb], acc[ob]);
    }
}

__device__ __forceinline__ void lds_store16(float* dst, const f32x16& v) {
  f32x4* d = reinterpret_cast<f32x4*>(dst);
#pragma unroll
  for (int q = 0; q < 4; ++q) d[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
}

// orders an item's LDS tables between their writers and readers: the item is one wave's (NT == 1) or NT waves' of the
// block (a block barrier; every wave of the block reaches each one the same number of times)
template <int NT>
__device__ __forceinline__ void item_fence() {
  if constexpr (NT == 1) wave_lds_fence();
  else __syncthreads();
}

// SiLU of egnn_common.h's PREC 2 forms with the derivative: in v = kS z (UNSCALE: the accumulator 16 kS z), out
// y = kS silu(z) in place and g = d silu / dz = s + (y / kS)(1 - s) with s the sigmoid the primal computed anyway
template <bool UNSCALE>
__device__ __forceinline__ void silu16_d(f32x16& m, f32x16& g) {
  const f32x2 c = {1.0f / F16_SX, 1.0f / F16_SX};
  constexpr float kSi = 1.0f / SILU_PRESCALE;
  f32x2 v[8], e[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    v[q] = f32x2{m[2 * q], m[2 * q + 1]};
    if (UNSCALE) v[q] = v[q] * F16_UNSCALE;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    e[q].x = __builtin_amdgcn_exp2f(v[q].x);
    e[q].y = __builtin_amdgcn_exp2f(v[q].y);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) e[q] = __builtin_elementwise_fma(e[q], c, c);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    e[q].x = __builtin_amdgcn_rcpf(e[q].x);
    e[q].y = __builtin_amdgcn_rcpf(e[q].y);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x2 y = v[q] * e[q];
    const f32x2 one = {1.0f, 1.0f};
    const f32x2 gq = __builtin_elementwise_fma(y * kSi, one - e[q], e[q]);
    m[2 * q] = y.x; m[2 * q + 1] = y.y;
    g[2 * q] = gq.x; g[2 * q + 1] = gq.y;
  }
}

}  // namespace pita
