// Native handle behind pita_egnn_wide_t, shared by the two kernels that serve it: the vector-pipe kernel
// (egnn_wide_kernel.hip: any hidden_nf <= 64, any particle count <= 64) and the matrix-pipe kernel
// (egnn_wide_mfma_kernel.hip, with its forward- and reverse-mode siblings: the particle systems they are instantiated for).
#pragma once
#include <cstdlib>
#include <vector>

#include "common.h"

namespace pita {

// LDS budgets of the wide kernels (gfx950: 160 KB per CU)
constexpr size_t kWideLdsBlock = 160 * 1024;      // the most one block can have: a matrix-pipe row that needs more for the
                                                  // handle's depth does not serve it
constexpr size_t kWideLdsOneBlock = 150 * 1024;   // vector pipe, kernels that run one block per CU: what a block may take
constexpr size_t kWideLdsTwoBlocks = 72 * 1024;   // vector pipe, two blocks per CU inside the 160 KB: cap per block

// The reference's state_dict of EGNN_dynamics_AD2_cat, flattened in parameter order, as per-layer views (egnn.py: E_GCL).
// The ONE place that knows the order: pita_egnn_wide_num_weights and the packers of both pipes read it.
struct WideLayerW {
  const float *e0w, *e0b, *e2w, *e2b;  // edge_mlp: [H][2H + 2], [H], [H][H], [H]
  const float *n0w, *n0b, *n2w, *n2b;  // node_mlp: [H][2H], [H], [H][H], [H]
  const float *c0w, *c0b, *c2w;        // coord_mlp: [H][H], [H], [H] (no bias)
  const float *aw, *ab;                // att_mlp: [H], [1]; null without attention
};
struct WideWeights {
  int H, ns, nf;                    // hidden width, static node features, nf = ns + 1 (t) + condition_beta
  const float *emb_w, *emb_b;       // embedding: [H][nf], [H] (embedding_out is dead: h_final is discarded,
  std::vector<WideLayerW> layer;    // egnn_dynamics_ad2_cat.py:187)
  int64_t count;                    // floats in all
};
// w null: the count alone
inline WideWeights wide_weights(const pita_egnn_wide_config& c, const float* w) {
  WideWeights W{};
  const int64_t H = W.H = c.hidden_nf;
  W.ns = c.n_static;
  const int64_t nf = W.nf = c.n_static + 1 + (c.condition_beta ? 1 : 0);
  int64_t at = 0;
  auto take = [&](int64_t k) {
    const float* p = w ? w + at : nullptr;
    at += k;
    return p;
  };
  W.emb_w = take(H * nf);
  W.emb_b = take(H);
  take(nf * H + nf);  // embedding_out
  for (int l = 0; l < c.n_layers; ++l) {
    WideLayerW v{};
    v.e0w = take(H * (2 * H + 2)); v.e0b = take(H); v.e2w = take(H * H); v.e2b = take(H);
    v.n0w = take(H * 2 * H); v.n0b = take(H); v.n2w = take(H * H); v.n2b = take(H);
    v.c0w = take(H * H); v.c0b = take(H); v.c2w = take(H);
    if (c.attention) { v.aw = take(H); v.ab = take(1); }
    W.layer.push_back(v);
  }
  W.count = at;
  return W;
}

// ---- parameter blocks of the vector-pipe kernels (egnn_wide_kernel.hip); the matrix-pipe launch wrappers read the call's
// arguments from them
struct WideParams {
  const float* w;
  const float* estatic;
  int n, dim, H, L, attention, tanh_on, has_beta;
  float coord_scale;
  long long B;
  int mode;  // 0 backbone forward (t = its time input), 1 denoiser, 2 score (t = h = sigma^2)
  const float* x;
  const float* t;
  const float* beta;
  float* out;
  int only_bad;  // recompute only the walkers whose `out` holds a non-finite value (repair pass behind the matrix-pipe kernel)
  // mode 3: n_steps Euler-Maruyama steps of the not-debiased reverse SDE in one launch (pita_egnn_wide_sampler_run)
  float* xs;               // [B, n*dim] walkers, in place
  const float* x_backup;   // only_bad: the walkers as they were before the matrix-pipe launch
  const float* step_tab;   // [n_steps][PITA_STEP_STRIDE]
  int n_steps;
  const float* noise;      // nullable [n_steps, B, n*dim]
  unsigned long long seed, walker_offset;
  long long step0;
  int remove_mean;
  double* stats_out;       // nullable [n_steps][4]
  const int* bad_from;     // only_bad: [B*n] first step whose moments the matrix-pipe launch left to this one
  const int* bad_flag;     // only_bad, nullable: 0 = the matrix-pipe launch left nothing non-finite, return at once
};
struct WideJvpParams {
  WideParams base;       // mode is ignored: the denoiser (mode 1) is differentiated
  const float* vx;       // nullable [B, n*dim]: position direction; null -> unit vector e_dir (dir >= 0) or zero (dir < 0)
  const float* vh;       // nullable [B]: direction in h
  int dir;
  float* dout;           // nullable [B, n*dim]
  float* dot_out;        // nullable: dot_out[b * dot_stride + dot_off] = <x_b, dD_b>
  long long dot_stride, dot_off;
  float* diag_acc;       // nullable: diag_acc[b] += dD[b, dir]; MULTI: [n*dim, B], diag_acc[dir * B + b] = dD[b, dir]
  const int* only_bad;   // nullable [B] (MULTI: [B * n*dim], one per item): process only what the matrix-pipe kernel
                         // flagged (egnn_wide_mfma_jvp_kernel.hip)
  // (walker, probe) items (pita_egnn_wide_trace_probes): item = walker * n_probes + probe, tangent input v_probe,
  // diag_acc[probe * B + walker] = <v_probe, dD>, only_bad one per item
  int n_probes;
  const float* probes;   // nullable [n_probes, B, n*dim]; null: Rademacher signs drawn in the kernel (common.h:
                         // philox_rademacher_word keyed seed, walker_offset + walker, step)
  unsigned long long seed, walker_offset;
  long long step;
};
// the kinds of work item of the two forward-mode kernels
enum { WIDE_JVP_ONE = 0 /* walker, one direction per launch */, WIDE_JVP_UNIT /* (walker, unit direction) */,
       WIDE_JVP_PROBE /* (walker, probe) */ };
struct WideVjpParams {
  WideParams base;   // x, t (= h), beta, out (nullable: the denoiser)
  const float* cot;  // nullable [B, n*dim]: cotangent (null: x)
  float* vjp;        // [B, n*dim]
  float* dot_h;      // nullable [B]
  float* dot_parts;  // nullable [B, 2] (needs dot_h): { c_out <cot, F>,  <cot, d(c_out F)/dh> = dot_h - c_s'(h) <cot, x> }
                     // as pita_egnn_vjp defines it; then dot_h = dot_parts[1] + c_s'(h) <cot, x>, added in fp32
  float* ws;         // checkpoints: [wave slot][L][2 n 64 + n 4]
  // repair mode behind the matrix-pipe kernel (egnn_wide_mfma_vjp_kernel.hip); mark null: every walker, as ever
  const int* mark;   // nullable [B]: compute and write only the walkers marked 1
  const int* flag;   // with mark: 0 = the matrix-pipe launch marked nobody, return at once
};

// a matrix-pipe table row (egnn_wide_mfma_common.h) and the parameter blocks of its three kernels
template <class P>
struct Wide64Row;
struct Wide64Params;
struct Wide64JvpParams;
struct Wide64VjpParams;

}  // namespace pita

struct pita_egnn_wide {
  pita_egnn_wide_config cfg;
  int device = -1;
  int n_cu = 256;
  // vector-pipe kernels
  pita::DeviceBuf w;        // packed weights, see WideLayer
  pita::DeviceBuf estatic;  // [n][64] embedding of the static node features + embedding bias, natural feature order
  // matrix-pipe kernels: the rows that serve this handle's particle system AND depth, decided once by wide64_prepare
  // (null: none; jvp64 / vjp64 only beside fwd64), and their weights (empty without fwd64)
  const pita::Wide64Row<pita::Wide64Params>* fwd64 = nullptr;
  const pita::Wide64Row<pita::Wide64JvpParams>* jvp64 = nullptr;
  const pita::Wide64Row<pita::Wide64VjpParams>* vjp64 = nullptr;
  pita::DeviceBuf m16h;     // [L][7 matrices][2 x 2 blocks] f16 two-piece fragments
  pita::DeviceBuf vecs64;   // embedding vectors + per-layer vectors, fragment order, f16-path scales folded in
  pita::DeviceBuf est64;    // [n][64] as estatic, fragment order
  pita::DeviceBuf m16t;     // reverse mode: [L][7 matrices][2 x 2 blocks] bf16 x 3 fragments of the unscaled transposes
  pita::DeviceBuf vecs64t;  // reverse mode: [L][w_r 64 | w_e 64] unscaled, fragment order
  pita::DeviceBuf flag;     // one int, set by the forward kernel when a walker comes out non-finite: the repair pass
                            // returns at once otherwise
  // scratch, grown on demand
  pita::DeviceBuf bk;       // fused sampler: backup of the walkers + per-particle bookkeeping for the repair pass
  pita::DeviceBuf jbad;     // int [B] marks of the forward-mode kernel (walkers left to the vector-pipe kernel);
                            // [B * n*d], one per (walker, direction) item, in pita_egnn_wide_jacobian_trace; [B * K], one
                            // per (walker, probe) item, in pita_egnn_wide_trace_probes
  pita::DeviceBuf jdiag;    // pita_egnn_wide_jacobian_trace: [n*d, B] diagonal entries dD[b, dir] before the reduction;
                            // pita_egnn_wide_trace_probes: [K, B] quadratic forms <v_k, dD> before the mean
  pita::DeviceBuf vjp_ws;   // reverse mode, vector pipe: per-wave checkpoints of the forward sweep
  pita::DeviceBuf vjp_ck;   // reverse mode, matrix pipe: the same, one region per resident item slot
  pita::DeviceBuf vmark;    // int [B] walkers the reverse-mode kernel left to the vector pipe; one flag word behind them
};

namespace pita {

// What the five entry points do with a handle: which matrix-pipe kernels run ahead of the vector-pipe ones.
// PITA_WIDE_NO_MFMA (read at every call): A/B against the vector-pipe kernels alone.
struct WidePlan {
  bool fwd, jvp, vjp;
};
inline WidePlan wide_plan(const pita_egnn_wide* net) {
  const bool on = net && net->fwd64 && getenv("PITA_WIDE_NO_MFMA") == nullptr;
  return {on, on && net->jvp64, on && net->vjp64};
}

// picks the rows (fwd64, jvp64, vjp64) and, where there is a forward row, packs and uploads the matrix-pipe weights;
// he: host [n][64] static embedding
int wide64_prepare(pita_egnn_wide* net, const WideWeights& W, const float* he);
const Wide64Row<Wide64JvpParams>* wide64_jvp_row(const pita_egnn_wide_config& cfg);
const Wide64Row<Wide64VjpParams>* wide64_vjp_row(const pita_egnn_wide_config& cfg);
// The launches ahead of the vector-pipe kernels (plan.fwd / .jvp / .vjp); each reads the call from the parameter block
// its vector-pipe sibling takes.
// evaluation modes 0-2 and the fused sampler (mode 3: bad_from device [B * n]); zeroes and passes net->flag
int wide64_forward(pita_egnn_wide* net, const WideParams& v, int* bad_from, hipStream_t stream);
// forward-mode derivative; kind WIDE_JVP_UNIT: all B * n*d (walker, unit direction) items in one launch, diag_acc[dir * B +
// b]; WIDE_JVP_PROBE: all B * n_probes (walker, probe) items, diag_acc[probe * B + b]; bad: device ints, one per item,
// zeroed by the caller, set to 1 for what is left to the vector-pipe kernel
int wide64_jvp(pita_egnn_wide* net, const WideJvpParams& v, int kind, int* bad, hipStream_t stream);
// reverse-mode sweep; mark: device [B] ints and flag: one int, zeroed by the caller: set to 1 for the walkers left to the
// vector-pipe kernel / when there is one
int wide64_vjp(pita_egnn_wide* net, const WideVjpParams& v, int* mark, int* flag, hipStream_t stream);

}  // namespace pita
