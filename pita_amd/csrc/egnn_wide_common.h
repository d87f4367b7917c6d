// Native handle behind pita_egnn_wide_t, shared by the two kernels that serve it: the vector-pipe kernel
// (egnn_wide_kernel.hip: any hidden_nf <= 64, any particle count <= 64) and the matrix-pipe kernel
// (egnn_wide_mfma_kernel.hip, with its forward- and reverse-mode siblings: the particle systems they are instantiated for).
#pragma once
#include "common.h"

struct pita_egnn_wide {
  pita_egnn_wide_config cfg;
  float* d_w = nullptr;        // vector-pipe kernel: packed weights, see WideLayer
  float* d_estatic = nullptr;  // [n][64] embedding of the static node features + embedding bias, natural feature order
  int device = -1;
  int n_cu = 256;
  // matrix-pipe kernel (null / 0 when the particle system has no instantiation)
  unsigned* d_m16h = nullptr;  // [L][7 matrices][2 x 2 blocks] f16 two-piece fragments
  float* d_vecs64 = nullptr;   // embedding vectors + per-layer vectors, fragment order, f16-path scales folded in
  float* d_est64 = nullptr;    // [n][64] as d_estatic, fragment order
  const void* shape64 = nullptr;
  // fused sampler on the matrix pipe: backup of the walkers + per-particle bookkeeping for the vector-pipe repair pass
  void* d_bk = nullptr;
  size_t bk_bytes = 0;
  int* d_flag = nullptr;  // set by the matrix-pipe kernel when a walker comes out non-finite: the repair pass returns at once otherwise
  int* d_jbad = nullptr;    // [B] flags of the matrix-pipe forward-mode kernel (walkers left to the vector-pipe kernel);
  size_t jbad_bytes = 0;    // [B * n*d], one per (walker, direction) item, in pita_egnn_wide_jacobian_trace
  float* d_jdiag = nullptr;  // pita_egnn_wide_jacobian_trace: [n*d, B] diagonal entries dD[b, dir] before the reduction
  size_t jdiag_bytes = 0;
  float* d_vjp_ws = nullptr;  // reverse-mode kernel (vector pipe): per-wave checkpoints of the forward sweep
  size_t vjp_ws_bytes = 0;
  // reverse-mode kernel on the matrix pipe (egnn_wide_mfma_vjp_kernel.hip)
  unsigned* d_m16t = nullptr;   // [L][7 matrices][2 x 2 blocks] bf16 x 3 fragments of the unscaled transposes
  float* d_vecs64t = nullptr;   // [L][w_r 64 | w_e 64] unscaled, fragment order
  float* d_vjp_ck = nullptr;    // checkpoints of the forward sweep, one region per resident item slot
  size_t vjp_ck_bytes = 0;
  int* d_vmark = nullptr;       // [B] walkers left to the vector-pipe kernel; one flag word sits behind them
  size_t vmark_bytes = 0;
};

namespace pita {
// packs and uploads the matrix-pipe kernel's weights when the particle system has an instantiation (leaves
// net->shape64 null otherwise); w: the flattened state_dict (pita_egnn_wide_create), he: host [n][64] static embedding
int wide64_prepare(pita_egnn_wide* net, const float* w, const float* he);
int wide64_launch(pita_egnn_wide* net, int what, const float* t, const float* x, const float* beta, float* out,
                  long long B, hipStream_t stream);
// n_steps fused Euler-Maruyama steps on the matrix-pipe kernel (mode 3 of egnn_wide64_kernel); bad_from: device [B * n]
int wide64_sampler(pita_egnn_wide* net, float* x, long long B, const float* step_tab, int n_steps, const float* noise,
                   unsigned long long seed, unsigned long long walker_offset, long long step0, int remove_mean,
                   double* stats_out, int* bad_from, hipStream_t stream);
// 1 when the forward-mode kernel on the matrix pipe has an instantiation for the net's particle system whose LDS fits
int wide64_jvp_available(const pita_egnn_wide* net);
// forward-mode derivative on the matrix pipe (egnn_wide_mfma_jvp_kernel.hip); returns 1 when the particle system has no
// instantiation; bad: device [B] ints, zeroed by the caller, set to 1 for walkers left to the vector-pipe kernel
int wide64_jvp(pita_egnn_wide* net, const float* h, const float* x, const float* beta, const float* vx, int dir,
               const float* vh, float* out, float* dout, float* dot_out, long long dot_stride, long long dot_off,
               float* diag_acc, int* bad, long long B, hipStream_t stream);
// the same over all B * n*d (walker, unit direction) items in one launch: diag[dir * B + b] = dD[b, dir], out (nullable)
// the denoiser; bad: device [B * n*d] ints, zeroed by the caller, one per item
int wide64_jvp_multi(pita_egnn_wide* net, const float* h, const float* x, const float* beta, float* out, float* diag,
                     int* bad, long long B, hipStream_t stream);
// 1 when the reverse-mode kernel on the matrix pipe has an instantiation for the net's particle system whose LDS fits
int wide64_vjp_available(const pita_egnn_wide* net);
// reverse-mode sweep on the matrix pipe (egnn_wide_mfma_vjp_kernel.hip); returns 1 when the particle system has no
// instantiation; mark: device [B] ints and flag: one int, zeroed by the caller: set to 1 for the walkers left to the
// vector-pipe kernel / when there is one
int wide64_vjp(pita_egnn_wide* net, const float* h, const float* x, const float* beta, const float* cot, float* out,
               float* vjp, float* dot_h, int* mark, int* flag, long long B, hipStream_t stream);
void wide64_release(pita_egnn_wide* net);
}  // namespace pita
