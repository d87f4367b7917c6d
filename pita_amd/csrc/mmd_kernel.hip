// Weighted per-population mix-RBF Gram sums between walker sets for gfx950 (pita_hip.h: pita_rbf_gram_sums), the device
// side of pita_amd.metrics.rbf_mmd2.  The reference's mmd.py was never restated in oracle/: the definition in the header
// is the specification (unpinned by construction, like DW4 and the POT W2).
//
// Three stages per set, all in stream order:
//  1. mmd_rows_finite_kernel: one wave per row, flag 1 where every coordinate of the row is finite.
//  2. mmd_weights_kernel: one block per population -- m, the two counts, the fp32 row weights (0 for a row left out) and
//     their fp64 sums, in weighted_moments_kernel's thread stride and reduction order (observables_kernels.hip).
//  3. rbf_gram_kernel: a block takes one (population, a-tile) and every nbg-th b-tile, 64 x 64 pairs per tile, both
//     tiles staged k-major in LDS, a 4 x 4 register sub-tile of pairs per thread; the pair matrix is never written.
//     rbf_gram_reduce_kernel adds the block partials of a population in a fixed order.
// The distance runs on the vector pipe with the difference first: the matrix pipe would need |a|^2 + |b|^2 - 2 a.b, whose
// rounding noise for two bit-identical rows (walkers copied by a resampling event) is multiplied by gamma = 5 000 at the
// smallest default bandwidth.
#include "common.h"

#include <cfloat>
#include <climits>
#include <cmath>

using namespace pita;

namespace {

constexpr int MMD_T = 256;                      // threads of a Gram block: 16 x 16, thread (ty, tx)
constexpr int MMD_TILE = 64;                    // rows of an a-tile and of a b-tile: 4 per thread on either side
constexpr int MMD_DK = 32;                      // coordinates of a row staged at once; longer rows are chunked, s stays in registers
constexpr int MMD_LD = MMD_TILE + 4;            // LDS row stride in floats: 16-byte aligned rows, conflict-free staging writes
constexpr int MMD_MAX_GAMMA = 16, MMD_MAX_DIM = 768;
constexpr int MMD_WT = 1024, MMD_WW = MMD_WT / 64;  // threads / waves of the one-block-per-population weights pass
constexpr long long MMD_BLOCKS = 4096;          // blocks per population the split over the b-tiles aims at ...
constexpr long long MMD_MIN_TILES = 8;          // ... while a block keeps at least this many b-tiles (cross mode)

struct MmdGammas { float c[MMD_MAX_GAMMA]; };   // c_s = (float)(-gamma_s * log2 e), kernel arguments

// Tiling of one population against its partner set; a function of (pop_size, n_b) alone, so that the partial sums of a
// population, and their order, depend neither on n_pop nor on p.  Self mode: nbt = na.
struct MmdPlan { long long na, nbt, nbg; };
inline MmdPlan mmd_plan(int64_t pop_size, int64_t n_b) {
  MmdPlan pl;
  pl.na = (pop_size + MMD_TILE - 1) / MMD_TILE;
  pl.nbt = n_b > 0 ? (n_b + MMD_TILE - 1) / MMD_TILE : pl.na;
  long long g = (MMD_BLOCKS + pl.na - 1) / pl.na;
  const long long most = pl.nbt / MMD_MIN_TILES > 1 ? pl.nbt / MMD_MIN_TILES : 1;
  pl.nbg = g < most ? g : most;
  return pl;
}
// Partial slots per population the workspace holds: an upper bound of na * nbg that grows with pop_size and with n_b.
inline long long mmd_partial_slots(const MmdPlan& pl) {
  const long long most = pl.nbt / MMD_MIN_TILES > 1 ? pl.nbt / MMD_MIN_TILES : 1;
  return pl.na + MMD_BLOCKS < pl.na * most ? pl.na + MMD_BLOCKS : pl.na * most;
}

__global__ void __launch_bounds__(MMD_T) mmd_rows_finite_kernel(const float* __restrict__ x, long long rows, int dim,
                                                                float* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * (MMD_T / 64);
  for (long long row = (long long)blockIdx.x * (MMD_T / 64) + (threadIdx.x >> 6); row < rows; row += stride) {
    const float* r = x + row * dim;
    bool bad = false;
    for (int k = lane; k < dim; k += 64) bad = bad || !(fabsf(r[k]) < INFINITY);  // NaN fails the comparison
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) flag[row] = any_bad ? 0.0f : 1.0f;
  }
}

// Population blockIdx.x: w holds the row flags on entry and the fp32 row weights on exit; info row = {m, sum w, sum w^2,
// n_bad, n_neg_inf}.  A row is left out (weight 0, n_bad) when its log-weight is NaN or +inf or its flag is 0; of the
// others, those with log-weight -inf have weight 0 (n_neg_inf).  m is over ALL finite log-weights of the population.
__global__ void __launch_bounds__(MMD_WT) mmd_weights_kernel(const float* __restrict__ logw, long long S, float* __restrict__ w,
                                                             double* __restrict__ info) {
  __shared__ double s_s[2][MMD_WW];
  __shared__ float s_mx[MMD_WW];
  __shared__ unsigned long long s_bad[MMD_WW], s_ninf[MMD_WW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long p = blockIdx.x;
  const float* a = logw ? logw + p * S : nullptr;
  float* wp = w + p * S;
  float mx = -INFINITY;
  unsigned long long bad = 0, ninf = 0;
  for (long long i = t; i < S; i += MMD_WT) {
    const float l = a ? a[i] : 0.0f;
    const bool lfin = l == l && fabsf(l) != INFINITY;
    if (a && lfin) mx = fmaxf(mx, l);
    if (l != l || l == INFINITY || wp[i] == 0.0f) ++bad;
    else if (l == -INFINITY) ++ninf;
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    bad += __shfl_xor(bad, o, 64);
    ninf += __shfl_xor(ninf, o, 64);
  }
  if (lane == 0) { s_mx[wv] = mx; s_bad[wv] = bad; s_ninf[wv] = ninf; }
  __syncthreads();
  mx = -INFINITY; bad = 0; ninf = 0;
  for (int k = 0; k < MMD_WW; ++k) { mx = fmaxf(mx, s_mx[k]); bad += s_bad[k]; ninf += s_ninf[k]; }
  const double m = mx > -INFINITY ? (double)mx : 0.0;

  double s0 = 0.0, s1 = 0.0;
  for (long long i = t; i < S; i += MMD_WT) {
    const float l = a ? a[i] : 0.0f;
    float wf = 0.0f;
    if (l == l && l != INFINITY && wp[i] != 0.0f) wf = a ? (float)exp((double)l - m) : 1.0f;  // -inf: exp gives 0
    wp[i] = wf;
    s0 += (double)wf;
    s1 = fma((double)wf, (double)wf, s1);
  }
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64);
    s1 += __shfl_xor(s1, o, 64);
  }
  if (lane == 0) { s_s[0][wv] = s0; s_s[1][wv] = s1; }
  __syncthreads();
  if (t == 0) {
    s0 = 0.0; s1 = 0.0;
    for (int k = 0; k < MMD_WW; ++k) { s0 += s_s[0][k]; s1 += s_s[1][k]; }
    double* o = info + 5 * p;
    o[0] = m; o[1] = s0; o[2] = s1; o[3] = (double)bad; o[4] = (double)ninf;
  }
}

// Coordinates [k0, k0 + kc) of the rows [row0, row0 + nrows) of src into dst[k * MMD_LD + r] (zeros elsewhere in the 32 x 64
// tile).  Thread t takes k = t % 8 + 8 * (t / 32 % 4) and the rows t / 8 % 4 + 4 * (t / 128) + 8 i: the 32 lanes of a
// half wave write 8 k x 4 rows, banks (4 k + r) % 32, all distinct; a wave reads 16 consecutive floats of 4 rows.
__device__ __forceinline__ void mmd_stage(float* dst, const float* __restrict__ src, long long row0, int nrows, int dim, int k0,
                                          int kc) {
  const int t = threadIdx.x;
  const int k = (t & 7) + 8 * ((t >> 5) & 3);
  const int r0 = ((t >> 3) & 3) + 4 * (t >> 7);
#pragma unroll
  for (int i = 0; i < MMD_TILE / 8; ++i) {
    const int r = r0 + 8 * i;
    float v = 0.0f;
    if (r < nrows && k < kc) v = src[(row0 + r) * dim + k0 + k];
    dst[k * MMD_LD + r] = v;
  }
}

// Block blockIdx.x = (p * na + ia) * nbg + bg: a-tile ia of population p against the b-tiles bg, bg + nbg, ... (self
// mode: ia + bg, ia + bg + nbg, ... -- only jb >= ia, an off-diagonal tile counted twice).  Thread (ty, tx) holds the
// pairs (4 ty + i, 4 tx + j): per k one ds_read_b128 of the a-tile (4 addresses per wave, broadcast) and one of the
// b-tile (16 consecutive slots, every bank once) feed 16 pairs.  Per pair, fp32: s = fmaf(d, d, s) over k in index order
// with d = a_k - b_k; ww = w_i * v_j; where ww > 0, sv = min(s, FLT_MAX), else sv = 0 (a row left out has weight 0 and may
// hold NaN: its s never reaches the exponential); e = v_exp_f32(c_s * sv); term = ww * e.  The 16 terms of a thread and
// tile are added in fp32 (i outer, j inner), everything above that in double: per thread over its tiles, xor-shuffle
// wave reduction, the four wave partials in index order.
template <int NG>
__global__ void __launch_bounds__(MMD_T) rbf_gram_kernel(const float* __restrict__ a, const float* __restrict__ wa,
                                                         const float* __restrict__ b, const float* __restrict__ wb,
                                                         long long S, long long M, int dim, long long na, long long nbt,
                                                         long long nbg, int self, MmdGammas gm,
                                                         double* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float As[MMD_DK * MMD_LD];
  __shared__ __attribute__((aligned(16))) float Bs[MMD_DK * MMD_LD];
  __shared__ float wAs[MMD_TILE], wBs[MMD_TILE];
  __shared__ double red[MMD_T / 64][NG];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const long long blk = blockIdx.x;
  const long long bg = blk % nbg, ia = (blk / nbg) % na, p = blk / (nbg * na);
  const float* ap = a + p * S * dim;
  const float* wap = wa + p * S;
  const float* bp = self ? ap : b;
  const float* wbp = self ? wap : wb;
  const long long a0 = ia * MMD_TILE;
  const int an = (int)(S - a0 < MMD_TILE ? S - a0 : MMD_TILE);
  const int nchunks = (dim + MMD_DK - 1) / MMD_DK;
  if (t < MMD_TILE) wAs[t] = t < an ? wap[a0 + t] : 0.0f;
  double dacc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) dacc[g] = 0.0;
  bool a_staged = false;
  for (long long jb = self ? ia + bg : bg; jb < nbt; jb += nbg) {
    const long long b0 = jb * MMD_TILE;
    const int bn = (int)(M - b0 < MMD_TILE ? M - b0 : MMD_TILE);
    float s[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[i][j] = 0.0f;
    for (int ch = 0; ch < nchunks; ++ch) {
      const int k0 = ch * MMD_DK;
      const int kc = dim - k0 < MMD_DK ? dim - k0 : MMD_DK;
      __syncthreads();  // the previous chunk and tile have been consumed
      if (nchunks > 1 || !a_staged) mmd_stage(As, ap, a0, an, dim, k0, kc);  // a row that fits stays for every b-tile
      mmd_stage(Bs, bp, b0, bn, dim, k0, kc);
      if (ch == 0 && t < MMD_TILE) wBs[t] = t < bn ? wbp[b0 + t] : 0.0f;
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < kc; ++k) {
        const float4 av = *reinterpret_cast<const float4*>(&As[k * MMD_LD + 4 * ty]);
        const float4 bv = *reinterpret_cast<const float4*>(&Bs[k * MMD_LD + 4 * tx]);
        const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float d = ar[i] - br[j];
            s[i][j] = fmaf(d, d, s[i][j]);
          }
      }
    }
    a_staged = true;
    float tacc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) tacc[g] = 0.0f;
    float wi[4], vj[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { wi[i] = wAs[4 * ty + i]; vj[i] = wBs[4 * tx + i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float ww = wi[i] * vj[j];
        const float sv = ww > 0.0f ? fminf(s[i][j], FLT_MAX) : 0.0f;
#pragma unroll
        for (int g = 0; g < NG; ++g) tacc[g] = tacc[g] + ww * __builtin_amdgcn_exp2f(gm.c[g] * sv);
      }
    const double mult = (self && jb != ia) ? 2.0 : 1.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) dacc[g] += mult * (double)tacc[g];
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    double v = dacc[g];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((t & 63) == 0) red[t >> 6][g] = v;
  }
  __syncthreads();
  if (t < NG) {
    double v = 0.0;
    for (int w = 0; w < MMD_T / 64; ++w) v += red[w][t];
    partials[blk * NG + t] = v;
  }
}

// sums[p, g] = the nparts block partials of population p: thread t adds partials t, t + 256, ..., xor-shuffle wave
// reduction, the four wave partials in index order.
__global__ void __launch_bounds__(MMD_T) rbf_gram_reduce_kernel(const double* __restrict__ partials, long long nparts, int ng,
                                                                double* __restrict__ sums) {
  __shared__ double red[MMD_T / 64];
  const int t = threadIdx.x;
  const long long p = blockIdx.x;
  const double* pp = partials + p * nparts * ng;
  for (int g = 0; g < ng; ++g) {
    double v = 0.0;
    for (long long i = t; i < nparts; i += MMD_T) v += pp[i * ng + g];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // red of the previous gamma has been read
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    if (t == 0) {
      double r = 0.0;
      for (int w = 0; w < MMD_T / 64; ++w) r += red[w];
      sums[p * ng + g] = r;
    }
  }
}

// Workspace, in this order: 8 doubles (info of b when the caller wants none) | the block partials, n_pop *
// mmd_partial_slots * 16 doubles | the row weights of a, n_pop * pop_size floats | those of b, n_b floats.  0 = the sizes
// overflow.
size_t mmd_workspace_bytes(int64_t n_pop, int64_t pop_size, int64_t n_b) {
  if (n_pop < 1 || pop_size < 1 || n_b < 0) return 0;
  if (pop_size > INT64_MAX / 8 / n_pop || n_b > INT64_MAX / 8) return 0;
  const MmdPlan pl = mmd_plan(pop_size, n_b);
  const long long per_pop = mmd_partial_slots(pl);
  if (n_pop > (INT64_MAX / 1024) / per_pop) return 0;
  const uint64_t floats = (uint64_t)n_pop * (uint64_t)pop_size + (uint64_t)n_b;
  const uint64_t bytes = 8ull * 8 + 8ull * MMD_MAX_GAMMA * (uint64_t)n_pop * (uint64_t)per_pop + 4ull * floats;
  return (size_t)((bytes + 7ull) & ~7ull);
}

int mmd_weights(const float* x, const float* logw, int64_t n_pop, int64_t pop_size, int dim, float* w, double* info,
                hipStream_t s) {
  const int64_t rows = n_pop * pop_size;
  hipLaunchKernelGGL(mmd_rows_finite_kernel, dim3(capped_grid((rows + 3) / 4, kGridCus * 16)), dim3(MMD_T), 0, s, x,
                     (long long)rows, dim, w);
  PITA_LAUNCH_CHECK();
  hipLaunchKernelGGL(mmd_weights_kernel, dim3((unsigned)n_pop), dim3(MMD_WT), 0, s, logw, (long long)pop_size, w, info);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

}  // namespace

extern "C" size_t pita_rbf_gram_workspace_bytes(int64_t n_pop, int64_t pop_size, int64_t n_b) {
  return mmd_workspace_bytes(n_pop, pop_size, n_b);
}

extern "C" int pita_rbf_gram_sums(const float* a, const float* logw_a, int64_t n_pop, int64_t pop_size, const float* b,
                                  const float* logw_b, int64_t n_b, int dim, const double* gammas, int n_gamma, double* sums,
                                  double* info_a, double* info_b, void* workspace, void* stream) {
  PITA_REQUIRE(a && gammas && sums && info_a && workspace, "pita_rbf_gram_sums: null a, gammas, sums, info_a or workspace");
  PITA_REQUIRE(n_pop >= 1 && pop_size >= 1, "pita_rbf_gram_sums: n_pop and pop_size must be >= 1 (got %lld, %lld)",
               (long long)n_pop, (long long)pop_size);
  PITA_REQUIRE(dim >= 1 && dim <= MMD_MAX_DIM && n_gamma >= 1 && n_gamma <= MMD_MAX_GAMMA,
               "pita_rbf_gram_sums: 1 <= dim <= %d and 1 <= n_gamma <= %d (got %d, %d)", MMD_MAX_DIM, MMD_MAX_GAMMA, dim, n_gamma);
  if (b)
    PITA_REQUIRE(n_b >= 1, "pita_rbf_gram_sums: n_b must be >= 1 with a set b (got %lld)", (long long)n_b);
  else
    PITA_REQUIRE(n_b == 0 && !logw_b, "pita_rbf_gram_sums: self mode (b = NULL) takes n_b = 0 and no logw_b (got n_b = %lld)",
                 (long long)n_b);
  MmdGammas gm;
  for (int g = 0; g < MMD_MAX_GAMMA; ++g) gm.c[g] = 0.0f;
  for (int g = 0; g < n_gamma; ++g) {
    PITA_REQUIRE(std::isfinite(gammas[g]) && gammas[g] >= 0.0, "pita_rbf_gram_sums: gamma %d = %g is not finite and >= 0", g,
                 gammas[g]);
    gm.c[g] = (float)(-gammas[g] * 1.4426950408889634);
  }
  const size_t bytes = mmd_workspace_bytes(n_pop, pop_size, n_b);
  const MmdPlan pl = mmd_plan(pop_size, n_b);
  const long long per_pop = pl.na * pl.nbg;
  if (bytes == 0 || n_pop > INT_MAX / per_pop || pop_size > INT64_MAX / MMD_MAX_DIM / n_pop || n_b > INT64_MAX / MMD_MAX_DIM)
    return fail(PITA_EUNSUPPORTED, "pita_rbf_gram_sums: n_pop = %lld, pop_size = %lld, n_b = %lld is too large", (long long)n_pop,
                (long long)pop_size, (long long)n_b);

  hipStream_t s = (hipStream_t)stream;
  double* ws_info_b = static_cast<double*>(workspace);
  double* partials = ws_info_b + 8;
  float* wa = reinterpret_cast<float*>(partials + (size_t)MMD_MAX_GAMMA * n_pop * mmd_partial_slots(pl));
  float* wb = wa + (size_t)n_pop * pop_size;
  int rc = mmd_weights(a, logw_a, n_pop, pop_size, dim, wa, info_a, s);
  if (rc != PITA_OK) return rc;
  if (b) {
    rc = mmd_weights(b, logw_b, 1, n_b, dim, wb, info_b ? info_b : ws_info_b, s);
    if (rc != PITA_OK) return rc;
  }
  const int self = b ? 0 : 1;
  const long long M = b ? n_b : pop_size;
  rc = dispatch_dim<MMD_MAX_GAMMA>(n_gamma, [&](auto ng) {
    constexpr int NG = decltype(ng)::value;
    hipLaunchKernelGGL(rbf_gram_kernel<NG>, dim3((unsigned)(n_pop * per_pop)), dim3(MMD_T), 0, s, a, wa, b, wb,
                       (long long)pop_size, M, dim, pl.na, pl.nbt, pl.nbg, self, gm, partials);
    PITA_LAUNCH_CHECK();
    return (int)PITA_OK;
  });
  if (rc != PITA_OK) return rc;
  hipLaunchKernelGGL(rbf_gram_reduce_kernel, dim3((unsigned)n_pop), dim3(MMD_T), 0, s, partials, per_pop, n_gamma, sums);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}
