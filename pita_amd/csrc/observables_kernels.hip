// Weighted per-population observables for gfx950 (pita_hip.h: pita_weighted_histogram, pita_pair_distance_histogram,
// pita_weighted_moments).  An extension: the reference's evaluation counts every walker once
// and treats the batch as one population.
//
// The batch is n_pop populations of pop_size walkers, population p in rows [p * pop_size, (p + 1) * pop_size).  Per
// population: m = max over the finite log-weights (0 when there is none), relative weight exp((double)logw - m).
//
// Histograms: the weighted bin sums are FIXED-POINT integers -- each value adds q = rint(w * 2^shift) to its bin -- so
// that a population's bits depend neither on the order of its walkers nor on how the blocks interleave (a float atomic
// sum depends on arrival order).  obs_info_kernel takes m and the two counts of every population, then the histogram
// proper runs, whose blocks each work on ONE population with LDS-privatised 64-bit bins and one 64-bit integer add per
// non-empty bin and block at the end, the design of histogram_kernel.  max and integer sums are exact in any order,
// hence so is everything the blocks derive from them.
#include "common.h"
#include "hist_common.h"

#include <climits>

using namespace pita;

namespace {

constexpr int OBS_T = 256;                        // threads of a histogram block
constexpr int OBS_ST = 1024, OBS_SW = OBS_ST / 64;  // threads / waves of a one-block-per-population pass
constexpr int OBS_MIN_SHIFT = 20, OBS_MAX_SHIFT = 40;
constexpr unsigned long long OBS_LEFT_OUT = ~0ull;  // q of a walker left out of every sum (a real q is <= 2^40)
// Blocks a launch aims at.  Every block ends with integer adds to its population's bins, and with one population these
// all meet on the same words: the streaming passes (values, log-weights) are fastest with few blocks, the pair kernel,
// whose blocks compute for much longer, with many (measured: tools/time_observables.py).
constexpr int OBS_GRID = 512, OBS_GRID_PAIRS = 2048;
constexpr int OBS_PAIR_W = 64, OBS_PAIR_FLOATS = 4096;  // walkers / coordinates a pair block stages at most

// fixed-point weight of walker `row` of a population (lw: the population's log-weights, null = unit weights)
__device__ __forceinline__ unsigned long long obs_weight_q(const float* lw, long long row, double m, int shift) {
  if (!lw) return 1ull << shift;
  const float a = lw[row];
  if (a != a || a == INFINITY) return OBS_LEFT_OUT;
  return (unsigned long long)rint(ldexp(exp((double)a - m), shift));  // -inf: exp gives 0
}

// ---- the pass before a histogram: m and the two counts of every population, by several blocks per population.  A
// maximum and integer counts are exact in any order, so the blocks combine them with integer atomics: while the two
// kernels run, row p of `info` (zeroed by the entry point) holds three 64-bit integers -- the maximum as an ordered key
// (0 = no finite entry), n_bad, n_neg_inf -- which the histogram blocks read (stream order); obs_info_finish_kernel
// turns the rows into the documented doubles afterwards.
// key: finite floats in ascending order as unsigned integers >= 0x00800000 (and +0 above -0, so that even the sign of a
// zero maximum does not depend on the order)
__device__ __forceinline__ unsigned obs_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ double obs_key_max(unsigned long long key) {  // no finite entry: 0
  const unsigned k = (unsigned)key;
  return k == 0u ? 0.0 : (double)__uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// Block blockIdx.x = p * bpi + b: entries b * OBS_T + t, then with stride bpi * OBS_T, of population p.
__global__ void __launch_bounds__(OBS_T) obs_info_kernel(const float* __restrict__ logw, long long S, int bpi,
                                                         unsigned long long* __restrict__ info) {
  __shared__ unsigned s_key[OBS_T / 64];
  __shared__ unsigned long long s_bad[OBS_T / 64], s_ninf[OBS_T / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long p = blockIdx.x / bpi, b = blockIdx.x % bpi;
  const float* a = logw + p * S;
  unsigned key = 0u;
  unsigned long long bad = 0, ninf = 0;
#pragma unroll 4
  for (long long i = b * OBS_T + t; i < S; i += (long long)bpi * OBS_T) {
    const float v = a[i];
    if (v != v || v == INFINITY) ++bad;
    else if (v == -INFINITY) ++ninf;
    else key = max(key, obs_key(v));
  }
  for (int o = 32; o > 0; o >>= 1) {
    key = max(key, (unsigned)__shfl_xor(key, o, 64));
    bad += __shfl_xor(bad, o, 64);
    ninf += __shfl_xor(ninf, o, 64);
  }
  if (lane == 0) { s_key[wv] = key; s_bad[wv] = bad; s_ninf[wv] = ninf; }
  __syncthreads();
  if (t == 0) {
    unsigned long long k = 0, nb = 0, ni = 0;
    for (int w = 0; w < OBS_T / 64; ++w) { k = max(k, (unsigned long long)s_key[w]); nb += s_bad[w]; ni += s_ninf[w]; }
    unsigned long long* o = info + 4 * p;
    if (k) atomicMax(o, k);
    if (nb) atomicAdd(o + 1, nb);
    if (ni) atomicAdd(o + 2, ni);
  }
}

// info row p as documented: {m, n_bad, n_neg_inf, shift}
__global__ void __launch_bounds__(OBS_T) obs_info_finish_kernel(double* __restrict__ info, long long n_pop, int shift) {
  const long long p = (long long)blockIdx.x * OBS_T + threadIdx.x;
  if (p >= n_pop) return;
  const unsigned long long* in = reinterpret_cast<const unsigned long long*>(info) + 4 * p;
  const unsigned long long k = in[0], nb = in[1], ni = in[2];
  double* o = info + 4 * p;
  o[0] = obs_key_max(k);
  o[1] = (double)nb;
  o[2] = (double)ni;
  o[3] = (double)shift;
}

// LDS of a histogram block, in 8-byte words: [ncopy][nbins] weight sums | [ncopy][nbins] counts | the kernel's own tail.
// ncopy copies of the bins (wave w adds to copy w % ncopy): four while the bins are few and the waves would contend.
__host__ __device__ inline int obs_ncopy(int nbins) { return nbins <= 256 ? 4 : 1; }

__device__ __forceinline__ void obs_bins_clear(unsigned long long* lds, int nbins, int ncopy) {
  for (int i = threadIdx.x; i < 2 * ncopy * nbins; i += OBS_T) lds[i] = 0ull;
}
__device__ __forceinline__ void obs_bins_add(unsigned long long* lds, int nbins, int ncopy, int bin, unsigned long long q) {
  unsigned long long* ws = lds + ((threadIdx.x >> 6) % ncopy) * nbins;
  atomicAdd(ws + ncopy * nbins + bin, 1ull);
  if (q) atomicAdd(ws + bin, q);
}
// one 64-bit integer add per non-empty bin of the block (after a __syncthreads)
__device__ __forceinline__ void obs_bins_flush(const unsigned long long* lds, int nbins, int ncopy,
                                               unsigned long long* __restrict__ wsum, unsigned long long* __restrict__ counts) {
  for (int i = threadIdx.x; i < nbins; i += OBS_T) {
    unsigned long long w = 0, c = 0;
    for (int k = 0; k < ncopy; ++k) { w += lds[k * nbins + i]; c += lds[(ncopy + k) * nbins + i]; }
    if (c) atomicAdd(counts + i, c);
    if (w) atomicAdd(wsum + i, w);
  }
}

// Block blockIdx.x = p * bpp + b: population p, values b * 256 + t, then with stride bpp * 256.
__global__ void __launch_bounds__(OBS_T) weighted_histogram_kernel(const float* __restrict__ v, const float* __restrict__ logw,
                                                                   long long S, long long per_walker, int bpp,
                                                                   const float* __restrict__ edges, int nbins, int shift,
                                                                   const unsigned long long* __restrict__ info,
                                                                   unsigned long long* __restrict__ wsum,
                                                                   unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned long long obs_lds[];  // bins | [nbins + 1] edges
  const int ncopy = obs_ncopy(nbins);
  float* e = reinterpret_cast<float*>(obs_lds + 2 * ncopy * nbins);
  obs_bins_clear(obs_lds, nbins, ncopy);
  for (int i = threadIdx.x; i <= nbins; i += OBS_T) e[i] = edges[i];
  __syncthreads();
  const long long p = blockIdx.x / bpp, b = blockIdx.x % bpp;
  const long long nv = S * per_walker;
  const float* vp = v + p * nv;
  const float* lw = logw ? logw + p * S : nullptr;
  const double m = obs_key_max(info[4 * p]);
  const float lo = e[0], hi = e[nbins];
  const float inv = (float)nbins / (hi - lo);
  const bool small = nv <= 0xffffffffll;  // 32-bit division for the walker of a value
  for (long long k = b * OBS_T + threadIdx.x; k < nv; k += (long long)bpp * OBS_T) {
    const int i = hist_bin(vp[k], e, nbins, lo, hi, inv);
    if (i < 0) continue;
    const long long row = per_walker == 1 ? k : (small ? (long long)((unsigned)k / (unsigned)per_walker) : k / per_walker);
    const unsigned long long q = obs_weight_q(lw, row, m, shift);
    if (q != OBS_LEFT_OUT) obs_bins_add(obs_lds, nbins, ncopy, i, q);
  }
  __syncthreads();
  obs_bins_flush(obs_lds, nbins, ncopy, wsum + p * nbins, counts + p * nbins);
}

// Pair distances from the coordinates.  Block blockIdx.x = p * bpp + b takes the chunks b, b + bpp, ... of W walkers of
// population p: coordinates and fixed-point weights of a chunk are staged in LDS, then the threads stride over the
// (walker, pair) items.  The n (n - 1) / 2 pairs i < j of a walker are walked as a rectangle of R = n / 2 rows by n
// columns: row r holds the n - 1 - r pairs (r, r + 1 ..) followed by the r + 1 pairs of row n - 2 - r (for even n the
// last row would meet itself, and its second half is skipped) -- two 32-bit divisions per item and no pair table.
// Arithmetic per pair, fp32 without contraction: delta_k = x_j[k] - x_i[k]; s = delta_0^2, s = s + delta_1^2, s = s +
// delta_2^2; r = sqrt(s) correctly rounded (the fp64 root of an fp32 number rounds to the correctly rounded fp32 root).
__global__ void __launch_bounds__(OBS_T) pair_distance_histogram_kernel(const float* __restrict__ x, const float* __restrict__ logw,
                                                                        long long S, int n, int d, int W, int bpp,
                                                                        const float* __restrict__ edges, int nbins, int shift,
                                                                        const unsigned long long* __restrict__ info,
                                                                        unsigned long long* __restrict__ wsum,
                                                                        unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned long long obs_lds[];  // bins | [W] q | [nbins + 1] edges | [W * n * d] coordinates
  const int ncopy = obs_ncopy(nbins);
  unsigned long long* qs = obs_lds + 2 * ncopy * nbins;
  float* e = reinterpret_cast<float*>(qs + W);
  float* xs = e + nbins + 1;
  obs_bins_clear(obs_lds, nbins, ncopy);
  for (int i = threadIdx.x; i <= nbins; i += OBS_T) e[i] = edges[i];
  __syncthreads();
  const long long p = blockIdx.x / bpp, b = blockIdx.x % bpp;
  const float* lw = logw ? logw + p * S : nullptr;
  const double m = obs_key_max(info[4 * p]);
  const float lo = e[0], hi = e[nbins];
  const float inv = (float)nbins / (hi - lo);
  const unsigned un = (unsigned)n, D = (unsigned)(n * d), Rn = (un / 2u) * un;
  const long long chunks = (S + W - 1) / W;
  for (long long c = b; c < chunks; c += bpp) {
    const long long w0 = c * W;
    const int nw = (int)(S - w0 < W ? S - w0 : W);
    __syncthreads();  // the previous chunk has been consumed
    const float* src = x + (p * S + w0) * (long long)D;
    for (int i = threadIdx.x; i < nw * (int)D; i += OBS_T) xs[i] = src[i];
    for (int i = threadIdx.x; i < nw; i += OBS_T) qs[i] = obs_weight_q(lw, w0 + i, m, shift);
    __syncthreads();
    const unsigned items = (unsigned)nw * Rn;
    for (unsigned it = threadIdx.x; it < items; it += OBS_T) {
      const unsigned w = it / Rn, tt = it - w * Rn;
      const unsigned r = tt / un, cc = tt - r * un, len = un - 1u - r;
      unsigned i, j;
      if (cc < len) {
        i = r; j = r + 1u + cc;
      } else {
        i = un - 2u - r; j = i + 1u + (cc - len);
        if (i == r) continue;  // even n, last row: its own second half
      }
      const unsigned long long q = qs[w];
      if (q == OBS_LEFT_OUT) continue;
      const float* xi = xs + w * D + i * (unsigned)d;
      const float* xj = xs + w * D + j * (unsigned)d;
      float dl = xj[0] - xi[0];
      float s = dl * dl;
      if (d > 1) { dl = xj[1] - xi[1]; s = s + dl * dl; }
      if (d > 2) { dl = xj[2] - xi[2]; s = s + dl * dl; }
      const int bin = hist_bin((float)sqrt((double)s), e, nbins, lo, hi, inv);
      if (bin >= 0) obs_bins_add(obs_lds, nbins, ncopy, bin, q);
    }
  }
  __syncthreads();
  obs_bins_flush(obs_lds, nbins, ncopy, wsum + p * nbins, counts + p * nbins);
}

// out row of population blockIdx.x: {m, sum w, sum w v, sum w v^2, n_bad, n_neg_inf}; ONE block, the thread stride, wave
// reduction and partial order of logweight_stats_block (sampler_kernels.hip), so the bits depend on the row order inside
// the population and on nothing else.  A walker is left out (n_bad) when its log-weight is NaN or +inf or its value is
// not finite; of the others, those with log-weight -inf have weight 0 (n_neg_inf).  m is the maximum over ALL finite
// log-weights of the population, as in the histograms.
__global__ void __launch_bounds__(OBS_ST) weighted_moments_kernel(const float* __restrict__ v, const float* __restrict__ logw,
                                                                  long long S, double* __restrict__ out) {
  __shared__ double s_s[3][OBS_SW];
  __shared__ float s_mx[OBS_SW];
  __shared__ unsigned long long s_bad[OBS_SW], s_ninf[OBS_SW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long p = blockIdx.x;
  const float* vp = v + p * S;
  const float* a = logw ? logw + p * S : nullptr;
  float mx = -INFINITY;
  unsigned long long bad = 0, ninf = 0;
  for (long long i = t; i < S; i += OBS_ST) {
    const float l = a ? a[i] : 0.0f, val = vp[i];
    const bool lfin = l == l && fabsf(l) != INFINITY;
    if (a && lfin) mx = fmaxf(mx, l);
    if (l != l || l == INFINITY || !(val == val && fabsf(val) != INFINITY)) ++bad;
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
  for (int k = 0; k < OBS_SW; ++k) { mx = fmaxf(mx, s_mx[k]); bad += s_bad[k]; ninf += s_ninf[k]; }
  const double m = mx > -INFINITY ? (double)mx : 0.0;

  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long i = t; i < S; i += OBS_ST) {
    const float l = a ? a[i] : 0.0f, val = vp[i];
    if (l == l && fabsf(l) != INFINITY && val == val && fabsf(val) != INFINITY) {
      const double w = a ? exp((double)l - m) : 1.0, wx = w * (double)val;
      s0 += w;
      s1 += wx;
      s2 = fma(wx, (double)val, s2);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64);
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  if (lane == 0) { s_s[0][wv] = s0; s_s[1][wv] = s1; s_s[2][wv] = s2; }
  __syncthreads();
  if (t == 0) {
    s0 = 0.0; s1 = 0.0; s2 = 0.0;
    for (int k = 0; k < OBS_SW; ++k) { s0 += s_s[0][k]; s1 += s_s[1][k]; s2 += s_s[2][k]; }
    double* o = out + 6 * p;
    o[0] = m; o[1] = s0; o[2] = s1; o[3] = s2; o[4] = (double)bad; o[5] = (double)ninf;
  }
}

// ---- dihedral angles (pita_hip.h: pita_dihedral_angles, pita_dihedral_histogram2d)
constexpr int DIH_ANGLE_W = 64, DIH_ANGLE_FLOATS = 4096;  // walkers / coordinates an angle block stages at most
constexpr int DIH_HIST_W = OBS_T, DIH_HIST_FLOATS = 8192;  // the same for a 2-D histogram block: one walker per thread
constexpr int DIH_MAX_DIH = 1024, DIH_MAX_PAIRS = 64, DIH_MAX_CELLS = 4096, DIH_MAX_ATOMS = 256;
constexpr int DIH_GRID = 512;  // blocks a 2-D histogram launch aims at: each clears and flushes up to 2 * 4096 cells

__device__ __forceinline__ float dih_dot(const float (&a)[3], const float (&b)[3]) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}
__device__ __forceinline__ void dih_cross(float (&n)[3], const float (&a)[3], const float (&b)[3]) {
  n[0] = __fsub_rn(__fmul_rn(a[1], b[2]), __fmul_rn(a[2], b[1]));
  n[1] = __fsub_rn(__fmul_rn(a[2], b[0]), __fmul_rn(a[0], b[2]));
  n[2] = __fsub_rn(__fmul_rn(a[0], b[1]), __fmul_rn(a[1], b[0]));
}
// Torsion angle in [-pi, pi] of the atoms q[0 .. 3] = (i, j, k, l) of one walker, r = its 3-D coordinates: the force
// field's formula and sign (ff_kernel.hip), in fp32 with every operation rounded on its own, in this order:
//   b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k;  n1 = b1 x b2, n2 = b2 x b3;
//   y = (b1 . n2) * sqrt(b2 . b2) (the root correctly rounded), xv = n1 . n2, dots as ((p0 + p1) + p2);  atan2f(y, xv).
// Collinear atoms give atan2f of two zeros, 0 (pi where xv is -0), a value like any other; NaN where y or xv is not
// finite (a non-finite coordinate among the four atoms, or products beyond the fp32 range).
__device__ __forceinline__ float dihedral_angle(const float* r, const int* q) {
  const float *xi = r + 3 * q[0], *xj = r + 3 * q[1], *xk = r + 3 * q[2], *xl = r + 3 * q[3];
  float b1[3], b2[3], b3[3], n1[3], n2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    b1[c] = __fsub_rn(xj[c], xi[c]);
    b2[c] = __fsub_rn(xk[c], xj[c]);
    b3[c] = __fsub_rn(xl[c], xk[c]);
  }
  dih_cross(n1, b1, b2);
  dih_cross(n2, b2, b3);
  const float y = __fmul_rn(dih_dot(b1, n2), (float)sqrt((double)dih_dot(b2, b2)));
  const float xv = dih_dot(n1, n2);
  if (!(fabsf(y) < INFINITY && fabsf(xv) < INFINITY)) return __uint_as_float(0x7fc00000u);
  return atan2f(y, xv);
}

// Block b takes the chunks b, b + gridDim.x, ... of W walkers: their rows are staged in LDS by coalesced reads (a
// thread that gathered its twelve floats from global memory would use a fraction of every line), then the threads
// stride over the (walker, dihedral) items, so that the stores are coalesced too.
__global__ void __launch_bounds__(OBS_T) dihedral_angles_kernel(const float* __restrict__ x, long long B, int D,
                                                                const int* __restrict__ quads, int n_dih, int W,
                                                                float* __restrict__ out) {
  extern __shared__ unsigned long long obs_lds[];  // [n_dih * 4] atoms | [W * D] coordinates
  int* qd = reinterpret_cast<int*>(obs_lds);
  float* xs = reinterpret_cast<float*>(qd + 4 * n_dih);
  for (int i = threadIdx.x; i < 4 * n_dih; i += OBS_T) qd[i] = quads[i];
  const long long chunks = (B + W - 1) / W;
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    const long long w0 = c * W;
    const int nw = (int)(B - w0 < W ? B - w0 : W);
    __syncthreads();  // the previous chunk has been consumed (first pass: the atoms are in place)
    const float* src = x + w0 * D;
    for (int i = threadIdx.x; i < nw * D; i += OBS_T) xs[i] = src[i];
    __syncthreads();
    float* dst = out + w0 * n_dih;
    const unsigned items = (unsigned)(nw * n_dih);
    for (unsigned it = threadIdx.x; it < items; it += OBS_T) {
      const unsigned w = it / (unsigned)n_dih, k = it - w * (unsigned)n_dih;
      dst[it] = dihedral_angle(xs + w * (unsigned)D, qd + 4 * k);
    }
  }
}

// Block blockIdx.x = (p * n_pair + pr) * bpp + b: pair pr of population p, the chunks b, b + bpp, ... of W walkers.  The
// rows of a chunk and its fixed-point weights are staged as above; thread t takes walker t of the chunk, computes the two
// angles of the pair (never written to memory), bins each on its own axis and adds to cell ia * nb + ib.
__global__ void __launch_bounds__(OBS_T) dihedral_histogram2d_kernel(const float* __restrict__ x, const float* __restrict__ logw,
                                                                     long long S, int D, const int* __restrict__ quads,
                                                                     int n_pair, int W, int bpp,
                                                                     const float* __restrict__ edges_a, int na,
                                                                     const float* __restrict__ edges_b, int nb, int shift,
                                                                     const unsigned long long* __restrict__ info,
                                                                     unsigned long long* __restrict__ wsum,
                                                                     unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned long long obs_lds[];  // cells | [W] q | [na + 1], [nb + 1] edges | [W * D] coordinates
  const int ncell = na * nb, ncopy = obs_ncopy(ncell);
  unsigned long long* qs = obs_lds + 2 * ncopy * ncell;
  float* ea = reinterpret_cast<float*>(qs + W);
  float* eb = ea + na + 1;
  float* xs = eb + nb + 1;
  obs_bins_clear(obs_lds, ncell, ncopy);
  for (int i = threadIdx.x; i <= na; i += OBS_T) ea[i] = edges_a[i];
  for (int i = threadIdx.x; i <= nb; i += OBS_T) eb[i] = edges_b[i];
  __syncthreads();
  const long long g = blockIdx.x / bpp, b = blockIdx.x % bpp;  // g = p * n_pair + pr: the cell array of the block
  const long long p = g / n_pair;
  const int* q8 = quads + 8 * (g % n_pair);
  int qa[4], qb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { qa[k] = q8[k]; qb[k] = q8[4 + k]; }
  const float* lw = logw ? logw + p * S : nullptr;
  const double m = obs_key_max(info[4 * p]);
  const float lo_a = ea[0], hi_a = ea[na], inv_a = (float)na / (hi_a - lo_a);
  const float lo_b = eb[0], hi_b = eb[nb], inv_b = (float)nb / (hi_b - lo_b);
  const long long chunks = (S + W - 1) / W;
  for (long long c = b; c < chunks; c += bpp) {
    const long long w0 = c * W;
    const int nw = (int)(S - w0 < W ? S - w0 : W);
    __syncthreads();  // the previous chunk has been consumed
    const float* src = x + (p * S + w0) * D;
    for (int i = threadIdx.x; i < nw * D; i += OBS_T) xs[i] = src[i];
    for (int i = threadIdx.x; i < nw; i += OBS_T) qs[i] = obs_weight_q(lw, w0 + i, m, shift);
    __syncthreads();
    for (int w = threadIdx.x; w < nw; w += OBS_T) {
      const unsigned long long q = qs[w];
      if (q == OBS_LEFT_OUT) continue;
      const float* r = xs + w * D;
      const int ia = hist_bin(dihedral_angle(r, qa), ea, na, lo_a, hi_a, inv_a);
      if (ia < 0) continue;
      const int ib = hist_bin(dihedral_angle(r, qb), eb, nb, lo_b, hi_b, inv_b);
      if (ib >= 0) obs_bins_add(obs_lds, ncell, ncopy, ia * nb + ib, q);
    }
  }
  __syncthreads();
  obs_bins_flush(obs_lds, ncell, ncopy, wsum + g * ncell, counts + g * ncell);
}

// shift = min(40, 62 - ceil(log2(pop_size * values_per_walker))), or -1 where that is below 20 (the product above 2^42)
int obs_shift(int64_t pop_size, int64_t values_per_walker) {
  const int64_t cap = (int64_t)1 << (62 - OBS_MIN_SHIFT);
  if (values_per_walker > cap / pop_size) return -1;
  const uint64_t nv = (uint64_t)pop_size * (uint64_t)values_per_walker;
  int c = 0;
  while (((uint64_t)1 << c) < nv) ++c;
  return 62 - c > OBS_MAX_SHIFT ? OBS_MAX_SHIFT : 62 - c;
}

// blocks per population: at most `want`, about `grid` blocks in all
int obs_blocks_per_pop(int64_t n_pop, int64_t want, int grid = OBS_GRID) {
  const int64_t cap = n_pop >= grid ? 1 : grid / n_pop;
  return (int)(want < cap ? (want < 1 ? 1 : want) : cap);
}

// Zeroes the outputs and launches the pass over the log-weights (none for unit weights: the zeroed rows already say "no
// finite entry, no counts"); the caller launches its histogram next and ends with obs_finish.
int obs_prepare(const float* logw, int64_t n_pop, int64_t pop_size, int nbins, unsigned long long* wsum,
                unsigned long long* counts, double* info, hipStream_t s) {
  PITA_HIP_CHECK(hipMemsetAsync(wsum, 0, sizeof(unsigned long long) * (size_t)n_pop * nbins, s));
  PITA_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * (size_t)n_pop * nbins, s));
  PITA_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(double) * 4 * (size_t)n_pop, s));
  if (!logw) return PITA_OK;
  const int bpi = obs_blocks_per_pop(n_pop, (pop_size + 32 * OBS_T - 1) / (32 * OBS_T));
  hipLaunchKernelGGL(obs_info_kernel, dim3((unsigned)(n_pop * bpi)), dim3(OBS_T), 0, s, logw, (long long)pop_size, bpi,
                     reinterpret_cast<unsigned long long*>(info));
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

int obs_finish(double* info, int64_t n_pop, int shift, hipStream_t s) {
  hipLaunchKernelGGL(obs_info_finish_kernel, dim3((unsigned)((n_pop + OBS_T - 1) / OBS_T)), dim3(OBS_T), 0, s, info,
                     (long long)n_pop, shift);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

}  // namespace

#define OBS_REQUIRE_SUPPORTED(cond, ...)                                  \
  do {                                                                    \
    if (!(cond)) return ::pita::fail(PITA_EUNSUPPORTED, __VA_ARGS__);     \
  } while (0)

extern "C" int pita_weighted_histogram(const float* v, const float* logw, int64_t n_pop, int64_t pop_size, int64_t per_walker,
                                       const float* edges, int nbins, unsigned long long* wsum, unsigned long long* counts,
                                       double* info, void* stream) {
  PITA_REQUIRE(v && edges && wsum && counts && info, "pita_weighted_histogram: null v, edges, wsum, counts or info");
  PITA_REQUIRE(n_pop >= 1 && pop_size >= 1 && per_walker >= 1,
               "pita_weighted_histogram: n_pop, pop_size and per_walker must be >= 1 (got %lld, %lld, %lld)", (long long)n_pop,
               (long long)pop_size, (long long)per_walker);
  PITA_REQUIRE(nbins >= 1 && nbins <= HIST_MAX_BINS, "pita_weighted_histogram: 1 <= nbins <= %d (got %d)", HIST_MAX_BINS, nbins);
  const int shift = obs_shift(pop_size, per_walker);
  OBS_REQUIRE_SUPPORTED(shift >= OBS_MIN_SHIFT,
                        "pita_weighted_histogram: pop_size * per_walker = %lld * %lld leaves a fixed-point shift below %d",
                        (long long)pop_size, (long long)per_walker, OBS_MIN_SHIFT);
  const int64_t nv = pop_size * per_walker;
  const int bpp = obs_blocks_per_pop(n_pop, (nv + 4 * OBS_T - 1) / (4 * OBS_T));
  OBS_REQUIRE_SUPPORTED(n_pop <= INT64_MAX / nv && n_pop <= INT_MAX / bpp, "pita_weighted_histogram: n_pop = %lld is too large",
                        (long long)n_pop);
  hipStream_t s = (hipStream_t)stream;
  const int rc = obs_prepare(logw, n_pop, pop_size, nbins, wsum, counts, info, s);
  if (rc != PITA_OK) return rc;
  const size_t lds = sizeof(unsigned long long) * 2 * obs_ncopy(nbins) * (size_t)nbins + sizeof(float) * ((size_t)nbins + 1);
  hipLaunchKernelGGL(weighted_histogram_kernel, dim3((unsigned)(n_pop * bpp)), dim3(OBS_T), lds, s, v, logw, (long long)pop_size,
                     (long long)per_walker, bpp, edges, nbins, shift, reinterpret_cast<const unsigned long long*>(info), wsum,
                     counts);
  PITA_LAUNCH_CHECK();
  return obs_finish(info, n_pop, shift, s);
}

extern "C" int pita_pair_distance_histogram(const float* x, const float* logw, int64_t n_pop, int64_t pop_size, int n_particles,
                                            int n_dim, const float* edges, int nbins, unsigned long long* wsum,
                                            unsigned long long* counts, double* info, void* stream) {
  PITA_REQUIRE(x && edges && wsum && counts && info, "pita_pair_distance_histogram: null x, edges, wsum, counts or info");
  PITA_REQUIRE(n_pop >= 1 && pop_size >= 1, "pita_pair_distance_histogram: n_pop and pop_size must be >= 1 (got %lld, %lld)",
               (long long)n_pop, (long long)pop_size);
  PITA_REQUIRE(n_particles >= 2 && n_particles <= 256 && n_dim >= 1 && n_dim <= 3,
               "pita_pair_distance_histogram: 2 <= n_particles <= 256 and 1 <= n_dim <= 3 (got %d, %d)", n_particles, n_dim);
  PITA_REQUIRE(nbins >= 1 && nbins <= HIST_MAX_BINS, "pita_pair_distance_histogram: 1 <= nbins <= %d (got %d)", HIST_MAX_BINS,
               nbins);
  const int64_t npairs = (int64_t)n_particles * (n_particles - 1) / 2;
  const int shift = obs_shift(pop_size, npairs);
  OBS_REQUIRE_SUPPORTED(shift >= OBS_MIN_SHIFT,
                        "pita_pair_distance_histogram: pop_size * pairs = %lld * %lld leaves a fixed-point shift below %d",
                        (long long)pop_size, (long long)npairs, OBS_MIN_SHIFT);
  const int D = n_particles * n_dim;
  int W = OBS_PAIR_FLOATS / D < OBS_PAIR_W ? OBS_PAIR_FLOATS / D : OBS_PAIR_W;  // >= 5: D <= 768
  if (pop_size < W) W = (int)pop_size;
  const int bpp = obs_blocks_per_pop(n_pop, (pop_size + W - 1) / W, OBS_GRID_PAIRS);
  OBS_REQUIRE_SUPPORTED(n_pop <= INT64_MAX / (pop_size * npairs) && n_pop <= INT_MAX / bpp,
                        "pita_pair_distance_histogram: n_pop = %lld is too large", (long long)n_pop);
  hipStream_t s = (hipStream_t)stream;
  const int rc = obs_prepare(logw, n_pop, pop_size, nbins, wsum, counts, info, s);
  if (rc != PITA_OK) return rc;
  const size_t lds = sizeof(unsigned long long) * (2 * obs_ncopy(nbins) * (size_t)nbins + (size_t)W) +
                     sizeof(float) * ((size_t)nbins + 1 + (size_t)W * D);
  hipLaunchKernelGGL(pair_distance_histogram_kernel, dim3((unsigned)(n_pop * bpp)), dim3(OBS_T), lds, s, x, logw,
                     (long long)pop_size, n_particles, n_dim, W, bpp, edges, nbins, shift,
                     reinterpret_cast<const unsigned long long*>(info), wsum, counts);
  PITA_LAUNCH_CHECK();
  return obs_finish(info, n_pop, shift, s);
}

extern "C" int pita_weighted_moments(const float* v, const float* logw, int64_t n_pop, int64_t pop_size, double* out,
                                     void* stream) {
  PITA_REQUIRE(v && out, "pita_weighted_moments: null v or out");
  PITA_REQUIRE(n_pop >= 1 && pop_size >= 1, "pita_weighted_moments: n_pop and pop_size must be >= 1 (got %lld, %lld)",
               (long long)n_pop, (long long)pop_size);
  OBS_REQUIRE_SUPPORTED(n_pop <= INT_MAX && n_pop <= INT64_MAX / pop_size, "pita_weighted_moments: n_pop = %lld is too large",
                        (long long)n_pop);
  hipLaunchKernelGGL(weighted_moments_kernel, dim3((unsigned)n_pop), dim3(OBS_ST), 0, (hipStream_t)stream, v, logw,
                     (long long)pop_size, out);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_dihedral_angles(const float* x, int64_t B, int n_atoms, const int32_t* quads, int n_dih, float* out,
                                    void* stream) {
  PITA_REQUIRE(quads && B >= 0 && (B == 0 || (x && out)), "pita_dihedral_angles: null x, quads or out, or B = %lld < 0",
               (long long)B);
  PITA_REQUIRE(n_atoms >= 4 && n_atoms <= DIH_MAX_ATOMS && n_dih >= 1 && n_dih <= DIH_MAX_DIH,
               "pita_dihedral_angles: 4 <= n_atoms <= %d and 1 <= n_dih <= %d (got %d, %d)", DIH_MAX_ATOMS, DIH_MAX_DIH,
               n_atoms, n_dih);
  const int D = 3 * n_atoms;
  OBS_REQUIRE_SUPPORTED(B <= INT64_MAX / (D > n_dih ? D : n_dih), "pita_dihedral_angles: B = %lld is too large", (long long)B);
  if (B == 0) return PITA_OK;
  int W = DIH_ANGLE_FLOATS / D < DIH_ANGLE_W ? DIH_ANGLE_FLOATS / D : DIH_ANGLE_W;  // >= 5: D <= 768
  if (B < W) W = (int)B;
  const size_t lds = sizeof(int) * 4 * (size_t)n_dih + sizeof(float) * (size_t)W * D;
  hipLaunchKernelGGL(dihedral_angles_kernel, dim3(capped_grid((B + W - 1) / W, kGridCus * 8)), dim3(OBS_T), lds,
                     (hipStream_t)stream, x, (long long)B, D, quads, n_dih, W, out);
  PITA_LAUNCH_CHECK();
  return PITA_OK;
}

extern "C" int pita_dihedral_histogram2d(const float* x, const float* logw, int64_t n_pop, int64_t pop_size, int n_atoms,
                                         const int32_t* quads, int n_pair, const float* edges_a, int nbins_a,
                                         const float* edges_b, int nbins_b, unsigned long long* wsum,
                                         unsigned long long* counts, double* info, void* stream) {
  PITA_REQUIRE(x && quads && edges_a && edges_b && wsum && counts && info,
               "pita_dihedral_histogram2d: null x, quads, edges_a, edges_b, wsum, counts or info");
  PITA_REQUIRE(n_pop >= 1 && pop_size >= 1, "pita_dihedral_histogram2d: n_pop and pop_size must be >= 1 (got %lld, %lld)",
               (long long)n_pop, (long long)pop_size);
  PITA_REQUIRE(n_atoms >= 4 && n_atoms <= DIH_MAX_ATOMS && n_pair >= 1 && n_pair <= DIH_MAX_PAIRS,
               "pita_dihedral_histogram2d: 4 <= n_atoms <= %d and 1 <= n_pair <= %d (got %d, %d)", DIH_MAX_ATOMS,
               DIH_MAX_PAIRS, n_atoms, n_pair);
  PITA_REQUIRE(nbins_a >= 1 && nbins_b >= 1, "pita_dihedral_histogram2d: nbins_a and nbins_b must be >= 1 (got %d, %d)",
               nbins_a, nbins_b);
  OBS_REQUIRE_SUPPORTED((int64_t)nbins_a * nbins_b <= DIH_MAX_CELLS,
                        "pita_dihedral_histogram2d: nbins_a * nbins_b = %d * %d is above the limit of %d cells (64 x 64: a "
                        "block keeps the sums and counts of its cells in LDS)", nbins_a, nbins_b, DIH_MAX_CELLS);
  const int shift = obs_shift(pop_size, 1);
  OBS_REQUIRE_SUPPORTED(shift >= OBS_MIN_SHIFT, "pita_dihedral_histogram2d: pop_size = %lld leaves a fixed-point shift below %d",
                        (long long)pop_size, OBS_MIN_SHIFT);
  const int D = 3 * n_atoms, ncell = nbins_a * nbins_b;
  int W = DIH_HIST_FLOATS / D < DIH_HIST_W ? DIH_HIST_FLOATS / D : DIH_HIST_W;  // >= 10: D <= 768
  if (pop_size < W) W = (int)pop_size;
  const int64_t groups_max = INT_MAX / ((int64_t)n_pair * ncell);  // the cell arrays of all populations: an int for obs_prepare
  OBS_REQUIRE_SUPPORTED(n_pop <= groups_max && n_pop <= INT64_MAX / pop_size / D,
                        "pita_dihedral_histogram2d: n_pop = %lld is too large", (long long)n_pop);
  const int64_t groups = n_pop * n_pair;
  const int bpp = obs_blocks_per_pop(groups, (pop_size + W - 1) / W, DIH_GRID);
  OBS_REQUIRE_SUPPORTED(groups <= INT_MAX / bpp, "pita_dihedral_histogram2d: n_pop = %lld is too large", (long long)n_pop);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = sizeof(unsigned long long) * (2 * obs_ncopy(ncell) * (size_t)ncell + (size_t)W) +
                     sizeof(float) * ((size_t)nbins_a + nbins_b + 2 + (size_t)W * D);
  PITA_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void*>(dihedral_histogram2d_kernel), lds));
  const int rc = obs_prepare(logw, n_pop, pop_size, n_pair * ncell, wsum, counts, info, s);
  if (rc != PITA_OK) return rc;
  hipLaunchKernelGGL(dihedral_histogram2d_kernel, dim3((unsigned)(groups * bpp)), dim3(OBS_T), lds, s, x, logw,
                     (long long)pop_size, D, quads, n_pair, W, bpp, edges_a, nbins_a, edges_b, nbins_b, shift,
                     reinterpret_cast<const unsigned long long*>(info), wsum, counts);
  PITA_LAUNCH_CHECK();
  return obs_finish(info, n_pop, shift, s);
}
