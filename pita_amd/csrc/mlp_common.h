// Pieces shared by the MLP kernels (mlp_kernel.hip: forward and fused sampler; mlp_jac_kernel.hip: forward-mode
// derivatives): kernel parameters, the activation / embedding math, the weight-block sources, the handle.
#pragma once
#include "egnn_common.h"

namespace pita {

struct MlpParams {
  const unsigned* w0;   // [NB][KC] blocks of MAT_W words: bf16 three-way split fragments ([piece][k-step][lane][4])
  const unsigned* wl;   // [L][NB][NB] blocks
  const unsigned* wf;   // [NBO][NB] blocks
  const unsigned* stream;  // all blocks once more in the order mlp_tile consumes them (null: emb_size/2 % 32 != 0)
  int S;
  const float* b0;   // [NB][32]  fragment order
  const float* bl;   // [L][NB][32]
  const float* bf;   // [NBO][32]
  const float* freqs;  // [E/2]
  int input_dim, out_dim, n_layers, emb, temp, KC, NBO;
  long long B;
  const float* t;
  const float* x;
  const float* beta;
  float* out;
};

__device__ __forceinline__ f32x16 mlp_bias(const float* b, int hh) {
  const f32x4* p = reinterpret_cast<const f32x4*>(b + hh * 16);
  f32x4 a = p[0], bq = p[1], c = p[2], d = p[3];
  f32x16 r;
  r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = bq.x; r[5] = bq.y; r[6] = bq.z; r[7] = bq.w;
  r[8] = c.x; r[9] = c.y; r[10] = c.z; r[11] = c.w; r[12] = d.x; r[13] = d.y; r[14] = d.z; r[15] = d.w;
  return r;
}

// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, i.e. fp32 rounding level) on v_rcp / v_exp: the library erff
// and sincosf (range reduction of angles up to ~1e4 rad) were 3/4 of the kernel's instructions
__device__ __forceinline__ float erf_as(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
  float pl = 1.061405429f;
  pl = fmaf(pl, t, -1.453152027f);
  pl = fmaf(pl, t, 1.421413741f);
  pl = fmaf(pl, t, -0.284496736f);
  pl = fmaf(pl, t, 0.254829592f);
  const float r = 1.0f - (pl * t) * __builtin_amdgcn_exp2f(-1.44269504088896341f * ax * ax);
  return copysignf(r, x);
}
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erf_as(v * 0.70710678118654752f)); }

// sin and cos of an fp32 angle in radians: the angle itself is the reference's fp32 value; its reduction to one
// revolution is done in fp64 (exact to 1e-13 rev for |angle| < 1e5), then the transcendental unit evaluates
// sin / cos of revolutions (absolute error ~1e-6, two orders below the sensitivity of sin to the fp32 rounding of such
// angles)
__device__ __forceinline__ void sincos_rev(float ang, float& sn, float& cs) {
  const double r = (double)ang * 0.15915494309189535;
  const float f = (float)(r - floor(r));
  sn = __builtin_amdgcn_sinf(f);
  cs = __builtin_amdgcn_cosf(f);
}

// ---- where a tile's weight blocks come from
// GlobalWeights: every wave streams its own copy of each block from L2 (600 KB per 32-walker tile-pass for the
//   128-wide net: the limit of the first version at large batches).
// StreamWeights: the four waves of a workgroup walk the same block sequence in lock step; each block is fetched once
//   per workgroup -- global -> registers while the previous block's MFMAs run, -> LDS, one barrier -- and read from LDS
//   by all four waves (double buffered).  The host packs the blocks in consumption order (`stream`).
struct GlobalWeights {
  const MlpParams& p;
  int lane;
  __device__ __forceinline__ WFrag<1> fetch(const unsigned* base, int idx) {
    WFrag<1> w;
    w.load(nullptr, base, idx, lane);
    return w;
  }
  __device__ __forceinline__ void done() {}
};

struct StreamWeights {
  const unsigned* stream;  // [S][MAT_W]
  unsigned* buf;           // LDS [2][MAT_W]
  int S, s, cur, tid, lane;
  uint2 pre[3];
  __device__ __forceinline__ void prime() {
    const uint2* g = reinterpret_cast<const uint2*>(stream);
    uint2* l = reinterpret_cast<uint2*>(buf);
#pragma unroll
    for (int q = 0; q < 3; ++q) l[tid + 256 * q] = g[tid + 256 * q];
    s = 0;
    cur = 0;
    __syncthreads();
  }
  __device__ __forceinline__ WFrag<1> fetch(const unsigned*, int) {
    const int nxt = (s + 1 == S) ? 0 : s + 1;
    const uint2* g = reinterpret_cast<const uint2*>(stream + (size_t)nxt * MAT_W);
#pragma unroll
    for (int q = 0; q < 3; ++q) pre[q] = g[tid + 256 * q];  // in flight while this block's MFMAs run
    WFrag<1> w;
    const u32x4* pl = reinterpret_cast<const u32x4*>(buf + cur * MAT_W) + lane;
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
#pragma unroll
      for (int st = 0; st < 2; ++st) w.w[pc][st] = pl[(pc * 2 + st) * 64];
    return w;
  }
  __device__ __forceinline__ void done() {
    uint2* l = reinterpret_cast<uint2*>(buf + (cur ^ 1) * MAT_W);
#pragma unroll
    for (int q = 0; q < 3; ++q) l[tid + 256 * q] = pre[q];
    __syncthreads();  // next block visible; everybody has read the current one
    cur ^= 1;
    s = (s + 1 == S) ? 0 : s + 1;
  }
};

}  // namespace pita

struct pita_mlp {
  pita_mlp_config cfg;
  float* d_all = nullptr;
  pita::MlpParams p{};
};
