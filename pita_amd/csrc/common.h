// Shared host/device helpers for libpita_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/pita_hip.h"

namespace pita {

// ---- error plumbing: thread-local message, integer codes (no exceptions cross the C ABI)
inline char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}
inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}
#define PITA_HIP_CHECK(expr)                                                              \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return ::pita::fail(PITA_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                          __FILE__, __LINE__);                                            \
  } while (0)
#define PITA_LAUNCH_CHECK() PITA_HIP_CHECK(hipGetLastError())
#define PITA_REQUIRE(cond, ...)                                   \
  do {                                                            \
    if (!(cond)) return ::pita::fail(PITA_EINVAL, __VA_ARGS__);   \
  } while (0)

constexpr int kWave = 64;  // CDNA wavefront

// Launch state that HIP keeps PER DEVICE -- the dynamic-LDS opt-in of a kernel (hipFuncSetAttribute), occupancy and CU
// counts -- is cached per device: a process that drives several GPUs (handles carry their device, PitaDeviceGuard) must
// not reuse the first device's answers on the second.
constexpr int kMaxDevices = 32;
inline int current_device_slot() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0) d = 0;
  return d % kMaxDevices;
}
template <class T>
struct PerDevice {
  T v[kMaxDevices] = {};
  T& get() { return v[current_device_slot()]; }
};

// The dynamic-LDS limit of a kernel (hipFuncAttributeMaxDynamicSharedMemorySize) is state of (device, kernel function),
// not of a handle: two handles that share an instantiation but need different sizes (other n_layers / n_particles) must
// not lower each other's limit, and a cache "this handle configured it" goes stale when another handle configures the
// same kernel smaller.  One table per device: kernel -> largest size configured; the attribute is only ever raised.
inline hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes) {
  static std::mutex mu;
  static std::unordered_map<const void*, size_t> configured[kMaxDevices];
  std::lock_guard<std::mutex> lock(mu);
  auto& m = configured[current_device_slot()];
  const auto it = m.find(kernel);
  if (it != m.end() && it->second >= bytes) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) m[kernel] = bytes;
  return e;
}

// Compute units of the current device; the first call per device asks HIP, later calls read the cache.
inline int device_cus(int& cus) {
  static PerDevice<int> cached;
  int& n = cached.get();
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    PITA_HIP_CHECK(hipGetDevice(&dev));
    PITA_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (prop.multiProcessorCount <= 0) return fail(PITA_EHIP, "device %d reports %d compute units", dev, prop.multiProcessorCount);
    n = prop.multiProcessorCount;
  }
  cus = n;
  return PITA_OK;
}

// Resident blocks per compute unit of `kernel` (registers and LDS decide): what the persistent grids multiply by
// device_cus.  Cached per device and kernel like ensure_dynamic_lds; a failed query or an answer of zero is an error.
inline int resident_blocks(const void* kernel, int threads, size_t dynamic_lds, int& blocks) {
  struct Entry { int threads; size_t lds; int blocks; };
  static std::mutex mu;
  static std::unordered_map<const void*, Entry> table[kMaxDevices];
  std::lock_guard<std::mutex> lock(mu);
  auto& m = table[current_device_slot()];
  const auto it = m.find(kernel);
  if (it == m.end() || it->second.threads != threads || it->second.lds != dynamic_lds) {
    int v = 0;
    PITA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, threads, dynamic_lds));
    if (v <= 0) return fail(PITA_EHIP, "a %d-thread block with %zu B of dynamic LDS does not fit a compute unit", threads, dynamic_lds);
    m[kernel] = Entry{threads, dynamic_lds, v};
    blocks = v;
    return PITA_OK;
  }
  blocks = it->second.blocks;
  return PITA_OK;
}
template <class K>
inline int resident_blocks(K* kernel, int threads, size_t dynamic_lds, int& blocks) {
  return resident_blocks(reinterpret_cast<const void*>(kernel), threads, dynamic_lds, blocks);
}

// Grid of a grid-striding kernel: one block per tile up to a cap; the fixed caps are kGridCus * k, k set at the call site.
constexpr long long kGridCus = 256;
inline unsigned capped_grid(long long tiles, long long cap) { return (unsigned)(tiles < cap ? tiles : cap); }

// Run-time value -> template argument of the kernel a generic lambda f names: f(std::integral_constant<int, D>{}) for d
// in [1, MAX] (checked by the caller; MAX takes what is left), f(std::true_type{} / std::false_type{}) for a flag.
template <int MAX, class F>
inline auto dispatch_dim(int d, F&& f) {
  if constexpr (MAX > 1) {
    if (d < MAX) return dispatch_dim<MAX - 1>(d, f);
  }
  return f(std::integral_constant<int, MAX>{});
}
template <class F>
inline auto dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// A handle's scratch buffer grown on demand to at least `bytes` (plus `tail` bytes behind them that the size does not
// count): the stream is drained first (an earlier launch may still use the old buffer), then the buffer is freed and
// allocated anew and its size recorded.  On failure the buffer is null and its size 0; the error is returned.
template <class T>
inline hipError_t grow_scratch(T*& buf, size_t& size, size_t bytes, hipStream_t stream, size_t tail = 0) {
  if (bytes <= size) return hipSuccess;
  hipError_t e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
  (void)hipFree(buf);
  buf = nullptr;
  size = 0;
  e = hipMalloc(&buf, bytes + tail);
  if (e != hipSuccess) {
    buf = nullptr;
    return e;
  }
  size = bytes;
  return hipSuccess;
}

// A device allocation that a handle owns: pointer plus the bytes it was sized for, freed with its owner.  grow() is
// grow_scratch (a scratch buffer); upload() sizes the buffer once and fills it from the host (a fixed allocation).
struct DeviceBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { (void)hipFree(ptr); }
  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
  hipError_t grow(size_t need, hipStream_t stream, size_t tail = 0) { return grow_scratch(ptr, bytes, need, stream, tail); }
  hipError_t upload(const void* host, size_t n) {
    const hipError_t e = grow(n, nullptr);
    return e != hipSuccess ? e : hipMemcpy(ptr, host, n, hipMemcpyHostToDevice);
  }
};

// ---- device math with explicit accuracy choices
// exp2/rcp map to single v_exp_f32 / v_rcp_f32 (about 1 ulp); used where the reference applies
// sigmoid-family activations (relative error ~1e-7, no cancellation).
__device__ __forceinline__ float fast_sigmoid(float v) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * v));
}
__device__ __forceinline__ float fast_silu(float v) { return v * fast_sigmoid(v); }
// tanh with small-argument series: the coordinate head of a fresh EGNN outputs ~1e-4, where
// 1 - 2/(1+e^{2v}) would lose all relative accuracy.
__device__ __forceinline__ float accurate_tanh(float v) {
  // both branches are evaluated and one is selected: the lanes of a wave nearly always need both anyway, and without
  // the divergent branch the callers' loops stay one basic block (same values as the branching form)
  const float a = fabsf(v);
  const float v2 = v * v;
  float p = 62.0f / 2835.0f;
  p = fmaf(p, v2, -17.0f / 315.0f);
  p = fmaf(p, v2, 2.0f / 15.0f);
  p = fmaf(p, v2, -1.0f / 3.0f);
  p = fmaf(p, v2, 1.0f);
  const float e = __builtin_amdgcn_exp2f(2.88539008177792681f * a);  // e^{2a}
  const float t = 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + e);
  return a < 0.25f ? v * p : copysignf(t, v);
}

// ---- Philox4x32-10 counter RNG + Box-Muller (the generator used when the caller passes no noise)
struct Philox {
  static constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  __host__ __device__ static inline void round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    uint64_t p0 = (uint64_t)M0 * c[0], p1 = (uint64_t)M1 * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    uint32_t n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
  }
  __host__ __device__ static inline void gen(uint32_t (&c)[4], uint64_t seed) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      round(c, k0, k1);
      k0 += W0;
      k1 += W1;
    }
  }
};

// Four standard normals for (seed, walker, step, particle).  Counter layout:
// c0,c1 = walker id (64 bit), c2 = step (low 32) , c3 = particle | (step high bits << 20).
__device__ __forceinline__ void philox_normal4(uint64_t seed, uint64_t walker, int64_t step, uint32_t particle,
                                               float (&z)[4]) {
  uint32_t c[4] = {(uint32_t)walker, (uint32_t)(walker >> 32), (uint32_t)step,
                   particle ^ ((uint32_t)((uint64_t)step >> 32) << 20)};
  Philox::gen(c, seed);
  // u in (0,1): 24 random bits + half-ulp offset
  const float s = 1.0f / 16777216.0f;
  float u0 = ((c[0] >> 8) + 0.5f) * s, u1 = ((c[1] >> 8) + 0.5f) * s;
  float u2 = ((c[2] >> 8) + 0.5f) * s, u3 = ((c[3] >> 8) + 0.5f) * s;
  // Box-Muller on the transcendental unit: v_log_f32 is log2, v_sin/v_cos take revolutions (no range reduction
  // needed for u in (0,1)); absolute error of a normal ~1e-6, far below the sampler's fp32 noise floor
  const float kM2Ln2 = -1.38629436111989062f;  // -2 ln 2
  float q0 = kM2Ln2 * __builtin_amdgcn_logf(u0), q1 = kM2Ln2 * __builtin_amdgcn_logf(u2);  // -2 ln u
  // The float32 sum (c >> 8) + 0.5f drops the half-ulp offset for words k >= 2^23 (ties to even): u is a multiple of 2^-24
  // there (1.0 for the last word).  That only matters where 1 - u is a few 2^-24 -- at 2^24 - k = 3 it made r 11 % short,
  // a normal 4.5e-5 off the documented sqrt(-2 ln((k + 0.5) / 2^24)) -- so the last 64 words take -2 ln(1 - e) = 2 e + e^2
  // (+ 2 e^3 / 3 < 1e-16) from e = 1 - u = (2^24 - k - 0.5) / 2^24, which float32 holds exactly.  Every other draw keeps
  // its bits; just above the cut the rounding of u costs a normal at most 1.1e-5.
  const uint32_t t0 = 16777216u - (c[0] >> 8), t1 = 16777216u - (c[2] >> 8);
  const float e0 = ((float)t0 - 0.5f) * s, e1 = ((float)t1 - 0.5f) * s;
  q0 = t0 <= 64u ? e0 * (2.0f + e0) : q0;
  q1 = t1 <= 64u ? e1 * (2.0f + e1) : q1;
  float r0 = __builtin_amdgcn_sqrtf(q0), r1 = __builtin_amdgcn_sqrtf(q1);
  float s0 = __builtin_amdgcn_sinf(u1), c0 = __builtin_amdgcn_cosf(u1);
  float s1 = __builtin_amdgcn_sinf(u3), c1 = __builtin_amdgcn_cosf(u3);
  z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}

// one uniform in (0,1) for (seed, walker, step, tag)
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t walker, int64_t step, uint32_t tag) {
  uint32_t c[4] = {(uint32_t)walker, (uint32_t)(walker >> 32), (uint32_t)step,
                   tag ^ ((uint32_t)((uint64_t)step >> 32) << 20)};
  Philox::gen(c, seed);
  return ((c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
}

// Rademacher signs of one particle's coordinates in Hutchinson probe `probe` (the estimator beside
// compute_divergence_exact in the reference's utils.py): keyed (seed, walker, step) like the normals above, counter tag
// 0x80000 | (probe << 10) | particle in c3; coordinate k of the particle is +1 where bit k of the FIRST output word is set,
// -1 where it is clear (rademacher_sign).  The tag is disjoint from the normals' (particle < 1 024 there) and from the MALA
// uniform's 0xFFFFF under the same key, stays below the step's high bits (bit 20 up) for probe < 256 and particle < 1 024
// -- the callers refuse anything larger --, and depends on neither the batch size nor the walker's place in it.  The ONE
// draw behind pita_rademacher_probes and the probe items of the wide forward-mode kernels.
constexpr int kMaxDrawnProbes = 256, kMaxProbeParticles = 1023;
__device__ __forceinline__ uint32_t philox_rademacher_word(uint64_t seed, uint64_t walker, int64_t step, uint32_t probe,
                                                           uint32_t particle) {
  uint32_t c[4] = {(uint32_t)walker, (uint32_t)(walker >> 32), (uint32_t)step,
                   (0x80000u | (probe << 10) | particle) ^ ((uint32_t)((uint64_t)step >> 32) << 20)};
  Philox::gen(c, seed);
  return c[0];
}
__device__ __forceinline__ float rademacher_sign(uint32_t word, int k) { return ((word >> k) & 1u) ? 1.0f : -1.0f; }

}  // namespace pita

// makes `device` current for the lifetime of the guard (no-op when it already is)
struct PitaDeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit PitaDeviceGuard(int device) {
    if (device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
  }
  ~PitaDeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  PitaDeviceGuard(const PitaDeviceGuard&) = delete;
  PitaDeviceGuard& operator=(const PitaDeviceGuard&) = delete;
};
