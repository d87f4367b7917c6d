// Parameter blocks shared by the pair-target kernels (energy_kernels.hip, ring_kernels.hip).
#pragma once
#include "common.h"

namespace pita {

enum { E_LJ = 0, E_DW = 1, E_LJS = 2 };  // E_LJS: LJ with the reference's cubic core below range_min (smooth=True)
template <int KIND> constexpr bool is_lj() { return KIND == E_LJ || KIND == E_LJS; }

struct PairParams {
  float inv_T, energy_factor, dist_eps, eps, rm2, osc_scale;  // LJ
  float cw, co;  // LJ fast paths: -inv_T * 24 ef eps / rm^2 (pair force weight), -inv_T * osc_scale
  float a, b, c, d0;                                          // DW
  float sm_min, sc0, sc1, sc2, sc3;  // E_LJS: below r = sm_min the pair energy is sc0 u^3 + sc1 u^2 + sc2 u + sc3, u = r - sm_min
};

struct DescentParams {
  float dt, noise_scale, sqrt_dt;
  int nsteps, remove_mean;
  unsigned long long seed, walker_offset;
  long long step0;
};

struct MalaParams {
  const float* noise;      // nullable [nsteps, B, n*d]
  const float* uniforms;   // nullable [nsteps, B]
  const long long* walker_ids;
  unsigned long long seed, walker_offset;
  long long step0, total;
  const double* dt_dev;
  int step_base, steps;      // this launch runs steps [step_base, step_base + steps) of the chain (adaptive: steps == 1)
  int adaptive, remove_mean;
  unsigned long long* sync;  // [chain steps] walkers accepted per step, added with an integer atomic; zeroed by the wrapper
};

// The per-population chain (pita_*_mala_pop): every population of pop_size consecutive Philox keys has its own step size,
// acceptance count and adaptation.  Population of a row: (key - pop_base) / pop_size, in [0, n_pop) by the caller's
// construction.  dt_dev is then [n_pop], sync [chain steps][n_pop], and `total` is not read (totals[pop] is).
struct MalaPopParams : MalaParams {
  const long long* totals;  // [n_pop] walkers the rates of a population are taken over
  double* dt_step;          // [2][n_pop] in the workspace: the step sizes of an adaptive chain's last two steps (mala_replay_dt)
  unsigned long long pop_base;
  long long pop_size;
  int n_pop;
};
template <bool POP> using MalaQ = std::conditional_t<POP, MalaPopParams, MalaParams>;

// The parameter blocks from the arguments of the C entry points: every pita_lj_* / pita_dw_* call builds its block here.
// (cw / co are read by the LJ13 and ring kernels only; no E_LJS instantiation reads them.)
inline PairParams lj_params(float temperature, float energy_factor, float dist_eps, float eps, float rm, float osc_scale) {
  PairParams p{};
  p.inv_T = 1.0f / temperature; p.energy_factor = energy_factor; p.dist_eps = dist_eps; p.eps = eps;
  p.rm2 = rm * rm; p.osc_scale = osc_scale;
  p.cw = -p.inv_T * (2.0f * energy_factor * eps * 12.0f / p.rm2); p.co = -p.inv_T * osc_scale;
  return p;
}
inline PairParams dw_params(float temperature, float a, float b, float c, float d0) {
  PairParams p{};
  p.inv_T = 1.0f / temperature; p.a = a; p.b = b; p.c = c; p.d0 = d0;
  return p;
}
// the caller's share of a chain's parameters; run_mala_chain fills in the launch's step range
inline MalaParams mala_params(const float* noise, const float* uniforms, const int64_t* walker_ids, uint64_t seed,
                              uint64_t walker_offset, int64_t step0, int64_t total, const double* dt_dev, int adaptive,
                              int remove_mean, void* workspace) {
  MalaParams q{};
  q.noise = noise; q.uniforms = uniforms; q.walker_ids = (const long long*)walker_ids; q.seed = seed;
  q.walker_offset = walker_offset; q.step0 = step0; q.total = total; q.dt_dev = dt_dev;
  q.adaptive = adaptive ? 1 : 0; q.remove_mean = remove_mean; q.sync = static_cast<unsigned long long*>(workspace);
  return q;
}

// (the workspace behind chain.sync: nsteps x n_pop counters, the spare slot, then dt_step)
inline MalaPopParams mala_pop_params(const MalaParams& chain, int nsteps, const int64_t* totals, int n_pop, int64_t pop_size,
                                     uint64_t pop_base) {
  MalaPopParams q{};
  static_cast<MalaParams&>(q) = chain;
  q.totals = (const long long*)totals; q.pop_base = pop_base; q.pop_size = pop_size; q.n_pop = n_pop;
  q.dt_step = reinterpret_cast<double*>(q.sync + (size_t)(nsteps > 0 ? nsteps : 0) * (size_t)n_pop + 1);
  return q;
}

#ifdef __HIPCC__
// Step size of chain step `step_base` of a fused chain: dt_dev[0] as the chain found it and, when adaptive,
// mala_adapt_kernel's rule (sampler_kernels.hip; sde_integration.py:439-443) replayed over the accepted counts
// sync[0 .. step_base) of the steps before, which earlier launches of the stream left.  rates_out, when given, receives
// the acceptance rates of those steps.
__device__ __forceinline__ double mala_replay_dt(const double* dt_dev, const unsigned long long* sync, int step_base,
                                                 long long total, int adaptive, float* rates_out = nullptr) {
  double dt = dt_dev[0];
  if (adaptive || rates_out)
    for (int s = 0; s < step_base; ++s) {
      const float rate = (float)(int)sync[s] / (float)total;
      if (rates_out) rates_out[s] = rate;
      if (adaptive) dt = ((double)rate > 0.55) ? dt * 1.1 : dt / 1.1;
    }
  return dt;
}

// The same for the population of one walker (Philox key `key`).  A walker's population has at least that walker, so
// totals[pop] > 0 here.  The replay is one application of the rule per launch instead of step_base of them (a walker
// cannot share the replay with its block: the block straddles populations): the launch of step s - 1 left its step
// sizes in dt_step[(s - 1) & 1], this one derives its own from them and the counts of step s - 1 -- the same chain of
// double operations from dt_dev[pop] on -- and leaves them in dt_step[s & 1], which no thread of this launch reads; stream
// order makes them visible to the next.  Every walker of a population computes the same value and stores it, once per
// tile: the stores of a wave to one address are one write, and no cross-lane operation means no call site has to be
// converged.
__device__ __forceinline__ int mala_pop_of(const MalaPopParams& q, unsigned long long key) {
  return (int)((key - q.pop_base) / (unsigned long long)q.pop_size);
}
__device__ __forceinline__ double mala_replay_dt(const MalaPopParams& q, int pop) {
  const int s = q.step_base;
  if (!q.adaptive || s == 0) return q.dt_dev[pop];
  double dt = s == 1 ? q.dt_dev[pop] : q.dt_step[(size_t)((s - 1) & 1) * q.n_pop + pop];
  const float rate = (float)(int)q.sync[(long long)(s - 1) * q.n_pop + pop] / (float)q.totals[pop];
  dt = ((double)rate > 0.55) ? dt * 1.1 : dt / 1.1;
  q.dt_step[(size_t)(s & 1) * q.n_pop + pop] = dt;
  return dt;
}

// A wave's accepted walkers split by population before they reach memory: add(pop, count) runs in one lane per distinct
// population among the wave's `live` lanes (one walker each), with the number of those that have `acc`.  Called by every
// lane of the wave.  A block's walkers are consecutive rows, so a wave seldom holds more than two populations.
template <class Add>
__device__ __forceinline__ void mala_count_by_pop(bool live, bool acc, int pop, Add&& add) {
  const int lane = threadIdx.x & 63;
  unsigned long long rem = __ballot(live);
  while (rem) {
    const int lead = __ffsll(rem) - 1;
    const int pl = __shfl(pop, lead, 64);
    const unsigned long long same = __ballot(live && pop == pl);
    const int c = __popcll(__ballot(live && pop == pl && acc));
    if (lane == lead && c) add(pl, c);
    rem &= ~same;
  }
}
#endif

// rates_out[s] and the final dt from the per-step counts of a fused chain (energy_kernels.hip)
int launch_mala_finish(double* dt_dev, const unsigned long long* sync, int nsteps, long long total, int adaptive,
                       float* rates_out, void* stream);

// rates_out[s][p] and the final dt[p] of a per-population chain; a population with totals[p] == 0 keeps its dt and gets
// NaN rates
int launch_mala_finish(double* dt_dev, const unsigned long long* sync, int nsteps, const long long* totals, int n_pop,
                       int adaptive, float* rates_out, void* stream);
inline int launch_mala_finish(double* dt_dev, int nsteps, const MalaParams& q, float* rates_out, void* stream) {
  return launch_mala_finish(dt_dev, q.sync, nsteps, q.total, q.adaptive, rates_out, stream);
}
inline int launch_mala_finish(double* dt_dev, int nsteps, const MalaPopParams& q, float* rates_out, void* stream) {
  return launch_mala_finish(dt_dev, q.sync, nsteps, q.totals, q.n_pop, q.adaptive, rates_out, stream);
}

// workspace of a fused chain: one counter per step (and one spare slot that callers have always sized their buffers with);
// per population: one counter per step and population, and the two rows of MalaPopParams::dt_step
inline size_t mala_workspace_bytes(int nsteps) { return 8 * (size_t)((nsteps > 0 ? nsteps : 0) + 1); }
inline size_t mala_pop_workspace_bytes(int nsteps, int n_pop) {
  const size_t P = (size_t)(n_pop > 0 ? n_pop : 0);
  return 8 * ((size_t)(nsteps > 0 ? nsteps : 0) * P + 1 + 2 * P);  // counters, the spare slot, dt_step
}
inline size_t mala_workspace_bytes(int nsteps, const MalaParams&) { return mala_workspace_bytes(nsteps); }
inline size_t mala_workspace_bytes(int nsteps, const MalaPopParams& q) { return mala_pop_workspace_bytes(nsteps, q.n_pop); }

// What every pita_*_mala_pop entry point checks before any device call.
inline int check_mala_pop_args(const char* who, int64_t B, int nsteps, const double* dt_dev, const int64_t* totals,
                               int n_pop, int64_t pop_size, const void* workspace) {
  PITA_REQUIRE(dt_dev && totals && workspace, "%s: null argument (dt_dev, totals, workspace)", who);
  PITA_REQUIRE(B >= 0 && nsteps >= 0, "%s: bad argument (B >= 0, n_steps >= 0)", who);
  PITA_REQUIRE(n_pop >= 1 && pop_size >= 1, "%s: bad argument (n_pop >= 1, pop_size >= 1)", who);
  PITA_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  return PITA_OK;
}

// The frame of every fused-chain entry point (pita_lj_mala, pita_dw_mala, pita_ff_mala and their _pop variants): zero the per-step counters, run
// the chain, derive rates and final dt.  A non-adaptive chain is one launch; an adaptive chain is one launch per step, and
// the order of the stream is what lets a step see the counts of the steps before it.  launch() starts the kernel for the
// step range it finds in q.
template <class Q, class Launch>
inline int run_mala_chain(int nsteps, double* dt_dev, float* rates_out, Q& q, void* stream, Launch&& launch) {
  PITA_REQUIRE(((uintptr_t)q.sync & 7) == 0, "fused MALA: workspace must be 8-byte aligned");
  PITA_HIP_CHECK(hipMemsetAsync(q.sync, 0, mala_workspace_bytes(nsteps, q), (hipStream_t)stream));
  q.steps = q.adaptive ? 1 : nsteps;
  for (q.step_base = 0; q.step_base < nsteps; q.step_base += q.steps) {
    const int rc = launch();
    if (rc != PITA_OK) return rc;
  }
  return launch_mala_finish(dt_dev, nsteps, q, rates_out, stream);
}

// Ring kernels (ring_kernels.hip): compile-time particle count, a walker's particles on the lanes of one wavefront,
// partner coordinates and partner forces by immediate-offset LDS reads / one cross-lane permute per pair.
// Return PITA_OK when they took the call, 1 when no instantiation covers (n, d, kind, parameters).
int ring_launch_energy(int kind, const float* x, float* logp, float* force, int64_t B, int n, int d, const PairParams& p,
                       void* stream);
int ring_launch_descent(int kind, float* x, const float* noise, int64_t B, int n, int d, const PairParams& p,
                        const DescentParams& q, void* stream);
int ring_launch_mala(int kind, float* x, float* logp, int64_t B, int n, int d, const PairParams& p, MalaParams q,
                     void* stream);
int ring_launch_mala(int kind, float* x, float* logp, int64_t B, int n, int d, const PairParams& p, MalaPopParams q,
                     void* stream);

}  // namespace pita
