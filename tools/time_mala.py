"""Timing of the MALA chain on the LJ13 target: fused launch (pita_lj_mala) against the launch-per-kernel path.
python tools/time_mala.py [B] [steps] [--target lj13|dw4] [--populations P] [--reps R]
--populations P adds a leg on P populations of B / P walkers, adaptive, fused: the coupled chain on the batch (one step
size), the P slice chains one after the other (independent populations as they could be had before) and the
per-population chain (pita_*_mala_pop), alternating, median and min-max over R timed calls each."""
import argparse, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=65536)
ap.add_argument("steps", nargs="?", type=int, default=100)
ap.add_argument("--target", default="lj13", choices=("lj13", "dw4"))
ap.add_argument("--populations", type=int, default=0)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
B, steps = a.B, a.steps
if a.target == "lj13":
    g = dict(np.load(os.path.join(ROOT, "tests/golden/post_lj13.npz")))
    e, DT = pa.LennardJonesEnergy(39, 13, 3), 3e-4
    base = torch.tensor(g["x0"])
    x0 = (base[torch.arange(B) % base.shape[0]] + 0.02 * torch.randn(B, 39)).cuda()
else:
    e, DT = pa.MultiDoubleWellEnergy(temperature=1.0), 0.05
    base = torch.tensor([[2.0, 2.0, -2.0, 2.0, -2.0, -2.0, 2.0, -2.0]])
    x0 = (base + 0.3 * torch.randn(B, 8)).cuda()
for adaptive in (False, True):
    for fused in (True, False):
        integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                         post_mcmc_steps=steps, dt_negative_time=DT, adaptive_mcmc=adaptive, seed=9)
        fn = (lambda: integ.metropolis_hastings_mala_adaptive(x0.clone(), e, dt_init=DT, fused=fused)) if adaptive else \
             (lambda: integ.metropolis_hastings_mala(x0.clone(), e, fused=fused))
        fn(); torch.cuda.synchronize()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
        dt = statistics.median(t)
        print(f"{a.target} B={B} steps={steps} adaptive={adaptive} fused={fused}: {dt / steps * 1e6:.1f} us per MALA step "
              f"(min {min(t) / steps * 1e6:.1f}, max {max(t) / steps * 1e6:.1f}; {2 * B * steps / dt:.3e} target evaluations/s)",
              flush=True)
if a.populations:
    P, S = a.populations, B // a.populations
    assert P * S == B, "B must be a multiple of --populations"
    integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                     post_mcmc_steps=steps, dt_negative_time=DT, adaptive_mcmc=True, seed=9)
    mala = lambda x, off, **kw: integ.metropolis_hastings_mala_adaptive(x, e, dt_init=DT, walker_offset=off, keep_order=True, **kw)
    legs = {"coupled": lambda: mala(x0, 0),
            "slices": lambda: [mala(x0[p * S:(p + 1) * S], p * S) for p in range(P)],
            "per-population": lambda: mala(x0, 0, pop_size=S)}
    t = {k: [] for k in legs}
    for fn in legs.values():
        fn(); torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in legs.items():
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t[k].append((time.perf_counter() - t0) / steps * 1e6)
    for k, v in t.items():
        print(f"{a.target} {P} x {S} walkers steps={steps} adaptive fused, {k}: median {statistics.median(v):.1f} us per MALA step "
              f"(min {min(v):.1f}, max {max(v):.1f})", flush=True)
