"""Timing of the MALA chain on the force-field target (peptides of tests/_peptides.py, GB on, cutoff 0.45 nm): the fused
chain (pita_ff_mala) against the launch-per-kernel path, alternating, in one process.
python tools/time_ff_mala.py [--targets ala2,ala3,ala4] [--batches 4096,16384] [--steps 100] [--reps 5] [--fused-only]
                             [--populations P]
Prints per case the median and min-max of the microseconds per MALA step of both paths.  --fused-only runs each case's
fused chain once after its warm-up (for a kernel trace: launches per chain).  --populations P adds, per case, a leg on P
populations of B / P walkers, adaptive and fused: the coupled chain (one step size), the P slice chains one after the
other, and the per-population chain (pita_ff_mala_pop), alternating."""
import argparse, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
from pita_amd.alp_energy import ForceFieldEnergy
from tests._peptides import peptide
ap = argparse.ArgumentParser()
ap.add_argument("--targets", default="ala2,ala3,ala4")
ap.add_argument("--batches", default="4096,16384")
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fused-only", action="store_true")
ap.add_argument("--populations", type=int, default=0)
a = ap.parse_args()
SCALE, DT = 0.1640, 2e-4
for name in a.targets.split(","):
    tabs, pos = peptide(name)
    n = pos.shape[0]
    e = ForceFieldEnergy(tabs, n_particles=n, temperature=300.0, data_normalization_factor=SCALE, cutoff=0.45)
    for B in (int(b) for b in a.batches.split(",")):
        gen = torch.Generator().manual_seed(B)
        x0 = torch.tensor(pos.reshape(-1), dtype=torch.float32)[None] + 0.004 * torch.randn(B, 3 * n, generator=gen)
        x0 = (x0 / SCALE).reshape(B, n, 3)
        x0 = (x0 - x0.mean(1, keepdim=True)).reshape(B, 3 * n).cuda()
        for adaptive in (False, True):
            integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                             post_mcmc_steps=a.steps, dt_negative_time=DT, adaptive_mcmc=adaptive, seed=9)
            if adaptive:
                fn = lambda fused: integ.metropolis_hastings_mala_adaptive(x0, e, dt_init=DT, fused=fused)
            else:
                fn = lambda fused: integ.metropolis_hastings_mala(x0, e, fused=fused)
            t = {True: [], False: []}
            for fused in ((True,) if a.fused_only else (True, False)):  # warm-up of both paths
                fn(fused); torch.cuda.synchronize()
            for _ in range(1 if a.fused_only else a.reps):
                for fused in ((True,) if a.fused_only else (True, False)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); fn(fused); torch.cuda.synchronize()
                    t[fused].append((time.perf_counter() - t0) / a.steps * 1e6)
            s = lambda v: f"median {statistics.median(v):7.1f} (min {min(v):7.1f}, max {max(v):7.1f})"
            line = f"{name} n={n} B={B} steps={a.steps} adaptive={adaptive}: fused {s(t[True])} us/step"
            if not a.fused_only:
                gain = statistics.median(t[False]) - statistics.median(t[True])
                spread = max(t[False]) - min(t[False])
                line += (f" | per-kernel {s(t[False])} us/step | gain {gain:6.1f} us/step, per-kernel spread {spread:5.1f}: "
                         f"{'beyond the spread' if gain > spread else 'WITHIN THE NOISE' if gain >= 0 else 'FUSED SLOWER'}")
            print(line, flush=True)
        if a.populations:
            P, S = a.populations, B // a.populations
            assert P * S == B, "every batch must be a multiple of --populations"
            mala = lambda x, off, **kw: integ.metropolis_hastings_mala_adaptive(x, e, dt_init=DT, walker_offset=off,
                                                                                keep_order=True, **kw)  # integ: the adaptive one
            legs = {"coupled": lambda: mala(x0, 0), "slices": lambda: [mala(x0[p * S:(p + 1) * S], p * S) for p in range(P)],
                    "per-population": lambda: mala(x0, 0, pop_size=S)}
            t = {k: [] for k in legs}
            for fn in legs.values():
                fn(); torch.cuda.synchronize()
            for _ in range(a.reps):
                for k, fn in legs.items():
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                    t[k].append((time.perf_counter() - t0) / a.steps * 1e6)
            for k, v in t.items():
                print(f"{name} n={n} {P} x {S} walkers steps={a.steps} adaptive fused, {k}: median {statistics.median(v):7.1f} "
                      f"(min {min(v):7.1f}, max {max(v):7.1f}) us/step", flush=True)
