"""Timing of resampling events over P independent populations of S = 2 048 LJ13 walkers (39 coordinates), P = 1, 8, 32.

(a) one event on the P * S walkers, through the C ABI on preallocated buffers (what is timed is the launches):
      fixed        pita_systematic_resample + pita_count_runs + pita_gather_rows on the whole batch (seven launches)
      adaptive     pita_adaptive_resample on the whole batch (one launch up to 2 048 walkers, gated passes above) + gather
      populations  pita_population_resample (one launch, one block per population) + gather
    the last two with theta = 1 (every event resamples) and theta = 0 (none does on these weights).  Warm-up, then
    alternating windows of `reps` events in one process, each window between two device events; median [min, max].
    At P = 1 the population event is checked against pita_adaptive_resample bit for bit before anything is timed.
(b) LJ13 in the debiased regime (hidden-32 EGNN, exact divergence, an event every second step, ess_threshold 0.5): one
    integrate_sde of P x 2 048 walkers with populations=P against P consecutive integrate_sde calls of 2 048 walkers
    (populations=None), alternating, host wall time between two synchronisations -- the host work of a run is part of what
    a user waits for --, in ms per population-step (time / (P * steps)); median [min, max].
usage: python tools/time_populations.py [reps] [rounds] [steps] [--pops 1,8,32] [--integrate-only] [--root DIR]; the
committed profile is the second of two runs.  ``--integrate-only``: (b) alone, for every P of ``--pops``; ``--root``: the
tree whose pita_amd is imported (host-cost comparisons of two trees on one library)."""
import argparse, copy, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=1000)
ap.add_argument("rounds", nargs="?", type=int, default=7)
ap.add_argument("steps", nargs="?", type=int, default=8)
ap.add_argument("--pops", default="1,8,32")
ap.add_argument("--integrate-only", action="store_true")
ap.add_argument("--root", default=ROOT)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import pita_amd as pa
from pita_amd.energy_net import EnergyNet
L, D, S = pa._lib.lib(), 39, 2048
reps, rounds, steps = args.reps, args.rounds, args.steps
POPS = tuple(int(v) for v in args.pops.split(","))


def cell(v):
    return f"{float(np.median(v)):8.1f} [{min(v):7.1f},{max(v):7.1f}]"


print(f"(a) one resampling event of P x {S} walkers, D = {D}, log-weights N(0, 1); us per event: median [min, max] of "
      f"{rounds} windows of {reps} events")
print(f"{'P':>3} {'B':>6} {'fixed':>26} {'adaptive th=1':>26} {'adaptive th=0':>26} {'populations th=1':>26} "
      f"{'populations th=0':>26}  pop1/fixed  pop1/adaptive1  pop0/adaptive0")
for P in () if args.integrate_only else POPS:
    B = P * S
    a = torch.from_numpy(np.concatenate([np.float32(np.random.default_rng(3000 + p).standard_normal(S)) for p in range(P)])).cuda()
    u = torch.from_numpy(np.random.default_rng(7).random(P)).cuda()
    x = torch.randn(B, D, device="cuda")
    out = torch.empty_like(x)
    ids, ids_p = (torch.empty(B, dtype=torch.int64, device="cuda") for _ in range(2))
    nu = torch.zeros((), dtype=torch.int64, device="cuda")
    stats, flag = torch.zeros(6, dtype=torch.float64, device="cuda"), torch.zeros((), dtype=torch.int32, device="cuda")
    nu_p = torch.zeros(P, dtype=torch.int64, device="cuda")
    stats_p, flag_p = torch.zeros(P, 6, dtype=torch.float64, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
    nxt = torch.empty(B, device="cuda")
    scratch = lambda n: torch.empty((int(n) + 7) // 8, dtype=torch.float64, device="cuda")
    ws, ws_a = scratch(L.pita_resample_workspace_bytes(B)), scratch(L.pita_adaptive_resample_workspace_bytes(B))
    ws_p = scratch(L.pita_population_resample_workspace_bytes(P, S))
    st = pa._lib.stream_ptr(a.device)
    u0 = float(u[0])

    def gather(i):
        pa._lib.check(L.pita_gather_rows(x.data_ptr(), i.data_ptr(), out.data_ptr(), B, D, st))

    def fixed():
        pa._lib.check(L.pita_systematic_resample(a.data_ptr(), B, u0, ids.data_ptr(), ws.data_ptr(), st))
        pa._lib.check(L.pita_count_runs(ids.data_ptr(), B, nu.data_ptr(), st))
        gather(ids)

    def adaptive(theta):
        pa._lib.check(L.pita_adaptive_resample(a.data_ptr(), B, u0, theta, ids.data_ptr(), nu.data_ptr(), stats.data_ptr(),
                                               flag.data_ptr(), ws_a.data_ptr(), st))
        gather(ids)

    def populations(theta):
        pa._lib.check(L.pita_population_resample(a.data_ptr(), P, S, u.data_ptr(), theta, ids_p.data_ptr(), nu_p.data_ptr(),
                                                 stats_p.data_ptr(), flag_p.data_ptr(), nxt.data_ptr(), ws_p.data_ptr(), st))
        gather(ids_p)

    cases = [fixed, lambda: adaptive(1.0), lambda: adaptive(0.0), lambda: populations(1.0), lambda: populations(0.0)]
    if P == 1:
        adaptive(1.0); populations(1.0); torch.cuda.synchronize()
        assert torch.equal(ids, ids_p) and int(nu) == int(nu_p[0]) and torch.equal(stats.view(torch.int64), stats_p[0].view(torch.int64))
    populations(0.0); torch.cuda.synchronize()
    assert int(flag_p.sum()) == 0 and bool((nu_p == S).all())
    populations(1.0); torch.cuda.synchronize()
    assert int(flag_p.sum()) == P
    for fn in cases:  # warm-up of every shape of the timed windows
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in cases]
    for _ in range(rounds):
        for k, fn in enumerate(cases):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / reps * 1e3)
    m = [float(np.median(v)) for v in t]
    print(f"{P:>3} {B:>6} " + " ".join(f"{cell(v):>26}" for v in t) + f"  {m[3] / m[0]:10.2f}  {m[3] / m[1]:14.2f}  {m[4] / m[2]:14.2f}")

print()
print(f"(b) LJ13 debiased, {steps} steps, an event every second step, ess_threshold 0.5; ms per population-step: median "
      f"[min, max] of {rounds} alternating runs (after one warm-up run of each)")
print(f"{'P':>3} {'one run, populations=P':>30} {'P runs of 2 048 walkers':>30}  one / consecutive")
KW = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True, agg="sum")
w = {k: torch.tensor(v) for k, v in np.load(os.path.join(ROOT, "tests", "golden", "egnn_weights_trainedlike.npz")).items()}
net = pa.EGNN_dynamics(13, 3, condition_temperature=True, precision="f16x2", **KW)
net.load_state_dict({k: v for k, v in w.items() if k in net.state_dict()})
sde = pa.VEReverseSDE(noise_schedule=pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7),
                      score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)), debias_inference=True)
gam = pa.ConstantAnnealingFactorSchedule(4 / 3)


class Geometry:  # nothing evaluates the target in these runs
    n_particles, n_spatial_dim = 13, 3


def run(x1, populations):
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=steps, start_resampling_step=0, end_resampling_step=steps,
                                     resampling_interval=2, num_negative_time_steps=0, post_mcmc_steps=0, seed=3,
                                     ess_threshold=0.5, populations=populations)
    return integ.integrate_sde(x1, Geometry(), gam, inverse_temperature=1.0)


for P in POPS if args.integrate_only else POPS[1:]:
    x1 = pa.Prior(scale=3.0, n_particles=13, spatial_dim=3, seed=2).sample(P * S)
    parts = [x1[p * S:(p + 1) * S].contiguous() for p in range(P)]
    together = lambda: run(x1, P)
    apart = lambda: [run(xp, None) for xp in parts]
    t = [[], []]
    for r in range(rounds + 1):
        for k, fn in enumerate((together, apart)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r > 0:
                t[k].append((time.perf_counter() - t0) * 1e3 / (P * steps))
    cells = [f"{float(np.median(v)):8.3f} [{min(v):7.3f},{max(v):7.3f}]" for v in t]
    print(f"{P:>3} {cells[0]:>30} {cells[1]:>30}  {np.median(t[0]) / np.median(t[1]):8.2f}")
