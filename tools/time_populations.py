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
``--blocks`` (instead of (a) and (b)): populations beyond 2 048 walkers, 65 536 LJ13 walkers split as 1 x 65 536 ...
32 x 2 048 (``--splits``):
(c) one event plus the row gather, theta = 1 and theta = 0, the protocol of (a):
      blocks       pita_population_resample_blocks (at most seven launches whatever P is) + gather
      loop         P pita_adaptive_resample calls on the slices, one add of the row offsets, one gather: the only way to
                   the same result without the entry point (no logw_next, which favours the loop)
      whole        pita_adaptive_resample on the whole batch as ONE population + gather: for scale, another result
      one launch   pita_population_resample + gather, where S <= 2 048
    Before timing, at every shape, blocks is checked against loop bit for bit (ids, statistics, decisions, counts).
(d) the protocol of (b) at 4 x 16 384 walkers: one integrate_sde with populations=4 against four consecutive runs of
    16 384 walkers (populations=None).
usage: python tools/time_populations.py [reps] [rounds] [steps] [--pops 1,8,32] [--integrate-only] [--blocks]
[--splits 1,2,4,8,16,32] [--root DIR]; the committed profiles are the second of two runs.  ``--integrate-only``: (b)
alone, for every P of ``--pops``; ``--root``: the tree whose pita_amd is imported (host-cost comparisons of two trees on
one library)."""
import argparse, copy, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=1000)
ap.add_argument("rounds", nargs="?", type=int, default=7)
ap.add_argument("steps", nargs="?", type=int, default=8)
ap.add_argument("--pops", default="1,8,32")
ap.add_argument("--integrate-only", action="store_true")
ap.add_argument("--blocks", action="store_true")
ap.add_argument("--splits", default="1,2,4,8,16,32")
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


def windows(cases):
    """us per call of every case: warm-up, then ``rounds`` alternating windows of ``reps`` calls between device events."""
    for fn in cases:
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
    return t


if not args.blocks:
    print(f"(a) one resampling event of P x {S} walkers, D = {D}, log-weights N(0, 1); us per event: median [min, max] of "
          f"{rounds} windows of {reps} events")
    print(f"{'P':>3} {'B':>6} {'fixed':>26} {'adaptive th=1':>26} {'adaptive th=0':>26} {'populations th=1':>26} "
          f"{'populations th=0':>26}  pop1/fixed  pop1/adaptive1  pop0/adaptive0")
for P in () if args.integrate_only or args.blocks else POPS:
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
    t = windows(cases)  # warm-up of every shape of the timed windows included
    m = [float(np.median(v)) for v in t]
    print(f"{P:>3} {B:>6} " + " ".join(f"{cell(v):>26}" for v in t) + f"  {m[3] / m[0]:10.2f}  {m[3] / m[1]:14.2f}  {m[4] / m[2]:14.2f}")

BT = 65536
for P in tuple(int(v) for v in args.splits.split(",")) if args.blocks else ():
    if P == int(args.splits.split(",")[0]):
        print(f"(c) one resampling event of {BT} walkers as P populations of S, D = {D}, log-weights N(0, 1); us per event: "
              f"median [min, max] of {rounds} windows of {reps} events")
        print(f"{'P':>3} {'S':>6} {'th':>3} {'blocks':>26} {'loop':>26} {'whole':>26} {'one launch':>26}  blocks/loop  "
              f"blocks/whole  blocks/one launch")
    Sb = BT // P
    a = torch.from_numpy(np.concatenate([np.float32(np.random.default_rng(3000 + p).standard_normal(Sb)) for p in range(P)])).cuda()
    u = torch.from_numpy(np.random.default_rng(7).random(P)).cuda()
    uh = u.cpu().tolist()
    x = torch.randn(BT, D, device="cuda")
    out = torch.empty_like(x)
    ids_b, ids_l, ids_g, ids_w, ids_o = (torch.empty(BT, dtype=torch.int64, device="cuda") for _ in range(5))
    base = torch.arange(P, device="cuda").repeat_interleave(Sb) * Sb
    new = lambda: (torch.zeros(P, dtype=torch.int64, device="cuda"), torch.zeros(P, 6, dtype=torch.float64, device="cuda"),
                   torch.zeros(P, dtype=torch.int32, device="cuda"))
    (nu_b, stats_b, flag_b), (nu_l, stats_l, flag_l), (nu_o, stats_o, flag_o), (nu_w, stats_w, flag_w) = new(), new(), new(), new()
    nxt = torch.empty(BT, device="cuda")
    scratch = lambda n: torch.empty((int(n) + 7) // 8, dtype=torch.float64, device="cuda")
    ws_b = scratch(L.pita_population_resample_blocks_workspace_bytes(P, Sb))
    ws_s, ws_w = scratch(L.pita_adaptive_resample_workspace_bytes(Sb)), scratch(L.pita_adaptive_resample_workspace_bytes(BT))
    ws_o = scratch(L.pita_population_resample_workspace_bytes(P, Sb))
    st = pa._lib.stream_ptr(a.device)
    one_launch = bool(L.pita_adaptive_resample_single_launch(Sb))

    def gather(i):
        pa._lib.check(L.pita_gather_rows(x.data_ptr(), i.data_ptr(), out.data_ptr(), BT, D, st))

    def blocks(theta):
        pa._lib.check(L.pita_population_resample_blocks(a.data_ptr(), P, Sb, u.data_ptr(), theta, ids_b.data_ptr(), nu_b.data_ptr(),
                                                        stats_b.data_ptr(), flag_b.data_ptr(), nxt.data_ptr(), ws_b.data_ptr(), st))
        gather(ids_b)

    def loop(theta):  # the stream serialises the calls, so one scratch serves all slices
        for p in range(P):
            pa._lib.check(L.pita_adaptive_resample(a.data_ptr() + 4 * p * Sb, Sb, uh[p], theta, ids_l.data_ptr() + 8 * p * Sb,
                                                   nu_l.data_ptr() + 8 * p, stats_l.data_ptr() + 48 * p,
                                                   flag_l.data_ptr() + 4 * p, ws_s.data_ptr(), st))
        torch.add(ids_l, base, out=ids_g)
        gather(ids_g)

    def whole(theta):
        pa._lib.check(L.pita_adaptive_resample(a.data_ptr(), BT, uh[0], theta, ids_w.data_ptr(), nu_w.data_ptr(),
                                               stats_w.data_ptr(), flag_w.data_ptr(), ws_w.data_ptr(), st))
        gather(ids_w)

    def one(theta):
        pa._lib.check(L.pita_population_resample(a.data_ptr(), P, Sb, u.data_ptr(), theta, ids_o.data_ptr(), nu_o.data_ptr(),
                                                 stats_o.data_ptr(), flag_o.data_ptr(), nxt.data_ptr(), ws_o.data_ptr(), st))
        gather(ids_o)

    for theta in (1.0, 0.0):
        blocks(theta); loop(theta); torch.cuda.synchronize()
        assert torch.equal(ids_b, ids_g) and torch.equal(nu_b, nu_l) and torch.equal(flag_b, flag_l)
        assert torch.equal(stats_b.view(torch.int64), stats_l.view(torch.int64)) and int(flag_b.sum()) == (P if theta else 0)
        cases = [lambda: blocks(theta), lambda: loop(theta), lambda: whole(theta)] + ([lambda: one(theta)] if one_launch else [])
        t = windows(cases)
        m = [float(np.median(v)) for v in t]
        last = f"{cell(t[3]):>26}" if one_launch else f"{'-':>26}"
        print(f"{P:>3} {Sb:>6} {theta:>3.0f} " + " ".join(f"{cell(v):>26}" for v in t[:3]) + f" {last}  {m[0] / m[1]:11.2f}  "
              f"{m[0] / m[2]:12.2f}  " + (f"{m[0] / m[3]:17.2f}" if one_launch else f"{'-':>17}"))

print()
if args.blocks:
    S, POPS, args.integrate_only = 16384, (4,), True
    print(f"(d) LJ13 debiased, {steps} steps, an event every second step, ess_threshold 0.5; ms per population-step: median "
          f"[min, max] of {rounds} alternating runs (after one warm-up run of each)")
else:
    print(f"(b) LJ13 debiased, {steps} steps, an event every second step, ess_threshold 0.5; ms per population-step: median "
          f"[min, max] of {rounds} alternating runs (after one warm-up run of each)")
print(f"{'P':>3} {'one run, populations=P':>30} {f'P runs of {S:,} walkers'.replace(',', ' '):>30}  one / consecutive")
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
