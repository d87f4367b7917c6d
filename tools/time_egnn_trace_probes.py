"""Timing of the Hutchinson estimate of trace(J_x D) on the hidden-32 EGNN (golden trained-like weights, 3 layers,
attention + tanh, temperature-conditioned): in one process on one device, alternating within each repetition,
  exact     EGNN_dynamics.jacobian_trace (all n*d unit directions),
  K x jvp   the path VEReverseSDE takes without shared_primal: rademacher_probes, K jvp(vx=v_k) launches, the mean of
            <v_k, dD_k> formed on the device in probe order (the code of VEReverseSDE._score_divergence_terms),
  probes    EGNN_dynamics.trace_probes (pita_egnn_trace_probes, probes drawn in the kernel), the denoiser included,
device-event timing, median and min-max over the timed repetitions, with the checksum and non-finite count of each result.
python tools/time_egnn_trace_probes.py [--system lj13|lj55] [--walkers B] [--probes 3,6,12] [--reps 7] [--warmup 2]
                                       [--precision f16x2] [--step] [--commit HASH]
Defaults: lj13 at 65 536 walkers with K = 3, 6, 12; lj55 at 32 768 walkers with K = 1, 4.
--step: time the whole debiased step VEReverseSDE.f instead (exact / hutchinson / hutchinson with shared_primal=True)."""
import argparse, copy, os, statistics, subprocess, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
from pita_amd.energy_net import EnergyNet
from pita_amd.utils import rademacher_probes
ap = argparse.ArgumentParser()
ap.add_argument("--system", choices=["lj13", "lj55"], default="lj13")
ap.add_argument("--walkers", type=int, default=None)
ap.add_argument("--probes", default=None)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--precision", default="f16x2")
ap.add_argument("--step", action="store_true")
ap.add_argument("--commit", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
assert a.reps >= 5, "the median of at least five timed repetitions"
N = {"lj13": 13, "lj55": 55}[a.system]
B = a.walkers or {"lj13": 65536, "lj55": 32768}[a.system]
Ks = [int(k) for k in (a.probes or {"lj13": "3,6,12", "lj55": "1,4"}[a.system]).split(",")]
commit = a.commit
if commit is None:
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
    commit = r.stdout.strip() if r.returncode == 0 else "unknown"
print(f"tools/time_egnn_trace_probes.py  commit {commit}  device {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
print(f"EGNN_dynamics({N}, 3, hidden_nf=32, n_layers=3, attention, tanh, condition_temperature, precision={a.precision}), "
      f"golden trained-like weights; B = {B}; {a.warmup} warm-up + {a.reps} timed repetitions per path, alternating, "
      "device events")
w = dict(np.load(os.path.join(ROOT, "tests/golden/egnn_weights_trainedlike.npz")))
net = pa.EGNN_dynamics(N, 3, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True,
                       condition_temperature=True, agg="sum", precision=a.precision)
net.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
x = pa.Prior(scale=3.0, n_particles=N, spatial_dim=3).sample(B)
h = torch.full((B,), 1.0).cuda()
beta = torch.ones(B).cuda()
KEY = dict(seed=11, walker_offset=0, step=5)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def k_jvp(K):  # VEReverseSDE._score_divergence_terms without shared_primal, statement for statement
    probes = rademacher_probes(B, N, 3, K, device=x.device, **KEY)
    acc = torch.zeros(B, device=x.device)
    D_S = None
    for k in range(K):
        out, dout = net.jvp(h, x, beta, vx=probes[k], want_primal=(k == 0), want_tangent=True)
        D_S = out if k == 0 else D_S
        acc = acc + (probes[k] * dout).sum(-1)
    return acc / float(K), D_S


def run(paths):
    """paths: name -> callable returning a tensor (or a tuple whose first item is one); alternating repetitions."""
    for _ in range(a.warmup):
        for f in paths.values():
            f()
    torch.cuda.synchronize()
    t, last = {k: [] for k in paths}, {}
    for _ in range(a.reps):
        for k, f in paths.items():
            ms, out = timed(f)
            t[k].append(ms)
            last[k] = out[0] if isinstance(out, tuple) else out
    for k in paths:
        v, o = t[k], last[k]
        print(f"  {k:34s} median {statistics.median(v):9.3f} ms (min {min(v):9.3f}, max {max(v):9.3f})   checksum "
              f"{float(o.double().sum()):.9e} nonfinite {int((~torch.isfinite(o)).sum())}")
    return {k: statistics.median(v) for k, v in t.items()}


if not a.step:
    paths = {"exact jacobian_trace": lambda: net.jacobian_trace(h, x, beta, want_denoiser=True)}
    for K in Ks:
        paths[f"K={K}: {K} x jvp + mean"] = lambda K=K: k_jvp(K)
        paths[f"K={K}: trace_probes"] = lambda K=K: net.trace_probes(h, x, beta, K, want_denoiser=True, **KEY)
    med = run(paths)
    for K in Ks:
        old, new = med[f"K={K}: {K} x jvp + mean"], med[f"K={K}: trace_probes"]
        print(f"  K={K}: trace_probes / (K x jvp + mean) = {new / old:.3f} ({100 * (1 - new / old):+.1f} % time saved); "
              f"against the exact trace {new / med['exact jacobian_trace']:.3f}")
else:
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    mk = lambda **kw: pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net),
                                      energy_net=EnergyNet(copy.deepcopy(net)), debias_inference=True, **kw)
    t = torch.tensor(0.5).cuda()
    f = lambda sde: (lambda: sde.f(t, x, 1.0, gam, None, None, probe_key=(11, 0, 5)).drift_A)
    paths = {"step, exact divergence": f(mk())}
    for K in Ks:
        paths[f"step, K={K}: K x jvp"] = f(mk(divergence="hutchinson", n_probes=K))
        paths[f"step, K={K}: shared_primal"] = f(mk(divergence="hutchinson", n_probes=K, shared_primal=True))
    med = run(paths)
    for K in Ks:
        old, new = med[f"step, K={K}: K x jvp"], med[f"step, K={K}: shared_primal"]
        print(f"  K={K}: step with shared_primal / step with K x jvp = {new / old:.3f}; against the exact step "
              f"{new / med['step, exact divergence']:.3f}")
