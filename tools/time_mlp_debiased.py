"""Time the debiased regime on the MLP backbone: GMM target, MyMLP(128 x 3, emb 128, D = 2) score and energy nets.

    python3 tools/time_mlp_debiased.py [OUT.txt]          (1 024, 65 536 and 2^20 walkers in one process)

Per batch: the backbone forward (pita_mlp_forward), the pita_mlp_jacobian launch of each net (score net: trace + D;
energy net: J^T x, <x, dD/dh>, the h split, D), the whole debiased step (VEReverseSDE.f + pita_em_step) and the
not-debiased fused step (pita_mlp_sampler_run, one step).  Device events around REPS calls after WARM warm-up calls;
the median of 5 such windows, in ms per call."""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pita_amd  # noqa: E402
from pita_amd import mlp  # noqa: E402
from pita_amd.energy_net import EnergyNet  # noqa: E402
from pita_amd.sde_integration import build_step_table  # noqa: E402

SIZES = (1024, 65536, 1 << 20)
WARM, REPS = 3, 10


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / REPS)
    return float(np.median(ms))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    w = {k[2:]: torch.tensor(v) for k, v in np.load(os.path.join(ROOT, "tests/golden/mlp_gmm_fwd.npz")).items()
         if k.startswith("w.")}
    s_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
    s_net.load_state_dict(w)
    e_net = copy.deepcopy(s_net)
    sched = pita_amd.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    gam = pita_amd.ConstantAnnealingFactorSchedule(4 / 3)
    sde = pita_amd.VEReverseSDE(noise_schedule=sched, score_net=pita_amd.ScoreNet(s_net), energy_net=EnergyNet(e_net),
                                debias_inference=True)
    L, dev = pita_amd._lib.lib(), torch.device("cuda")
    t = torch.tensor(0.5)
    tab = build_step_table(sched, gam, torch.tensor([0.5]), 1e-2, 1.0, 1.0).to(dev)
    row = tab[0].cpu()
    lines = [f"{torch.cuda.get_device_name()}, GMM / MyMLP(128 x 3, emb 128, D = 2), t = 0.5; ms per call "
             f"(median of 5 windows of {REPS} calls)",
             f"{'walkers':>9} {'forward':>9} {'jac_score':>10} {'jac_energy':>11} {'debiased':>9} {'fused_step':>11} "
             f"{'jac/fwd':>8}"]
    print(lines[0])
    print(lines[1])
    for B in SIZES:
        g = torch.Generator(device="cpu").manual_seed(B)
        x = (torch.randn(B, 2, generator=g) * 40.0).to(dev)
        h = torch.full((B,), float(sched.h(t.reshape(1))[0]), device=dev)
        cn, xs = torch.log(h) / 8, x / torch.sqrt(1 + h)[:, None]
        xw = x.clone()

        def debiased_step():
            terms = sde.f(t, xw, 1.0, gam, None, None)
            L.pita_em_step(xw.data_ptr(), terms.drift_X.data_ptr(), 0, B, 1, 2, float(row[pita_amd._lib.ST_DT]),
                           float(row[pita_amd._lib.ST_NOISE_SCALE]), float(row[pita_amd._lib.ST_SQRT_DT]), 1, 0, 0, 0,
                           0, pita_amd._lib.stream_ptr(dev))

        r = dict(
            forward=timed(lambda: s_net(cn, xs)),
            jac_score=timed(lambda: s_net.jacobian_trace(h, x, 1.0, want_denoiser=True)),
            jac_energy=timed(lambda: e_net.vjp(h, x, 1.0, want_dot_h=True, want_h_parts=True)),
            debiased=timed(debiased_step),
            fused_step=timed(lambda: s_net.sampler_run(xw, tab, 1, seed=3, remove_mean=False)))
        ln = (f"{B:>9} {r['forward']:>9.4f} {r['jac_score']:>10.4f} {r['jac_energy']:>11.4f} {r['debiased']:>9.4f} "
              f"{r['fused_step']:>11.4f} {r['jac_energy'] / r['forward']:>8.2f}")
        print(ln, flush=True)
        lines.append(ln)
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
