"""What the dot_parts split of the wide EGNN reverse sweep (pita_egnn_wide_vjp_parts) buys in dUt_dt = dE_theta/dh dh/dt of
the debiased regime (VEReverseSDE(debias_inference=True).f, no pinning), per time point, against the fp64 oracle:
python tools/wide_dedh_probe.py <atoms: 22, 33 or 42> [--times 0.1,0.15,0.3] [--walkers 6]
Net: 22 atoms the golden egnn_ad2cat_h64_fwd net, 33 / 42 the seeded hidden 64 x 5 net (attention + tanh, coordinate head
x 200) of tests/test_wide_vjp_gpu.py.  Walkers: x = remove_mean(randn s) (1 + sqrt h), generator seed 12, s = 1 at 22 atoms
and 1.5 above, beta = 1.25, Elucidating(0.01, 80, 7).  Per time point: mean |error| of dUt_dt assembled from the split
and from the form through <D, x> and <x, dD/dh> (vjp_h_parts switched off), the fp32 oracle's own error (the same autograd
in float32), and the mean |error| of s1 = c_out <x, F> and s2 = <x, d(c_out F)/dh> themselves (fp32 oracle's beside them).
The sibling of tools/long_terms_probe.py (LJ13 long fixtures) for the peptide backbone."""
import argparse, copy, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
from oracle import pita_oracle as O
from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
from pita_amd.energy_net import EnergyNet
ap = argparse.ArgumentParser()
ap.add_argument("atoms", type=int, choices=(22, 33, 42))
ap.add_argument("--times", default="0.1,0.15,0.3")
ap.add_argument("--walkers", type=int, default=6)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
n, B = a.atoms, a.walkers
if n == 22:
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "egnn_ad2cat_h64_fwd.npz")))
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=64, n_layers=5, tanh=True, attention=True, condition_beta=True)
    net.load_state_dict({k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("w.")})
else:
    torch.manual_seed(100 + n)
    net = EGNN_dynamics_AD2_cat(n, 3, hidden_nf=64, n_layers=5, tanh=True, attention=True, condition_beta=True)
    with torch.no_grad():
        for prm in net.parameters():
            if prm.dim() == 2 and prm.shape == (1, 64):
                prm.mul_(200.0)
w = {k: v.detach().clone() for k, v in net.state_dict().items()}
sched, osched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7), O.Elucidating(0.01, 80.0, 7)
sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                      debias_inference=True)
gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
z = O.remove_mean(torch.randn(B, 3 * n, generator=torch.Generator().manual_seed(12)) * (1.0 if n == 22 else 1.5), n, 3)
beta = 1.25


def oracle(t, hq, x, dtype):
    """(dUt_dt at t, s1 and s2 at h = hq) of the oracle in ``dtype``, as fp64"""
    wd = {k: v.to(dtype) for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, n, 3, n_layers=5, tanh=True, attention=True)
    tt = torch.full((B,), t, dtype=dtype).requires_grad_(True)
    (dU,) = torch.autograd.grad(O.energy_theta(bb, osched.h(tt), x.to(dtype), beta).sum(), tt)
    hd = torch.full((B,), hq, dtype=dtype).requires_grad_(True)
    c_s, c_in, c_out, c_noise = O.edm_coeffs(hd)
    s1 = c_out * (bb(c_noise, c_in[:, None] * x.to(dtype), beta * torch.ones(B, dtype=dtype)) * x.to(dtype)).sum(1)
    (s2,) = torch.autograd.grad(s1.sum(), hd)
    return dU.double(), s1.detach().double(), s2.double()


print(f"tools/wide_dedh_probe.py {n} atoms, hidden 64 x 5, attention + tanh, {B} walkers, beta {beta}; device "
      f"{torch.cuda.get_device_name(0)}; reverse mode on the matrix pipe: {net.vjp_uses_matrix_pipe('cuda:0')}")
mean = lambda v: float(v.abs().mean())
for t in (float(v) for v in a.times.split(",")):
    h = float(osched.h(torch.tensor(t, dtype=torch.float64)))
    x = z * (1.0 + h ** 0.5)
    hq = float(torch.tensor(h, dtype=torch.float32))  # the h the kernel is given for the pieces
    (U64, a64, b64), (U32, a32, b32) = oracle(t, hq, x, torch.float64), oracle(t, hq, x, torch.float32)
    tc, xs = torch.tensor(t).cuda(), x.cuda()
    split = sde.f(tc, xs, beta, gam, None, None, resampling_interval=1).dUt_dt.cpu().double()
    EGNN_dynamics_AD2_cat.vjp_h_parts = False
    try:
        old = sde.f(tc, xs, beta, gam, None, None, resampling_interval=1).dUt_dt.cpu().double()
    finally:
        EGNN_dynamics_AD2_cat.vjp_h_parts = True
    ht = torch.full((B,), hq, dtype=torch.float32).cuda()
    parts = net.vjp(ht, xs, torch.full((B,), beta).cuda(), want_dot_h=True, want_h_parts=True)[3].cpu().double()
    e32 = mean(U32 - U64)
    print(f"t={t:<5g} h={h:.2e} |dUt_dt| {mean(U64):.3e}: split {mean(split - U64):.3e} ({mean(split - U64) / e32:.2f} x fp32 "
          f"oracle)  old form {mean(old - U64):.3e} ({mean(old - U64) / e32:.2f} x)  fp32 oracle {e32:.3e} | s1 |want| "
          f"{mean(a64):.3e} err {mean(parts[:, 0] - a64):.3e} (fp32 oracle {mean(a32 - a64):.3e})  s2 |want| {mean(b64):.3e} err "
          f"{mean(parts[:, 1] - b64):.3e} (fp32 oracle {mean(b32 - b64):.3e})", flush=True)
