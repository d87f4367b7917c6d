"""pita_ff_logp_force and pita_ff_descent on the amber-sized peptides of tests/_peptides.py (GB-OBC1 on, reaction-field
cutoff 2 nm as in the serialized System): 22 atoms (ALA2), 33 (zwitterionic ALA3), 42 (ACE-ALA3-NME) at 4 096,
16 384 and 262 144 walkers.  Device events around REPS launches after a warm-up; prints us per launch and walker-evals/s
(a descent launch of S steps is S walker-evals per walker), and the launch plan the kernel was given (walkers per block
and dynamic LDS, restated here from pita_ff_create's arithmetic; the rocprofv3 kernel trace shows the LDS the launch
really took).

    python tools/time_ff_sizes.py [--reps 20] [--steps 10] [--sizes ala2,ala3,ala4] [--batches 4096,16384,262144]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pita_amd.alp_energy import ALPEnergy  # noqa: E402
from tests._peptides import peptide, peptide_system_xml  # noqa: E402

SCALE = 0.1640


def launch_plan(t, lds_limit):
    """(walkers per block, LDS bytes of pita_ff_logp_force, of pita_ff_descent): pita_ff_create's plan, restated."""
    pad = lambda b: (b + 15) // 16 * 16
    n, nb, na, nt = len(t["charge"]), len(t["bond_idx"]), len(t["angle_idx"]), len(t["tors_idx"])
    npair, ent = n * (n - 1) // 2, 2 * nb + 3 * na + 4 * nt
    blob = sum(pad(b) for b in (8 * nb, 8 * nb, 12 * na, 8 * na, 16 * nt, 12 * nt, 8 * nt, 8 * npair, 16 * npair,
                                16 * n if "gb_radius" in t else 0, 12 * (n + 1), 4 * max(ent, 1)))
    per_logp, per_descent = 4 * (9 * n + 3 * ent), 4 * (15 * n + 3 * ent)
    w = 256 // n
    while w > 0 and blob + w * per_descent > lds_limit:
        w -= 1
    return w, blob + w * per_logp, blob + w * per_descent


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="ala2,ala3,ala4")
    ap.add_argument("--batches", default="4096,16384,262144")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_ff_sizes.py measures on the GPU"
    prop = torch.cuda.get_device_properties(0)
    limit = max(getattr(prop, "shared_memory_per_block_optin", 0), getattr(prop, "shared_memory_per_block", 0))
    print(f"device {prop.name}: per-block LDS limit {limit} B (torch's device properties)", flush=True)
    for name in args.sizes.split(","):
        t, pos = peptide(name)
        n = len(t["charge"])
        e = ALPEnergy(dimensionality=3 * n, n_particles=n, temperature=300.0, data_normalization_factor=SCALE,
                      energy_batch_size=1 << 30, system_xml=peptide_system_xml(name))
        wpb, lds_l, lds_d = launch_plan(t, limit)
        print(f"{name}: {n} atoms, {len(t['bond_idx'])} bonds, {len(t['angle_idx'])} angles, {len(t['tors_idx'])} torsion "
              f"terms; plan {wpb} walkers/block, LDS {lds_l} B (logp_force) / {lds_d} B (descent)", flush=True)
        for B in (int(b) for b in args.batches.split(",")):
            gen = torch.Generator().manual_seed(B)
            x = ((torch.tensor(pos.reshape(-1), dtype=torch.float32)[None] + 0.004 * torch.randn(B, 3 * n, generator=gen))
                 / SCALE).cuda()
            logp = torch.empty(B, device="cuda")
            force = torch.empty_like(x)
            us_f = timed(lambda: force_eval(e, x, logp, force), args.reps)
            xd = x.clone()
            us_d = timed(lambda: e.fused_descent(xd, args.steps, 1e-9, 0.0, 0.0, seed=1), args.reps)
            assert torch.isfinite(logp).all() and torch.isfinite(force).all() and torch.isfinite(xd).all()
            print(f"  B={B:7d}  logp_force {us_f:9.1f} us  {B / us_f * 1e6:.3e} walker-evals/s   "
                  f"descent({args.steps} steps) {us_d:9.1f} us  {B * args.steps / us_d * 1e6:.3e} walker-evals/s", flush=True)


def force_eval(e, x, logp, force):
    """pita_ff_logp_force into preallocated outputs (the timed call: no allocation inside the window)."""
    from pita_amd import _lib

    _lib.check(_lib.lib().pita_ff_logp_force(e._native(), x.data_ptr(), logp.data_ptr(), force.data_ptr(), x.shape[0],
                                             _lib.stream_ptr(x.device)), "pita_ff_logp_force")


if __name__ == "__main__":
    main()
