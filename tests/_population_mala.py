"""Inputs and references of tests/test_population_mala_gpu.py: the per-population MALA chain
(``WeightedSDEIntegrator._mala(..., pop_size=S)``, the ``_pop`` entry points) against the chain as it was -- one
population's slice run on its own through ``_mala`` with ``walker_offset`` = its first row.

Shapes: the smallest at which a block's walkers straddle populations on every route (S is no multiple of the walkers a
block or a wave holds), three populations, hence more than one block or wave group.  The populations start from
differently perturbed walkers (``jitter``: cold to hot), so that their acceptance rates -- and with them their adapted
step sizes -- part ways within the chain."""
import collections

import numpy as np
import torch

from oracle import pita_oracle as O

Case = collections.namedtuple("Case", "target fused S steps dt jitter")

CASES = {
    # LJ13: the 128-walker LDS tile (fused) and mala_accept_kernel's 19 walkers per block (launch per kernel)
    "lj13": Case("lj13", True, 80, 12, 1.2e-3, (0.004, 0.03, 0.15, 0.015)),
    "lj13_per_kernel": Case("lj13", False, 80, 12, 1.2e-3, (0.004, 0.03, 0.15, 0.015)),
    # LJ55: ring kernel, one walker per wave, four per block
    "lj55": Case("lj55", True, 5, 8, 1e-3, (0.005, 0.03, 0.12, 0.015)),
    # DW4: ring kernel, sixteen walkers per wave
    "dw4": Case("dw4", True, 24, 12, 0.05, (0.05, 0.3, 1.0, 0.15)),
    # the 22-atom synthetic force field: 11 walkers per block
    "ff22": Case("ff22", True, 16, 12, 2e-4, (0.001, 0.004, 0.012, 0.002)),
    # GMM: no fused route, 256 walkers per block in the launch-per-kernel chain
    "gmm": Case("gmm", False, 32, 12, 2.0, (0.3, 2.0, 8.0, 1.0)),
}


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def target_and_walkers(pa, golden, case, n_pop, seed=0):
    """(target, x [n_pop * S, D] on the device): population p perturbed with ``case.jitter[p]``."""
    gen = torch.Generator().manual_seed(1000 + seed)
    S = case.S
    if case.target == "lj13":
        e = pa.LennardJonesEnergy(39, 13, 3)
        base = torch.tensor(golden("post_lj13.npz")["x0"], dtype=torch.float32)
        rows = [base[torch.arange(S) % base.shape[0]] + case.jitter[p] * torch.randn(S, 39, generator=gen) for p in range(n_pop)]
        x = O.remove_mean(torch.cat(rows), 13, 3)
    elif case.target == "lj55":
        e = pa.LennardJonesEnergy(165, 55, 3)
        grid = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        pts = grid[np.argsort((grid ** 2).sum(-1), kind="stable")[:55]] * 1.09
        base = torch.tensor(pts, dtype=torch.float32).reshape(1, 165)
        x = O.remove_mean(torch.cat([base + case.jitter[p] * torch.randn(S, 165, generator=gen) for p in range(n_pop)]), 55, 3)
    elif case.target == "dw4":
        e = pa.MultiDoubleWellEnergy(temperature=1.0)
        base = torch.tensor([[2.0, 2.0], [-2.0, 2.0], [-2.0, -2.0], [2.0, -2.0]]).reshape(1, 8)
        x = O.remove_mean(torch.cat([base + case.jitter[p] * torch.randn(S, 8, generator=gen) for p in range(n_pop)]), 4, 2)
    elif case.target == "ff22":
        from tests import _ff_shapes as FS

        tables, pos = FS.base_system("ala2")
        e = FS.energy({k: v.copy() for k, v in tables.items()}, 22)
        x = torch.cat([FS.walkers(pos, S, 500 + 10 * seed + p, sd=case.jitter[p]) for p in range(n_pop)])
    else:
        e = pa.GMM()
        locs = e.locs.cpu()
        x = torch.cat([locs[torch.randint(0, locs.shape[0], (S,), generator=gen)] + case.jitter[p] * torch.randn(S, 2, generator=gen)
                       for p in range(n_pop)])
    return e, x.contiguous().cuda()


def integrator(pa, case, adaptive, seed=9, **kw):
    return pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                    post_mcmc_steps=case.steps, dt_negative_time=case.dt, adaptive_mcmc=adaptive, seed=seed, **kw)


def replay_dt(dt, rates, adaptive=True):
    """mala_adapt_kernel's rule on the host: the same double arithmetic on the same fp32 rates."""
    if adaptive:
        for r in rates:
            dt = dt * 1.1 if r > 0.55 else dt / 1.1
    return dt


def slice_chains(integ, e, x, case, n_pop, adaptive, base=0):
    """The reference: the chain as it was on every population's slice -> [(rows, rates as python floats, final dt)]."""
    S, out = case.S, []
    for p in range(n_pop):
        rows, rates = integ._mala(x[p * S:(p + 1) * S].contiguous(), e, adaptive, case.dt, walker_offset=base + p * S,
                                  keep_order=True, return_acceptance_rate=True, fused=case.fused)
        out.append((rows, rates, replay_dt(case.dt, rates, adaptive)))
    return out


def population_chain(integ, e, x, case, adaptive, base=0):
    """The per-population chain on the whole batch -> (rows, pooled rates, rates [steps, P], final dt [P], n_valid [P])."""
    rows, pooled = integ._mala(x, e, adaptive, case.dt, walker_offset=base, keep_order=True, return_acceptance_rate=True,
                               fused=case.fused, pop_size=case.S)
    rates, dt_dev, totals = integ._mala_pop_state
    return rows, pooled, rates, dt_dev, totals


def coupled_chain(integ, e, x, case, adaptive, base=0):
    """The chain as it was on the whole batch: one step size for all populations."""
    return integ._mala(x, e, adaptive, case.dt, walker_offset=base, keep_order=True, return_acceptance_rate=True,
                       fused=case.fused)


class FusedSpy:
    """Counts the fused launches a target takes, and how many of them were per-population chains."""

    def __init__(self, e):
        self.taken = self.per_population = 0
        inner = getattr(e, "fused_mala", None)
        if inner is None:
            return

        def fused_mala(x, logp, num_steps, dt_dev, adaptive, total, *a, **kw):
            out = inner(x, logp, num_steps, dt_dev, adaptive, total, *a, **kw)
            self.taken += out is not None
            self.per_population += out is not None and not isinstance(total, int)
            return out

        e.fused_mala = fused_mala
