"""The fused MALA chain on the force-field target (pita_ff_mala, ForceFieldEnergy.fused_mala) on the amber-sized
peptides of tests/_peptides.py: bit for bit the launch-per-kernel chain of WeightedSDEIntegrator._mala (non-adaptive:
one launch; adaptive: one launch per step), a walker's chain independent of its batch and of its slot in a block, the
fp64 oracle's MALA step, and reruns that give the same bits.  Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests._peptides import peptide

pytestmark = pytest.mark.gpu
SCALE = 0.1640
SIZES = {"ala2": 22, "ala3": 33, "ala4": 42, "chain64": 64}
DT = 2e-4  # acceptance falls from ~0.98 to below 0.55 within a few steps: the adaptive rule moves both ways


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def _system(name, gb=True):
    tabs, pos = peptide(name)
    if not gb:
        tabs = {k: v for k, v in tabs.items() if not k.startswith("gb_")}
    ff_t = {k: torch.as_tensor(v) for k, v in tabs.items()}
    ff_t = {k: (v.long() if "idx" in k else v.double()) for k, v in ff_t.items()}
    return tabs, ff_t, pos


def _walkers(pos, B, seed, sd=0.004):
    gen = torch.Generator().manual_seed(seed)
    n = pos.shape[0]
    x = torch.tensor(pos.reshape(-1), dtype=torch.float32)[None] + sd * torch.randn(B, 3 * n, generator=gen)
    return O.remove_mean(x / SCALE, n, 3)


def _energy(name, gb=True, cutoff=0.45):
    from pita_amd.alp_energy import ForceFieldEnergy

    tabs, ff_t, pos = _system(name, gb)
    e = ForceFieldEnergy(tabs, n_particles=SIZES[name], temperature=300.0, data_normalization_factor=SCALE, cutoff=cutoff)
    return e, ff_t, pos


class _Spy:
    """Counts the fused launches an energy object takes and keeps the step-size tensor of the last one."""

    def __init__(self, e):
        self.taken, self.dt_dev, inner = 0, None, e.fused_mala

        def fused_mala(x, logp, num_steps, dt_dev, *a, **kw):
            out = inner(x, logp, num_steps, dt_dev, *a, **kw)
            self.taken += out is not None
            self.dt_dev = dt_dev
            return out

        e.fused_mala = fused_mala


def _chain(pa, e, x0, steps, adaptive, fused, mean_free=True, seed=9, walker_offset=0, **kw):
    integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                     post_mcmc_steps=steps, dt_negative_time=DT, adaptive_mcmc=adaptive,
                                     should_mean_free=mean_free, seed=seed)
    if adaptive:
        out = integ.metropolis_hastings_mala_adaptive(x0.clone(), e, dt_init=DT, return_acceptance_rate=True, fused=fused,
                                                      walker_offset=walker_offset, **kw)
    else:
        out = integ.metropolis_hastings_mala(x0.clone(), e, return_acceptance_rate=True, fused=fused,
                                             walker_offset=walker_offset, **kw)
    return out[0], out[1], integ


def _replay_dt(rates):
    """The adaptive rule of mala_adapt_kernel on the host: the same double arithmetic on the same fp32 rates."""
    dt = DT
    for r in rates:
        dt = dt * 1.1 if r > 0.55 else dt / 1.1
    return dt


@pytest.mark.parametrize("B", [5, 777, 4099])
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("name", ["ala2", "ala3", "ala4"])
def test_ff_fused_mala_equals_per_step(pa, name, adaptive, B):
    """fused == launch-per-kernel, bit for bit: walkers, acceptance rates and (adaptive) the final step size; Philox and
    injected noise / uniforms; with and without centring; ragged last tile (B not a multiple of the walkers per block)."""
    steps = 6
    e, _, pos = _energy(name)
    n = SIZES[name]
    x0 = _walkers(pos, B, 100 + B).cuda()
    spy = _Spy(e)
    gen = torch.Generator().manual_seed(B + steps)
    for mean_free in (True, False):
        for inject in (False, True):
            kw = {}
            if inject:
                kw = dict(noise=torch.randn(steps, B, 3 * n, generator=gen).cuda(),
                          uniforms=torch.rand(steps, B, generator=gen).cuda())
            before = spy.taken
            xf, rf, _ = _chain(pa, e, x0, steps, adaptive, True, mean_free, **kw)
            assert spy.taken == before + 1, "the fused chain was not taken"
            dt_fused = float(spy.dt_dev.item())
            xs, rs, _ = _chain(pa, e, x0, steps, adaptive, False, mean_free, **kw)
            assert spy.taken == before + 1
            print(f"[ff mala {name} B={B} adaptive={adaptive} mean_free={mean_free} inject={inject}] rates {rf}")
            assert torch.equal(xf, xs), (mean_free, inject)
            assert rf == rs and len(rf) == steps
            assert torch.isfinite(xf).all() and not torch.equal(xf, x0)
            # the per-kernel chain's step size follows from its rates by mala_adapt_kernel's rule
            assert dt_fused == (_replay_dt(rs) if adaptive else DT)
            if B >= 100:  # a chain that accepts and rejects, and whose adaptive rule moves the step size both ways
                assert max(rf) > 0.55 > min(rf), rf


@pytest.mark.parametrize("adaptive", [False, True])
def test_ff_fused_mala_sets_nonfinite_walker_aside(pa, adaptive):
    """A non-finite walker in the middle is set aside and re-appended last; Philox keys follow the ORIGINAL indices
    (walker_ids) in both paths."""
    B, steps = 777, 6
    e, _, pos = _energy("ala3")
    spy = _Spy(e)
    xb = _walkers(pos, B, 31).cuda()
    xb[B // 3, 1] = float("inf")
    outs = []
    for fused in (True, False):
        x, r, integ = _chain(pa, e, xb, steps, adaptive, fused)
        outs.append((x, r))
    assert spy.taken == 1
    assert torch.equal(outs[0][0][:-1], outs[1][0][:-1]) and outs[0][1] == outs[1][1]
    assert integ._last_mala_valid == B - 1 and torch.isinf(outs[0][0][-1, 1]) and torch.isinf(outs[1][0][-1, 1])
    assert torch.isfinite(outs[0][0][:-1]).all() and len(outs[0][1]) == steps


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("name,gb", [("chain64", True), ("ala2", False)])
def test_ff_fused_mala_large_table_and_no_gb(pa, name, gb, adaptive):
    """chain64: more than 64 KB of interaction tables, fewer walkers per block than 256 / n; ALA2 without the implicit
    solvent: the other branch of the evaluation.  fused == per-step bit for bit."""
    B, steps = 1031, 6
    e, _, pos = _energy(name, gb)
    spy = _Spy(e)
    x0 = _walkers(pos, B, 41).cuda()
    xf, rf, _ = _chain(pa, e, x0, steps, adaptive, True)
    xs, rs, _ = _chain(pa, e, x0, steps, adaptive, False)
    print(f"[ff mala {name} gb={gb} adaptive={adaptive}] rates {rf}")
    assert spy.taken == 1
    assert torch.equal(xf, xs) and rf == rs and len(rf) == steps
    assert torch.isfinite(xf).all() and not torch.equal(xf, x0)
    assert float(spy.dt_dev.item()) == (_replay_dt(rs) if adaptive else DT)


def test_ff_fused_mala_walker_independence(pa):
    """A walker's chain depends neither on the batch it comes in nor on its slot in a block: the rows of the 4 099-walker
    chain equal the chains of sub-batches run with walker_offset = their first row (non-adaptive: the adaptive step size
    depends on the whole batch by definition)."""
    steps = 6
    e, _, pos = _energy("ala4")
    spy = _Spy(e)
    x0 = _walkers(pos, 4099, 8).cuda()
    xf, _, _ = _chain(pa, e, x0, steps, False, True)
    for lo, cnt in ((0, 1), (4098, 1), (3, 7), (2048, 7)):
        xq, _, _ = _chain(pa, e, x0[lo:lo + cnt].contiguous(), steps, False, True, walker_offset=lo)
        assert torch.equal(xq, xf[lo:lo + cnt]), (lo, cnt)
    assert spy.taken == 5


@pytest.mark.parametrize("name", ["ala2", "ala4"])
def test_ff_fused_mala_vs_oracle(pa, name):
    """Three fused steps with injected draws against oracle.mala_step + remove_mean in fp64, step by step (the fused
    chain is rerun with 1, 2, 3 steps from the same start).  The rule and the two bounds of
    test_ff_peptides_gpu.test_peptide_mala_vs_oracle: decisions agree except where the oracle's log-ratio is within 0.1
    of log u; positions agree to rel 1e-5 where all decisions of the walker so far agreed."""
    n = SIZES[name]
    e, ff_t, pos = _energy(name)
    spy = _Spy(e)
    lf = lambda x: O.ff_logp_force(x.double(), ff_t, e.kT, SCALE, 0.45)
    B, steps = 256, 3
    gen = torch.Generator().manual_seed(12)
    x0 = _walkers(pos, B, 13)
    noise = torch.randn(steps, B, 3 * n, generator=gen)
    us = torch.rand(steps, B, generator=gen)
    xd = x0.double()
    lp = lf(xd)[0]
    prev = x0.double()
    agree = torch.ones(B, dtype=torch.bool)
    accepted = 0
    for k in range(steps):
        out, _, _ = _chain(pa, e, x0.cuda(), k + 1, False, True, noise=noise[:k + 1].cuda(), uniforms=us[:k + 1].cuda())
        out = out.cpu().double()
        g0 = lf(xd)[1]
        xp = xd + 0.5 * DT * g0 + np.sqrt(DT) * noise[k].double()
        lpp, gp = lf(xp)
        ratio = (lpp - lp) + (-((xd - xp - 0.5 * DT * gp) ** 2).sum(1) + ((xp - xd - 0.5 * DT * g0) ** 2).sum(1)) / (2 * DT)
        xo, lp_new, acc = O.mala_step(xd, lp, lf, DT, noise[k].double(), torch.log(us[k].double()))
        xo = O.remove_mean(xo, n, 3)
        # the fused chain's decision of this step, for walkers whose history agreed (their previous state is the oracle's)
        hip_acc = (out - prev).norm(dim=1) > 0.5 * (xp - xd).norm(dim=1)
        same = hip_acc == acc
        near = (ratio - torch.log(us[k].double())).abs() < 0.1
        assert bool((same | near | ~agree).all()), (k, int((agree & ~same).sum()), int((agree & ~same & ~near).sum()))
        agree &= same
        print(f"[ff mala oracle {name}] step {k}: histories agree on {int(agree.sum())} of {B}, oracle accepted "
              f"{int(acc.sum())}, rel {rel(out[agree], xo[agree]):.2e}")
        assert rel(out[agree], xo[agree]) < 1e-5
        accepted += int(acc.sum())
        xd, lp, prev = xo, lp_new, out
    assert spy.taken == steps
    assert 0 < accepted < steps * B  # a chain that accepts and rejects
    assert bool(agree.any())  # the position check above was not empty


def test_ff_fused_mala_rerun_bitwise(pa):
    """The 4 099-walker adaptive ALA4 chain twice in one process: identical walkers, rates and step size (the per-step
    counters are integer atomics: nothing depends on the order of the blocks)."""
    steps = 6
    e, _, pos = _energy("ala4")
    spy = _Spy(e)
    x0 = _walkers(pos, 4099, 8).cuda()
    runs = []
    for _ in range(2):
        x, r, _ = _chain(pa, e, x0, steps, True, True)
        runs.append((x, r, float(spy.dt_dev.item())))
    assert spy.taken == 2
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    assert len(runs[0][1]) == steps and runs[0][2] == _replay_dt(runs[0][1])
