"""The per-population MALA chain (``mcmc_per_population=True``; pita_*_mala_pop, pita_mala_{propose,accept,adapt}_pop):
every population's walkers, acceptance rates and final step size equal, bit for bit, the chain as it was run on that
population's slice alone -- on every route, adaptive and not, with set-aside walkers, as a shard of a larger run and
through ``integrate_sde``.  Inputs and the reference: tests/_population_mala.py.  Run on an MI355X: pytest -m gpu."""
import copy

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _population_mala as PM
from tests._population_mala import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def f32(values):
    return torch.tensor(values, dtype=torch.float32)


def assert_population_is_its_slice(got, ref, p, S, adaptive):
    """Population p of the per-population chain ``got`` against its slice chain ``ref[p]``: rows, rates, step size."""
    rows, _, rates, dt_dev, totals = got
    ref_rows, ref_rates, ref_dt = ref[p]
    assert torch.equal(bits(rows[p * S:(p + 1) * S]), bits(ref_rows)), p
    assert torch.equal(bits(rates[:, p].cpu()), bits(f32(ref_rates))), (p, rates[:, p].tolist(), ref_rates)
    assert float(dt_dev[p]) == ref_dt, (p, float(dt_dev[p]), ref_dt)


# ------------------------------------------------------------------------------------------------- cases 1 and 3
@pytest.mark.parametrize("adaptive", (True, False))
@pytest.mark.parametrize("name", list(PM.CASES))
def test_every_population_is_its_slice_chain(pa, golden, name, adaptive):
    """Three populations whose blocks straddle them.  Adaptive: the slice chains end with at least two distinct step sizes
    and the coupled chain returns other bits (conditions of the test, asserted on the reference).  Not adaptive: the
    per-population chain IS the coupled chain -- same walkers, step size untouched, the same accepted walkers per step."""
    case, P = PM.CASES[name], 3
    S = case.S
    e, x = PM.target_and_walkers(pa, golden, case, P)
    spy = PM.FusedSpy(e)
    integ = PM.integrator(pa, case, adaptive)
    ref = PM.slice_chains(integ, e, x, case, P, adaptive)
    coupled, coupled_rates = PM.coupled_chain(integ, e, x, case, adaptive)
    before = spy.taken
    got = PM.population_chain(integ, e, x, case, adaptive)
    rows, pooled, rates, dt_dev, totals = got
    assert spy.taken - before == spy.per_population == int(case.fused), "the route the case names was not the one taken"
    print(f"[population mala {name} adaptive={adaptive}] slice rates {[r[1] for r in ref]} step sizes {[r[2] for r in ref]} "
          f"coupled rates {coupled_rates}")
    assert all(len(r[1]) == case.steps for r in ref) and bool(torch.isfinite(rows).all())
    assert any(max(r[1]) > 0.0 for r in ref)  # a chain that moves
    if adaptive:
        assert len({r[2] for r in ref}) >= 2, "the populations' step sizes never part: the case shows nothing"
        assert any(not torch.equal(bits(coupled[p * S:(p + 1) * S]), bits(ref[p][0])) for p in range(P)), \
            "the coupled chain equals the slice chains: the case cannot tell the feature from its absence"
    for p in range(P):
        assert_population_is_its_slice(got, ref, p, S, adaptive)
    assert rates.shape == (case.steps, P) and rates.dtype == torch.float32
    assert dt_dev.shape == (P,) and dt_dev.dtype == torch.float64 and totals.tolist() == [S] * P
    # the pooled rate per step: sum_p rate_p n_p / sum_p n_p in float64
    want = (rates.cpu().double().numpy() * S).sum(1) / (P * S)
    assert pooled == want.tolist()
    if not adaptive:
        assert torch.equal(bits(rows), bits(coupled))
        assert dt_dev.tolist() == [case.dt] * P
        accepted = np.rint(rates.cpu().double().numpy() * S).sum(1)
        assert accepted.tolist() == np.rint(np.array(coupled_rates) * (P * S)).tolist()


# ------------------------------------------------------------------------------------------------- case 2
@pytest.mark.parametrize("name", ("lj13", "lj13_per_kernel", "dw4"))
def test_set_aside_walkers_and_an_empty_population(pa, golden, name):
    """Three rows of population 1 and all of population 3 have a non-finite log-density (a NaN coordinate): they come back
    untouched in their places, the other populations equal their slice chains (Philox keys follow the original rows, the
    rates are taken over the valid rows), the empty population keeps its step size and has NaN rates."""
    case, P = PM.CASES[name], 4
    S = case.S
    e, x = PM.target_and_walkers(pa, golden, case, P, seed=1)
    holes = [S + 1, S + S // 2, 2 * S - 1]
    x[holes, 0] = float("nan")
    x[3 * S:, 1] = float("nan")
    integ = PM.integrator(pa, case, True)
    ref = PM.slice_chains(integ, e, x, case, P, True)
    got = PM.population_chain(integ, e, x, case, True)
    rows, pooled, rates, dt_dev, totals = got
    assert totals.tolist() == [S, S - 3, S, 0] and integ._last_mala_valid == 3 * S - 3
    gone = holes + list(range(3 * S, 4 * S))
    assert torch.equal(bits(rows[gone]), bits(x[gone]))
    keep = torch.ones(P * S, dtype=torch.bool, device="cuda")
    keep[gone] = False
    assert bool(torch.isfinite(rows[keep]).all()) and bool((rows[keep] != x[keep]).any())
    assert len({r[2] for r in ref[:3]}) >= 2
    for p in range(3):
        assert_population_is_its_slice(got, ref, p, S, True)
    assert ref[3][1] == [] and torch.equal(bits(ref[3][0]), bits(x[3 * S:]))  # the chain as it was: nothing to run
    assert bool(torch.isnan(rates[:, 3]).all()) and float(dt_dev[3]) == case.dt
    nv = np.array([S, S - 3, S], np.float64)
    assert pooled == ((rates[:, :3].cpu().double().numpy() * nv).sum(1) / nv.sum()).tolist()


# ------------------------------------------------------------------------------------------------- case 4
@pytest.mark.parametrize("name", ("lj13", "lj13_per_kernel", "ff22"))
def test_a_shard_is_its_rows_of_the_whole_run(pa, golden, name):
    """What a rank of a two-rank run computes: the two middle populations of four as one call with walker_offset = S (the
    key of its first row, which is also the base of its populations) equal rows [S, 3S) of the four-population call."""
    case, P = PM.CASES[name], 4
    S = case.S
    e, x = PM.target_and_walkers(pa, golden, case, P, seed=2)
    integ = PM.integrator(pa, case, True)
    rows, _, rates, dt_dev, _ = PM.population_chain(integ, e, x, case, True)
    shard = PM.population_chain(integ, e, x[S:3 * S].contiguous(), case, True, base=S)
    assert torch.equal(bits(shard[0]), bits(rows[S:3 * S]))
    assert torch.equal(bits(shard[2]), bits(rates[:, 1:3])) and torch.equal(bits(shard[3]), bits(dt_dev[1:3]))
    assert len(set(dt_dev.tolist())) >= 2


# ------------------------------------------------------------------------------------------------- cases 5 and 6
KW = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True, agg="sum")


def _lj13_leg(pa, golden):
    """LJ13, not debiased, the fused sampler, N = 4: 2 populations of 64 walkers near the minimum (A, B) or hot (C)."""
    from pita_amd.energy_net import EnergyNet

    w = {k: torch.tensor(v) for k, v in golden("egnn_weights_trainedlike.npz").items()}
    net = pa.EGNN_dynamics(13, 3, condition_temperature=True, precision="f16x2", **KW)
    net.load_state_dict({k: v for k, v in w.items() if k in net.state_dict()})
    # a schedule that ends where it starts, close to the data: the walkers reach the chain as cold or as hot as they set out
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.001, sigma_max=0.004, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=False)
    S, gen = 64, torch.Generator().manual_seed(41)
    base = torch.tensor(golden("post_lj13.npz")["x0"], dtype=torch.float32)
    base = base[torch.arange(S) % base.shape[0]]
    A, B, C = (O.remove_mean(base + sd * torch.randn(S, 39, generator=gen), 13, 3).cuda() for sd in (0.004, 0.006, 0.25))
    kw = dict(sde=sde, num_integration_steps=4, start_resampling_step=0, end_resampling_step=4, resampling_interval=2,
              num_negative_time_steps=0, post_mcmc_steps=8, dt_negative_time=1.2e-3, seed=3)
    return kw, pa.LennardJonesEnergy(39, 13, 3), (A, B, C), S


def _gmm_leg(pa, golden):
    """The GMM + MLP SDE of tests/test_populations_gpu.py on a short, cold schedule: walkers at the modes (A, B) or far
    from them (C)."""
    from pita_amd import mlp
    from pita_amd.energy_net import EnergyNet

    s_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
    s_net.load_state_dict({k[2:]: torch.tensor(v) for k, v in golden("mlp_gmm_fwd.npz").items() if k.startswith("w.")})
    torch.manual_seed(17)
    e_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=0.05, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(s_net), energy_net=EnergyNet(e_net),
                          debias_inference=False)
    target = pa.GMM()
    S, gen = 32, torch.Generator().manual_seed(42)
    locs = target.locs.cpu()
    A, B, C = ((locs[torch.randint(0, locs.shape[0], (S,), generator=gen)] + sd * torch.randn(S, 2, generator=gen)).cuda()
               for sd in (0.3, 0.5, 9.0))
    kw = dict(sde=sde, num_integration_steps=4, start_resampling_step=0, end_resampling_step=4, resampling_interval=2,
              num_negative_time_steps=0, post_mcmc_steps=8, dt_negative_time=3.0, should_mean_free=False, seed=5)
    return kw, target, (A, B, C), S


@pytest.mark.parametrize("leg", (_lj13_leg, _gmm_leg), ids=("lj13", "gmm"))
def test_through_integrate_sde(pa, golden, leg):
    """populations=2, adaptive_mcmc=True: with mcmc_per_population the runs [A, B] and [A, C] return the same bits for
    population 0; without it they do not (the condition of the test).  last_mcmc_stats has the stated shapes and is None
    without the mode; a run twice gives the same bits; acceptance_rate_list is the pooled rate of last_mcmc_stats."""
    kw, target, (A, B, C), S = leg(pa, golden)
    gam, U = pa.ConstantAnnealingFactorSchedule(4 / 3), [[0.3, 0.8], [0.55, 0.05]]
    steps = kw["post_mcmc_steps"]

    def run(x1, per_population):
        integ = pa.WeightedSDEIntegrator(populations=2, adaptive_mcmc=True, mcmc_per_population=per_population, **kw)
        out = integ.integrate_sde(x1, target, gam, inverse_temperature=1.0, resample_u=U)
        return out[0], out[4], integ.last_mcmc_stats

    ab, ac = torch.cat([A, B]), torch.cat([A, C])
    (x_ab, r_ab, s_ab), (x_ac, r_ac, s_ac) = run(ab, True), run(ac, True)
    (c_ab, cr_ab, cs_ab), (c_ac, cr_ac, _) = run(ab, False), run(ac, False)
    print(f"[population mala integrate_sde] per population: {s_ab['acceptance_rate'].T.tolist()} / "
          f"{s_ac['acceptance_rate'].T.tolist()} step sizes {s_ab['step_size']} / {s_ac['step_size']}; coupled {cr_ab} / {cr_ac}")
    assert cs_ab is None
    assert not torch.equal(bits(c_ab[:S]), bits(c_ac[:S])), "the coupled chains agree on population 0: nothing to show"
    assert torch.equal(bits(x_ab[:S]), bits(x_ac[:S]))
    assert not torch.equal(bits(x_ab[S:]), bits(x_ac[S:])) and bool(torch.isfinite(x_ab).all())
    for s in (s_ab, s_ac):
        assert sorted(s) == ["acceptance_rate", "n_valid", "step_size"]
        assert s["acceptance_rate"].shape == (steps, 2) and s["acceptance_rate"].dtype == np.float32
        assert s["step_size"].shape == (2,) and s["step_size"].dtype == np.float64
        assert s["n_valid"].shape == (2,) and s["n_valid"].dtype == np.int64
    assert np.array_equal(s_ab["acceptance_rate"][:, 0], s_ac["acceptance_rate"][:, 0])
    assert s_ab["step_size"][0] == s_ac["step_size"][0] and s_ac["step_size"][0] != s_ac["step_size"][1]
    for r, s in ((r_ab, s_ab), (r_ac, s_ac)):
        nv = s["n_valid"].astype(np.float64)
        assert len(r) == steps and r == ((s["acceptance_rate"].astype(np.float64) * nv).sum(1) / nv.sum()).tolist()
    again = run(ac, True)
    assert torch.equal(bits(again[0]), bits(x_ac)) and again[1] == r_ac
    assert all(np.array_equal(again[2][k], s_ac[k]) for k in s_ac)


def test_flag_off_is_the_chain_as_it_was(pa, golden, monkeypatch):
    """populations=P without the mode: no per-population entry point is reached, and the run is the run without the chain
    followed by ``_mala(..., keep_order=True)`` called as before (``_mala`` does not advance the run counter, so the
    Philox keys agree), bit for bit."""
    kw, target, (A, B, C), S = _lj13_leg(pa, golden)
    L = pa._lib.lib()

    def refuse(*a, **k):
        raise AssertionError("mcmc_per_population=False must not reach the per-population entry points")

    for symbol in ("pita_lj_mala_pop", "pita_mala_propose_pop", "pita_mala_accept_pop", "pita_mala_adapt_pop"):
        monkeypatch.setattr(L, symbol, refuse)
    gam, U, x1 = pa.ConstantAnnealingFactorSchedule(4 / 3), [[0.3, 0.8], [0.55, 0.05]], torch.cat([A, C])
    steps, dt = kw.pop("post_mcmc_steps"), kw["dt_negative_time"]
    whole = pa.WeightedSDEIntegrator(populations=2, adaptive_mcmc=True, post_mcmc_steps=steps, **kw)
    assert whole.mcmc_per_population is False
    x, _, _, _, rates = whole.integrate_sde(x1, target, gam, inverse_temperature=1.0, resample_u=U)
    assert whole.last_mcmc_stats is None and len(rates) == steps
    parts = pa.WeightedSDEIntegrator(populations=2, adaptive_mcmc=True, post_mcmc_steps=0, **kw)
    before = parts.integrate_sde(x1, target, gam, inverse_temperature=1.0, resample_u=U)[0]
    parts.post_mcmc_steps = steps
    want = parts._mala(before, target, True, dt, keep_order=True, return_acceptance_rate=True)
    assert torch.equal(bits(x), bits(want[0])) and rates == want[1] and not torch.equal(bits(x), bits(before))
