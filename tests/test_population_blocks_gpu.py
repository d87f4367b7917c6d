"""pita_population_resample_blocks and ``WeightedSDEIntegrator(populations=P)`` beyond 2 048 walkers per population: P
independent populations of ANY size, one resampling event each in a fixed number of launches.  Run on an MI355X:
pytest -m gpu.

Inputs: tests/_populations.py at the shapes of tests/_population_blocks.py.  The reference of every population is the
single-population path (``sample_cat_sys_adaptive`` on its slice) with equal bit patterns, and float64 numpy for the
statistics: ``max`` and the counts exactly, ``ess`` and ``ess_fraction`` to rtol 1e-9 and ``log_mean_weight`` to atol
1e-9 (sums of at most 5 000 non-negative doubles: relative error <= 5000 * 2^-53 ~ 5.6e-13 in any order), every decision
as numpy's (margins: tests/test_population_blocks_cpu.py)."""
import numpy as np
import pytest
import torch

from tests import _population_blocks as PB
from tests import _population_mala as PM
from tests import _populations as PP
from tests._population_blocks import bits, by_loop, raw_call, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


# ------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("S,P", PB.SHAPES)
def test_every_population_is_the_single_population_event(pa, S, P):
    from pita_amd.utils import sample_cat_sys_population_blocks

    a = torch.from_numpy(PP.batch(S, P)).cuda()
    u = torch.from_numpy(PP.uniforms(P))
    ud = u.cuda()
    ref = np.stack([PP.ref_stats(S, p) for p in range(P)])
    base = torch.arange(P, device="cuda").repeat_interleave(S) * S
    for theta in PP.THETAS:
        got = sample_cat_sys_population_blocks(a, P, theta, ud if theta != 0.6 else u)  # uniforms on the device or the host
        ids, flags, stats, counts, nxt = got
        assert ids.shape == (P * S,) and flags.shape == (P,) and stats.shape == (P, 6) and counts.shape == (P,)
        assert nxt.shape == (P * S,) and nxt.dtype == torch.float32
        assert same(got, by_loop(a, P, theta, u)), (S, P, theta)
        # float64 numpy: the statistics and every decision
        h = stats.cpu().numpy()
        assert np.array_equal(h[:, [0, 4, 5]], ref[:, [0, 4, 5]])
        np.testing.assert_allclose(h[:, 2], ref[:, 2], rtol=1e-9, atol=0)
        np.testing.assert_allclose(h[:, 3], ref[:, 3], rtol=1e-9, atol=0)
        assert np.abs(h[:, 1] - ref[:, 1]).max() <= 1e-9
        want = np.array([PP.expect_event(ref[p], theta, S) for p in range(P)])
        assert np.array_equal(flags.cpu().numpy() != 0, want), (S, P, theta)
        assert want.all() or theta < 1.0
        # where a population did not resample: identity and S distinct parents; ids stay inside their own rows
        keep = torch.from_numpy(~want).cuda()
        assert torch.equal((ids - base).reshape(P, S)[keep], torch.arange(S, device="cuda").expand(int(keep.sum()), S))
        assert bool((counts[keep] == S).all()) and bool(((ids - base >= 0) & (ids - base < S)).all())
        assert bool(((counts >= 1) & (counts <= S)).all())
        # logw_next out of place, written over the log-weights, and left out; n_unique left out
        expect = torch.where(flags.repeat_interleave(S) != 0, torch.zeros_like(a), a)
        assert torch.equal(bits(nxt), bits(expect))
        alias = a.clone()
        rc, *raw = raw_call(pa, alias, P, S, ud, theta, alias)
        assert rc == 0 and same(raw, (ids, flags, stats, counts)) and torch.equal(bits(alias), bits(expect))
        rc, *raw = raw_call(pa, a, P, S, ud, theta, None)
        assert rc == 0 and same(raw, (ids, flags, stats, counts))
        bufs = PB.sentinel_buffers(P, S)
        rc, *raw = raw_call(pa, a, P, S, ud, theta, None, bufs, with_counts=False)
        assert rc == 0 and same(raw[:3], (ids, flags, stats)) and bool((bufs[3] == -7).all())


@pytest.mark.parametrize("P", (1, 3))
@pytest.mark.parametrize("S", PB.SMALL_SIZES)
def test_two_routes_same_bits(pa, S, P):
    """Where one block holds a population both entry points exist: output for output the same."""
    from pita_amd.utils import sample_cat_sys_population_blocks, sample_cat_sys_populations

    a = torch.from_numpy(PP.batch(S, P)).cuda()
    u = torch.from_numpy(PP.uniforms(P)).cuda()
    for theta in PP.THETAS:
        assert same(sample_cat_sys_population_blocks(a, P, theta, u), sample_cat_sys_populations(a, P, theta, u)), theta


def test_more_populations_than_grid_rows(pa):
    """70 000 populations of 3 walkers: beyond the 65 535 rows of a grid's second dimension the blocks stride over the
    populations.  The reference is the one-launch route (a loop of 70 000 single events would take minutes)."""
    from pita_amd.utils import sample_cat_sys_population_blocks, sample_cat_sys_populations

    P, S = 70000, 3
    gen = torch.Generator().manual_seed(91)
    a = (torch.randn(P * S, generator=gen) * 2.0).cuda()
    u = torch.rand(P, generator=gen, dtype=torch.float64).cuda()
    for theta in (1.0, 0.6):
        got, ref = sample_cat_sys_population_blocks(a, P, theta, u), sample_cat_sys_populations(a, P, theta, u)
        assert same(got, ref), theta
        assert 0 < int(ref[1][65535:].sum()) and (theta == 1.0 or int(ref[1][65535:].sum()) < P - 65535)


@pytest.mark.parametrize("S", (2049, 4097))
def test_populations_are_isolated(pa, S):
    """A NaN, a +inf or an all -inf population changes its own event only and is forced at every theta; permuting the
    populations permutes the outputs; a rerun repeats every bit."""
    from pita_amd.utils import sample_cat_sys_population_blocks as blocks

    P, victim = 6, 2
    clean_h = PP.batch(S, P).reshape(P, S).copy()
    u = torch.from_numpy(PP.uniforms(P)).cuda()
    others = [p for p in range(P) if p != victim]
    for theta in PP.THETAS:
        clean = blocks(torch.from_numpy(clean_h.reshape(-1)).cuda(), P, theta, u)
        assert same(clean, blocks(torch.from_numpy(clean_h.reshape(-1)).cuda(), P, theta, u))
        for poison in ("nan", "inf", "all -inf"):
            bad_h = clean_h.copy()
            if poison == "all -inf":
                bad_h[victim] = -np.inf
            else:
                bad_h[victim, S // 3] = np.nan if poison == "nan" else np.inf
            bad = torch.from_numpy(bad_h.reshape(-1)).cuda()
            got = blocks(bad, P, theta, u)
            assert same(got, by_loop(bad, P, theta, u)), (S, theta, poison)
            ids, flags, stats, counts, nxt = got
            assert int(flags[victim]) == 1, (S, theta, poison)  # forced at every threshold, theta = 0 included
            row = stats[victim].cpu().numpy()
            assert (row[4], row[5]) == ((0, S) if poison == "all -inf" else (1, 0)) and (poison != "all -inf" or row[2] == 0)
            assert bool((nxt.reshape(P, S)[victim] == 0).all())
            own = ids.reshape(P, S)[victim] - victim * S
            assert bool(((own >= 0) & (own < S)).all())
            for t_bad, t_clean in zip(got, clean):  # the neighbours: bit-equal to the call without the poison
                assert torch.equal(bits(t_bad.reshape(P, -1)[others]), bits(t_clean.reshape(P, -1)[others])), (S, theta, poison)
        perm = torch.tensor([3, 0, 5, 1, 2, 4], device="cuda")
        shuffled = torch.from_numpy(clean_h).cuda()[perm].reshape(-1).contiguous()
        got = blocks(shuffled, P, theta, u[perm])
        rows = torch.arange(P, device="cuda")[:, None] * S
        assert torch.equal(got[0].reshape(P, S) - rows, (clean[0].reshape(P, S) - rows)[perm])
        for t_got, t_clean in zip(got[1:], clean[1:]):
            assert torch.equal(bits(t_got.reshape(P, -1)), bits(t_clean.reshape(P, -1)[perm]))


def test_a_refused_call_touches_no_device_buffer(pa):
    """Invalid arguments with DEVICE buffers: PITA_EINVAL, the sentinels stay, and the same buffers serve a valid call."""
    P, S = 2, 2049
    a = torch.from_numpy(PP.batch(S, P)).cuda()
    u = torch.tensor([0.3, 0.7], dtype=torch.float64, device="cuda")
    bufs = PB.sentinel_buffers(P, S)
    nxt = torch.full((P * S,), -7.0, device="cuda")
    for kw in (dict(P=0), dict(S=0), dict(theta=1.5), dict(theta=float("nan")), dict(theta=-0.25)):
        args = dict(dict(P=P, S=S, theta=0.5), **kw)
        rc, *_ = raw_call(pa, a, args["P"], args["S"], u, args["theta"], nxt, bufs)
        assert rc == -1 and "pita_population_resample_blocks" in pa._lib.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs) and bool((nxt == -7).all())
    rc, *raw = raw_call(pa, a, P, S, u, 0.5, nxt, bufs)
    assert rc == 0 and same(raw + [nxt], by_loop(a, P, 0.5, u))


# ------------------------------------------------------------------------------------------------- the integrator
def _gmm_sde(pa, golden, debias, sigma_max):
    from pita_amd import mlp
    from pita_amd.energy_net import EnergyNet

    s_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
    s_net.load_state_dict({k[2:]: torch.tensor(v) for k, v in golden("mlp_gmm_fwd.npz").items() if k.startswith("w.")})
    torch.manual_seed(17)
    e_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=sigma_max, rho=7)
    return pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(s_net), energy_net=EnergyNet(e_net),
                           debias_inference=debias)


def _gmm_run(pa, sde, N, ess_threshold):
    gam, target = pa.ConstantAnnealingFactorSchedule(4 / 3), pa.GMM()

    def run(x, nz, u, populations):
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                         resampling_interval=2, num_negative_time_steps=0, post_mcmc_steps=0,
                                         should_mean_free=False, resample_at_end=True, ess_threshold=ess_threshold,
                                         populations=populations)
        out = integ.integrate_sde(x, target, gam, inverse_temperature=1.0, noise=nz, resample_u=u)
        return out[0], out[1], out[2], integ.last_weight_stats

    return run


@pytest.mark.parametrize("P,S", ((2, 2049), (3, 3000)))
@pytest.mark.parametrize("ess_threshold", (None, 0.6))
def test_gmm_populations_are_separate_runs(pa, golden, monkeypatch, ess_threshold, P, S):
    """MyMLP on the GMM target, debiased, an event every second step, resample_at_end: one run of P x S walkers equals,
    slice by slice and bit for bit, the P runs of S walkers with populations=None.  Every event of the run takes the
    multi-block route, none the one-launch one."""
    import pita_amd.sde_integration as SI

    N = 10
    run = _gmm_run(pa, _gmm_sde(pa, golden, True, 80.0), N, ess_threshold)
    gen = torch.Generator().manual_seed(79)
    x1 = (torch.randn(P * S, 2, generator=gen) * 40.0).cuda()
    noise = torch.randn(N, P * S, 2, generator=gen).cuda()
    U = torch.rand(N // 2 + 1, P, generator=gen, dtype=torch.float64)  # five due events and the one at the end
    slices = [run(x1[p * S:(p + 1) * S].contiguous(), noise[:, p * S:(p + 1) * S].contiguous(), U[:, p].tolist(), None)
              for p in range(P)]

    def refuse(*a, **k):
        raise AssertionError("a population beyond 2 048 walkers must not reach the one-launch event")

    calls, inner = [], SI.sample_cat_sys_population_blocks
    monkeypatch.setattr(SI, "sample_cat_sys_populations", refuse)
    monkeypatch.setattr(SI, "sample_cat_sys_population_blocks", lambda *a, **k: calls.append(1) or inner(*a, **k))
    x, logw, counts, st = run(x1, noise, U, P)
    assert len(calls) == N // 2 + 1
    assert logw.shape == (N + 1, P * S) and len(counts) == N + 1 and bool(torch.isfinite(logw).all())
    total = np.zeros(N + 1, np.int64)
    for p, (xp, wp, cp, sp) in enumerate(slices):
        sl = slice(p * S, (p + 1) * S)
        assert torch.equal(bits(x[sl]), bits(xp)), p
        assert torch.equal(bits(logw[:, sl]), bits(wp)), p
        total += np.array(cp)
        assert list(st["n_unique"][:, p]) == cp[:N], p
        assert (sp is None) == (ess_threshold is None)
        if sp is not None:
            assert st["log_z"][p] == sp["log_z"]
            for k in ("ess", "ess_fraction", "log_mean_weight", "resampled"):
                assert np.array_equal(st[k][:, p], sp[k], equal_nan=k != "resampled"), (k, p)
    assert counts == [int(v) for v in total]
    due = np.arange(N) % 2 == 1
    assert st["populations"] == P and st["log_z"].shape == (P,) and np.isfinite(st["log_z"]).all()
    assert np.array_equal(st["resampled"][due], st["ess_fraction"][due] <= (1.0 if ess_threshold is None else ess_threshold))
    assert st["n_unique"][due].max() <= S and (st["n_unique"][~due] == S).all()


def test_small_populations_keep_the_one_launch_event(pa, golden, monkeypatch):
    """Routing guard: at S = 128 the integrator calls ``sample_cat_sys_populations`` and never the multi-block entry."""
    import pita_amd.sde_integration as SI

    N, P, S = 4, 2, 128
    run = _gmm_run(pa, _gmm_sde(pa, golden, True, 80.0), N, 0.6)
    gen = torch.Generator().manual_seed(83)
    x1 = (torch.randn(P * S, 2, generator=gen) * 40.0).cuda()
    noise = torch.randn(N, P * S, 2, generator=gen).cuda()
    U = torch.rand(N // 2 + 1, P, generator=gen, dtype=torch.float64)

    def refuse(*a, **k):
        raise AssertionError("a population of 128 walkers must not reach the multi-block event")

    calls, inner = [], SI.sample_cat_sys_populations
    monkeypatch.setattr(SI, "sample_cat_sys_population_blocks", refuse)
    monkeypatch.setattr(pa._lib.lib(), "pita_population_resample_blocks", refuse)
    monkeypatch.setattr(SI, "sample_cat_sys_populations", lambda *a, **k: calls.append(1) or inner(*a, **k))
    x, logw, counts, st = run(x1, noise, U, P)
    assert len(calls) == N // 2 + 1 and bool(torch.isfinite(x).all()) and st["populations"] == P


def test_per_population_mala_beyond_one_block(pa, golden):
    """2 x 2 049 walkers through ``integrate_sde`` with ``mcmc_per_population=True`` (the GMM leg of
    tests/test_population_mala_gpu.py: a short cold schedule, population 0 at the modes, population 1 far from them):
    each population's rows, rates and final step size equal the chain as it was on its slice alone.

    The inputs are chosen so that the two step sizes part: near a mode the target is a Gaussian of variance 1.72, where a
    chain forgets its start within a few steps and every population then hovers at the 0.55 threshold of the adaptation
    alike.  So the chain is short and starts at a step size of 5: a float64 numpy model of it (2 049 walkers, four seeds)
    accepts 0.38-0.40 then 0.47-0.48 of the walkers started 0.1 from the modes (the step size falls twice) and 0.79-0.82
    then 0.61-0.63 of those started 20 from them (it rises twice) -- every rate at least 0.06 from the threshold, five
    standard deviations of a rate over 2 049 walkers (0.011)."""
    case = PM.Case("gmm", False, 2049, 2, 5.0, (0.1, 20.0))
    P, S = 2, case.S
    target = pa.GMM()
    gen = torch.Generator().manual_seed(42)
    locs = target.locs.cpu()
    x1 = torch.cat([locs[torch.randint(0, locs.shape[0], (S,), generator=gen)] + sd * torch.randn(S, 2, generator=gen)
                    for sd in case.jitter]).cuda()
    kw = dict(sde=_gmm_sde(pa, golden, False, 0.05), num_integration_steps=4, start_resampling_step=0,
              end_resampling_step=4, resampling_interval=2, num_negative_time_steps=0, dt_negative_time=case.dt,
              should_mean_free=False, seed=5, populations=P, adaptive_mcmc=True)
    gam, U = pa.ConstantAnnealingFactorSchedule(4 / 3), [[0.3, 0.8], [0.55, 0.05]]
    whole = pa.WeightedSDEIntegrator(post_mcmc_steps=case.steps, mcmc_per_population=True, **kw)
    x = whole.integrate_sde(x1, target, gam, inverse_temperature=1.0, resample_u=U)[0]
    got = whole.last_mcmc_stats
    # the reference: the same run without the chain, then the chain as it was on every slice (``_mala`` does not advance
    # the run counter, so the Philox keys agree)
    parts = pa.WeightedSDEIntegrator(post_mcmc_steps=0, **kw)
    before = parts.integrate_sde(x1, target, gam, inverse_temperature=1.0, resample_u=U)[0]
    parts.post_mcmc_steps = case.steps
    ref = PM.slice_chains(parts, target, before, case, P, True)
    assert got["acceptance_rate"].shape == (case.steps, P) and got["n_valid"].tolist() == [S] * P
    for p, (rows, rates, dt) in enumerate(ref):
        assert torch.equal(bits(x[p * S:(p + 1) * S]), bits(rows)), p
        assert np.array_equal(got["acceptance_rate"][:, p], np.array(rates, np.float32)), p
        assert got["step_size"][p] == dt, p
    assert ref[0][2] != ref[1][2], "the populations' step sizes never part: the case shows nothing"
    assert not torch.equal(bits(x), bits(before))
