"""pita_population_resample and ``WeightedSDEIntegrator(populations=P)``: P independent populations of S walkers, one
resampling event each in one launch.  Run on an MI355X: pytest -m gpu.

Inputs and margins: tests/_populations.py.  The reference of every population is the single-population path
(``sample_cat_sys_adaptive`` on its slice) with ``torch.equal`` / equal bit patterns, and float64 numpy for the
statistics: ``max`` and the counts exactly, ``ess`` to rtol 1e-9 and ``log_mean_weight`` to atol 1e-9 (the derivation of
tests/test_adaptive_resample_gpu.py; the sums here are of at most 2 048 terms), every decision as numpy's."""
import copy

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _populations as PP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def same(r0, r1):
    return all(torch.equal(bits(a), bits(b)) for a, b in zip(r0, r1))


def by_loop(logits, n_pop, theta, u=None, out=None):
    """``sample_cat_sys_populations`` as a loop of single-population events over the slices."""
    from pita_amd.utils import sample_cat_sys_adaptive

    logits = logits.reshape(-1)
    S, dev = logits.numel() // n_pop, logits.device
    if out is None:
        out = (torch.empty(n_pop, device=dev, dtype=torch.int32), torch.empty(n_pop, 6, device=dev, dtype=torch.float64),
               torch.empty(n_pop, device=dev, dtype=torch.int64))
    flags, stats, counts = out
    uh = u.cpu().tolist()
    ids = [sample_cat_sys_adaptive(S, logits[p * S:(p + 1) * S], theta, uh[p], out=(flags[p], stats[p], counts[p]))[0] + p * S
           for p in range(n_pop)]
    nxt = torch.where(flags.repeat_interleave(S) != 0, torch.zeros_like(logits), logits)
    return torch.cat(ids), flags, stats, counts, nxt


def raw_call(pa, a, P, S, u, theta, logw_next, bufs=None):
    """pita_population_resample through the raw entry point: (rc, ids, flags, stats, counts)."""
    L = pa._lib.lib()
    dev = a.device
    if bufs is None:
        bufs = (torch.empty(P * S, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                torch.empty(P, 6, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.int64, device=dev))
    ids, flags, stats, counts = bufs
    ws = torch.empty(max(1, (int(L.pita_population_resample_workspace_bytes(P, S)) + 7) // 8), dtype=torch.float64, device=dev)
    rc = L.pita_population_resample(a.data_ptr(), P, S, u.data_ptr(), theta, ids.data_ptr(), counts.data_ptr(),
                                    stats.data_ptr(), flags.data_ptr(), pa._lib.ptr(logw_next), ws.data_ptr(),
                                    pa._lib.stream_ptr(dev))
    return rc, ids, flags, stats, counts


# ------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("P", PP.POPS)
@pytest.mark.parametrize("S", PP.SIZES)
def test_every_population_is_the_single_population_event(pa, S, P):
    """P = 300: more blocks than the chip has compute units.  P = 1: pita_adaptive_resample, output for output."""
    from pita_amd.utils import sample_cat_sys_populations

    a = torch.from_numpy(PP.batch(S, P)).cuda()
    u = torch.from_numpy(PP.uniforms(P))
    ud = u.cuda()
    ref = np.stack([PP.ref_stats(S, p) for p in range(P)])
    base = torch.arange(P, device="cuda").repeat_interleave(S) * S
    for theta in PP.THETAS:
        got = sample_cat_sys_populations(a, P, theta, ud if theta != 0.6 else u)  # uniforms on the device or on the host
        ids, flags, stats, counts, nxt = got
        assert ids.shape == (P * S,) and flags.shape == (P,) and stats.shape == (P, 6) and counts.shape == (P,)
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
        # where a population did not resample: identity and S distinct parents; its ids stay inside its own rows
        keep = torch.from_numpy(~want).cuda()
        assert torch.equal((ids - base).reshape(P, S)[keep], torch.arange(S, device="cuda").expand(int(keep.sum()), S))
        assert bool((counts[keep] == S).all()) and bool(((ids - base >= 0) & (ids - base < S)).all())
        assert bool(((counts >= 1) & (counts <= S)).all())
        # logw_next out of place and written over the log-weights
        expect = torch.where(flags.repeat_interleave(S) != 0, torch.zeros_like(a), a)
        assert torch.equal(bits(nxt), bits(expect))
        alias = a.clone()
        rc, *raw = raw_call(pa, alias, P, S, ud, theta, alias)
        assert rc == 0 and same(raw, (ids, flags, stats, counts)) and torch.equal(bits(alias), bits(expect))
        rc, *raw = raw_call(pa, a, P, S, ud, theta, None)  # logw_next is optional
        assert rc == 0 and same(raw, (ids, flags, stats, counts))


@pytest.mark.parametrize("S", (63, 1025, 2048))
def test_populations_are_isolated(pa, S):
    """A NaN, a +inf or an all -inf population changes its own event only; permuting the populations permutes the
    outputs; a rerun repeats every bit."""
    from pita_amd.utils import sample_cat_sys_populations

    P, victim = 6, 2
    clean_h = PP.batch(S, P).reshape(P, S).copy()
    u = torch.from_numpy(PP.uniforms(P)).cuda()
    others = [p for p in range(P) if p != victim]
    for theta in (0.0, 0.6):
        clean = sample_cat_sys_populations(torch.from_numpy(clean_h.reshape(-1)).cuda(), P, theta, u)
        assert same(clean, sample_cat_sys_populations(torch.from_numpy(clean_h.reshape(-1)).cuda(), P, theta, u))
        for poison in ("nan", "inf", "all -inf"):
            bad_h = clean_h.copy()
            if poison == "all -inf":
                bad_h[victim] = -np.inf
            else:
                bad_h[victim, S // 3] = np.nan if poison == "nan" else np.inf
            bad = torch.from_numpy(bad_h.reshape(-1)).cuda()
            got = sample_cat_sys_populations(bad, P, theta, u)
            assert same(got, by_loop(bad, P, theta, u)), (S, theta, poison)
            ids, flags, stats, counts, nxt = got
            assert int(flags[victim]) == 1, (S, theta, poison)  # forced at every threshold, theta = 0 included
            row = stats[victim].cpu().numpy()
            assert (row[4], row[5]) == ((0, S) if poison == "all -inf" else (1, 0)) and (poison != "all -inf" or row[2] == 0)
            assert bool((nxt.reshape(P, S)[victim] == 0).all())
            for t_bad, t_clean in zip(got, clean):  # the neighbours: bit-equal to the call without the poison
                rb, rc = t_bad.reshape(P, -1)[others], t_clean.reshape(P, -1)[others]
                assert torch.equal(bits(rb), bits(rc)), (S, theta, poison)
        perm = torch.tensor([3, 0, 5, 1, 2, 4], device="cuda")
        shuffled = torch.from_numpy(clean_h).cuda()[perm].reshape(-1).contiguous()
        got = sample_cat_sys_populations(shuffled, P, theta, u[perm])
        rows = torch.arange(P, device="cuda")[:, None] * S
        assert torch.equal(got[0].reshape(P, S) - rows, (clean[0].reshape(P, S) - rows)[perm])
        for t_got, t_clean in zip(got[1:], clean[1:]):
            assert torch.equal(bits(t_got.reshape(P, -1)), bits(t_clean.reshape(P, -1)[perm]))


def test_host_entry_refuses_a_population_that_does_not_fit(pa):
    from pita_amd.utils import sample_cat_sys_populations

    P, S = 2, PP.MAX_S + 1
    a = torch.from_numpy(PP.batch(PP.MAX_S, 3)).cuda()[:P * S].contiguous()
    u = torch.tensor([0.3, 0.7], dtype=torch.float64, device="cuda")
    with pytest.raises(pa._lib.PitaHipError) as err:
        sample_cat_sys_populations(a, P, 0.5, u)
    assert err.value.code == -2 and str(PP.MAX_S) in str(err.value)
    bufs = (torch.full((P * S,), -7, dtype=torch.int64, device="cuda"), torch.full((P,), -7, dtype=torch.int32, device="cuda"),
            torch.full((P, 6), -7.0, dtype=torch.float64, device="cuda"), torch.full((P,), -7, dtype=torch.int64, device="cuda"))
    nxt = torch.full((P * S,), -7.0, device="cuda")
    rc, *_ = raw_call(pa, a, P, S, u, 0.5, nxt, bufs)
    assert rc == -2
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs) and bool((nxt == -7).all())
    with pytest.raises(ValueError):
        sample_cat_sys_populations(a, 4, 0.5, None)  # 4 098 log-weights do not split into 4 populations
    with pytest.raises(ValueError):
        sample_cat_sys_populations(a[:8], 2, 0.5, torch.tensor([0.3, 1.0], dtype=torch.float64))
    rc, ids, flags, stats, counts = raw_call(pa, a, P, PP.MAX_S, u, 0.5, nxt, bufs)  # the same buffers, a valid call
    assert rc == 0
    ref = by_loop(a[:P * PP.MAX_S], P, 0.5, u)
    assert same((ids[:P * PP.MAX_S], flags, stats, counts, nxt[:P * PP.MAX_S]), ref)


# ------------------------------------------------------------------------------------------------- the integrator
KW = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True, agg="sum")
LJ_STEPS, LJ_S = 8, 64


class _Geometry:  # what WeightedSDEIntegrator reads from the target when nothing evaluates it
    n_particles, n_spatial_dim = 13, 3


@pytest.fixture(scope="module")
def lj13(pa, golden):
    """run(populations, ess_threshold, resample_u) -> (x, logweights, counts, last_weight_stats): the golden LJ13 net
    (hidden 32), 192 walkers, 8 steps, an event every second step, injected noise, no descent and no MALA."""
    from pita_amd.energy_net import EnergyNet

    w = {k: torch.tensor(v) for k, v in golden("egnn_weights_trainedlike.npz").items()}
    net = pa.EGNN_dynamics(13, 3, condition_temperature=True, precision="f16x2", **KW)
    net.load_state_dict({k: v for k, v in w.items() if k in net.state_dict()})
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gen = torch.Generator().manual_seed(22)
    B = 3 * LJ_S
    x1 = (O.remove_mean(torch.randn(B, 39, generator=gen), 13, 3) * 80.0).cuda()
    noise = torch.randn(LJ_STEPS, B, 39, generator=gen).cuda()

    def run(populations, ess_threshold, resample_u, debias=True, at_end=False):
        sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                              debias_inference=debias)
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=LJ_STEPS, start_resampling_step=0,
                                         end_resampling_step=LJ_STEPS, resampling_interval=2, num_negative_time_steps=0,
                                         post_mcmc_steps=0, seed=3, ess_threshold=ess_threshold, populations=populations,
                                         resample_at_end=at_end)
        target = pa.LennardJonesEnergy(39, 13, 3) if at_end else _Geometry()  # the end-of-run reweighting evaluates it
        x, logw, counts, _, _ = integ.integrate_sde(x1, target, pa.ConstantAnnealingFactorSchedule(4 / 3),
                                                    inverse_temperature=1.0, noise=noise, resample_u=resample_u)
        return x, logw, counts, integ.last_weight_stats

    return run


LJ_U = [[0.3, 0.6, 0.9], [0.15, 0.45, 0.75], [0.0, 0.999999, 0.5], [0.21, 0.01, 0.77]]  # [events, populations]


def assert_same_run(r0, r1):
    (x0, w0, c0, s0), (x1, w1, c1, s1) = r0, r1
    assert torch.equal(bits(x0), bits(x1)) and torch.equal(bits(w0), bits(w1)) and c0 == c1
    assert all(isinstance(c, int) for c in c0)
    assert (s0 is None) == (s1 is None)
    if s0 is not None:
        assert list(s0) == list(s1)
        for k in s0:
            assert np.array_equal(s0[k], s1[k], equal_nan=k not in ("resampled", "n_unique", "populations")), k


@pytest.mark.parametrize("ess_threshold", (None, 0.6))
def test_lj13_debiased_in_situ(pa, lj13, monkeypatch, ess_threshold):
    """3 populations x 64 walkers: the run with the kernel equals the run with a loop of single-population events."""
    import pita_amd.sde_integration as SI

    new = lj13(3, ess_threshold, LJ_U)
    calls = []
    monkeypatch.setattr(SI, "sample_cat_sys_populations", lambda *a, **k: calls.append(1) or by_loop(*a, **k))
    old = lj13(3, ess_threshold, LJ_U)
    assert len(calls) == len(LJ_U)  # one call per due event
    assert_same_run(new, old)
    x, logw, counts, st = new
    N, P = LJ_STEPS, 3
    assert logw.shape == (N, P * LJ_S) and len(counts) == N and bool(torch.isfinite(x).all())
    assert st["populations"] == P and st["log_z"].shape == (P,) and st["log_z"].dtype == np.float64
    for k in ("ess", "ess_fraction", "log_mean_weight", "resampled", "n_unique"):
        assert st[k].shape == (N, P), k
    due = np.arange(N) % 2 == 1
    assert np.isfinite(st["ess"][due]).all() and np.isnan(st["ess"][~due]).all() and not st["resampled"][~due].any()
    if ess_threshold is None:
        assert st["resampled"][due].all()
    assert counts == [int(v) for v in st["n_unique"].sum(1)] and all(c == P * LJ_S for c in np.array(counts)[~due])
    rows = logw.cpu().numpy().reshape(N, P, LJ_S)
    for s in np.nonzero(due)[0]:
        for p in range(P):
            assert st["resampled"][s, p] == (not rows[s, p].any())  # the weights are reset exactly where it resampled
            assert st["resampled"][s, p] or st["n_unique"][s, p] == LJ_S
    tail = np.array([PP.np_stats(rows[-1, p])[1] for p in range(P)])
    want = np.where(st["resampled"], st["log_mean_weight"], 0.0).sum(0) + tail
    assert np.abs(st["log_z"] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("debias", (True, False))
@pytest.mark.parametrize("ess_threshold", (None, 0.6))
def test_one_population_is_the_default(pa, lj13, monkeypatch, ess_threshold, debias):
    """populations=1 equals populations=None bit for bit at 192 walkers; populations=None launches no new kernel."""
    import pita_amd.sde_integration as SI

    one = lj13(1, ess_threshold, [[u[0]] for u in LJ_U], debias)

    def refuse(*a, **k):
        raise AssertionError("populations=None must not reach the population kernel")

    monkeypatch.setattr(SI, "sample_cat_sys_populations", refuse)
    monkeypatch.setattr(pa._lib.lib(), "pita_population_resample", refuse)
    none = lj13(None, ess_threshold, [u[0] for u in LJ_U], debias)
    assert torch.equal(bits(one[0]), bits(none[0])) and torch.equal(bits(one[1]), bits(none[1])) and one[2] == none[2]
    s1, s0 = one[3], none[3]
    assert s1["populations"] == 1 and (s0 is None) == (ess_threshold is None)
    if s0 is not None:
        assert s1["log_z"][0] == s0["log_z"]
        for k in ("ess", "ess_fraction", "log_mean_weight", "resampled"):
            assert np.array_equal(s1[k][:, 0], s0[k], equal_nan=k != "resampled"), k


def test_one_population_is_the_default_with_resample_at_end(pa, lj13):
    """The default regime (log-weights identically zero until the end) with ``resample_at_end``: populations=1 equals
    populations=None bit for bit, a threshold of 1 is the fixed schedule, and its events are the due steps."""
    N, U = LJ_STEPS, LJ_U + [[0.62, 0.33, 0.08]]  # four due events and the one at the end
    due = np.arange(N) % 2 == 1
    runs = {}
    for ess_threshold in (None, 0.6, 1.0):
        one = lj13(1, ess_threshold, [[u[0]] for u in U], False, at_end=True)
        none = lj13(None, ess_threshold, [u[0] for u in U], False, at_end=True)
        assert one[1].shape == (N + 1, 3 * LJ_S) and len(one[2]) == N + 1
        assert torch.equal(bits(one[0]), bits(none[0])) and torch.equal(bits(one[1]), bits(none[1])) and one[2] == none[2]
        s1, s0 = one[3], none[3]
        assert s1["populations"] == 1 and (s0 is None) == (ess_threshold is None)
        if s0 is not None:
            assert s1["log_z"][0] == s0["log_z"]
            for k in ("ess", "ess_fraction", "log_mean_weight", "resampled"):
                assert np.array_equal(s1[k][:, 0], s0[k], equal_nan=k != "resampled"), (ess_threshold, k)
        runs[ess_threshold] = (one, none)
    for always, fixed in zip(runs[1.0], runs[None]):
        assert torch.equal(bits(always[0]), bits(fixed[0])) and torch.equal(bits(always[1]), bits(fixed[1]))
        assert always[2] == fixed[2]
    assert np.array_equal(runs[1.0][0][3]["resampled"][:, 0], due) and np.array_equal(runs[1.0][1][3]["resampled"], due)


def _gmm_sde(pa, golden):
    from pita_amd import mlp
    from pita_amd.energy_net import EnergyNet

    s_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
    s_net.load_state_dict({k[2:]: torch.tensor(v) for k, v in golden("mlp_gmm_fwd.npz").items() if k.startswith("w.")})
    torch.manual_seed(17)
    e_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    return lambda debias: pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(s_net), energy_net=EnergyNet(e_net),
                                          debias_inference=debias)


@pytest.mark.parametrize("ess_threshold", (None, 0.6))
def test_gmm_populations_are_separate_runs(pa, golden, ess_threshold):
    """MyMLP on the GMM target, debiased, resample_at_end: one run of 4 x 128 walkers equals, slice by slice and bit for
    bit, the four 128-walker runs (the MLP kernels' per-walker results do not depend on the batch)."""
    sde = _gmm_sde(pa, golden)(True)
    N, P, S = 10, 4, 128
    gen = torch.Generator().manual_seed(79)
    x1 = (torch.randn(P * S, 2, generator=gen) * 40.0).cuda()
    noise = torch.randn(N, P * S, 2, generator=gen).cuda()
    U = torch.rand(N // 2 + 1, P, generator=gen, dtype=torch.float64)  # five due events and the one at the end
    gam, target = pa.ConstantAnnealingFactorSchedule(4 / 3), pa.GMM()

    def run(x, nz, u, populations):
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                         resampling_interval=2, num_negative_time_steps=0, post_mcmc_steps=0,
                                         should_mean_free=False, resample_at_end=True, ess_threshold=ess_threshold,
                                         populations=populations)
        out = integ.integrate_sde(x, target, gam, inverse_temperature=1.0, noise=nz, resample_u=u)
        return out[0], out[1], out[2], integ.last_weight_stats

    x, logw, counts, st = run(x1, noise, U, P)
    assert logw.shape == (N + 1, P * S) and len(counts) == N + 1 and bool(torch.isfinite(logw).all())
    total = np.zeros(N + 1, np.int64)
    for p in range(P):
        sl = slice(p * S, (p + 1) * S)
        xp, wp, cp, sp = run(x1[sl].contiguous(), noise[:, sl].contiguous(), U[:, p].tolist(), None)
        assert torch.equal(bits(x[sl]), bits(xp)), p
        assert torch.equal(bits(logw[:, sl]), bits(wp)), p
        total += np.array(cp)
        assert list(st["n_unique"][:, p]) == cp[:N], p
        if sp is not None:
            assert st["log_z"][p] == sp["log_z"]
            for k in ("ess", "ess_fraction", "log_mean_weight", "resampled"):
                assert np.array_equal(st[k][:, p], sp[k], equal_nan=k != "resampled"), (k, p)
    assert counts == [int(v) for v in total]
    due = np.arange(N) % 2 == 1
    assert st["populations"] == P and st["log_z"].shape == (P,) and np.isfinite(st["log_z"]).all()
    assert np.array_equal(st["resampled"][due], st["ess_fraction"][due] <= (1.0 if ess_threshold is None else ess_threshold))


class _HolesInTheTarget:
    """The GMM target with a non-finite log-density on chosen rows of the FULL batch (what the chain sees first)."""

    def __init__(self, base, B, rows):
        self.base, self.B, self.rows = base, B, rows

    def __call__(self, x, return_force=False):
        out = self.base(x, return_force=return_force)
        if x.shape[0] == self.B:
            logp = out[0] if return_force else out
            logp[self.rows] = torch.tensor([float("nan"), float("-inf"), float("inf")], device=logp.device)[: len(self.rows)]
        return out


def test_set_aside_rows_return_to_their_places(pa, golden):
    """Quirk Q7: walkers whose target log-density is not finite before MALA are set aside; the default appends them
    behind the valid ones, a run with populations puts them back, so that row r stays in population r // S."""
    sde = _gmm_sde(pa, golden)(False)
    N, P, S = 4, 2, 32
    B = P * S
    rows = [5, 40, 63]
    gen = torch.Generator().manual_seed(80)
    x1 = (torch.randn(B, 2, generator=gen) * 40.0).cuda()
    noise = torch.randn(N, B, 2, generator=gen).cuda()
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    U = [[0.3, 0.8], [0.55, 0.05]]

    def run(populations, mala_steps, u):
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                         resampling_interval=2, num_negative_time_steps=0, post_mcmc_steps=mala_steps,
                                         dt_negative_time=1e-3, should_mean_free=False, seed=5, populations=populations)
        return integ.integrate_sde(x1, _HolesInTheTarget(pa.GMM(), B, rows), gam, inverse_temperature=1.0, noise=noise,
                                   resample_u=u)[0]

    before, after = run(P, 0, U), run(P, 3, U)
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[rows] = False
    assert torch.equal(bits(after[rows]), bits(before[rows]))  # set aside, untouched, in their own rows
    assert bool((after[keep] != before[keep]).any(1).sum() >= (B - len(rows)) // 2)  # the chain moved the others
    # the same chain in the default order: [valid, set-aside] (one population, so that the two runs resample alike)
    b1, a1 = run(1, 0, [[u[0]] for u in U]), run(1, 3, [[u[0]] for u in U])
    a0 = run(None, 3, [u[0] for u in U])
    assert torch.equal(bits(a1[rows]), bits(b1[rows]))
    assert torch.equal(bits(a0[:B - len(rows)]), bits(a1[keep])) and torch.equal(bits(a0[B - len(rows):]), bits(b1[rows]))
