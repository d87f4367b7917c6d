"""pita_logweight_stats / pita_adaptive_resample and ``WeightedSDEIntegrator(ess_threshold=...)``: resampling events
decided on the device from the effective sample size of the log-weights.  Run on an MI355X: pytest -m gpu.

Inputs: ``a = float32(s * default_rng(1000 + B).standard_normal(B))`` for B = 1 and 2 walkers, a partial wave, one and two
virtual blocks of 1 024, the last one-launch size (2 048, the measured threshold: DESIGN.md 4.4), the first gated size
(2 049), 16 384 and 16 385 and a ragged multi-block size, s = 0, 0.5, 1, 2.  The reference of the statistics is numpy in
float64; its ESS fractions of these inputs lie at least 0.05 away from the two intermediate thresholds (0.6 and 0.2,
asserted below), so no decision hinges on rounding.

Tolerances: every sum is of at most 2^20 non-negative doubles, in any order relative error <= B * 2^-53 ~ 1.2e-10 per
sum, three sums in the ESS ratio: ``ess`` to rtol 1e-9, ``log_mean_weight`` to atol 1e-9, ``max`` and the counts exactly.
Where an event resamples the ids are pita_systematic_resample's with ``torch.equal``, for any input."""
import copy

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 1024, 1025, 2048, 2049, 16384, 16385, 70001)
SCALES = (0, 0.5, 1, 2)
THETAS = (1.0, 0.6, 0.2, 0.0)
U0S = (0.0, 0.3, 0.999999)
EDGE_SIZES = (2048, 16385)
KW = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True, agg="sum")


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def weights(B, s):
    return np.float32(s * np.random.default_rng(1000 + B).standard_normal(B))


def np_stats(a):
    """(max, log mean weight, ess, ess / B, #NaN or +inf, #-inf) of float32 log-weights in float64 numpy."""
    a = np.asarray(a, np.float64)
    bad = np.isnan(a) | (a == np.inf)
    ninf = a == -np.inf
    fin = a[~(bad | ninf)]
    m = fin.max() if fin.size else 0.0
    w = np.exp(fin - m)
    s1, s2 = w.sum(), (w * w).sum()
    ess = s1 * s1 / s2 if s1 > 0 else 0.0
    with np.errstate(divide="ignore"):
        lmw = m + np.log(s1 / a.size)
    return np.array([m, lmw, ess, ess / a.size, bad.sum(), ninf.sum()], np.float64)


def expect_event(st, theta, B):
    return theta >= 1.0 or st[4] > 0 or st[2] <= theta * B


def lib_stats(pa, a):
    """pita_logweight_stats through the raw entry point: float64 [6] on the device."""
    L = pa._lib.lib()
    out = torch.full((6,), -1.0, dtype=torch.float64, device=a.device)
    assert L.pita_logweight_stats_workspace_bytes(a.numel()) == 0
    pa._lib.check(L.pita_logweight_stats(a.data_ptr(), a.numel(), out.data_ptr(), None, pa._lib.stream_ptr(a.device)))
    return out


def assert_stats(got, ref):
    got = np.asarray(got, np.float64)
    assert got[0] == ref[0] and got[4] == ref[4] and got[5] == ref[5], (got, ref)
    if np.isfinite(ref[1]):
        assert abs(got[1] - ref[1]) <= 1e-9, (got, ref)
    else:
        assert got[1] == ref[1], (got, ref)
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got[3], ref[3], rtol=1e-9, atol=0)


def reference_ids(a, u0):
    from pita_amd.sde_integration import _count_distinct
    from pita_amd.utils import sample_cat_sys

    ids, _ = sample_cat_sys(a.numel(), a, u0)
    return ids, int(_count_distinct(ids))


def check_event(pa, a, theta, u0, ref, ref_ids=None):
    """One adaptive event against the numpy decision and (where it resamples) the fixed-schedule kernels."""
    from pita_amd.utils import sample_cat_sys_adaptive

    B = a.numel()
    ids, resampled, stats, n_unique = sample_cat_sys_adaptive(B, a, theta, u0)
    want = bool(expect_event(ref, theta, B))
    assert bool(resampled.item()) == want, (B, theta, u0, stats.tolist(), ref)
    assert torch.equal(bits(stats), bits(lib_stats(pa, a)))  # the event's statistics are pita_logweight_stats', bit for bit
    if want:
        rid, rn = ref_ids if ref_ids is not None else reference_ids(a, u0)
        assert torch.equal(ids, rid), (B, theta, u0)
        assert int(n_unique) == rn
    else:
        assert torch.equal(ids, torch.arange(B, device=a.device)) and int(n_unique) == B
    return want


def check_documented_fraction(B, s, f):
    """The fp64 ESS fractions of the inputs as documented with them, and their distance from the intermediate thresholds."""
    if s == 0:
        assert f == 1.0
    elif s == 0.5:
        assert f >= 0.766
    elif B >= 63:
        assert (0.352 <= f <= 0.444) if s == 1 else f <= 0.090
    elif B == 2:
        assert abs(f - (0.6705 if s == 1 else 0.5309)) < 5e-5
    assert min(abs(f - 0.6), abs(f - 0.2)) >= 0.05, (B, s, f)


@pytest.mark.parametrize("B", SIZES)
def test_stats_against_fp64_numpy(pa, B):
    from pita_amd.metrics import logweight_stats

    for s in SCALES:
        a_h = weights(B, s)
        ref = np_stats(a_h)
        check_documented_fraction(B, s, ref[3])
        a = torch.from_numpy(a_h).cuda()
        got = lib_stats(pa, a)
        assert_stats(got.cpu().numpy(), ref)
        d = logweight_stats(a)
        assert list(d) == ["max", "log_mean_weight", "ess", "ess_fraction", "n_bad", "n_neg_inf"]
        assert all(isinstance(v, float) for v in d.values())
        assert np.array_equal(np.array(list(d.values())), got.cpu().numpy())


def test_stats_of_a_matrix_go_row_by_row(pa):
    from pita_amd.metrics import logweight_stats

    rows = np.stack([weights(1025, s) for s in SCALES])
    d = logweight_stats(torch.from_numpy(rows).cuda())
    for k in range(len(SCALES)):
        one = logweight_stats(torch.from_numpy(rows[k]).cuda())
        for name, v in d.items():
            assert v.shape == (len(SCALES),) and v.dtype == np.float64 and v[k] == one[name]


@pytest.mark.parametrize("B", SIZES)
def test_ids_follow_the_numpy_decision(pa, B):
    for s in SCALES:
        a_h = weights(B, s)
        ref = np_stats(a_h)
        a = torch.from_numpy(a_h).cuda()
        for u0 in U0S:
            ref_ids = reference_ids(a, u0)
            for theta in THETAS:
                took = check_event(pa, a, theta, u0, ref, ref_ids)
                assert took or theta < 1.0   # theta = 1 resamples on every input, s = 0 included
                assert not (took and theta == 0.0)  # theta = 0 never resamples on these inputs
        assert_stats(_event_stats(a, 0.6), ref)


def _event_stats(a, theta):
    from pita_amd.utils import sample_cat_sys_adaptive

    return sample_cat_sys_adaptive(a.numel(), a, theta, 0.3)[2].cpu().numpy()


@pytest.mark.parametrize("B", EDGE_SIZES)
def test_edge_inputs(pa, B):
    base = weights(B, 1)
    rng = np.random.default_rng(7)

    dominant = np.zeros(B, np.float32)
    dominant[7] = 80.0
    ref = np_stats(dominant)
    assert abs(ref[2] - 1.0) < 1e-6
    a = torch.from_numpy(dominant).cuda()
    assert_stats(lib_stats(pa, a).cpu().numpy(), ref)
    for theta in THETAS:
        assert check_event(pa, a, theta, 0.3, ref) == (theta > 0.0)  # ESS ~ 1: taken at every positive threshold

    some = base.copy()
    some[rng.choice(B, 100, replace=False)] = -np.inf
    ref = np_stats(some)
    assert ref[5] == 100 and ref[4] == 0
    a = torch.from_numpy(some).cuda()
    assert_stats(lib_stats(pa, a).cpu().numpy(), ref)
    for theta in THETAS:
        check_event(pa, a, theta, 0.3, ref)

    nothing = np.full(B, -np.inf, np.float32)
    ref = np_stats(nothing)
    assert ref[2] == 0.0 and ref[5] == B
    a = torch.from_numpy(nothing).cuda()
    assert_stats(lib_stats(pa, a).cpu().numpy(), ref)
    for theta in THETAS:
        assert check_event(pa, a, theta, 0.3, ref)  # ESS 0 <= theta B: taken at every threshold

    for poison in (np.nan, np.inf):
        bad = base.copy()
        bad[B // 3] = poison
        ref = np_stats(bad)
        assert ref[4] == 1
        a = torch.from_numpy(bad).cuda()
        assert_stats(lib_stats(pa, a).cpu().numpy(), ref)
        for theta in THETAS:
            assert check_event(pa, a, theta, 0.3, ref)  # a bad weight forces the event, even at theta = 0


def test_path_selection(pa):
    L = pa._lib.lib()
    assert L.pita_adaptive_resample_single_launch(0) == 0
    assert L.pita_adaptive_resample_single_launch(1) == 1
    assert L.pita_adaptive_resample_single_launch(2048) == 1  # the documented threshold: both sides are in SIZES
    assert L.pita_adaptive_resample_single_launch(2049) == 0
    assert L.pita_adaptive_resample_single_launch(16384) == 0
    assert L.pita_adaptive_resample_single_launch(70001) == 0


@pytest.mark.parametrize("B", (2048, 16384, 70001))
def test_rerun_repeats_every_bit(pa, B):
    from pita_amd.utils import sample_cat_sys_adaptive

    a = torch.from_numpy(weights(B, 1)).cuda()
    for theta in (0.6, 0.2):  # an event that resamples and one that does not
        r0 = sample_cat_sys_adaptive(B, a, theta, 0.3)
        r1 = sample_cat_sys_adaptive(B, a, theta, 0.3)
        for t0, t1 in zip(r0, r1):
            assert torch.equal(bits(t0), bits(t1))


def test_bad_arguments_are_refused_before_any_launch(pa):
    L = pa._lib.lib()
    B = 2048
    a = torch.from_numpy(weights(B, 1)).cuda()
    ids = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    nu = torch.full((), -7, dtype=torch.int64, device="cuda")
    stats = torch.full((6,), -7.0, dtype=torch.float64, device="cuda")
    flag = torch.full((), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(1, (int(L.pita_adaptive_resample_workspace_bytes(B)) + 7) // 8), dtype=torch.float64, device="cuda")
    st = pa._lib.stream_ptr(a.device)

    def call(B=B, u0=0.3, theta=0.5, ids_ptr=ids.data_ptr()):
        return L.pita_adaptive_resample(a.data_ptr(), B, u0, theta, ids_ptr, nu.data_ptr(), stats.data_ptr(),
                                        flag.data_ptr(), ws.data_ptr(), st)

    for kw in (dict(B=0), dict(theta=1.5), dict(theta=float("nan")), dict(u0=1.0), dict(u0=-0.1), dict(ids_ptr=None)):
        assert call(**kw) != 0, kw
        assert pa._lib.last_error()
    assert L.pita_logweight_stats(a.data_ptr(), 0, stats.data_ptr(), None, st) != 0
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and int(nu) == -7 and int(flag) == -7 and bool((stats == -7.0).all())
    assert call() == 0  # the same buffers with good arguments
    torch.cuda.synchronize()
    assert int(flag) in (0, 1) and float(stats[4]) == 0.0


# ---------------------------------------------------------------------------------------------- integrator
class _Geometry:  # what WeightedSDEIntegrator reads from the target when nothing evaluates it
    n_particles, n_spatial_dim = 13, 3


N_STEPS, WALKERS = 6, 64
GAMMAS = (4 / 3, 8 / 3, 16 / 3, 32 / 3)


@pytest.fixture(scope="module")
def lj13(pa, golden):
    """run(ess_threshold, interval, gamma) -> (x, logweights, counts, last_weight_stats): the golden LJ13 net, 64 walkers,
    6 steps, injected noise and uniforms, exact divergence, no descent and no MALA."""
    from pita_amd.energy_net import EnergyNet

    w = {k: torch.tensor(v) for k, v in golden("egnn_weights_trainedlike.npz").items()}
    net = pa.EGNN_dynamics(13, 3, condition_temperature=True, precision="f16x2", **KW)
    net.load_state_dict({k: v for k, v in w.items() if k in net.state_dict()})
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gen = torch.Generator().manual_seed(21)
    x1 = (O.remove_mean(torch.randn(WALKERS, 39, generator=gen), 13, 3) * 80.0).cuda()
    noise = torch.randn(N_STEPS, WALKERS, 39, generator=gen).cuda()

    def run(ess_threshold, interval=1, gamma=GAMMAS[0]):
        sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                              debias_inference=True)
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N_STEPS, start_resampling_step=0,
                                         end_resampling_step=N_STEPS, resampling_interval=interval,
                                         num_negative_time_steps=0, post_mcmc_steps=0, batch_size=WALKERS, seed=3,
                                         ess_threshold=ess_threshold)
        x, logw, counts, _, _ = integ.integrate_sde(x1, _Geometry(), pa.ConstantAnnealingFactorSchedule(gamma),
                                                    inverse_temperature=1.0, noise=noise,
                                                    resample_u=[0.3, 0.6, 0.9, 0.15, 0.45, 0.75])
        return x, logw, counts, integ.last_weight_stats

    return run


def test_integrator_threshold_one_is_the_fixed_schedule(lj13):
    x0, w0, c0, s0 = lj13(None)
    x1, w1, c1, s1 = lj13(1.0)
    assert s0 is None
    assert torch.equal(bits(x0), bits(x1)) and torch.equal(bits(w0), bits(w1)) and c0 == c1
    assert s1["resampled"].dtype == bool and s1["resampled"].shape == (N_STEPS,) and s1["resampled"].all()
    assert all(s1[k].shape == (N_STEPS,) and s1[k].dtype == np.float64 for k in ("ess", "ess_fraction", "log_mean_weight"))


def test_integrator_threshold_zero_never_resamples(lj13):
    x0, w0, c0, _ = lj13(None, interval=-1)
    x1, w1, c1, s1 = lj13(0.0)
    assert bool(torch.isfinite(w1).all())
    assert torch.equal(bits(x0), bits(x1)) and torch.equal(bits(w0), bits(w1))
    assert c1 == [WALKERS] * N_STEPS and not s1["resampled"].any()
    assert np.isfinite(s1["ess"]).all()  # an event was due at every step


@pytest.fixture(scope="module")
def intermediate(lj13):
    """(gamma, theta): the threshold in the widest gap between the sorted ESS fractions of the never-resampling run; gamma
    is scaled up from 4/3 (GAMMAS) until those fractions span at least 0.05.  On the MI355X gamma = 4/3 already does: the
    sorted fractions of the six steps are 0.035, 0.035, 0.035, 0.036, 0.052, 0.195, so theta = 0.124 and the run with it
    alternates between steps that keep their weights and steps that resample."""
    for gamma in GAMMAS:
        f = np.sort(lj13(0.0, gamma=gamma)[3]["ess_fraction"])
        print(f"gamma = {gamma:.4f}: sorted ESS fractions of the never-resampling run {f}")
        if f[-1] - f[0] >= 0.05:
            k = int(np.argmax(np.diff(f)))
            return gamma, float(0.5 * (f[k] + f[k + 1]))
    pytest.fail(f"the ESS fractions span less than 0.05 at every gamma of {GAMMAS}: {f}")


def test_integrator_intermediate_threshold(pa, lj13, intermediate):
    gamma, theta = intermediate
    x, logw, counts, st = lj13(theta, gamma=gamma)
    print(f"gamma = {gamma:.4f}, theta = {theta:.6f}: ess = {st['ess']}, resampled = {st['resampled']}")
    assert st["resampled"].any()  # the run follows the never-resampling one up to its first fraction below theta
    rows = logw.cpu().numpy()
    for s in range(N_STEPS):
        assert st["resampled"][s] == (st["ess"][s] <= theta * WALKERS), s
        assert st["resampled"][s] == (not rows[s].any()), s  # the weights are reset exactly where the event resampled
        if not st["resampled"][s]:
            assert counts[s] == WALKERS
            ref = np_stats(rows[s])
            np.testing.assert_allclose(st["ess"][s], ref[2], rtol=1e-9, atol=0)
            np.testing.assert_allclose(st["ess_fraction"][s], ref[3], rtol=1e-9, atol=0)
            assert abs(st["log_mean_weight"][s] - ref[1]) <= 1e-9
        else:
            assert 1 <= counts[s] <= WALKERS
    log_z = st["log_mean_weight"][st["resampled"]].sum() + np_stats(rows[-1])[1]
    assert abs(st["log_z"] - log_z) <= 1e-9 * max(1.0, abs(log_z))


def test_integrator_intermediate_threshold_repeats_every_bit(lj13, intermediate):
    gamma, theta = intermediate
    x0, w0, c0, s0 = lj13(theta, gamma=gamma)
    x1, w1, c1, s1 = lj13(theta, gamma=gamma)
    assert torch.equal(bits(x0), bits(x1)) and torch.equal(bits(w0), bits(w1)) and c0 == c1
    assert s0["log_z"] == s1["log_z"]
    for k in ("ess", "ess_fraction", "log_mean_weight", "resampled"):
        assert np.array_equal(s0[k], s1[k], equal_nan=k != "resampled")
