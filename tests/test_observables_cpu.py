"""Weighted per-population observables without a GPU: the three entry points bind and refuse bad arguments before any
device call, the weighted 1-D transport helper agrees with scipy / a numpy quantile merge, ``population_summary``'s
arithmetic, and the shared references of the GPU tests are what they claim to be."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _observables as OB

NAMES = ("pita_weighted_histogram", "pita_pair_distance_histogram", "pita_weighted_moments")


@pytest.fixture(scope="module")
def built():
    from pita_amd import build as _b

    _b.build(verbose=False)
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def test_new_prototypes_bind_and_the_abi_version_stays(built):
    L = built._lib.lib()
    for name in NAMES:
        assert name in built._lib.EXPORTS
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    assert L.pita_abi_version() == 13 == built._lib.ABI_VERSION


def test_bad_arguments_come_back_as_error_codes_without_a_gpu(built):
    """Every check precedes the first HIP call: host buffers stand in for the device pointers and are never touched."""
    L = built._lib.lib()
    P, S, NB = 3, 64, 10
    buf = {k: ctypes.create_string_buffer(4096) for k in ("v", "logw", "edges", "wsum", "counts", "info", "out")}
    before = {k: v.raw for k, v in buf.items()}
    addr = {k: ctypes.addressof(v) for k, v in buf.items()}

    def hist(n_pop=P, pop_size=S, per_walker=1, nbins=NB, **ptr):
        a = dict(addr, **ptr)
        return L.pita_weighted_histogram(a["v"], a["logw"], n_pop, pop_size, per_walker, a["edges"], nbins, a["wsum"],
                                         a["counts"], a["info"], None)

    def pair(n_pop=P, pop_size=S, n_particles=13, n_dim=3, nbins=NB, **ptr):
        a = dict(addr, **ptr)
        return L.pita_pair_distance_histogram(a["v"], a["logw"], n_pop, pop_size, n_particles, n_dim, a["edges"], nbins,
                                              a["wsum"], a["counts"], a["info"], None)

    def mom(n_pop=P, pop_size=S, **ptr):
        a = dict(addr, **ptr)
        return L.pita_weighted_moments(a["v"], a["logw"], n_pop, pop_size, a["out"], None)

    def refused(fn, code, **kw):
        assert fn(**kw) == code, (fn.__name__, kw)
        assert built._lib.last_error().startswith(symbol[fn] + ":"), (fn.__name__, kw, built._lib.last_error())

    symbol = {hist: "pita_weighted_histogram", pair: "pita_pair_distance_histogram", mom: "pita_weighted_moments"}

    common = (dict(v=None), dict(n_pop=0), dict(n_pop=-3), dict(pop_size=0), dict(pop_size=-1))
    bins = (dict(edges=None), dict(wsum=None), dict(counts=None), dict(info=None), dict(nbins=0), dict(nbins=1025),
            dict(nbins=-1))
    for kw in common + bins + (dict(per_walker=0), dict(per_walker=-2)):
        refused(hist, -1, **kw)
    for kw in common + bins + (dict(n_particles=1), dict(n_particles=257), dict(n_dim=0), dict(n_dim=4)):
        refused(pair, -1, **kw)
    for kw in common + (dict(out=None),):
        refused(mom, -1, **kw)
    # PITA_EUNSUPPORTED: more than 2^42 values per population leave a fixed-point shift below 20
    refused(hist, -2, pop_size=2 ** 42 + 1)
    refused(hist, -2, pop_size=2 ** 30, per_walker=2 ** 13)
    refused(hist, -2, pop_size=2 ** 62, per_walker=2 ** 62)
    refused(pair, -2, pop_size=2 ** 42, n_particles=3)
    assert OB.shift_of(2 ** 42, 1) == 20 and OB.shift_of(2 ** 42 + 1, 1) == 19
    assert all(buf[k].raw == before[k] for k in buf)


def test_shift_formula_and_shared_inputs():
    import math

    for S, k in ((1, 1), (1, 7), (63, 1), (2048, 7), (257, 32640), (2 ** 21, 1), (2 ** 22 + 1, 1), (3, 2 ** 30)):
        assert OB.shift_of(S, k) == min(40, 62 - math.ceil(math.log2(S * k)))
    assert OB.shift_of(2048, 7) == 40 and OB.shift_of(2 ** 22 + 1, 1) == 39
    a = OB.logweights(63, 5).reshape(5, 63)
    m, n_bad, n_ninf, bad, w = OB.ref_info(a, 5, 63)
    assert [OB.flavour(p, 0) for p in range(5)] == list(OB.FLAVOURS)
    assert n_bad.tolist() == [0, 3, 0, 0, 0] and n_ninf.tolist() == [0, 2, 63, 0, 0] and m[2] == 0.0
    assert a[0].max() - a[0].min() > 10 and w[3].max() == 1.0 and np.sort(w[3])[-2] < np.exp(-59.9)
    assert np.all(w[2] == 0) and np.all(w[1][bad[1]] == 0)
    d = OB.pair_distances(4, 2, 3, 1)
    x = OB.coords(4, 2, 3, 1).reshape(3, 4, 2)
    assert d.shape == (3, 6) and d.dtype == np.float32
    dl = x[1, 3] - x[1, 1]  # pair (1, 3) is number 4 of the upper triangle of 4
    assert d[1, 4] == np.sqrt(np.float32(dl[0] * dl[0]) + np.float32(dl[1] * dl[1]))


def test_weighted_w1_against_scipy_and_w2_against_a_numpy_merge():
    from scipy.stats import wasserstein_distance

    from pita_amd import metrics

    rng = np.random.default_rng(11)
    for na, nb in ((1, 1), (5, 3), (1000, 1000), (3000, 1777)):
        a, b = rng.normal(0.0, 2.0, na), rng.normal(0.5, 1.0, nb)
        wa, wb = rng.uniform(0.0, 1.0, na) ** 3, np.exp(rng.normal(0.0, 3.0, nb))
        if nb > 3:
            wb[::5] = 0.0  # walkers of weight 0 (log-weight -inf)
        ta, tb, twa, twb = (torch.from_numpy(v) for v in (a, b, wa, wb))
        w1 = metrics._w_1d_weighted(ta, twa, tb, twb, 1)
        assert w1 == pytest.approx(wasserstein_distance(a, b, u_weights=wa, v_weights=wb), rel=1e-12)
        w1u = metrics._w_1d_weighted(ta, None, tb, twb, 1)
        assert w1u == pytest.approx(wasserstein_distance(a, b, v_weights=wb), rel=1e-12)
        for p in (1, 2):
            assert metrics._w_1d_weighted(ta, twa, tb, twb, p) == pytest.approx(OB.w_1d_weighted_numpy(a, wa, b, wb, p), rel=1e-11)


def test_equal_weights_reproduce_the_unweighted_helper():
    from pita_amd import metrics

    rng = np.random.default_rng(12)
    for na, nb in ((1, 1), (800, 800), (1200, 500), (7, 4000)):
        a, b = torch.from_numpy(rng.normal(0.0, 2.0, na)), torch.from_numpy(rng.normal(0.5, 1.0, nb))
        for p in (1, 2):
            want = metrics._w_1d(a, b, p)
            assert metrics._w_1d_weighted(a, None, b, None, p) == pytest.approx(want, rel=1e-12, abs=1e-12)
            assert metrics._w_1d_weighted(a, torch.full((na,), 0.37, dtype=torch.float64), b, torch.full((nb,), 5.0), p) == \
                pytest.approx(want, rel=1e-12, abs=1e-12)


def test_relative_weights_and_weighted_energy_distances_on_cpu_tensors():
    from pita_amd import metrics

    lw = torch.tensor([0.0, float("nan"), -float("inf"), float("inf"), -1.0])
    assert torch.equal(metrics._relative_weights(lw), torch.tensor([1.0, 0.0, 0.0, 0.0, np.exp(-1.0)], dtype=torch.float64))
    assert torch.equal(metrics._relative_weights(torch.tensor([-float("inf")] * 2)), torch.zeros(2, dtype=torch.float64))
    rng = np.random.default_rng(13)
    pred, true = torch.from_numpy(rng.normal(0, 30, 300)), torch.from_numpy(rng.normal(2, 25, 500))
    pred[3], pred[100] = 1e4, -2e3  # cropped at the default threshold
    plain = metrics.energy_distances(pred, true, prefix="t")
    zero = metrics.energy_distances(pred, true, prefix="t", pred_logweights=torch.zeros(300, dtype=torch.float64))
    assert plain.keys() == zero.keys() and plain["t/num_cropped"] == zero["t/num_cropped"] == 2
    for k in plain:
        assert zero[k] == pytest.approx(plain[k], rel=1e-12, abs=1e-12), k
    mult = rng.integers(1, 6, 300)
    rep = metrics.energy_distances(torch.from_numpy(np.repeat(pred.numpy(), mult)), true, prefix="t")
    wtd = metrics.energy_distances(pred, true, prefix="t", pred_logweights=torch.from_numpy(np.log(mult.astype(np.float64))))
    for k in rep:
        if k != "t/num_cropped":
            assert wtd[k] == pytest.approx(rep[k], rel=1e-12, abs=1e-12), k


def test_population_summary_arithmetic():
    from pita_amd import metrics

    a = np.array([1.0, 2.0, 4.0, 9.0])
    s = metrics.population_summary(a)
    assert s["n_used"] == 4 and s["mean"] == 4.0 and s["stderr"] == pytest.approx(a.std(ddof=1) / 2.0, rel=1e-15)
    s = metrics.population_summary([1.0, np.nan, 3.0, np.inf])
    assert s["n_used"] == 2 and s["mean"] == 2.0 and s["stderr"] == pytest.approx(np.sqrt(2.0) / np.sqrt(2.0), rel=1e-15)
    s = metrics.population_summary([np.nan, 5.0])
    assert s["n_used"] == 1 and s["mean"] == 5.0 and np.isnan(s["stderr"])
    s = metrics.population_summary([np.nan, np.nan])
    assert s["n_used"] == 0 and np.isnan(s["mean"]) and np.isnan(s["stderr"])
    rows = np.array([[1.0, 2.0, 3.0], [np.nan, 0.0, 0.0], [3.0, 2.0, 7.0], [5.0, 5.0, 5.0]])  # a row with a NaN is not used
    s = metrics.population_summary(rows)
    used = rows[[0, 2, 3]]
    assert s["n_used"] == 3 and np.array_equal(s["mean"], used.mean(0))
    assert np.allclose(s["stderr"], used.std(0, ddof=1) / np.sqrt(3.0), rtol=1e-15, atol=0)
    s = metrics.population_summary(rows[:2])
    assert s["n_used"] == 1 and np.array_equal(s["mean"], rows[0]) and s["stderr"].shape == (3,) and np.isnan(s["stderr"]).all()
