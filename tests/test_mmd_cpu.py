"""Mix-RBF MMD without a GPU: the two entry points bind and refuse bad arguments before any device call, the workspace
size, the host-side validation of pita_amd.metrics.rbf_mmd2, and the shared references of the GPU tests (tests/_mmd.py)
are what they claim to be -- the fp64 oracle on cases with a closed form, the float32 restatement against the oracle."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _mmd as MM

NAMES = ("pita_rbf_gram_workspace_bytes", "pita_rbf_gram_sums")


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
        assert getattr(L, name).argtypes is not None
    assert L.pita_rbf_gram_sums.restype is ctypes.c_int and L.pita_rbf_gram_workspace_bytes.restype is ctypes.c_size_t
    assert L.pita_abi_version() == 13 == built._lib.ABI_VERSION


def test_bad_arguments_come_back_as_error_codes_without_a_gpu(built):
    """Every check precedes the first HIP call: host buffers stand in for the device pointers and are never touched."""
    L = built._lib.lib()
    buf = {k: ctypes.create_string_buffer(4096) for k in ("a", "lwa", "b", "lwb", "sums", "info_a", "info_b", "ws")}
    before = {k: v.raw for k, v in buf.items()}
    addr = {k: ctypes.addressof(v) for k, v in buf.items()}

    def call(n_pop=3, pop_size=64, n_b=10, dim=3, gammas=(0.5, 2.0), n_gamma=None, self_mode=False, **ptr):
        a = dict(addr, **ptr)
        if self_mode:
            a.update(b=ptr.get("b"), lwb=ptr.get("lwb"))
        g = None if gammas is None else (ctypes.c_double * max(len(gammas), 1))(*gammas)
        return L.pita_rbf_gram_sums(a["a"], a["lwa"], n_pop, pop_size, a["b"], a["lwb"], n_b, dim, g,
                                    len(gammas or ()) if n_gamma is None else n_gamma, a["sums"], a["info_a"], a["info_b"],
                                    a["ws"], None)

    def refused(code, **kw):
        assert call(**kw) == code, kw
        assert built._lib.last_error().startswith("pita_rbf_gram_sums"), (kw, built._lib.last_error())

    for kw in (dict(a=None), dict(sums=None), dict(info_a=None), dict(ws=None), dict(gammas=None, n_gamma=2),
               dict(n_pop=0), dict(n_pop=-3), dict(pop_size=0), dict(pop_size=-1),
               dict(dim=0), dict(dim=769), dict(dim=-3), dict(gammas=(), n_gamma=0), dict(gammas=(1.0,) * 17),
               dict(gammas=(0.5, -1.0)), dict(gammas=(float("nan"),)), dict(gammas=(1.0, float("inf"))),
               dict(self_mode=True, n_b=5), dict(self_mode=True, n_b=0, lwb=addr["lwb"]), dict(self_mode=True, n_b=-1),
               dict(n_b=0), dict(n_b=-2)):
        refused(-1, **kw)
    refused(-2, n_pop=2 ** 40, pop_size=2 ** 40)
    refused(-2, n_pop=2 ** 31, pop_size=64)
    assert all(buf[k].raw == before[k] for k in buf)


def test_workspace_bytes_is_monotone_and_nonzero(built):
    f = built._lib.lib().pita_rbf_gram_workspace_bytes
    assert f(1, 1, 0) > 0 and f(1, 1, 1) > 0 and f(1, 1, 0) % 8 == 0
    for P, S, M in ((1, 1, 0), (1, 64, 7), (3, 257, 300), (32, 2048, 10000), (1, 65536, 65536), (1, 65536, 0)):
        base = f(P, S, M)
        assert base >= 4 * (P * S + M)  # the fp32 row weights of both sets live there
        assert f(P + 1, S, M) > base and f(P, S + 1, M) >= base  # (rounded up to 8 bytes)
        assert M == 0 or f(P, S, M + 1) >= base  # (n_b = 0 is self mode: another tiling)
        assert f(P, 2 * S + 64, M) > base and (M == 0 or f(P, S, 2 * M + 64) > base)
    assert f(0, 64, 0) == 0 and f(1, 0, 0) == 0 and f(1, 1, -1) == 0 and f(2 ** 40, 2 ** 40, 0) == 0


def test_oracle_two_point_masses_have_the_closed_form():
    for n in (1, 5, 16):
        g = np.array(MM.gammas_for(n))
        for d in (0.0, 0.07, 1.3):
            x, y = np.zeros((1, 3), np.float32), np.array([[d, 0.0, 0.0]], np.float32)
            got = MM.oracle_mmd2(x, None, 1, y, None, list(g))[0]
            want = 2 * n - 2 * np.exp(-g * float(np.float32(d)) ** 2).sum()
            assert abs(got - want) <= 1e-12 * n


def test_oracle_mmd_of_a_set_with_itself_is_zero_when_biased():
    x = MM.coords(65, 39)
    assert abs(MM.oracle_mmd2(x, None, 1, x, None, MM.gammas_for(5))[0]) <= 1e-12


def test_oracle_integer_weights_equal_repeated_rows():
    rng = np.random.default_rng(11)
    x, y = MM.coords(40, 3), MM.coords(30, 3, seed=1)
    k = rng.integers(1, 5, 40)
    kw = k[None, :].astype(np.float64)
    g = MM.gammas_for(5)
    rep = np.repeat(np.asarray(x), k, axis=0)
    ones = np.ones((1, rep.shape[0]))
    s_xy, r_xy = MM.oracle_sums(x, kw, y, np.ones(30), g), MM.oracle_sums(rep, ones, y, np.ones(30), g)
    s_xx, r_xx = MM.oracle_sums(x, kw, None, None, g), MM.oracle_sums(rep, ones, None, None, g)
    assert np.abs(s_xy - r_xy).max() <= 1e-12 * r_xy.max() and np.abs(s_xx - r_xx).max() <= 1e-12 * r_xx.max()
    s_yy = MM.oracle_sums(y, np.ones((1, 30)), None, None, g)[0]
    weighted = MM.mmd2_from(s_xx, s_xy, s_yy, [k.sum()], [(k * k).sum()], 30.0, 30.0, True)[0]
    assert np.abs(weighted - MM.oracle_mmd2(rep, None, 1, y, None, g)).max() <= 1e-12


def test_oracle_unbiased_formula_is_the_sum_over_distinct_pairs():
    x, y = np.asarray(MM.coords(23, 3), np.float64), np.asarray(MM.coords(17, 3, seed=1), np.float64)
    g = MM.gammas_for(5)
    rng = np.random.default_rng(5)
    lw = rng.uniform(-2, 0, 23).astype(np.float32)
    w = np.exp(lw.astype(np.float64) - lw.max())

    def k(u, v):
        return sum(np.exp(-gam * ((u - v) ** 2).sum()) for gam in g)

    xx = sum(w[i] * w[j] * k(x[i], x[j]) for i in range(23) for j in range(23) if i != j) / sum(
        w[i] * w[j] for i in range(23) for j in range(23) if i != j)
    yy = sum(k(y[i], y[j]) for i in range(17) for j in range(17) if i != j) / (17 * 16)
    xy = sum(w[i] * k(x[i], y[j]) for i in range(23) for j in range(17)) / (w.sum() * 17)
    got = MM.oracle_mmd2(x.astype(np.float32), lw, 1, y.astype(np.float32), None, g, biased=False)[0]
    assert abs(got - (xx + yy - 2 * xy)) <= 1e-12 * len(g)


def test_restatement_error_against_the_oracle():
    """The float32 restatement against the fp64 oracle on the GPU tests' own inputs -- every accuracy case, the unit-weight
    cases and the host-layer cases --, on the normalised scale: required <= 1e-7, so that the GPU tests' bound of 8 x this
    error stays within 3.4 x of its floor of 2^-22 = 2.4e-7.  Measured here: 3.2e-8 at most; at the five shapes (S, M, D) =
    (257, 300, 39), (257, 300, 3), (65, 7, 1), (300, 300, 165), (257, 257, 66) cross / self 2.4e-8 / 3.0e-8, 0.9e-8 /
    0.5e-8, 2.9e-8 / 3.2e-8, 1.3e-8 / 0, 2.2e-8 / 3.1e-8.  (When the metric was specified, <= 2e-8 was expected
    at these shapes; these inputs do not reach that: with the family's log-weight flavours, spread 12, a
    population's effective sample size is about S / 6, so the fp32 rounding of the row weights -- 1.5e-8 of the 3.0e-8 at
    (257, 300, 39), self -- does not average out, and at sigma = 100 every e sits just below 1, where float32 is 6e-8
    apart.)"""
    worst = 0.0
    keys = list(MM.CASES) + [k[:5] + (0, k[5], True) for k in MM.UNIT_CASES]
    for k in keys:
        c = MM.case(*k)
        e_cross = MM.normalised_error(c["cross32"], c["cross64"], c["norm_cross"])
        e_self = MM.normalised_error(c["self32"], c["self64"], c["norm_self"])
        print(f"restatement error {k}: cross {e_cross:.3e} self {e_self:.3e}")
        worst = max(worst, e_cross, e_self)
    for P in (1, 5):
        worst = max(worst, MM.host_case(P)["e32"])
    assert worst <= 1e-7


def test_host_validation_raises_before_any_device_call(built):
    """CPU tensors throughout: a ValueError from the host checks comes before the device check would refuse them."""
    from pita_amd import metrics

    x, y = torch.from_numpy(np.array(MM.coords(64, 3))), torch.from_numpy(np.array(MM.coords(10, 3, seed=1)))
    lw = torch.zeros(64)
    for kw in (dict(sigma_list=()), dict(sigma_list=(1.0, 0.0)), dict(sigma_list=(-1.0,)), dict(sigma_list=(float("nan"),)),
               dict(sigma_list=(float("inf"),)), dict(sigma_list=(1.0,) * 17), dict(populations=3), dict(populations=0),
               dict(populations=128), dict(logweights=lw[:63]), dict(test_logweights=lw[:9]),
               dict(test_self={"sums": np.zeros(5)}), dict(test_self={"sums": np.zeros(5), "info": np.zeros(5),
                                                                      "gammas": np.ones(5), "rows": 10})):
        with pytest.raises(ValueError):
            metrics.rbf_mmd2(x, y, **kw)
    for a, b in ((x, y[:, :2]), (x[0], y), (x, y[:0]), (torch.zeros(4, 769), torch.zeros(4, 769))):
        with pytest.raises(ValueError):
            metrics.rbf_mmd2(a, b)
    with pytest.raises(built._lib.PitaHipError):
        metrics.rbf_mmd2(x, y)  # valid arguments on the CPU: no fallback
    with pytest.raises(built._lib.PitaHipError):
        metrics.mix_rbf_mmd2(x, y, MM.SIGMAS)
