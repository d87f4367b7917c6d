"""Mix-RBF MMD on the MI355X (pita_rbf_gram_sums, pita_amd.metrics.rbf_mmd2) against the fp64 numpy oracle of
tests/_mmd.py.  Errors are taken on the normalised scale |S_dev - S_64| / (sum w * sum v); the bound of a case is
max(8 x the error of the float32 restatement on the same inputs, 2^-22), the restatement's error computed at run time.
The figures printed here are kept in profiles/r20_mmd.txt."""
import numpy as np
import pytest
import torch

from tests import _mmd as MM
from tests import _observables as OB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # the shared references stay read-only


def gram(x, lw, P, y, lv, gammas):
    """(sums [P, n], info_a [P, 5], info_b [5] or None) of one pita_rbf_gram_sums call; y None = self mode"""
    from pita_amd import metrics

    x = dev(x)
    return metrics._rbf_gram(x, dev(lw), P, x.shape[0] // P, dev(y), dev(lv), [float(g) for g in gammas])


def check_info(got, ref):
    assert np.array_equal(got[..., 0], ref[..., 0]) and np.array_equal(got[..., 3:], ref[..., 3:]), (got, ref)
    assert np.all(np.abs(got[..., 1:3] - ref[..., 1:3]) <= 1e-12 * np.abs(ref[..., 1:3])), (got, ref)


@pytest.mark.parametrize("S,M,D,P,n_gamma,offset,b_weighted", MM.CASES)
def test_sums_and_info_against_the_fp64_oracle(pa, S, M, D, P, n_gamma, offset, b_weighted):
    """Cross and self mode with the five log-weight flavours on a (the populations of a case cycle through them from
    ``offset``) and unit or clean weights on b.  Measured on an MI355X (profiles/r20_mmd.txt)."""
    c = MM.case(S, M, D, P, n_gamma, offset, b_weighted)
    cross, info_a, info_b = gram(c["x"], c["lw"], P, c["y"], c["lv"], c["gammas"])
    self_, info_s, _ = gram(c["x"], c["lw"], P, None, None, c["gammas"])
    check_info(info_a, c["info_a"])
    check_info(info_s, c["info_a"])
    check_info(info_b, c["info_b"])
    for name, got, ref, ref32, norm in (("cross", cross, c["cross64"], c["cross32"], c["norm_cross"]),
                                        ("self", self_, c["self64"], c["self32"], c["norm_self"])):
        e32 = MM.normalised_error(ref32, ref, norm)
        err = MM.normalised_error(got, ref, norm)
        print(f"mmd {name} S={S} M={M} D={D} P={P} n_gamma={n_gamma}: device {err:.3e} restatement {e32:.3e} "
              f"bound {MM.bound(e32):.3e}")
        assert e32 <= 1e-7
        assert err <= MM.bound(e32)
        dead = (norm <= 0).reshape(-1)
        assert (got[dead] == 0).all()  # a population without weight: sums of exactly 0


@pytest.mark.parametrize("S,M,D,P,n_gamma,b_weighted", MM.UNIT_CASES)
def test_unit_weights_on_the_samples(pa, S, M, D, P, n_gamma, b_weighted):
    """logw_a = NULL, with unit and with clean weights on b."""
    c = MM.case(S, M, D, P, n_gamma, 0, b_weighted, True)
    cross, info_a, info_b = gram(c["x"], None, P, c["y"], c["lv"], c["gammas"])
    self_, _, _ = gram(c["x"], None, P, None, None, c["gammas"])
    assert np.array_equal(info_a, np.tile([0.0, S, S, 0.0, 0.0], (P, 1)))
    if b_weighted:
        check_info(info_b, c["info_b"])
    else:
        assert np.array_equal(info_b, [0.0, M, M, 0.0, 0.0])
    for name, got, ref, ref32, norm in (("cross", cross, c["cross64"], c["cross32"], c["norm_cross"]),
                                        ("self", self_, c["self64"], c["self32"], c["norm_self"])):
        e32, err = MM.normalised_error(ref32, ref, norm), MM.normalised_error(got, ref, norm)
        print(f"mmd unit {name} S={S} M={M} D={D} P={P} n_gamma={n_gamma} b_weighted={b_weighted}: device {err:.3e} "
              f"restatement {e32:.3e}")
        assert e32 <= 1e-7 and err <= MM.bound(e32)


@pytest.mark.parametrize("S,M", [(257, 300), (63, 7)])
def test_duplicate_rows_are_exact(pa, S, M):
    """gamma = 5e5 alone and rows more than 0.05 apart in coordinate 0 unless they coincide: every other pair underflows
    to 0, a coincident pair gives s = 0 and e = 1 exactly, and the sums are the integer numbers of coincident pairs."""
    x, y, eq_xx, eq_xy = MM.duplicates(S, M)
    assert eq_xx > S and eq_xy > 0
    s_xx, _, _ = gram(x, None, 1, None, None, [5e5])
    s_xy, _, _ = gram(x, None, 1, y, None, [5e5])
    s_cp, _, _ = gram(x, None, 1, x, None, [5e5])
    assert s_xx[0, 0] == eq_xx and s_xy[0, 0] == eq_xy and s_cp[0, 0] == eq_xx


@pytest.mark.parametrize("S,D,P", [(257, 39, 3), (65, 3, 5), (1025, 3, 2)])
def test_self_mode_equals_the_cross_call_against_a_copy(pa, S, D, P):
    """The diagonal tiles and the symmetric off-diagonal ones (visited once, counted twice); S = 1025 splits the b-tiles
    of an a-tile over several blocks.  With a gamma so large that only the diagonal survives the sum is sum w^2 exactly
    (each term (w_i * w_i) * 1 in fp32, the same products the weights pass takes in double, up to their fp32 rounding)."""
    x, lw = MM.coords(P * S, D), OB.logweights(S, P, 0)
    g = MM.gammas_for(5)
    w, _ = MM.weights64(lw, P, S)
    norm = w.sum(1)[:, None] ** 2
    self_, info, _ = gram(x, lw, P, None, None, g)
    for p in range(P):
        cross, _, _ = gram(x[p * S:(p + 1) * S], lw[p * S:(p + 1) * S], 1, x[p * S:(p + 1) * S], lw[p * S:(p + 1) * S], g)
        err = MM.normalised_error(self_[p:p + 1], cross, norm[p:p + 1])
        print(f"mmd self vs copy S={S} D={D} p={p}: {err:.3e}")
        assert err <= MM.FLOOR
    ones = np.zeros(P * S, np.float32)
    far = MM.coords(P * S, D).copy()
    far[:, 0] += np.tile(4.0 * np.arange(S, dtype=np.float32), P)  # rows of a population more than 2 apart: gamma = 1e6 kills the pairs
    diag, info1, _ = gram(far, ones, P, None, None, [1e6])
    assert np.array_equal(diag[:, 0], info1[:, 2]) and np.array_equal(info1[:, 2], np.full(P, float(S)))
    lw2 = np.where(np.arange(P * S) % 3 == 1, -np.inf, 0.0).astype(np.float32)  # weights 1 and 0
    diag2, info2, _ = gram(far, lw2, P, None, None, [1e6])
    assert np.array_equal(diag2[:, 0], info2[:, 2]) and (info2[:, 2] > 0).all() and (info2[:, 2] < S).all()


@pytest.mark.parametrize("S,M,D,P", [(257, 300, 39, 5), (1025, 1100, 3, 3)])
def test_population_bits_do_not_depend_on_the_call(pa, S, M, D, P):
    """Population p of a P-population call equals the call on its slice alone, bit for bit, in both modes, and two runs
    give equal bits ((1025, 1100): several blocks per a-tile, several a-tiles)."""
    x, y = MM.coords(P * S, D), MM.coords(M, D, seed=1)
    lw, lv = OB.logweights(S, P, 0), OB.logweights(M, 1, 0, seed=5)
    g = MM.gammas_for(5)
    cross, ia, ib = gram(x, lw, P, y, lv, g)
    self_, isf, _ = gram(x, lw, P, None, None, g)
    again = gram(x, lw, P, y, lv, g)
    assert cross.tobytes() == again[0].tobytes() and ia.tobytes() == again[1].tobytes() and ib.tobytes() == again[2].tobytes()
    assert self_.tobytes() == gram(x, lw, P, None, None, g)[0].tobytes()
    for p in range(P):
        sl = slice(p * S, (p + 1) * S)
        c1, i1, _ = gram(x[sl], lw[sl], 1, y, lv, g)
        s1, j1, _ = gram(x[sl], lw[sl], 1, None, None, g)
        assert c1.tobytes() == cross[p:p + 1].tobytes() and s1.tobytes() == self_[p:p + 1].tobytes(), p
        assert i1.tobytes() == ia[p:p + 1].tobytes() and j1.tobytes() == isf[p:p + 1].tobytes(), p


def test_rows_left_out_change_nothing_but_n_bad(pa):
    """Rows with a NaN or inf coordinate in a or b, and rows with a NaN or +inf log-weight: the output is that of the call
    with those rows removed, to the bound, and n_bad counts them."""
    S, M, D, g = 257, 300, 39, MM.gammas_for(5)
    x, y = MM.coords(S, D).copy(), MM.coords(M, D, seed=1).copy()
    lw, lv = OB.logweights(S, 1, 0).copy(), OB.logweights(M, 1, 0, seed=5).copy()
    x[3, 0], x[64, D - 1], x[200, 17], x[256, 33] = np.nan, np.inf, -np.inf, np.nan
    y[0, 5], y[299, 38], y[63, 0] = np.inf, np.nan, -np.inf
    lw[10], lw[128], lw[3] = np.nan, np.inf, np.inf
    lv[7] = np.nan
    ka = ~(MM.row_bad(x) | np.isnan(lw) | (lw == np.inf))
    kb = ~(MM.row_bad(y) | np.isnan(lv) | (lv == np.inf))
    assert (~ka).sum() == 6 and (~kb).sum() == 4
    cross, ia, ib = gram(x, lw, 1, y, lv, g)
    self_, isf, _ = gram(x, lw, 1, None, None, g)
    cross_k, ia_k, ib_k = gram(x[ka], lw[ka], 1, y[kb], lv[kb], g)
    self_k, _, _ = gram(x[ka], lw[ka], 1, None, None, g)
    assert ia[0, 3] == 6 and ib[3] == 4 and isf[0, 3] == 6 and ia_k[0, 3] == 0 and ib_k[3] == 0
    assert np.isfinite(cross).all() and np.isfinite(self_).all()
    assert ia[0, 0] == ia_k[0, 0] and ib[0] == ib_k[0] and ia[0, 4] == ia_k[0, 4]
    assert abs(ia[0, 1] - ia_k[0, 1]) <= 1e-12 * ia_k[0, 1] and abs(ib[1] - ib_k[1]) <= 1e-12 * ib_k[1]
    w, info = MM.weights64(lw, 1, S, MM.row_bad(x))
    v, info_v = MM.weights64(lv, 1, M, MM.row_bad(y))
    check_info(ia, info)
    check_info(ib, info_v[0])
    ref, ref32 = MM.oracle_sums(x, w, y, v[0], g), MM.restated_sums(x, w, y, v[0], g)
    norm = np.array([[w.sum() * v.sum()]])
    b = MM.bound(MM.normalised_error(ref32, ref, norm))
    for got in (cross, cross_k):
        assert MM.normalised_error(got, ref, norm) <= b
    refs = MM.oracle_sums(x, w, None, None, g)
    bs = MM.bound(MM.normalised_error(MM.restated_sums(x, w, None, None, g), refs, norm * 0 + w.sum() ** 2))
    for got in (self_, self_k):
        assert MM.normalised_error(got, refs, norm * 0 + w.sum() ** 2) <= bs


def test_population_without_weight_gives_zero_sums_and_nan(pa):
    from pita_amd import metrics

    S, M, D = 65, 7, 3
    x, y = MM.coords(3 * S, D), MM.coords(M, D, seed=1)
    lw = OB.logweights(S, 3, 0).copy().reshape(3, S)
    lw[1] = -np.inf
    lw = lw.reshape(-1)
    cross, ia, _ = gram(x, lw, 3, y, None, MM.gammas_for(5))
    self_, _, _ = gram(x, lw, 3, None, None, MM.gammas_for(5))
    assert (cross[1] == 0).all() and (self_[1] == 0).all() and ia[1].tolist() == [0.0, 0.0, 0.0, 0.0, float(S)]
    for biased in (True, False):
        r = metrics.rbf_mmd2(dev(x), dev(y), logweights=dev(lw), populations=3, biased=biased)
        assert np.isnan(r["mmd2"][[1, 2]]).all() and np.isfinite(r["mmd2"][0])  # (population 2 has the all -inf flavour)
        assert r["sum_w"][1] == 0 and r["n_neg_inf"][1] == S


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("biased", [True, False])
def test_rbf_mmd2_against_the_oracle(pa, P, biased):
    """Absolute bound 4 n_sigma x the bound of the sums: k_xx, k_yy and twice k_xy each carry one normalised error per
    bandwidth.  Every population has clean log-weights here (tests/_mmd.py host_case: the unbiased estimator divides by
    W^2 - W2, which the flavour with one dominant walker makes 1e-24 of W^2)."""
    from pita_amd import metrics

    c = MM.host_case(P)
    r = metrics.rbf_mmd2(dev(c["x"]), dev(c["y"]), MM.SIGMAS, logweights=dev(c["lw"]), populations=P,
                         test_logweights=dev(c["lv"]), biased=biased)
    ref = MM.oracle_mmd2(c["x"], c["lw"], P, c["y"], c["lv"], c["gammas"], biased)
    b = 4 * len(MM.SIGMAS) * MM.bound(c["e32"])
    err = np.abs(r["mmd2"] - ref)
    print(f"rbf_mmd2 P={P} biased={biased}: max error {err.max():.3e} bound {b:.3e} (restatement {c['e32']:.3e})")
    assert np.isfinite(ref).all() and (err <= b).all()
    assert r["mmd2_per_sigma"].shape == (P, 5) and r["k_xx"].shape == (P, 5) and r["k_xy"].shape == (P, 5) and r["k_yy"].shape == (5,)
    assert np.array_equal(r["log_scale"], c["info_a"][:, 0]) and (r["n_bad"] == 0).all() and (r["n_neg_inf"] == 0).all()
    # the test-set sums passed back in: the same bits, one device call fewer
    r2 = metrics.rbf_mmd2(dev(c["x"]), dev(c["y"]), MM.SIGMAS, logweights=dev(c["lw"]), populations=P,
                          test_logweights=dev(c["lv"]), biased=biased, test_self=r["test_self"])
    for k in ("mmd2", "mmd2_per_sigma", "k_xx", "k_xy", "k_yy", "sum_w", "sum_w2"):
        assert r[k].tobytes() == r2[k].tobytes(), k


def test_mix_rbf_mmd2_is_the_dict_entry_and_the_errors_are_value_errors(pa):
    from pita_amd import metrics

    x, y = dev(MM.coords(257, 39)), dev(MM.coords(300, 39, seed=1))
    for biased in (True, False):
        v = metrics.mix_rbf_mmd2(x, y, MM.SIGMAS, biased=biased)
        assert isinstance(v, float) and v == metrics.rbf_mmd2(x, y, MM.SIGMAS, biased=biased)["mmd2"][0]
    assert metrics.mix_rbf_mmd2(x, x, MM.SIGMAS) == 0.0 or abs(metrics.mix_rbf_mmd2(x, x, MM.SIGMAS)) <= 4 * 5 * MM.FLOOR
    for kw in (dict(sigma_list=()), dict(sigma_list=(0.0,)), dict(sigma_list=(float("nan"),)), dict(populations=2),
               dict(logweights=torch.zeros(256, device="cuda")), dict(logweights=torch.zeros(257)),
               dict(test_logweights=torch.zeros(299, device="cuda")), dict(test_self={"sums": np.zeros(5)})):
        with pytest.raises(ValueError):
            metrics.rbf_mmd2(x, y, **kw)
    with pytest.raises(ValueError):
        metrics.rbf_mmd2(x, y[:, :38])
    with pytest.raises(ValueError):
        metrics.rbf_mmd2(x, y.cpu())


def test_mid_size_run_against_fp64_torch_on_the_device(pa):
    """2 048 x 1 024 x 39: the b-tiles of an a-tile are split over several blocks in both modes.  The reference is an fp64 torch
    computation on the device with the differences first."""
    from pita_amd import metrics

    S, M, D, P = 2048, 1024, 39, 1
    x, y = dev(MM.coords(P * S, D)), dev(MM.coords(M, D, seed=1))
    lw_h = OB.logweights(S, P, 0)
    lw = dev(lw_h)
    w_h, info = MM.weights64(lw_h, P, S)
    w = torch.from_numpy(w_h).cuda()
    g = MM.gammas_for(5)
    x64, y64 = x.double().reshape(P, S, D), y.double()

    def sums64(a, wa, b, wb):
        out = torch.zeros(len(g), dtype=torch.float64, device="cuda")
        for lo in range(0, a.shape[0], 256):
            s = (a[lo:lo + 256, None, :] - b[None, :, :]).pow(2).sum(-1)
            ww = wa[lo:lo + 256, None] * wb[None, :]
            out += torch.stack([(ww * torch.exp(-gam * s)).sum() for gam in g])
        return out.cpu().numpy()

    ones = torch.ones(M, dtype=torch.float64, device="cuda")
    s_xx = np.stack([sums64(x64[p], w[p], x64[p], w[p]) for p in range(P)])
    s_xy = np.stack([sums64(x64[p], w[p], y64, ones) for p in range(P)])
    s_yy = sums64(y64, ones, y64, ones)
    cross, ia, ib = metrics._rbf_gram(x, lw, P, S, y, None, g)
    self_, _, _ = metrics._rbf_gram(x, lw, P, S, None, None, g)
    check_info(ia, info)
    W = w_h.sum(1)[:, None]
    e_c, e_s = MM.normalised_error(cross, s_xy, W * M), MM.normalised_error(self_, s_xx, W * W)
    print(f"mmd mid-size: cross {e_c:.3e} self {e_s:.3e} floor {MM.FLOOR:.3e}")
    assert e_c <= MM.FLOOR and e_s <= MM.FLOOR
    r = metrics.rbf_mmd2(x, y, MM.SIGMAS, logweights=lw, populations=P)
    ref = MM.mmd2_from(s_xx, s_xy, s_yy, w_h.sum(1), (w_h * w_h).sum(1), float(M), float(M), True)[0]
    assert np.abs(r["mmd2"] - ref).max() <= 4 * 5 * MM.FLOOR
