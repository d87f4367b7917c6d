"""pita_weighted_histogram, pita_pair_distance_histogram, pita_weighted_moments and the host layer over them in
pita_amd.metrics.  Run on an MI355X: pytest -m gpu.

Inputs and numpy references: tests/_observables.py.  Bounds:

* counts, m, n_bad, n_neg_inf and the shift are exact;
* per bin |wsum * 2^-shift - numpy.histogram(weights=exp(logw - m) in fp64)| <= n_bin * 2^-shift: each of the n_bin
  contributions is rounded to the fixed-point grid (half a unit), the factor 2 over that covers the device exp's last
  ulps and numpy's own summation rounding, both orders of magnitude smaller (numpy's once its running sum is kept
  exact, see ``ref_histogram``: taken as it is, numpy.histogram(weights=...) alone is off by some 200 units at 10^5
  values);
* the raw fixed-point sums and the counts are bitwise (``torch.equal``) independent of the order of the walkers inside a
  population, of the order of the populations, of n_pop and of the run;
* each moment sum agrees with numpy fp64 to 1e-11 * sum w |term| (reordering 4 096 terms gives 4.5e-13, the rest covers
  ulp differences of exp)."""
import numpy as np
import pytest
import torch

from tests import _observables as OB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # the shared references stay read-only


def check_histogram(h, counts, wref, m, n_bad, n_ninf, shift, tag):
    got_c = h.counts.cpu().numpy()
    assert got_c.dtype == np.int64 and np.array_equal(got_c, counts), (tag, np.abs(got_c - counts).max())
    assert h.shift == shift and np.array_equal(h.log_scale, m) and np.array_equal(h.n_bad, n_bad) and \
        np.array_equal(h.n_neg_inf, n_ninf), (tag, h.shift, shift, h.log_scale, m, h.n_bad, n_bad, h.n_neg_inf, n_ninf)
    raw = h.raw.cpu().numpy()
    assert raw.dtype == np.int64 and (raw >= 0).all()
    # (a sum above 2^53 rounds in the conversion: 2^-53 of a value <= n_bin, far inside the bound)
    err = np.abs(raw.astype(np.float64) * 2.0 ** -shift - wref)
    assert (err <= counts * 2.0 ** -shift).all(), (tag, err.max(), (err * 2.0 ** shift).max())
    assert np.array_equal(h.weights.cpu().numpy(), raw.astype(np.float64) * 2.0 ** -shift)


# ------------------------------------------------------------------------------------------------- value histogram
@pytest.mark.parametrize("nbins", [1, 100, 1024])
@pytest.mark.parametrize("P", [1, 3, 40])
@pytest.mark.parametrize("S", [1, 63, 257, 2048])
def test_weighted_histogram_against_numpy(pa, S, P, nbins):
    from pita_amd import metrics

    for per_walker in (1, 7):
        shift = OB.shift_of(S, per_walker)
        assert shift == 40
        lw = OB.logweights(S, P, offset=(S + nbins + per_walker) % 5)
        m, n_bad, n_ninf, _, _ = OB.ref_info(lw, P, S)
        base = OB.values(S, P, per_walker)
        for kind in ("uniform", "nonuniform"):
            edges = OB.edges_for(kind, nbins, base)
            v = OB.on_edges(base, edges)
            counts, wref = OB.ref_histogram(v, lw, P, S, per_walker, edges)
            h = metrics.weighted_histogram(dev(v), edges, dev(lw), populations=P, per_walker=per_walker)
            check_histogram(h, counts, wref, m, n_bad, n_ninf, shift, (S, P, nbins, per_walker, kind))
            # unit weights: the sums are the counts on the fixed-point grid, and the counts are pita_histogram's
            u = metrics.weighted_histogram(dev(v), edges, None, populations=P, per_walker=per_walker)
            assert torch.equal(u.raw, u.counts << shift)
            assert np.array_equal(u.log_scale, np.zeros(P)) and not u.n_bad.any() and not u.n_neg_inf.any() and u.shift == shift
            plain = torch.stack([metrics.histogram(dev(v.reshape(P, -1)[p]), edges) for p in range(min(P, 3))])
            assert torch.equal(u.counts[:min(P, 3)], plain)


def test_a_dominant_weight_and_an_empty_population(pa):
    """One entry 60 above the rest: every other weight quantises to 0 (e^-60 * 2^40 << 1/2), the sum is exactly 2^shift in
    one bin; a population of -inf weights sums to 0 everywhere, keeps its counts, and its density row is NaN."""
    from pita_amd import metrics

    S, P = 257, 5
    lw = OB.logweights(S, P, offset=0).reshape(P, S)
    v = OB.values(S, P, 1).reshape(P, S)
    v[3, (2 * S) // 3] = 2.0
    edges = np.linspace(-1, 5, 13).astype(np.float32)
    h = metrics.weighted_histogram(dev(v), edges, dev(lw), populations=P)
    raw = h.raw.cpu().numpy()
    assert raw[3].sum() == 2 ** 40 and raw[3, 6] == 2 ** 40 and h.log_scale[3] == lw[3].max()
    assert raw[2].sum() == 0 and h.counts[2].sum() > 0 and h.n_neg_inf[2] == S
    dens = h.density(edges)
    assert np.isnan(dens[2]).all() and np.isfinite(dens[[0, 1, 3, 4]]).all()
    assert np.allclose((dens[[0, 1, 3, 4]] * np.diff(edges.astype(np.float64))).sum(1), 1.0, rtol=0, atol=1e-12)


def shuffled(rng, P, S, *arrays_with_width):
    """the same permutation of the walkers inside each population applied to every (array, per-walker width) pair"""
    perm = np.concatenate([p * S + rng.permutation(S) for p in range(P)])
    return [a.reshape(P * S, w)[perm].reshape(a.shape) for a, w in arrays_with_width]


@pytest.mark.parametrize("S,P,nbins,per_walker", [(257, 3, 100, 7), (2048, 40, 1024, 1), (63, 5, 1, 1)])
def test_weighted_histogram_is_bitwise_independent_of_order_and_placement(pa, S, P, nbins, per_walker):
    from pita_amd import metrics

    rng = np.random.default_rng(77)
    lw = OB.logweights(S, P, offset=0)
    base = OB.values(S, P, per_walker)
    edges = OB.edges_for("uniform", nbins, base)
    v = OB.on_edges(base, edges)
    run = lambda vv, ll, pp: metrics.weighted_histogram(dev(vv), edges, dev(ll), populations=pp, per_walker=per_walker)
    h = run(v, lw, P)
    again = run(v, lw, P)
    assert torch.equal(h.raw, again.raw) and torch.equal(h.counts, again.counts)
    v2, lw2 = shuffled(rng, P, S, (v, per_walker), (lw, 1))
    assert not np.array_equal(lw2, lw, equal_nan=True)
    g = run(v2, lw2, P)
    assert torch.equal(h.raw, g.raw) and torch.equal(h.counts, g.counts)
    order = rng.permutation(P)
    g = run(v.reshape(P, -1)[order], lw.reshape(P, -1)[order], P)
    assert torch.equal(h.raw[dev(order)], g.raw) and torch.equal(h.counts[dev(order)], g.counts)
    for p in sorted({0, 1 % P, 2 % P, 3 % P, P - 1}):
        g = run(v.reshape(P, -1)[p], lw.reshape(P, -1)[p], 1)
        assert torch.equal(h.raw[p:p + 1], g.raw) and torch.equal(h.counts[p:p + 1], g.counts), p
        assert g.log_scale[0] == h.log_scale[p] and g.n_bad[0] == h.n_bad[p] and g.n_neg_inf[0] == h.n_neg_inf[p]


@pytest.mark.parametrize("n", [0, 1, 1000, 2 ** 20 + 3])
def test_entry_point_counts_equal_pita_histogram(pa, n):
    L = pa._lib.lib()
    rng = np.random.default_rng(5 + n)
    v = rng.normal(2.0, 1.5, n).astype(np.float32)
    edges = np.histogram_bin_edges(np.float32([-1.0, 4.5]), bins=100).astype(np.float32)
    if n >= 1000:
        v[:101] = edges
        v[200:203] = [np.nan, np.inf, -np.inf]
    tv, te = dev(v), dev(edges)
    want = torch.full((100,), -1, dtype=torch.int64, device="cuda")
    st = pa._lib.stream_ptr(te.device)
    pa._lib.check(L.pita_histogram(pa._lib.ptr(tv) if n else None, n, te.data_ptr(), 100, want.data_ptr(), st))
    wsum, counts = (torch.full((1, 100), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    info = torch.empty(1, 4, dtype=torch.float64, device="cuda")
    rc = L.pita_weighted_histogram(tv.data_ptr() if n else None, None, 1, n, 1, te.data_ptr(), 100, wsum.data_ptr(),
                                   counts.data_ptr(), info.data_ptr(), st)
    if n == 0:  # an empty population is refused (pop_size >= 1) and nothing is written; pita_histogram writes zeros
        assert rc == -1 and int(want.sum()) == 0 and int(counts.sum()) == -100
        return
    pa._lib.check(rc)
    assert torch.equal(counts[0], want) and int(want.sum()) > 0
    shift = OB.shift_of(n, 1)
    assert torch.equal(wsum, counts << shift) and info.cpu().tolist() == [[0.0, 0.0, 0.0, float(shift)]]


# ------------------------------------------------------------------------------------------------- pair distances
class _Target:
    """what pair_distance_histogram reads from an energy function"""
    should_normalize = False

    def __init__(self, n, d):
        self.n_particles, self.n_spatial_dim = n, d


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("S", [1, 63, 257])
@pytest.mark.parametrize("n,d", [(2, 3), (4, 2), (13, 3), (22, 3), (55, 3), (256, 3)])
def test_pair_distance_histogram(pa, n, d, S, P):
    from pita_amd import metrics

    npairs = n * (n - 1) // 2
    shift = OB.shift_of(S, npairs)
    assert shift == min(40, 62 - int(np.ceil(np.log2(S * npairs))))
    x, dist = OB.coords(n, d, S, P), OB.pair_distances(n, d, S, P)
    lw = OB.logweights(S, P, offset=(n + S) % 5)
    m, n_bad, n_ninf, _, _ = OB.ref_info(lw, P, S)
    tx, tl, td = dev(x), dev(lw), dev(dist)
    rng = np.random.default_rng(n + S + P)
    full = np.histogram_bin_edges(dist, bins=100).astype(np.float32)
    mean = float(dist.mean(dtype=np.float64))
    cut = np.histogram_bin_edges(dist, bins=37, range=(0.6 * mean, 1.2 * mean)).astype(np.float32)  # cuts both tails off
    assert (np.diff(full) > 0).all() and (np.diff(cut) > 0).all()
    for edges in (full, cut):
        counts, wref = OB.ref_histogram(dist, lw, P, S, npairs, edges)
        h = metrics.pair_distance_histogram(_Target(n, d), tx, edges, tl, populations=P)
        check_histogram(h, counts, wref, m, n_bad, n_ninf, shift, (n, d, S, P, len(edges)))
        w = metrics.weighted_histogram(td, edges, tl, populations=P, per_walker=npairs)
        assert torch.equal(h.raw, w.raw) and torch.equal(h.counts, w.counts)
        u = metrics.pair_distance_histogram(_Target(n, d), tx, edges, None, populations=P)
        assert torch.equal(u.raw, u.counts << shift)
        clean = dev(np.flatnonzero(n_bad == 0))  # no walker left out there: the counts are the weighted call's
        assert torch.equal(u.counts[clean], h.counts[clean]) and int(u.counts.sum()) >= int(h.counts.sum())
    # order and placement, bitwise
    again = metrics.pair_distance_histogram(_Target(n, d), tx, cut, tl, populations=P)
    assert torch.equal(h.raw, again.raw) and torch.equal(h.counts, again.counts)
    x2, lw2 = shuffled(rng, P, S, (x, n * d), (lw, 1))
    g = metrics.pair_distance_histogram(_Target(n, d), dev(x2), cut, dev(lw2), populations=P)
    assert torch.equal(h.raw, g.raw) and torch.equal(h.counts, g.counts)
    order = rng.permutation(P)
    g = metrics.pair_distance_histogram(_Target(n, d), dev(x.reshape(P, -1)[order]), cut, dev(lw.reshape(P, -1)[order]), populations=P)
    assert torch.equal(h.raw[dev(order)], g.raw) and torch.equal(h.counts[dev(order)], g.counts)
    for p in range(P):
        g = metrics.pair_distance_histogram(_Target(n, d), dev(x.reshape(P, -1)[p]), cut, dev(lw.reshape(P, -1)[p]), populations=1)
        assert torch.equal(h.raw[p:p + 1], g.raw) and torch.equal(h.counts[p:p + 1], g.counts), p


# ------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("P", [1, 3, 40])
@pytest.mark.parametrize("S", [1, 63, 1025, 4096])
def test_weighted_moments(pa, S, P):
    from pita_amd import metrics

    L = pa._lib.lib()
    for offset in range(5 if P == 1 else 2):
        lw = OB.logweights(S, P, offset=offset)
        for v in (OB.values(S, P, 1), np.random.default_rng(S + P).normal(-3.0, 2.0, P * S).astype(np.float32)):
            want, mag = OB.ref_moments(v, lw, P, S)
            tv, tl = dev(v), dev(lw)
            out = torch.full((P, 6), -1.0, dtype=torch.float64, device="cuda")
            st = pa._lib.stream_ptr(tv.device)
            pa._lib.check(L.pita_weighted_moments(tv.data_ptr(), tl.data_ptr(), P, S, out.data_ptr(), st))
            got = out.cpu().numpy()
            assert np.array_equal(got[:, [0, 4, 5]], want[:, [0, 4, 5]]), (S, P, offset)
            err = np.abs(got[:, 1:4] - want[:, 1:4])
            assert (err <= 1e-11 * mag).all(), (S, P, offset, (err / np.maximum(mag, 1e-300)).max())
            for p in sorted({0, P // 2, P - 1}):  # a population's row does not depend on n_pop or on its place
                one = torch.empty(1, 6, dtype=torch.float64, device="cuda")
                pa._lib.check(L.pita_weighted_moments(tv[p * S:].data_ptr(), tl[p * S:].data_ptr(), 1, S, one.data_ptr(), st))
                assert torch.equal(one[0].view(torch.int64), out[p].view(torch.int64)), (S, P, p)
            r = metrics.weighted_mean(tv, tl, populations=P)
            with np.errstate(invalid="ignore", divide="ignore"):
                mean = np.where(got[:, 1] > 0, got[:, 2] / got[:, 1], np.nan)
                var = np.where(got[:, 1] > 0, got[:, 3] / got[:, 1] - mean * mean, np.nan)
            assert np.array_equal(r["mean"], mean, equal_nan=True) and np.array_equal(r["n_bad"], want[:, 4])
            assert np.array_equal(r["var"], var, equal_nan=True)
            if np.isfinite(v).all():
                for p in sorted({0, P - 1}):
                    s = metrics.logweight_stats(tl[p * S:(p + 1) * S])
                    assert r["ess"][p] == s["ess"] and r["ess_fraction"][p] == s["ess_fraction"], (S, P, p)
        # unit weights
        v = np.random.default_rng(S).normal(1.0, 2.0, P * S).astype(np.float32)
        r = metrics.weighted_mean(dev(v), None, populations=P)
        v64 = v.astype(np.float64).reshape(P, S)
        assert np.allclose(r["mean"], v64.mean(1), rtol=1e-11, atol=1e-11) and np.allclose(r["var"], v64.var(1), rtol=1e-9, atol=1e-11)
        assert np.array_equal(r["ess"], np.full(P, float(S))) and np.array_equal(r["ess_fraction"], np.ones(P))


# ------------------------------------------------------------------------------------------------- host layer
@pytest.fixture(scope="module")
def lj13(pa):
    from oracle import pita_oracle as O

    energy = pa.LennardJonesEnergy(39, 13, 3)
    gen = torch.Generator().manual_seed(21)
    base = O.remove_mean(torch.randn(1, 39, generator=gen) * 0.9, 13, 3)
    test_set = O.remove_mean(base + 0.08 * torch.randn(1000, 39, generator=gen), 13, 3).cuda()
    samples = O.remove_mean(base + 0.10 * torch.randn(256, 39, generator=gen), 13, 3).cuda()
    return energy, samples, test_set


def test_sample_histograms_default_path_is_unchanged(pa, lj13):
    from pita_amd import metrics

    energy, samples, test_set = lj13
    h = metrics.sample_histograms(energy, samples, test_set)
    assert sorted(h) == ["dist_edges", "dist_samples", "dist_test", "energy_edges", "energy_samples", "energy_test"]
    d_test, d_gen = energy.interatomic_dist(test_set).reshape(-1).float(), energy.interatomic_dist(samples).reshape(-1).float()
    d_edges = np.histogram_bin_edges(torch.stack([d_test.min(), d_test.max()]).cpu().numpy().astype(np.float32), bins=100)
    e_test, e_gen = -energy(test_set).float(), -energy(samples).float()
    em = torch.stack([e_test.min(), e_test.max()]).cpu().numpy().astype(np.float32)
    e_edges = np.histogram_bin_edges(em, bins=100, range=(float(em[0]) - 10, float(em[1]) + 10))
    dens = lambda v, e: metrics._density(metrics.histogram(v, e), e)
    for key, want in (("dist_edges", d_edges), ("dist_test", dens(d_test, d_edges)), ("dist_samples", dens(d_gen, d_edges)),
                      ("energy_edges", e_edges), ("energy_test", dens(e_test, e_edges)), ("energy_samples", dens(e_gen, e_edges))):
        assert np.array_equal(h[key], want), key


def test_sample_histograms_weighted_and_per_population(pa, lj13):
    from pita_amd import metrics

    energy, samples, test_set = lj13
    plain = metrics.sample_histograms(energy, samples, test_set)
    zero = metrics.sample_histograms(energy, samples, test_set, logweights=torch.zeros(256, device="cuda"), populations=1)
    for key in plain:
        assert np.allclose(zero[key], plain[key], rtol=0, atol=1e-12), key
    for side in ("dist", "energy"):
        assert zero[f"{side}_samples_pop"].shape == (1, 100) and np.isnan(zero[f"{side}_samples_stderr"]).all()
    four = metrics.sample_histograms(energy, samples, test_set, populations=4)
    lw = torch.from_numpy(OB.logweights(64, 4, offset=4)).cuda()  # clean, clean, with non-finite entries, all -inf
    wtd = metrics.sample_histograms(energy, samples, test_set, logweights=lw, populations=4)
    e_gen = -energy(samples).float()
    for p in range(4):
        sl = slice(64 * p, 64 * (p + 1))
        alone = metrics.sample_histograms(energy, samples[sl], test_set)
        for side in ("dist", "energy"):
            assert np.allclose(four[f"{side}_samples_pop"][p], alone[f"{side}_samples"], rtol=0, atol=1e-12), (side, p)
        want = metrics.weighted_histogram(e_gen[sl], wtd["energy_edges"], lw[sl]).density(wtd["energy_edges"])[0]
        assert np.array_equal(wtd["energy_samples_pop"][p], want, equal_nan=True), p
        want = metrics.pair_distance_histogram(energy, samples[sl], wtd["dist_edges"], lw[sl]).density(wtd["dist_edges"])[0]
        assert np.array_equal(wtd["dist_samples_pop"][p], want, equal_nan=True), p
    for side in ("dist", "energy"):
        pop = four[f"{side}_samples_pop"]
        assert pop.shape == (4, 100)
        assert np.allclose(four[f"{side}_samples"], pop.mean(0), rtol=0, atol=1e-15)
        assert np.allclose(four[f"{side}_samples_stderr"], pop.std(0, ddof=1) / 2.0, rtol=1e-14, atol=0)
        pop = wtd[f"{side}_samples_pop"]  # the all -inf population has no estimate and is left out of the error bar
        assert np.isnan(pop[3]).all() and np.isfinite(pop[:3]).all()
        assert np.allclose(wtd[f"{side}_samples"], pop[:3].mean(0), rtol=0, atol=1e-15)
        assert np.allclose(wtd[f"{side}_samples_stderr"], pop[:3].std(0, ddof=1) / np.sqrt(3.0), rtol=1e-14, atol=0)


def test_weighted_energy_distances_and_interatomic_w2(pa, lj13):
    from pita_amd import metrics

    energy, samples, test_set = lj13
    pred, true = energy(samples), energy(test_set)
    pred = pred.clone()
    pred[5] = 5000.0  # one cropped entry
    plain = metrics.energy_distances(pred, true, prefix="val")
    zero = metrics.energy_distances(pred, true, prefix="val", pred_logweights=torch.zeros(256, device="cuda"))
    assert plain.keys() == zero.keys()
    for k in plain:
        assert zero[k] == pytest.approx(plain[k], rel=1e-12, abs=1e-12), k
    mult = np.random.default_rng(3).integers(1, 5, 256)
    tm = torch.from_numpy(mult).cuda()
    rep = metrics.energy_distances(pred.repeat_interleave(tm), true, prefix="val")
    wtd = metrics.energy_distances(pred, true, prefix="val", pred_logweights=torch.log(tm.double()))
    for k in rep:
        if k != "val/num_cropped":
            assert wtd[k] == pytest.approx(rep[k], rel=1e-12, abs=1e-12), k
    mask = ((pred < -1000) | (pred > 1000)).cpu().numpy()
    assert mask[5] and wtd["val/num_cropped"] == int(mask.sum()) and rep["val/num_cropped"] == int(mult[mask].sum())
    w2 = metrics.interatomic_w2(energy, samples, test_set)
    assert metrics.interatomic_w2(energy, samples, test_set, pred_logweights=torch.zeros(256, device="cuda")) == \
        pytest.approx(w2, rel=1e-12)
    assert metrics.interatomic_w2(energy, samples, test_set, pred_logweights=torch.log(tm.double())) == \
        pytest.approx(metrics.interatomic_w2(energy, samples.repeat_interleave(tm, dim=0), test_set), rel=1e-12)
