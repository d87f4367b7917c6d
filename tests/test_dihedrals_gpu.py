"""pita_dihedral_angles, pita_dihedral_histogram2d and the host layer over them in pita_amd.metrics.  Run on an MI355X:
pytest -m gpu.

Inputs and numpy references: tests/_dihedrals.py.  Bounds:

* angles: |wrap(theta_gpu - theta_fp64)| <= max(8 * e32, 4 ulp of pi), e32 = the largest error of the numpy float32
  restatement against fp64 ON THE SAME INPUTS -- the bound comes from the reference, never from the kernel.  The factor 8
  covers the device's atan2f differing from the C library's by a few ulp and that difference being amplified by the same
  conditioning; everything before atan2f is the same correctly rounded arithmetic;
* counts, m, n_bad, n_neg_inf and the shift are exact: the counts are the restated bin rule applied per axis to the
  library's OWN angles, bit for bit;
* per cell |raw * 2^-shift - sum of exp(logw - m) in fp64| <= n_cell * 2^-shift, the bound of tests/test_observables_gpu.py
  for the reason given there (half a unit of the fixed-point grid per contribution, the rest for the device exp's ulps);
* raw sums and counts are bitwise (``torch.equal``) independent of the order of the walkers inside a population, of the
  order of the populations, of n_pop and of the run."""
import numpy as np
import pytest
import torch

from tests import _dihedrals as DH
from tests import _observables as OB

pytestmark = pytest.mark.gpu

FULL = np.linspace(-np.pi, np.pi, 65).astype(np.float32)


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # the shared references stay read-only


def gpu_angles(x, quads):
    from pita_amd import metrics

    return metrics.dihedral_angles(dev(x), quads).cpu().numpy()


# ------------------------------------------------------------------------------------------------- angles
@pytest.mark.parametrize("B", [1, 63, 257, 2048])
@pytest.mark.parametrize("name", ["ala2", "ala3", "ala4"])
def test_angles_against_fp64(pa, name, B):
    """Measured on an MI355X (profiles/r17_dihedrals.txt), largest error over the twelve cases, in radians: numpy float32
    restatement 3.05e-7, device 3.22e-7 (per case the two are equal or within 10 % of each other; bounds 0.95e-6 .. 2.4e-6)."""
    w = DH.walkers(name, B)
    x, quads = w["x"], w["quads"]
    ref = DH.ref_angles64(x, quads)
    e32 = np.abs(DH.wrap(DH.ref_angles32(x, quads).astype(np.float64) - ref)).max()
    bound = max(8.0 * e32, DH.ANGLE_FLOOR)
    got = gpu_angles(x, quads)
    assert got.shape == (B, len(quads)) and got.dtype == np.float32 and (np.abs(got) <= DH.PI32).all()
    err = np.abs(DH.wrap(got.astype(np.float64) - ref)).max()
    print(f"dihedral angles {name} x {B}: numpy float32 error {e32:.3e}, device error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (name, B, err, e32, bound)
    # [B, n, 3] is the same input, one quad alone the same column, and the run does not matter
    from pita_amd import metrics

    again = metrics.dihedral_angles(dev(x).reshape(B, w["n"], 3), quads[-1])
    assert again.shape == (B, 1) and np.array_equal(again.cpu().numpy()[:, 0], got[:, -1])
    # reflection: every operation before atan2f is odd or even in the reflected coordinate, exactly
    refl = gpu_angles(DH.reflect(x), quads)
    inner = (got != 0) & (np.abs(got) != DH.PI32)
    assert inner.mean() > 0.99 and np.array_equal(refl[inner], -got[inner])


def test_planted_angles_and_many_dihedrals(pa):
    x64 = DH.planted()
    x = x64.astype(np.float32)
    quad = [(0, 1, 2, 3)]
    ref = DH.ref_angles64(x, quad)
    e32 = np.abs(DH.wrap(DH.ref_angles32(x, quad).astype(np.float64) - ref)).max()
    bound = max(8.0 * e32, DH.ANGLE_FLOOR)
    got = gpu_angles(x, quad)
    err = np.abs(DH.wrap(got.astype(np.float64) - ref)).max()
    print(f"dihedral angles planted x {len(x)}: numpy float32 error {e32:.3e}, device error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, e32, bound)
    assert np.abs(DH.wrap(got[:, 0].astype(np.float64) - DH.PLANTED_T)).max() <= 4 * DH.ANGLE_FLOOR  # rounded coordinates
    refl = gpu_angles(DH.reflect(x), quad)
    inner = (got != 0) & (np.abs(got) != DH.PI32)
    assert np.array_equal(refl[inner], -got[inner]) and np.array_equal(np.abs(refl[~inner]), np.abs(got[~inner]))
    # documented special values: collinear atoms give 0, a non-finite coordinate gives NaN in the quads that use the atom
    line = np.float32([[0, 0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 0, 0, 1, 0]])
    assert gpu_angles(line, [(0, 1, 2, 3)])[0, 0] == 0.0
    for bad in (np.nan, np.inf, -np.inf):
        y = np.array(DH.walkers("four", 63)["x"]).reshape(63, 4, 3)
        y = np.concatenate([y, y[:, :1] + 1.0], 1)  # a fifth atom
        y[5, 4, 1] = bad
        a = gpu_angles(y.reshape(63, 15), [(0, 1, 2, 3), (1, 2, 3, 4), (4, 0, 1, 2)])
        assert np.isnan(a[5, 1:]).all() and np.isfinite(a[5, 0]) and np.isfinite(np.delete(a, 5, 0)).all()
    # the largest table: 1024 dihedrals over 256 atoms, a batch that is no multiple of the staged chunk; the bound is
    # taken over the well-conditioned (walker, quad) items, as everywhere
    rng = np.random.default_rng(8)
    big = rng.normal(0.0, 1.0, (21, 256 * 3)).astype(np.float32)
    quads = np.stack([rng.permutation(256)[:4] for _ in range(1024)])
    quads[-1] = (255, 0, 254, 1)
    ok = DH.conditioned(big, quads)
    assert ok.mean() > 0.1 and ok[:, -1].any()
    ref = DH.ref_angles64(big, quads)
    e32 = np.abs(DH.wrap(DH.ref_angles32(big, quads).astype(np.float64) - ref))[ok].max()
    got = gpu_angles(big, quads)
    err = np.abs(DH.wrap(got.astype(np.float64) - ref))[ok].max()
    print(f"dihedral angles 256 atoms x 21 x 1024: numpy float32 error {e32:.3e}, device error {err:.3e}")
    assert np.isfinite(got).all() and err <= max(8.0 * e32, DH.ANGLE_FLOOR), (err, e32)
    from pita_amd import metrics

    assert metrics.dihedral_angles(torch.empty(0, 66, device="cuda"), quad).shape == (0, 1)


# ------------------------------------------------------------------------------------------------- 2-D histogram
def nonuniform_edges(n, seed):
    rng = np.random.default_rng(seed)
    e = np.unique(np.concatenate([[-np.pi, np.pi], rng.uniform(-np.pi, np.pi, n - 1)]).astype(np.float32))
    assert e.size == n + 1
    return e


CASES = [  # name, pop_size, P, n_pair, (edges_a, edges_b)
    ("four", 1, 1, 3, (1, 1)),
    ("ala2", 63, 3, 1, (7, 5)),
    ("ala4", 257, 3, 3, (64, 64)),
    ("ala2", 2048, 1, 1, (64, 64)),
    ("ala4", 63, 40, 3, (7, 5)),
    ("ala2", 257, 40, 1, "nonuniform"),
    ("four", 2048, 3, 3, (64, 64)),
    ("ala3", 257, 1, 1, (1, 1)),
    ("four", 63, 40, 1, (64, 64)),
]


def case_inputs(name, S, P, n_pair, bins):
    w = DH.walkers(name, S * P)
    pairs = w["pairs"][:n_pair]
    assert pairs.shape == (n_pair, 2, 4)
    if bins == "nonuniform":
        ea, eb = nonuniform_edges(7, 1), nonuniform_edges(5, 2)
    else:
        ea, eb = (np.linspace(-np.pi, np.pi, b + 1).astype(np.float32) for b in bins)
    return w["x"], pairs, ea, eb


def check_against_own_angles(h, x, pairs, lw, P, S, ea, eb, tag):
    from pita_amd import metrics

    n_pair = len(pairs)
    angles = metrics.dihedral_angles(dev(x), pairs.reshape(-1, 4))
    cols = [(2 * k, 2 * k + 1) for k in range(n_pair)]
    counts, wref = DH.ref_histogram2d(angles.cpu().numpy(), cols, lw, P, S, ea, eb)
    shift = OB.shift_of(S, 1)
    got_c, raw = h.counts.cpu().numpy(), h.raw.cpu().numpy()
    assert got_c.shape == (P, n_pair, len(ea) - 1, len(eb) - 1) and got_c.dtype == np.int64 and raw.dtype == np.int64
    assert np.array_equal(got_c, counts), (tag, np.abs(got_c - counts).sum())
    if lw is None:
        m, n_bad, n_ninf = np.zeros(P), np.zeros(P), np.zeros(P)
    else:
        m, n_bad, n_ninf, _, _ = OB.ref_info(lw, P, S)
    assert h.shift == shift and np.array_equal(h.log_scale, m) and np.array_equal(h.n_bad, n_bad) and \
        np.array_equal(h.n_neg_inf, n_ninf), (tag, h.shift, shift, h.log_scale, m, h.n_bad, n_bad, h.n_neg_inf, n_ninf)
    assert (raw >= 0).all()
    err = np.abs(raw.astype(np.float64) * 2.0 ** -shift - wref)
    assert (err <= counts * 2.0 ** -shift).all(), (tag, err.max(), (err * 2.0 ** shift).max())
    assert np.array_equal(h.weights.cpu().numpy(), raw.astype(np.float64) * 2.0 ** -shift)
    assert np.array_equal(h.edges_a, ea) and np.array_equal(h.edges_b, eb)
    return angles


@pytest.mark.parametrize("name,S,P,n_pair,bins", CASES)
def test_histogram_against_the_librarys_own_angles(pa, name, S, P, n_pair, bins):
    from pita_amd import metrics

    x, pairs, ea, eb = case_inputs(name, S, P, n_pair, bins)
    tx = dev(x)
    for offset in range(5 if P == 1 else 2):  # every flavour of log-weights in every place
        lw = OB.logweights(S, P, offset=offset)
        h = metrics.ramachandran_histogram(tx, pairs, logweights=dev(lw), populations=P, edges=(ea, eb))
        angles = check_against_own_angles(h, x, pairs, lw, P, S, ea, eb, (name, S, P, n_pair, offset))
        # the edges cover the circle and the coordinates are finite: the marginals are the 1-D weighted histograms, bit for bit
        for axis, e in ((0, ea), (1, eb)):
            raw_m, counts_m = h.marginal(axis)
            assert raw_m.shape == (P, n_pair, len(e) - 1)
            for k in range(n_pair):
                one = metrics.weighted_histogram(angles[:, 2 * k + axis].contiguous(), e, dev(lw), populations=P)
                assert torch.equal(raw_m[:, k], one.raw) and torch.equal(counts_m[:, k], one.counts), (axis, k, offset)
    u = metrics.ramachandran_histogram(tx, pairs, populations=P, edges=(ea, eb))
    check_against_own_angles(u, x, pairs, None, P, S, ea, eb, (name, S, P, n_pair, "unit"))
    assert torch.equal(u.raw, u.counts << u.shift) and int(u.counts.sum()) == P * S * n_pair
    if bins == (64, 64):  # the default edges
        d = metrics.ramachandran_histogram(tx, pairs, populations=P)
        assert torch.equal(d.raw, u.raw) and torch.equal(d.counts, u.counts) and np.array_equal(d.edges_a, FULL)
        d = metrics.ramachandran_histogram(tx, pairs, bins=64, populations=P, edges=FULL)
        assert torch.equal(d.raw, u.raw) and torch.equal(d.counts, u.counts)


def shuffled(rng, P, S, *arrays_with_width):
    """the same permutation of the walkers inside each population applied to every (array, per-walker width) pair"""
    perm = np.concatenate([p * S + rng.permutation(S) for p in range(P)])
    return [a.reshape(P * S, w)[perm].reshape(a.shape) for a, w in arrays_with_width]


@pytest.mark.parametrize("name,S,P,n_pair,bins", [CASES[2], CASES[5], CASES[6], CASES[3]])
def test_histogram_is_bitwise_independent_of_order_and_placement(pa, name, S, P, n_pair, bins):
    from pita_amd import metrics

    rng = np.random.default_rng(78)
    x, pairs, ea, eb = case_inputs(name, S, P, n_pair, bins)
    lw = OB.logweights(S, P, offset=0)
    run = lambda xx, ll, pp: metrics.ramachandran_histogram(dev(xx.reshape(-1, x.shape[1])), pairs, logweights=dev(ll.reshape(-1)),
                                                            populations=pp, edges=(ea, eb))
    h = run(x, lw, P)
    again = run(x, lw, P)
    assert torch.equal(h.raw, again.raw) and torch.equal(h.counts, again.counts) and int(h.counts.sum()) > 0
    x2, lw2 = shuffled(rng, P, S, (x, x.shape[1]), (lw, 1))
    assert not np.array_equal(lw2, lw, equal_nan=True)
    g = run(x2, lw2, P)
    assert torch.equal(h.raw, g.raw) and torch.equal(h.counts, g.counts)
    order = rng.permutation(P)
    g = run(x.reshape(P, -1)[order], lw.reshape(P, -1)[order], P)
    assert torch.equal(h.raw[dev(order)], g.raw) and torch.equal(h.counts[dev(order)], g.counts)
    for p in sorted({0, 1 % P, 2 % P, 3 % P, P - 1}):
        g = run(x.reshape(P, -1)[p], lw.reshape(P, -1)[p], 1)
        assert torch.equal(h.raw[p:p + 1], g.raw) and torch.equal(h.counts[p:p + 1], g.counts), p
        assert g.log_scale[0] == h.log_scale[p] and g.n_bad[0] == h.n_bad[p] and g.n_neg_inf[0] == h.n_neg_inf[p]


def test_left_out_items(pa):
    from pita_amd import metrics

    S, P = 257, 3
    w = DH.walkers("ala4", S * P)
    x, pairs = np.array(w["x"]), w["pairs"]
    tx = dev(x)
    # a NaN coordinate in the atom that only pair 0's b-quad uses among the six quads: the N that ends psi of residue 1 is
    # also in phi and psi of residue 2, so take pair 2's last N (psi of the last residue), and make that pair number 0
    order = pairs[[2, 0, 1]]
    atom = int(order[0, 1, 3])
    assert (order.reshape(-1, 4) == atom).sum() == 1
    full = metrics.ramachandran_histogram(tx, order, bins=16, populations=P)
    hit = [5, S + 7, 2 * S + 256]
    for bad in (np.nan, np.inf):
        y = x.copy().reshape(S * P, -1, 3)
        y[hit, atom, 2] = bad
        h = metrics.ramachandran_histogram(dev(y.reshape(S * P, -1)), order, bins=16, populations=P)
        assert torch.equal(h.counts[:, 1:], full.counts[:, 1:]) and torch.equal(h.raw[:, 1:], full.raw[:, 1:])
        assert h.counts[:, 0].sum(dim=(1, 2)).tolist() == [S - 1] * P and int(full.counts[:, 0].sum()) == S * P
        gone = full.counts[:, 0] - h.counts[:, 0]  # one cell per population lost the walker, phi's row unchanged
        assert (gone >= 0).all() and gone.sum(dim=(1, 2)).tolist() == [1] * P
        assert torch.equal(h.marginal(0)[1][:, 0] + gone.sum(dim=2), full.marginal(0)[1][:, 0])
        assert not h.n_bad.any()  # n_bad counts log-weights, not coordinates
    # edges over half the circle drop the rest: on the a-axis only, then on both
    whole = np.linspace(-np.pi, np.pi, 17).astype(np.float32)
    half = whole[8:].copy()  # [0, pi]: its bins are bins 8 .. 15 of `whole`
    assert half[0] == 0.0 and half.size == 9
    lw = OB.logweights(S, P, offset=0)
    f = metrics.ramachandran_histogram(tx, pairs, logweights=dev(lw), populations=P, edges=whole)
    a = metrics.ramachandran_histogram(tx, pairs, logweights=dev(lw), populations=P, edges=(half, whole))
    assert torch.equal(a.raw, f.raw[:, :, 8:]) and torch.equal(a.counts, f.counts[:, :, 8:])
    b = metrics.ramachandran_histogram(tx, pairs, logweights=dev(lw), populations=P, edges=(half, half))
    assert torch.equal(b.raw, f.raw[:, :, 8:, 8:]) and torch.equal(b.counts, f.counts[:, :, 8:, 8:])
    assert 0 < int(b.counts.sum()) < int(a.counts.sum()) < int(f.counts.sum())
    # an all -inf population (flavour 2): no weight, its counts kept, no density
    assert OB.flavour(2, 0) == "all_neg_inf" and f.n_neg_inf[2] == S
    assert int(f.raw[2].sum()) == 0 and int(f.counts[2].sum()) == S * len(pairs)
    dens = f.density()
    assert np.isnan(dens[2]).all() and np.isfinite(dens[:2]).all()


class _Normalising:
    """what the dihedral entry points read from an energy function"""
    should_normalize = True

    def unnormalize(self, x):
        return x * 0.25 + 0.125  # the test applies the same torch ops to the other side


def test_host_layer(pa):
    from pita_amd import metrics

    S, P = 256, 4
    w = DH.walkers("ala4", S * P)
    pairs, tx = w["pairs"], dev(w["x"])
    lw = dev(OB.logweights(S, P, offset=3))  # one dominant, clean, clean, with non-finite entries
    target = _Normalising()
    h = metrics.ramachandran_histogram(target.unnormalize(tx), pairs, bins=24, logweights=lw, populations=P)
    g = metrics.ramachandran_histogram(tx, pairs, bins=24, logweights=lw, populations=P, energy_function=target)
    assert torch.equal(h.raw, g.raw) and torch.equal(h.counts, g.counts) and int(h.counts.sum()) > 0
    assert torch.equal(metrics.dihedral_angles(tx, pairs[0], energy_function=target),
                       metrics.dihedral_angles(target.unnormalize(tx), pairs[0]))
    dens = h.density()
    assert dens.shape == (P, 3, 24, 24) and dens.dtype == np.float64 and np.isfinite(dens).all()
    area = np.outer(np.diff(h.edges_a.astype(np.float64)), np.diff(h.edges_b.astype(np.float64)))
    assert np.allclose((dens * area).sum(axis=(2, 3)), 1.0, rtol=0, atol=1e-12)
    s = metrics.population_summary(dens)
    assert s["n_used"] == P and s["mean"].shape == (3, 24, 24) and s["stderr"].shape == (3, 24, 24)
    assert np.allclose(s["mean"], dens.mean(0), rtol=0, atol=1e-15)
    raw_a, counts_a = h.marginal(0)
    assert torch.equal(raw_a, h.raw.sum(3)) and torch.equal(counts_a, h.counts.sum(3)) and raw_a.dtype == torch.int64
    assert torch.equal(h.marginal(1)[1], h.counts.sum(2))
    with pytest.raises(ValueError):
        h.marginal(2)
    with pytest.raises(pa._lib.PitaHipError) as e:  # 65 x 64 cells: refused by the library, the limit in the message
        metrics.ramachandran_histogram(tx, pairs, populations=P, edges=(np.linspace(-3, 3, 66), FULL))
    assert e.value.code == -2 and "4096" in str(e.value)


def test_chirality_fraction(pa):
    from pita_amd import metrics

    S, P = 128, 2
    w = DH.walkers("ala2", S * P)
    names, res = DH.topology("ala2")
    quads, _ = metrics.chirality_quads(names, res)
    assert quads.tolist() == [[8, 6, 14, 10]]
    x = np.array(w["x"])
    x[S:S + 40] = DH.reflect(x[S:S + 40])  # population 1: 40 of 128 walkers mirrored
    theta = DH.ref_angles64(x, quads)
    r = x.reshape(S * P, -1, 3).astype(np.float64)
    triple = np.einsum("bi,bi->b", r[:, 6] - r[:, 8], np.cross(r[:, 14] - r[:, 8], r[:, 10] - r[:, 8]))
    assert np.array_equal(np.sign(np.sin(theta[:, 0])), np.sign(triple)) and np.abs(np.sin(theta)).min() > 0.1
    want = (np.sin(theta) > 0).reshape(P, S).mean(1)
    assert want[1] in (40 / 128, 88 / 128) and want[0] in (0.0, 1.0)
    f = metrics.chirality_fraction(dev(x), quads, populations=P)
    assert f.shape == (P, 1) and f.dtype == np.float64 and np.array_equal(f[:, 0], want)
    assert np.array_equal(metrics.chirality_fraction(dev(DH.reflect(x)), quads, populations=P)[:, 0], 1.0 - want)
    # weighted: the self-normalised sum of the indicator, per population
    lw = OB.logweights(S, P, offset=0)  # clean, with non-finite entries
    _, _, _, bad, wt = OB.ref_info(lw, P, S)
    pos = (np.sin(theta[:, 0]) > 0).reshape(P, S)
    want_w = (wt * pos).sum(1) / wt.sum(1)
    fw = metrics.chirality_fraction(dev(x), quads, logweights=dev(lw), populations=P)
    assert np.allclose(fw[:, 0], want_w, rtol=1e-11, atol=1e-13)
    fr = metrics.chirality_fraction(dev(DH.reflect(x)), quads, logweights=dev(lw), populations=P)
    assert np.allclose(fr[:, 0], 1.0 - want_w, rtol=1e-11, atol=1e-13)
