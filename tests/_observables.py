"""Shared inputs and numpy references of the weighted-observable tests (tests/test_observables_cpu.py,
tests/test_observables_gpu.py).  Everything is seeded through ``numpy.random.default_rng`` and computed once per shape."""
import functools

import numpy as np

MIN_SHIFT, MAX_SHIFT = 20, 40
FLAVOURS = ("clean", "nonfinite", "all_neg_inf", "one_dominant", "clean")


def shift_of(pop_size, values_per_walker):
    """min(40, 62 - ceil(log2(pop_size * values_per_walker))) in exact integer arithmetic."""
    return min(MAX_SHIFT, 62 - (pop_size * values_per_walker - 1).bit_length())


def flavour(p, offset):
    return FLAVOURS[(p + offset) % len(FLAVOURS)]


def logweights(S, P, offset=0, seed=0):
    """float32 [P * S] log-weights with a spread of about 12; population p has flavour (p + offset) % 5: clean, with NaN /
    +inf / -inf entries, all -inf, or one entry 60 above the rest (every other weight then quantises to 0)."""
    rng = np.random.default_rng(7000 + 131 * S + 17 * P + seed)
    a = rng.uniform(-9.0, 3.0, (P, S)).astype(np.float32)
    for p in range(P):
        f = flavour(p, offset)
        if f == "nonfinite":
            a[p, (S // 2) % S] = -np.inf
            a[p, (S // 3) % S] = np.inf
            a[p, 0] = np.nan
            if S > 8:
                a[p, S - 1] = -np.inf
                a[p, S - 2] = np.nan
        elif f == "all_neg_inf":
            a[p] = -np.inf
        elif f == "one_dominant":
            a[p, (2 * S) // 3] = np.float32(a[p].max() + 60.0)
    return a.reshape(-1)


def ref_info(lw, P, S):
    """(m [P] float64, n_bad [P], n_neg_inf [P], bad mask [P, S], relative weights [P, S] float64 with 0 where bad)."""
    a = np.asarray(lw, np.float32).reshape(P, S)
    bad = np.isnan(a) | (a == np.inf)
    ninf = a == -np.inf
    fin = np.isfinite(a)
    m = np.array([a[p][fin[p]].max() if fin[p].any() else 0.0 for p in range(P)], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(bad, 0.0, np.exp(a.astype(np.float64) - m[:, None]))
    return m, bad.sum(1).astype(np.float64), ninf.sum(1).astype(np.float64), bad, w


def ref_histogram(values, lw, P, S, per_walker, edges):
    """numpy.histogram per population on the walkers that are not left out: (counts int64 [P, nb], weighted float64 [P, nb]).
    ``lw`` None = unit weights.

    numpy.histogram(weights=w) over explicit edges takes differences of a running fp64 sum over the SORTED sample: at
    10^5 values of weight up to 1 that running sum loses about sqrt(65 536) ulps of a number in the thousands, some 200
    units of 2^-40 -- far more than the half unit per contribution that the tests bound.  The weights are therefore
    split as w = hi + lo, hi = rint(w * 2^20) * 2^-20: every partial sum of the hi parts is an integer multiple of 2^-20
    below 2^33 and exact in fp64, the lo parts (|lo| <= 2^-21, w - hi is exact) sum to at most a few units whose
    rounding is some 2^-50.  The reference is numpy.histogram(weights=hi) + numpy.histogram(weights=lo), the same
    sum by linearity, with numpy's own rounding orders of magnitude below the bound."""
    v = np.asarray(values, np.float32).reshape(P, S * per_walker)
    if lw is None:
        bad, w = np.zeros((P, S), bool), np.ones((P, S))
    else:
        _, _, _, bad, w = ref_info(lw, P, S)
    nb = len(edges) - 1
    counts, wsum = np.zeros((P, nb), np.int64), np.zeros((P, nb), np.float64)
    for p in range(P):
        keep = np.repeat(~bad[p], per_walker) & np.isfinite(v[p])
        counts[p] = np.histogram(v[p][keep], bins=edges)[0]
        wk = np.repeat(w[p], per_walker)[keep]
        hi = np.rint(wk * 2.0 ** 20) * 2.0 ** -20
        wsum[p] = np.histogram(v[p][keep], bins=edges, weights=hi)[0] + np.histogram(v[p][keep], bins=edges, weights=wk - hi)[0]
    return counts, wsum


def values(S, P, per_walker, seed=0):
    """float32 [P * S * per_walker]: N(2, 1.5) with NaN, +-inf and far-out entries sprinkled in."""
    rng = np.random.default_rng(9000 + 31 * S + 7 * P + per_walker + seed)
    v = rng.normal(2.0, 1.5, P * S * per_walker).astype(np.float32)
    n = v.size
    if n >= 16:
        v[n // 5] = np.nan
        v[n // 4] = np.inf
        v[n // 3] = -np.inf
        v[n // 2] = 1e6
    return v


def edges_for(kind, nbins, v):
    """uniform: numpy's own edges over a range that cuts part of the sample off; nonuniform: sorted random edges.  Some
    values are then moved exactly onto edges by the caller (``on_edges``)."""
    if kind == "uniform":
        e = np.histogram_bin_edges(v[np.isfinite(v)], bins=nbins, range=(-1.0, 4.5)).astype(np.float32)
        assert (np.diff(e) > 0).all()
        return e
    rng = np.random.default_rng(50 + nbins)
    e = np.unique(rng.uniform(-1.0, 4.5, nbins + 1).astype(np.float32))
    assert e.size == nbins + 1
    return e


def on_edges(v, edges):
    """a copy of v with a few entries placed exactly on bin edges (first, last and inner ones)"""
    v = v.copy()
    e = np.asarray(edges, np.float32)
    pick = np.unique(np.concatenate([[0, len(e) - 1], np.arange(0, len(e), max(1, len(e) // 7))]))
    for k, j in enumerate(pick):
        if 2 * k + 1 < v.size:
            v[2 * k + 1] = e[j]
    return v


def coords(n, d, S, P):
    rng = np.random.default_rng(1234 + 1000 * n + 10 * d + S + 7 * P)
    return rng.normal(0.0, 1.0, (P * S, n * d)).astype(np.float32)


@functools.lru_cache(maxsize=4)
def pair_distances(n, d, S, P):
    """The stated arithmetic in numpy float32: delta = x_j - x_i (i < j), s = d0 * d0, s = s + d1 * d1, s = s + d2 * d2,
    r = sqrt(s); numpy rounds every one of these operations on its own and its float32 sqrt is correctly rounded.
    Returns float32 [P * S, n (n - 1) / 2] in numpy.triu_indices order (read-only)."""
    x = coords(n, d, S, P).reshape(P * S, n, d)
    iu = np.triu_indices(n, 1)
    out = np.empty((P * S, iu[0].size), np.float32)
    for lo in range(0, P * S, 64):
        c = x[lo:lo + 64]
        dl = c[:, iu[1]] - c[:, iu[0]]
        s = dl[..., 0] * dl[..., 0]
        for k in range(1, d):
            s = s + dl[..., k] * dl[..., k]
        out[lo:lo + 64] = np.sqrt(s)
    assert out.dtype == np.float32
    out.setflags(write=False)
    return out


def ref_moments(v, lw, P, S):
    """float64 [P, 6] = {m, sum w, sum w v, sum w v^2, n_bad, n_neg_inf} and [P, 3] the sums of |terms| for the bound."""
    v = np.asarray(v, np.float32).reshape(P, S)
    if lw is None:
        a = np.zeros((P, S), np.float32)
    else:
        a = np.asarray(lw, np.float32).reshape(P, S)
    m, _, _, lbad, w = ref_info(a, P, S)
    bad = lbad | ~np.isfinite(v)
    ninf = (a == -np.inf) & ~bad
    v64 = np.where(bad, 0.0, v.astype(np.float64))
    w = np.where(bad, 0.0, w)
    out = np.stack([m, w.sum(1), (w * v64).sum(1), (w * v64 * v64).sum(1), bad.sum(1).astype(float), ninf.sum(1).astype(float)], 1)
    mag = np.stack([w.sum(1), (w * np.abs(v64)).sum(1), (w * v64 * v64).sum(1)], 1)
    return out, mag


def w_1d_weighted_numpy(a, wa, b, wb, p):
    """Quantile merge of two weighted empirical measures in plain numpy loops over the merged grid."""
    ia, ib = np.argsort(a, kind="stable"), np.argsort(b, kind="stable")
    a, wa, b, wb = np.asarray(a, float)[ia], np.asarray(wa, float)[ia], np.asarray(b, float)[ib], np.asarray(wb, float)[ib]
    wa, wb = wa / wa.sum(), wb / wb.sum()
    i = j = 0
    ra, rb, cost = wa[0], wb[0], 0.0  # weight left in the current atom of either side
    while True:
        while ra <= 0 and i < len(a) - 1:
            i += 1
            ra = wa[i]
        while rb <= 0 and j < len(b) - 1:
            j += 1
            rb = wb[j]
        step = min(ra, rb)
        if step <= 0:
            break
        cost += step * abs(a[i] - b[j]) ** p
        ra -= step
        rb -= step
        if (ra <= 1e-18 and i == len(a) - 1) or (rb <= 1e-18 and j == len(b) - 1):
            break
    return cost
