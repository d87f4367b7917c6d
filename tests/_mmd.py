"""Shared inputs and numpy references of the mix-RBF MMD tests (tests/test_mmd_cpu.py, tests/test_mmd_gpu.py).  The
reference's mmd.py is not restated in oracle/: the definition in include/pita_hip.h is the specification, and the fp64
reference of it lives here.  Everything is seeded and computed once per shape."""
import functools

import numpy as np

from tests import _observables as OB

SIGMAS = (0.01, 0.1, 1.0, 10.0, 100.0)
FLOOR = 2.0 ** -22  # per-term relative error that cannot average out: two rounded weights, their product, the term
#                     product and a one-ulp exponential, 5 x 2^-24 rounded up to a power of two
MARGIN = 8          # the family's margin for a device exp2 and a different summation order
LOG2E = 1.4426950408889634


def gammas_for(n):
    """n = 5: the default bandwidths; 1: sigma = 1; 16: gamma = 0 and fifteen more over seven decades."""
    if n == 5:
        return [1.0 / (2.0 * s * s) for s in SIGMAS]
    if n == 1:
        return [0.5]
    assert n == 16
    return [0.0] + [float(v) for v in np.logspace(-3.0, 4.0, 15)]


@functools.lru_cache(maxsize=None)
def coords(rows, D, seed=0):
    """float32 [rows, D] (read-only): rows alternate between a tight cluster (pair distances^2 near 1e-3, where gamma =
    5 000 still sees them) and a wide one (near 0.5), both around a centre away from the origin."""
    rng = np.random.default_rng(4242 + 1000 * D + 7 * rows + seed)
    scale = np.where(np.arange(rows) % 2 == 0, 0.02, 0.5)[:, None] / np.sqrt(D)
    x = (0.3 + scale * rng.normal(0.0, 1.0, (rows, D))).astype(np.float32)
    x.setflags(write=False)
    return x


def row_bad(x):
    return ~np.isfinite(np.asarray(x)).all(axis=-1)


def weights64(lw, P, S, cbad=None):
    """fp64 relative weights [P, S] (0 for a row left out) and info [P, 5] = {m, sum w32, sum w32^2, n_bad, n_neg_inf} with
    the sums over the weights rounded to float32 once, as the device uses them.  ``lw`` None = unit weights."""
    a = np.zeros((P, S), np.float32) if lw is None else np.asarray(lw, np.float32).reshape(P, S)
    m, _, _, lbad, w = OB.ref_info(a, P, S)
    bad = lbad if cbad is None else lbad | np.asarray(cbad).reshape(P, S)
    ninf = (a == -np.inf) & ~bad
    w = np.where(bad, 0.0, w)
    w32 = w.astype(np.float32).astype(np.float64)
    info = np.stack([m, w32.sum(1), (w32 * w32).sum(1), bad.sum(1).astype(float), ninf.sum(1).astype(float)], 1)
    return w, info


def _clean(x):
    return np.where(row_bad(x)[:, None], 0.0, np.asarray(x, np.float64))


def oracle_sums(a, w, b, v, gammas):
    """fp64 Gram sums [P, n]: a [P * S, D], w [P, S] fp64 weights (0 = left out), b [M, D], v [M]; differences first.
    ``b`` None: every population against itself."""
    P, S = w.shape
    a64 = _clean(a).reshape(P, S, -1)
    out = np.zeros((P, len(gammas)))
    for p in range(P):
        y, vy = (a64[p], w[p]) if b is None else (_clean(b), np.asarray(v, np.float64))
        for lo in range(0, S, 64):
            d = a64[p, lo:lo + 64, None, :] - y[None, :, :]
            s = (d * d).sum(-1)
            ww = w[p, lo:lo + 64, None] * vy[None, :]
            for g, gam in enumerate(gammas):
                out[p, g] += np.where(ww > 0, ww * np.exp(-gam * s), 0.0).sum()
    return out


def restated_sums(a, w, b, v, gammas):
    """The stated arithmetic in numpy float32, every operation rounded on its own: d = a_k - b_k, s = fmaf(d, d, s) over k
    in index order (the fused step in float64 -- the product of two float32 is exact there -- then rounded to float32: that
    differs from fmaf only on a double-rounding tie), s = min(s, FLT_MAX), ww = w32_i * v32_j, sv = s where ww > 0 else 0,
    e = exp2(c * sv) in float32 with c = float32(-gamma * log2 e), term = ww * e; the terms are summed in float64."""
    P, S = w.shape
    a32 = np.asarray(a, np.float32).reshape(P, S, -1)
    w32 = w.astype(np.float32)
    cs = [np.float32(-g * LOG2E) for g in gammas]
    out = np.zeros((P, len(gammas)))
    fmax = np.float32(np.finfo(np.float32).max)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for p in range(P):
            y, vy = (a32[p], w32[p]) if b is None else (np.asarray(b, np.float32), np.asarray(v, np.float64).astype(np.float32))
            for lo in range(0, S, 64):
                x = a32[p, lo:lo + 64]
                s = np.zeros((x.shape[0], y.shape[0]), np.float32)
                for k in range(x.shape[1]):
                    d = x[:, None, k] - y[None, :, k]
                    assert d.dtype == np.float32
                    s = (s.astype(np.float64) + d.astype(np.float64) * d.astype(np.float64)).astype(np.float32)
                ww = w32[p, lo:lo + 64, None] * vy[None, :]
                sv = np.where(ww > 0, np.fmin(s, fmax), np.float32(0.0))
                for g, c in enumerate(cs):
                    term = ww * np.exp2(c * sv)
                    assert term.dtype == np.float32
                    out[p, g] += term.astype(np.float64).sum()
    return out


def mmd2_from(s_xx, s_xy, s_yy, W, W2, V, V2, biased):
    """mmd2 [P] and its per-bandwidth parts [P, n] from the sums (s_xx, s_xy [P, n], s_yy [n]) and the weight sums."""
    W, W2 = np.asarray(W, np.float64)[:, None], np.asarray(W2, np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        if biased:
            k_xx = np.where(W > 0, s_xx / (W * W), np.nan)
            k_yy = s_yy / (V * V) if V > 0 else np.full_like(s_yy, np.nan)
        else:
            k_xx = np.where(W * W - W2 > 0, (s_xx - W2) / (W * W - W2), np.nan)
            k_yy = (s_yy - V2) / (V * V - V2) if V * V - V2 > 0 else np.full_like(s_yy, np.nan)
        k_xy = np.where(W * V > 0, s_xy / (W * V), np.nan)
    per = k_xx + k_yy[None, :] - 2.0 * k_xy
    return per.sum(1), per


def oracle_mmd2(x, lw, P, y, lv, gammas, biased=True):
    """fp64 mmd2 [P] of x [P * S, D] (log-weights lw or None) against y [M, D] (lv or None), exact double weights."""
    S, M = x.shape[0] // P, y.shape[0]
    w, _ = weights64(lw, P, S, row_bad(x))
    v, _ = weights64(lv, 1, M, row_bad(y))
    s_xx, s_xy = oracle_sums(x, w, None, None, gammas), oracle_sums(x, w, y, v[0], gammas)
    s_yy = oracle_sums(y, v, None, None, gammas)[0]
    return mmd2_from(s_xx, s_xy, s_yy, w.sum(1), (w * w).sum(1), v.sum(), (v * v).sum(), biased)[0]


# (S, M, D, P, n_gamma, flavour offset of a, log-weights on b): the smallest shapes at which the tiling can go wrong --
# one row, one short of and one past a 64-row tile, several tiles with a ragged last one; rows shorter than, equal to and
# longer than the 32-coordinate chunk (39 = 32 + 7, 165 = 5 x 32 + 5).  Every log-weight flavour appears (P = 5 holds all).
CASES = (
    (257, 300, 39, 1, 5, 0, False),
    (257, 300, 3, 3, 5, 1, True),
    (65, 7, 1, 5, 5, 0, True),
    (300, 300, 165, 1, 5, 3, False),
    (257, 257, 66, 1, 5, 0, True),
    (1, 1, 3, 3, 1, 0, False),
    (63, 1, 39, 5, 16, 2, False),
    (1, 300, 165, 1, 16, 0, True),
    (65, 300, 32, 3, 1, 2, False),
    (63, 7, 33, 1, 5, 3, True),
)
# (S, M, D, P, n_gamma, log-weights on b) with unit weights on the samples
UNIT_CASES = ((257, 300, 39, 3, 5, False), (65, 7, 3, 1, 16, True))
# (S, M, D) of the first five cases: tests/test_mmd_cpu.py lists the restatement's own error at these
RESTATEMENT_SHAPES = ((257, 300, 39), (257, 300, 3), (65, 7, 1), (300, 300, 165), (257, 257, 66))


@functools.lru_cache(maxsize=None)
def case(S, M, D, P, n_gamma, offset, b_weighted, unit_a=False):
    """Inputs and references of one accuracy case (computed once, shared): x, lw (None = unit), y, lv, gammas, fp64 weights,
    info, the oracle's cross and self sums, the restatement's, and the normalisers sum w * sum v."""
    x, y = coords(P * S, D), coords(M, D, seed=1)
    lw = None if unit_a else OB.logweights(S, P, offset)
    lv = OB.logweights(M, 1, 0, seed=5) if b_weighted else None
    g = gammas_for(n_gamma)
    w, info_a = weights64(lw, P, S)
    v, info_b = weights64(lv, 1, M)
    out = {"x": x, "lw": lw, "y": y, "lv": lv, "gammas": g, "w": w, "v": v[0], "info_a": info_a, "info_b": info_b[0],
           "cross64": oracle_sums(x, w, y, v[0], g), "self64": oracle_sums(x, w, None, None, g),
           "cross32": restated_sums(x, w, y, v[0], g), "self32": restated_sums(x, w, None, None, g)}
    W, V = w.sum(1)[:, None], v.sum()
    out["norm_cross"], out["norm_self"] = W * V, W * W
    return out


@functools.lru_cache(maxsize=None)
def host_case(P, S=257, M=300, D=39):
    """Inputs of the host-layer test: P populations of CLEAN log-weights each (the unbiased estimator divides by W^2 - W2,
    which is 1e-24 W^2 for the flavour with one dominant walker: no fp32 kernel can serve that), clean weights on the
    test set, the default bandwidths; e32 = the restatement's error over the three Gram sums."""
    x, y = coords(P * S, D), coords(M, D, seed=1)
    lw = np.concatenate([OB.logweights(S, 1, 0, seed=p) for p in range(P)])
    lv = OB.logweights(M, 1, 0, seed=5)
    g = gammas_for(5)
    w, info_a = weights64(lw, P, S)
    v, _ = weights64(lv, 1, M)
    W, V = w.sum(1)[:, None], v.sum()
    e32 = max(normalised_error(restated_sums(x, w, y, v[0], g), oracle_sums(x, w, y, v[0], g), W * V),
              normalised_error(restated_sums(x, w, None, None, g), oracle_sums(x, w, None, None, g), W * W),
              normalised_error(restated_sums(y, v, None, None, g), oracle_sums(y, v, None, None, g), np.array([[V * V]])))
    return {"x": x, "lw": lw, "y": y, "lv": lv, "gammas": g, "w": w, "info_a": info_a, "e32": e32}


def normalised_error(got, ref, norm):
    """max over the populations with a positive normaliser of |got - ref| / (sum w * sum v)"""
    keep = (norm > 0).reshape(-1)
    if not keep.any():
        return 0.0
    return float((np.abs(got - ref)[keep] / norm.reshape(-1, 1)[keep]).max())


def bound(restated_err):
    return max(MARGIN * restated_err, FLOOR)


def duplicates(S, M, D=3):
    """Rows on a lattice of spacing 0.0625 in coordinate 0 (distinct rows are more than 0.05 apart there), then some rows
    copied onto others within a 64-row tile and across tiles; returns x [S, D], y [M, D] (y shares rows with x) and the
    integer numbers of coincident ordered pairs (x, x) and (x, y)."""
    rng = np.random.default_rng(99 + S + M)
    x = rng.normal(0.0, 1.0, (S, D)).astype(np.float32)
    x[:, 0] = 0.0625 * np.arange(S)
    for dst, src in ((1, 0), (5, 0), (S - 1, 3), (S // 2, 3), (min(70, S - 2), 2), (min(130, S - 3), 2)):
        x[dst] = x[src]
    y = rng.normal(0.0, 1.0, (M, D)).astype(np.float32)
    y[:, 0] = -1.0 - 0.0625 * np.arange(M)
    for j in range(0, M, 3):
        y[j] = x[(7 * j) % S]
    eq_xx = int((x[:, None, :] == x[None, :, :]).all(-1).sum())
    eq_xy = int((x[:, None, :] == y[None, :, :]).all(-1).sum())
    return x, y, eq_xx, eq_xy
