"""Shared inputs of the population tests (test_populations_cpu.py, test_populations_gpu.py): P populations of S
log-weights, ``a[p] = float32(SC[p % 4] * default_rng(5000 + 131 * S + p).standard_normal(S))`` with SC = (0, 0.5, 1, 2),
and their float64 numpy statistics.

Margins (numpy, float64, checked by the CPU test): over S in SIZES and p < 300 no ESS fraction lies closer than 1.06e-4
to 0.6 or 0.2, the two intermediate thresholds; the kernel's fp64 sums agree with numpy's to 1e-9 (at most 2 048
non-negative doubles per sum: relative error <= 2048 * 2^-53 ~ 2.3e-13 in any order, three sums in the ESS ratio), so
every decision of every population is asserted.  From S = 63 up each threshold has populations on both sides."""
import functools

import numpy as np

SIZES = (1, 2, 63, 1024, 1025, 2048)
POPS = (1, 3, 40, 300)
SC = (0, 0.5, 1, 2)
THETAS = (1.0, 0.6, 0.2, 0.0)
MAX_S = 2048


@functools.lru_cache(maxsize=None)
def weights(S, p):
    """Population p of S walkers (float32 numpy, read-only)."""
    a = np.float32(SC[p % 4] * np.random.default_rng(5000 + 131 * S + p).standard_normal(S))
    a.setflags(write=False)
    return a


def batch(S, P):
    """[P * S] float32: populations 0 .. P - 1 back to back."""
    return np.concatenate([weights(S, p) for p in range(P)])


def uniforms(P):
    """Per-population uniforms cycling through (0.0, 0.3, 0.999999, p / P)."""
    return np.array([(0.0, 0.3, 0.999999, p / P)[p % 4] for p in range(P)], np.float64)


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


@functools.lru_cache(maxsize=None)
def ref_stats(S, p):
    st = np_stats(weights(S, p))
    st.setflags(write=False)
    return st


def expect_event(st, theta, B):
    return bool(theta >= 1.0 or st[4] > 0 or st[2] <= theta * B)
