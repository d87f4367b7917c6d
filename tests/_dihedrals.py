"""Shared inputs and numpy references of the dihedral tests (tests/test_dihedrals_cpu.py, tests/test_dihedrals_gpu.py).
Everything is seeded through ``numpy.random.default_rng`` and computed once per shape.

The angle of a quad (i, j, k, l) as pita_hip.h states it:
    b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k;  n1 = b1 x b2, n2 = b2 x b3;
    y = (b1 . n2) * sqrt(b2 . b2), xv = n1 . n2, dots as ((p0 + p1) + p2);  theta = atan2(y, xv)."""
import functools

import numpy as np

from tests import _peptides as PEP

PI32 = np.float32(np.pi)
ANGLE_FLOOR = 4 * 2.0 ** -22  # 4 ulp of pi in float32, 9.5e-7
BOND_ANGLE_RANGE, MIN_B2 = (60.0, 150.0), 0.05  # the well-conditioned walkers of the angle-tolerance tests
PLANTED_T = np.array([0.0, 0.5 * np.pi, -0.5 * np.pi, np.pi, -np.pi, np.pi - 1e-3, -np.pi + 1e-3, np.pi - 5e-4, -np.pi + 5e-4,
                      0.3, -1.1, 2.0, -2.9, 1e-4, -1e-4] + list(np.linspace(-3.0, 3.0, 25)))


def _bonds(x, quads):
    r = x.reshape(x.shape[0], -1, 3)
    q = np.asarray(quads).reshape(-1, 4)
    return (r[:, q[:, 1]] - r[:, q[:, 0]], r[:, q[:, 2]] - r[:, q[:, 1]], r[:, q[:, 3]] - r[:, q[:, 2]])


def ref_angles64(x, quads):
    """fp64 [B, n_dih] from coordinates of any float dtype (taken to fp64 first)."""
    b1, b2, b3 = _bonds(np.asarray(x, np.float64), quads)
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    y = (b1 * n2).sum(-1) * np.sqrt((b2 * b2).sum(-1))
    return np.arctan2(y, (n1 * n2).sum(-1))


def ref_angles32(x, quads):
    """The stated operation order in numpy float32, every operation rounded on its own (numpy's float32 sqrt is
    correctly rounded; its arctan2 is the C library's atan2f); NaN where y or xv is not finite, as documented."""
    b1, b2, b3 = _bonds(np.asarray(x, np.float32), quads)
    assert b1.dtype == np.float32

    def cross(a, b):
        return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)

    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    with np.errstate(invalid="ignore", over="ignore"):
        n1, n2 = cross(b1, b2), cross(b2, b3)
        y = dot(b1, n2) * np.sqrt(dot(b2, b2))
        xv = dot(n1, n2)
        out = np.where(np.isfinite(y) & np.isfinite(xv), np.arctan2(y, xv), np.float32(np.nan))
    assert out.dtype == np.float32
    return out


def wrap(d):
    """a difference of angles on the circle, in (-pi, pi]"""
    d = np.asarray(d, np.float64)
    return -((-d + np.pi) % (2 * np.pi) - np.pi)


def bin_of(v, edges):
    """hist_bin restated without arithmetic: searchsorted(edges, v, 'right') - 1, v == last edge in the last bin, -1 for
    a value outside the edges or a NaN."""
    v, e = np.asarray(v, np.float32), np.asarray(edges, np.float32)
    i = np.searchsorted(e, v, "right") - 1
    i = np.where(v == e[-1], len(e) - 2, i)
    with np.errstate(invalid="ignore"):
        return np.where((v >= e[0]) & (v <= e[-1]), i, -1)


def topology(name):
    """(atom names, residue index per atom) of a ``tests._peptides`` sequence"""
    seq = PEP.SEQUENCES[name]
    names = [nm for nm, _, _ in PEP._topology(seq)[0]]
    res = [r for r, s in enumerate(seq) for _ in PEP._RES[s][0]]
    assert len(names) == len(res)
    return names, res


def last_atom_quad(name):
    """a proper torsion (a bonded chain) that ends at the last atom of the system"""
    t, _ = PEP.peptide(name)
    n = len(t["charge"])
    bonds = {tuple(sorted(b)) for b in t["bond_idx"].tolist()}
    for q in t["tors_idx"].tolist():
        if n - 1 in (q[0], q[3]) and all(tuple(sorted(q[k:k + 2])) in bonds for k in range(3)):
            return tuple(q)
    raise AssertionError(name)


def _rotations(rng, B):
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, b, c, d = q.T
    return np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], -1),
                     np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], -1),
                     np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], -1)], 1)


def conditioned(x, quads):
    """bool [B, n_dih]: the quad's two bond angles inside BOND_ANGLE_RANGE and |b2| >= MIN_B2"""
    b1, b2, b3 = _bonds(np.asarray(x, np.float64), quads)

    def angle(u, v):
        c = (u * v).sum(-1) / (np.linalg.norm(u, axis=-1) * np.linalg.norm(v, axis=-1))
        return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))

    lo, hi = BOND_ANGLE_RANGE
    aj, ak = angle(-b1, b2), angle(-b2, b3)
    return (aj >= lo) & (aj <= hi) & (ak >= lo) & (ak <= hi) & (np.linalg.norm(b2, axis=-1) >= MIN_B2)


def well_conditioned(x, quads):
    """per walker: every quad ``conditioned``"""
    return conditioned(x, quads).all(axis=1)


@functools.lru_cache(maxsize=None)
def peptide_walkers(name, B, seed=0):
    """Walkers round the built geometry of ``peptide(name)``: per-walker Gaussian jitter of 0.01 nm, a random rigid
    rotation and a translation of about 1 nm.  Walkers whose test quads (phi / psi of every residue and the torsion that
    ends at the last atom) are not ``well_conditioned`` are redrawn.  Returns a dict: ``x`` float32 [B, n * 3]
    (read-only), ``n``, ``pairs`` int64 [n_pair, 2, 4], ``quads`` int64 [2 n_pair + 1, 4] and ``redrawn``, the fraction of
    draws that were rejected."""
    _, pos = PEP.peptide(name)
    n = pos.shape[0]
    pairs, _ = phi_psi(name)
    quads = np.concatenate([pairs.reshape(-1, 4), np.array([last_atom_quad(name)])])
    rng = np.random.default_rng(4000 + 13 * n + B + seed)
    x = np.empty((B, n * 3), np.float32)
    todo, drawn = np.arange(B), 0
    while todo.size:
        k = todo.size
        y = pos[None] + rng.normal(0.0, 0.01, (k, n, 3))
        y = np.einsum("bij,bnj->bni", _rotations(rng, k), y) + rng.normal(0.0, 1.0, (k, 1, 3))
        x[todo] = y.reshape(k, -1).astype(np.float32)
        drawn += k
        todo = todo[~well_conditioned(x[todo], quads)]
    x.setflags(write=False)
    return {"x": x, "n": n, "pairs": pairs, "quads": quads, "redrawn": 1.0 - B / drawn}


def phi_psi(name):
    from pita_amd import metrics

    return metrics.phi_psi_quads(*topology(name))


@functools.lru_cache(maxsize=None)
def four_atom_walkers(B, seed=0):
    """Gaussian four-atom walkers (no conditioning: for the tests that compare the library with itself) and three pairs of
    quads over them; the same dict as ``peptide_walkers``."""
    rng = np.random.default_rng(600 + B + seed)
    x = rng.normal(0.0, 1.0, (B, 12)).astype(np.float32)
    x.setflags(write=False)
    pairs = np.array([[(0, 1, 2, 3), (1, 0, 2, 3)], [(3, 0, 1, 2), (0, 2, 1, 3)], [(2, 3, 0, 1), (1, 3, 2, 0)]])
    return {"x": x, "n": 4, "pairs": pairs, "quads": pairs.reshape(-1, 4), "redrawn": 0.0}


def walkers(name, B, seed=0):
    return four_atom_walkers(B, seed) if name == "four" else peptide_walkers(name, B, seed)


def planted(t=PLANTED_T):
    """fp64 [len(t), 12]: p1 = (1, 0, 0), p2 = 0, p3 = (0, 0, 1), p4 = (cos t, sin t, 1), whose dihedral (0, 1, 2, 3) is t"""
    t = np.asarray(t, np.float64)
    x = np.zeros((t.size, 4, 3))
    x[:, 0, 0] = 1.0
    x[:, 2, 2] = 1.0
    x[:, 3] = np.stack([np.cos(t), np.sin(t), np.ones_like(t)], -1)
    return x.reshape(t.size, 12)


def reflect(x):
    """x -> -x in the first coordinate of every atom (exact in any float format)"""
    r = np.array(x).reshape(len(x), -1, 3)
    r[..., 0] = -r[..., 0]
    return r.reshape(np.shape(x))


def ref_histogram2d(angles, pairs_cols, lw, P, S, edges_a, edges_b):
    """From per-walker angles [P * S, n_col] (column pair ``pairs_cols[k]`` = (a, b) of pair k): counts int64 and fp64
    weight sums [P, n_pair, nb_a, nb_b] over the walkers that are not left out, with ``tests._observables.ref_info``'s
    weights (``lw`` None = unit weights)."""
    from tests import _observables as OB

    na, nb = len(edges_a) - 1, len(edges_b) - 1
    if lw is None:
        bad, w = np.zeros((P, S), bool), np.ones((P, S))
    else:
        _, _, _, bad, w = OB.ref_info(lw, P, S)
    counts = np.zeros((P, len(pairs_cols), na, nb), np.int64)
    wsum = np.zeros(counts.shape, np.float64)
    for k, (ca, cb) in enumerate(pairs_cols):
        ia = bin_of(angles[:, ca], edges_a).reshape(P, S)
        ib = bin_of(angles[:, cb], edges_b).reshape(P, S)
        keep = (ia >= 0) & (ib >= 0) & ~bad
        for p in range(P):
            np.add.at(counts[p, k], (ia[p][keep[p]], ib[p][keep[p]]), 1)
            np.add.at(wsum[p, k], (ia[p][keep[p]], ib[p][keep[p]]), w[p][keep[p]])
    return counts, wsum
