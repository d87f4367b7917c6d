"""Dihedral observables without a GPU: the two entry points bind and refuse bad arguments before any device call, the
topology helpers of pita_amd.metrics, the host-side validation, and the shared references of the GPU tests
(tests/_dihedrals.py) are what they claim to be -- the planted angles, the oracle's sign convention, the reflection."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _dihedrals as DH

NAMES = ("pita_dihedral_angles", "pita_dihedral_histogram2d")


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
    buf = {k: ctypes.create_string_buffer(4096) for k in ("x", "logw", "quads", "ea", "eb", "wsum", "counts", "info", "out")}
    before = {k: v.raw for k, v in buf.items()}
    addr = {k: ctypes.addressof(v) for k, v in buf.items()}

    def angles(B=64, n_atoms=22, n_dih=3, **ptr):
        a = dict(addr, **ptr)
        return L.pita_dihedral_angles(a["x"], B, n_atoms, a["quads"], n_dih, a["out"], None)

    def hist(n_pop=3, pop_size=64, n_atoms=22, n_pair=2, nbins_a=8, nbins_b=6, **ptr):
        a = dict(addr, **ptr)
        return L.pita_dihedral_histogram2d(a["x"], a["logw"], n_pop, pop_size, n_atoms, a["quads"], n_pair, a["ea"], nbins_a,
                                           a["eb"], nbins_b, a["wsum"], a["counts"], a["info"], None)

    def refused(fn, code, **kw):
        assert fn(**kw) == code, (fn.__name__, kw)
        assert built._lib.last_error().startswith("pita_dihedral_" + fn.__name__), (fn.__name__, kw, built._lib.last_error())

    hist.__name__ = "histogram2d"
    for kw in (dict(x=None), dict(quads=None), dict(out=None), dict(B=-1), dict(n_atoms=3), dict(n_atoms=257), dict(n_atoms=-4),
               dict(n_dih=0), dict(n_dih=1025), dict(n_dih=-1)):
        refused(angles, -1, **kw)
    assert angles(B=0) == 0 and angles(B=0, x=None, out=None) == 0  # an empty batch is a no-op
    for kw in (dict(x=None), dict(quads=None), dict(ea=None), dict(eb=None), dict(wsum=None), dict(counts=None), dict(info=None),
               dict(n_pop=0), dict(n_pop=-3), dict(pop_size=0), dict(pop_size=-1), dict(n_atoms=3), dict(n_atoms=257),
               dict(n_pair=0), dict(n_pair=65), dict(nbins_a=0), dict(nbins_b=0), dict(nbins_a=-1), dict(nbins_b=-5)):
        refused(hist, -1, **kw)
    assert hist(logw=None, n_pop=0) == -1  # (a null logw alone is unit weights, not an error)
    # PITA_EUNSUPPORTED: more than 4096 cells, and the message names the limit; a fixed-point shift below 20
    for na, nb in ((4097, 1), (1, 4097), (64, 65), (65, 64), (2 ** 16, 2 ** 16)):
        refused(hist, -2, nbins_a=na, nbins_b=nb)
        assert "4096" in built._lib.last_error()
    refused(hist, -2, pop_size=2 ** 42 + 1)
    refused(hist, -2, n_pop=2 ** 62, pop_size=2 ** 40)
    refused(angles, -2, B=2 ** 62)
    assert all(buf[k].raw == before[k] for k in buf)


def test_phi_psi_and_chirality_quads_on_the_peptide_topologies():
    from pita_amd import metrics

    assert metrics.ALDP_PHI_PSI == ((4, 6, 8, 14), (6, 8, 14, 16))
    for name, n_pair, n_cb in (("ala2", 1, 1), ("ala3", 1, 3), ("ala4", 3, 3)):
        names, res = DH.topology(name)
        quads, residues = metrics.phi_psi_quads(names, res)
        assert quads.shape == (n_pair, 2, 4) and quads.dtype.kind == "i" and len(residues) == n_pair
        for (phi, psi), r in zip(quads.tolist(), residues.tolist()):
            assert [names[i] for i in phi] == ["C", "N", "CA", "C"] and [names[i] for i in psi] == ["N", "CA", "C", "N"]
            assert [res[i] for i in phi] == [r - 1, r, r, r] and [res[i] for i in psi] == [r, r, r, r + 1]
            assert phi[1:] == psi[:3]
        if name == "ala2":
            assert tuple(map(tuple, quads[0].tolist())) == metrics.ALDP_PHI_PSI and residues.tolist() == [1]
        cq, cres = metrics.chirality_quads(names, res)
        assert cq.shape == (n_cb, 4) and len(cres) == n_cb
        for q, r in zip(cq.tolist(), cres.tolist()):
            assert [names[i] for i in q] == ["CA", "N", "C", "CB"] and {res[i] for i in q} == {r}
    q, r = metrics.phi_psi_quads(["N", "CA", "C"], [0, 0, 0])  # no neighbours: nothing, in the documented shapes
    assert q.shape == (0, 2, 4) and r.shape == (0,)
    with pytest.raises(ValueError):
        metrics.phi_psi_quads(["N", "CA"], [0])


def test_fp64_reference_returns_the_planted_angle():
    x = DH.planted()
    got = DH.ref_angles64(x, [(0, 1, 2, 3)])[:, 0]
    assert np.abs(DH.wrap(got - DH.PLANTED_T)).max() <= 1e-12
    t = DH.PLANTED_T
    assert {0.0, np.pi, -np.pi, 0.5 * np.pi, -0.5 * np.pi} <= set(t.tolist())
    assert ((np.pi - np.abs(t) > 0) & (np.pi - np.abs(t) <= 1e-3)).sum() >= 4
    # the float32 restatement on the rounded coordinates stays within a few ulp of pi of it
    got32 = DH.ref_angles32(x.astype(np.float32), [(0, 1, 2, 3)])[:, 0]
    assert got32.dtype == np.float32 and np.abs(DH.wrap(got32.astype(np.float64) - t)).max() <= 4 * DH.ANGLE_FLOOR


def test_the_convention_is_the_oracles():
    """oracle.ff_energy on one torsion with k = 1, n = 1, phase = pi / 2 is 1 + cos(theta - pi / 2) = 1 + sin(theta): that
    pins the sign of theta, which cos alone would not."""
    from oracle import pita_oracle as O

    ff = {"bond_idx": torch.zeros(0, 2, dtype=torch.long), "bond_par": torch.zeros(0, 2, dtype=torch.float64),
          "angle_idx": torch.zeros(0, 3, dtype=torch.long), "angle_par": torch.zeros(0, 2, dtype=torch.float64),
          "tors_idx": torch.tensor([[0, 1, 2, 3]]), "tors_par": torch.tensor([[1.0, 0.5 * np.pi, 1.0]], dtype=torch.float64),
          "charge": torch.zeros(4, dtype=torch.float64), "sigma": torch.zeros(4, dtype=torch.float64),
          "epsilon": torch.zeros(4, dtype=torch.float64), "exc_idx": torch.zeros(0, 2, dtype=torch.long),
          "exc_par": torch.zeros(0, 3, dtype=torch.float64)}
    x = np.concatenate([DH.planted(), np.array(DH.four_atom_walkers(63)["x"], np.float64)])
    theta = DH.ref_angles64(x, [(0, 1, 2, 3)])[:, 0]
    E = O.ff_energy(torch.from_numpy(x), ff).numpy()
    assert np.abs(E - (1.0 + np.sin(theta))).max() <= 1e-12
    assert np.abs(np.sin(theta)).max() > 0.9 and (np.sin(theta) > 0.1).any() and (np.sin(theta) < -0.1).any()


def test_reflection_negates_every_reference_angle():
    for w in (DH.walkers("ala2", 63), DH.walkers("ala4", 63), DH.walkers("four", 63)):
        a = DH.ref_angles64(w["x"], w["quads"])
        assert np.abs(a).min() > 0 and np.array_equal(DH.ref_angles64(DH.reflect(w["x"]), w["quads"]), -a)
        a32 = DH.ref_angles32(w["x"], w["quads"])
        assert np.array_equal(DH.ref_angles32(DH.reflect(w["x"]), w["quads"]), -a32)


def test_shared_walkers_are_well_conditioned_and_seldom_redrawn():
    for name, n, n_pair in (("ala2", 22, 1), ("ala3", 33, 1), ("ala4", 42, 3)):
        w = DH.walkers(name, 2048)
        assert w["n"] == n and w["x"].shape == (2048, 3 * n) and w["x"].dtype == np.float32 and w["pairs"].shape == (n_pair, 2, 4)
        assert w["redrawn"] <= 0.01, (name, w["redrawn"])
        assert DH.well_conditioned(w["x"], w["quads"]).all()
        assert w["quads"][-1].max() == n - 1  # a quad that uses the last atom
        assert np.ptp(w["x"].reshape(2048, n, 3).mean(1), axis=0).min() > 2.0  # translated, not centred
    bad = np.array([[0, 0, 0, 1, 0, 0, 1.001, 0.001, 0, 2, 1, 0]], np.float64)  # atoms 0, 1, 2 nearly collinear
    assert not DH.well_conditioned(bad, [(0, 1, 2, 3)])[0]


def test_bin_rule_restatement_is_numpys():
    rng = np.random.default_rng(3)
    for edges in (np.linspace(-np.pi, np.pi, 65).astype(np.float32), np.unique(rng.uniform(-3, 3, 8).astype(np.float32))):
        v = np.concatenate([rng.uniform(-3.5, 3.5, 2000).astype(np.float32), edges, [np.nan, np.inf, -np.inf]]).astype(np.float32)
        i = DH.bin_of(v, edges)
        keep = i >= 0
        assert np.array_equal(np.bincount(i[keep], minlength=len(edges) - 1), np.histogram(v[np.isfinite(v)], bins=edges)[0])
        assert i[v == edges[-1]].tolist() == [len(edges) - 2] and (i[~np.isfinite(v)] == -1).all()
        assert ((v[~keep] < edges[0]) | (v[~keep] > edges[-1]) | np.isnan(v[~keep])).all()


def test_host_validation_raises_before_any_device_call():
    """CPU tensors throughout: a ValueError from the host checks comes before the device check would refuse them."""
    from pita_amd import metrics

    x = torch.from_numpy(np.array(DH.walkers("ala2", 64)["x"]))
    phi, psi = metrics.ALDP_PHI_PSI
    for fn in (lambda q: metrics.dihedral_angles(x, q), lambda q: metrics.chirality_fraction(x, q)):
        for bad in ((4, 6, 8, 22), (-1, 6, 8, 14), (4, 6, 6, 14), (4, 6, 8, 4)):
            with pytest.raises(ValueError):
                fn([bad])
        with pytest.raises(ValueError):
            fn([(4, 6, 8)])
    for bad in ((phi, (6, 8, 14, 22)), ((4, 4, 8, 14), psi), (phi, (6, 8, 14, -2))):
        with pytest.raises(ValueError):
            metrics.ramachandran_histogram(x, [bad])
    with pytest.raises(ValueError):
        metrics.ramachandran_histogram(x, [phi])  # quads, not pairs of quads
    for P in (3, 0, 128):
        with pytest.raises(ValueError):
            metrics.ramachandran_histogram(x, metrics.ALDP_PHI_PSI, populations=P)
    with pytest.raises(ValueError):
        metrics.ramachandran_histogram(x[:, :65], metrics.ALDP_PHI_PSI)
    with pytest.raises(ValueError):
        metrics.ramachandran_histogram(x, metrics.ALDP_PHI_PSI, edges=np.array([0.0, 1.0, 1.0], np.float32))
    with pytest.raises(built_error()):
        metrics.ramachandran_histogram(x, metrics.ALDP_PHI_PSI)  # valid arguments on the CPU: no fallback


def built_error():
    from pita_amd import _lib

    return _lib.PitaHipError
