"""Host side of the amber-sized force-field target (no GPU): the generated peptide systems have the term counts of
real amber14 alanine peptides, survive the serialized-System round trip exactly, and pita_ff_create refuses an atom
count beyond one thread per (walker, atom) before it touches a device."""
import numpy as np
import pytest

from tests._peptides import SEQUENCES, peptide, peptide_system_xml

# system -> (atoms, minimum bonds, angles, torsion terms): amber14 ACE-ALA-NME, zwitterionic ALA3, ACE-ALA3-NME
MIN_TERMS = {"ala2": (22, 21, 36, 64), "ala3": (33, 32, 57, 100), "ala4": (42, 41, 72, 130), "chain64": (64, 63, 0, 0),
             **{k: (n, n - 1, 0, 0) for k, n in dict(ace_nme=12, gly1=19, chain65=65, chain73=73, chain85=85, chain86=86,
                                                      chain89=89, chain92=92).items()}}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_generated_peptide_term_counts(name):
    t, pos = peptide(name)
    n, nb, na, nt = MIN_TERMS[name]
    assert len(t["charge"]) == n and pos.shape == (n, 3)
    assert len(t["bond_idx"]) >= nb and len(t["angle_idx"]) >= na and len(t["tors_idx"]) >= nt
    per, phase = t["tors_par"][:, 0], t["tors_par"][:, 1]
    assert per.max() == 6 and set(per) <= {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}
    assert {0.3, 1.1, 0.0, float(np.pi)} <= set(phase)  # generic phases as well as 0 and pi
    # every torsion quadruple is a connected path or an improper round a bonded centre; every index is an atom
    assert t["tors_idx"].min() >= 0 and t["tors_idx"].max() < n and t["exc_idx"].max() < n
    # bonds and angles sit at equilibrium in the generated geometry
    r = np.linalg.norm(pos[t["bond_idx"][:, 0]] - pos[t["bond_idx"][:, 1]], axis=1)
    np.testing.assert_allclose(r, t["bond_par"][:, 0], rtol=1e-12)
    # no two atoms outside the exclusion / 1-4 lists closer than 0.18 nm
    listed = {tuple(sorted(p)) for p in t["exc_idx"].tolist()}
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    free = [d[i, j] for i in range(n) for j in range(i + 1, n) if (i, j) not in listed]
    assert min(free) > 0.18
    # the generator is deterministic
    t2, pos2 = peptide(name)
    assert all(np.array_equal(t[k], t2[k]) for k in t) and np.array_equal(pos, pos2)


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_generated_peptide_system_xml_round_trip(name):
    """tables -> OpenMM-serialized System -> tables_from_openmm_xml gives the same tables bit for bit."""
    from pita_amd.alp_energy import tables_from_openmm_xml

    t, _ = peptide(name)
    tt, opts = tables_from_openmm_xml(peptide_system_xml(name))
    assert opts == {"cutoff": 2.0, "rf_dielectric": 78.3, "gb_solute_dielectric": 1.0, "gb_solvent_dielectric": 78.5}
    assert set(tt) == set(t)
    for k, v in t.items():
        assert np.array_equal(np.asarray(tt[k], dtype=np.float64).reshape(v.shape), v.astype(np.float64)), k


def test_ff_create_rejects_more_atoms_than_threads():
    """n_atoms above 256 (one thread per (walker, atom) in a 256-thread block) is PITA_EINVAL (code -1), decided from
    the arguments alone: no device is needed to get the answer."""
    import pita_amd
    from pita_amd.alp_energy import ForceFieldEnergy

    n = 300
    tabs = dict(bond_idx=np.stack([np.arange(n - 1), np.arange(1, n)], 1), bond_par=np.tile([0.15, 2e5], (n - 1, 1)),
                charge=np.zeros(n), sigma=np.full(n, 0.3), epsilon=np.full(n, 0.1))
    e = ForceFieldEnergy(tabs, n_particles=n, temperature=300.0, device="cpu")
    with pytest.raises(pita_amd._lib.PitaHipError, match=r"code -1\).*n_atoms must be in \[2,256\]"):
        e._native()
