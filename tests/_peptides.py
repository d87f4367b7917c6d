"""Amber-shaped peptide systems for the force-field tests and timing tools (no oracle import here).

Built from residue templates (ACE, ALA, GLY, NME and the charged termini of a zwitterion) and their bond graph:
every angle and every proper dihedral of the graph, propers expanded into 1-4 PeriodicTorsionForce terms, impropers
at the carbonyl carbons and the amide nitrogens, 1-2 / 1-3 exclusions and scaled 1-4 exceptions (amber's 1/1.2 and
1/2), GB-OBC1 radii and scale factors, and a geometry built from the equilibrium bond lengths and angles on an
extended backbone.  Parameters have amber14 magnitudes but are not amber14's (those are outside the reference tree):
the sizes and the shape of the tables are what these systems stand for.
"""
import numpy as np

from tests._synthetic import openmm_system_xml

# atom type -> (element, sigma nm, epsilon kJ/mol, GB radius nm, GB scale)
_TYPES = {"C": ("C", 0.3400, 0.3598, 0.17, 0.72), "CT": ("C", 0.3400, 0.4577, 0.17, 0.72),
          "O": ("O", 0.2960, 0.8786, 0.15, 0.85), "O2": ("O", 0.2960, 0.8786, 0.15, 0.85),
          "N": ("N", 0.3250, 0.7113, 0.155, 0.79), "N3": ("N", 0.3250, 0.7113, 0.155, 0.79),
          "H": ("H", 0.1069, 0.0657, 0.13, 0.85), "H1": ("H", 0.2471, 0.0657, 0.12, 0.85),
          "HC": ("H", 0.2650, 0.0657, 0.12, 0.85), "HP": ("H", 0.1960, 0.0657, 0.12, 0.85)}
# residue templates: atoms (name, type, charge) and the bonds inside the residue; C of one residue bonds N of the next
_RES = {
    "ACE": ([("CH3", "CT", -0.366), ("HH31", "HC", 0.112), ("HH32", "HC", 0.112), ("HH33", "HC", 0.112),
             ("C", "C", 0.597), ("O", "O", -0.568)],
            [("CH3", "HH31"), ("CH3", "HH32"), ("CH3", "HH33"), ("CH3", "C"), ("C", "O")]),
    "ALA": ([("N", "N", -0.416), ("H", "H", 0.272), ("CA", "CT", 0.034), ("HA", "H1", 0.082), ("CB", "CT", -0.183),
             ("HB1", "HC", 0.060), ("HB2", "HC", 0.060), ("HB3", "HC", 0.060), ("C", "C", 0.597), ("O", "O", -0.568)],
            [("N", "H"), ("N", "CA"), ("CA", "HA"), ("CA", "CB"), ("CB", "HB1"), ("CB", "HB2"), ("CB", "HB3"),
             ("CA", "C"), ("C", "O")]),
    "GLY": ([("N", "N", -0.416), ("H", "H", 0.272), ("CA", "CT", -0.025), ("HA2", "H1", 0.070), ("HA3", "H1", 0.070),
             ("C", "C", 0.597), ("O", "O", -0.568)],
            [("N", "H"), ("N", "CA"), ("CA", "HA2"), ("CA", "HA3"), ("CA", "C"), ("C", "O")]),
    "NME": ([("N", "N", -0.416), ("H", "H", 0.272), ("CH3", "CT", -0.149), ("HH31", "H1", 0.098),
             ("HH32", "H1", 0.098), ("HH33", "H1", 0.098)],
            [("N", "H"), ("N", "CH3"), ("CH3", "HH31"), ("CH3", "HH32"), ("CH3", "HH33")]),
    "NALA": ([("N", "N3", 0.141), ("H1", "H", 0.200), ("H2", "H", 0.200), ("H3", "H", 0.200), ("CA", "CT", 0.096),
              ("HA", "HP", 0.089), ("CB", "CT", -0.060), ("HB1", "HC", 0.030), ("HB2", "HC", 0.030), ("HB3", "HC", 0.030),
              ("C", "C", 0.616), ("O", "O", -0.572)],
             [("N", "H1"), ("N", "H2"), ("N", "H3"), ("N", "CA"), ("CA", "HA"), ("CA", "CB"), ("CB", "HB1"), ("CB", "HB2"),
              ("CB", "HB3"), ("CA", "C"), ("C", "O")]),
    "CALA": ([("N", "N", -0.382), ("H", "H", 0.268), ("CA", "CT", -0.175), ("HA", "H1", 0.107), ("CB", "CT", -0.209),
              ("HB1", "HC", 0.076), ("HB2", "HC", 0.076), ("HB3", "HC", 0.076), ("C", "C", 0.772), ("O", "O2", -0.806),
              ("OXT", "O2", -0.806)],
             [("N", "H"), ("N", "CA"), ("CA", "HA"), ("CA", "CB"), ("CB", "HB1"), ("CB", "HB2"), ("CB", "HB3"),
              ("CA", "C"), ("C", "O"), ("C", "OXT")]),
}
SEQUENCES = {
    "ala2": ["ACE", "ALA", "NME"],                                        # alanine dipeptide, 22 atoms
    "ala3": ["NALA", "ALA", "CALA"],                                      # zwitterionic tri-alanine, 33 atoms
    "ala4": ["ACE", "ALA", "ALA", "ALA", "NME"],                          # ACE-(ALA)3-NME, 42 atoms
    "chain64": ["NALA", "ALA", "ALA", "GLY", "GLY", "GLY", "CALA"],       # capacity test, 64 atoms
    # tests/_ff_shapes.py: both sides of every step of the launch plan (walkers per block), up to the first chain refused
    "ace_nme": ["ACE", "NME"],                                            # 12 atoms
    "gly1": ["ACE", "GLY", "NME"],                                        # 19 atoms: 13 walkers = 247 threads
    "chain65": ["NALA"] + 6 * ["GLY"] + ["CALA"],                         # 65 atoms: 3 per block, set by the threads
    "chain73": ["ACE"] + 4 * ["ALA"] + 3 * ["GLY"] + ["NME"],             # 73 atoms: 2 per block, 256 / n gives 3
    "chain85": ["ACE", "ALA"] + 9 * ["GLY"] + ["NME"],                    # 85 atoms: 1 per block, 256 / n gives 3
    "chain86": ["ACE"] + 6 * ["ALA"] + 2 * ["GLY"] + ["NME"],             # 86 atoms: 1 per block, 256 / n gives 2
    "chain89": ["ACE"] + 7 * ["ALA"] + ["GLY", "NME"],                    # 89 atoms: the largest accepted (160 KB of LDS)
    "chain92": ["ACE"] + 8 * ["ALA"] + ["NME"],                           # 92 atoms: refused, 169 104 B
}
# equilibrium bond lengths (nm) and force constants (kJ/mol/nm^2) by element pair
_BOND = {("C", "C"): (0.1522, 2.653e5), ("C", "H"): (0.1090, 2.845e5), ("C", "N"): (0.1335, 4.101e5),
         ("C", "O"): (0.1229, 4.761e5), ("H", "N"): (0.1010, 3.632e5)}


def _topology(seq):
    atoms, bonds, carbonyl_c, amide_n = [], [], [], []
    prev_c = None
    for res in seq:
        names, inner = _RES[res]
        at = {nm: len(atoms) + k for k, (nm, _, _) in enumerate(names)}
        atoms += [(nm, ty, q) for nm, ty, q in names]
        bonds += [(at[a], at[b]) for a, b in inner]
        if prev_c is not None:
            bonds.append((prev_c, at["N"]))
            amide_n.append(at["N"])
        if "C" in at and "O" in at:
            carbonyl_c.append(at["C"])
        prev_c = at.get("C")
    return atoms, bonds, carbonyl_c, amide_n


def _geometry(n, bonds, elem, prio, rng):
    """Cartesian positions (nm) from the bond graph, breadth first: each atom placed from its parent, grandparent and a
    third atom at the equilibrium bond length and angle (109.47 deg at sp3 centres, 120 deg at carbonyl carbons and
    amide nitrogens), siblings 120 (sp3) or 180 (sp2) deg apart round the parent bond, the backbone atom trans (an
    extended chain, omega 180 deg), dihedrals jittered by ~3 deg."""
    nbr = [[] for _ in range(n)]
    for a, b in bonds:
        nbr[a].append(b); nbr[b].append(a)
    sp2 = [len(nbr[i]) == 3 and elem[i] in "CN" for i in range(n)]
    length = lambda i, j: _BOND[tuple(sorted((elem[i], elem[j])))][0]
    pos = np.zeros((n, 3))
    parent = [-1] * n
    a1 = nbr[0][0]
    pos[a1] = [length(0, a1), 0.0, 0.0]
    parent[a1] = 0
    order, placed = [0, a1], {0, a1}
    for p in order:
        kids = sorted((c for c in nbr[p] if c not in placed), key=lambda c: (prio[c], c))
        if not kids:
            continue
        g = parent[p] if parent[p] >= 0 else a1
        ref = pos[parent[g]] if parent[g] >= 0 and parent[g] != p else pos[g] + np.array([0.0, 1.0, 0.3])
        bc = pos[p] - pos[g]; bc /= np.linalg.norm(bc)
        nv = np.cross(pos[g] - ref, bc); nv /= np.linalg.norm(nv)
        m = np.stack([bc, np.cross(nv, bc), nv], 1)
        th = np.radians(120.0 if sp2[p] else 109.47)
        step = np.pi if sp2[p] else 2 * np.pi / 3
        for s, c in enumerate(kids):
            dih = np.pi + s * step + rng.normal(0.0, 0.05)
            r0 = length(c, p)
            pos[c] = pos[p] + m @ np.array([-r0 * np.cos(th), r0 * np.sin(th) * np.cos(dih), r0 * np.sin(th) * np.sin(dih)])
            parent[c] = p
            placed.add(c)
            order.append(c)
    return pos


def peptide(name, seed=0):
    """(tables, positions in nm) of the named system (``SEQUENCES``); tables as ``tests._synthetic.synthetic_peptide``
    plus gb_radius / gb_scale.  Deterministic in ``seed``."""
    return _system(*_topology(SEQUENCES[name]), np.random.default_rng(seed))


def molecule(atoms, bonds, seed=0):
    """(tables, positions in nm) of a hand-written bond graph: ``atoms`` = [(name, type of ``_TYPES``, charge)],
    ``bonds`` = [(i, j)] between elements that ``_BOND`` pairs; geometry and parameters as ``peptide`` sets them (every
    angle and proper of the graph, exclusions and scaled 1-4 pairs, GB by type), no impropers.  Tables without a term
    are empty arrays of the right width."""
    return _system(list(atoms), [tuple(b) for b in bonds], [], [], np.random.default_rng(seed))


def _system(atoms, bonds, carbonyl_c, amide_n, rng):
    n = len(atoms)
    elem = [_TYPES[ty][0] for _, ty, _ in atoms]
    nbr = {i: set() for i in range(n)}
    for a, b in bonds:
        nbr[a].add(b); nbr[b].add(a)
    angles = sorted({(a, j, c) for j in range(n) for a in nbr[j] for c in nbr[j] if a < c})
    propers = sorted({(a, j, k, d) for (j, k) in bonds + [(b, a) for a, b in bonds] if j < k
                      for a in nbr[j] - {k} for d in nbr[k] - {j} if a != d})
    prio = [0 if nm in ("N", "CA", "C", "CH3") else (2 if e == "H" else 1) for (nm, _, _), e in zip(atoms, elem)]
    pos = _geometry(n, bonds, elem, prio, rng)
    # bonded parameters: bonds and angles at the built geometry's lengths / angles (so the geometry is at equilibrium)
    bond_par = [(float(np.linalg.norm(pos[a] - pos[b])), _BOND[tuple(sorted((elem[a], elem[b])))][1]) for a, b in bonds]
    ang = lambda a, j, c: float(np.arccos(np.clip(np.dot(pos[a] - pos[j], pos[c] - pos[j]) /
                                                  (np.linalg.norm(pos[a] - pos[j]) * np.linalg.norm(pos[c] - pos[j])), -1, 1)))
    angle_par = [(ang(a, j, c), 418.4 if "H" in (elem[a], elem[c]) else 527.2 + 100 * rng.random()) for a, j, c in angles]
    # propers: 1-4 PeriodicTorsionForce terms each (more on heavy-atom backbone dihedrals, as amber's phi / psi have),
    # distinct periodicities up to 6, generic phases as well as 0 and pi
    tors_idx, tors_par = [], []
    for q in propers:
        heavy = sum(elem[i] != "H" for i in q)
        n_terms = int(rng.integers(2, 5)) if heavy == 4 else (int(rng.integers(1, 3)) if heavy >= 2 else 1)
        for per in sorted(rng.choice(np.arange(1, 7), n_terms, replace=False)):
            tors_idx.append(q)
            tors_par.append((float(per), float(rng.choice([0.0, np.pi, 0.3, 1.1])), float(rng.uniform(0.3, 8.0))))
    # impropers (amber order: the centre third): carbonyl C (neighbours..., C, O) and amide N (..., N, H), period 2, pi
    for c in carbonyl_c:
        o = next(i for i in nbr[c] if elem[i] == "O")
        others = sorted(nbr[c] - {o})
        tors_idx.append((others[0], others[1], c, o)); tors_par.append((2.0, np.pi, 43.932))
    for nn in amide_n:
        h = next(i for i in nbr[nn] if elem[i] == "H")
        others = sorted(nbr[nn] - {h})
        tors_idx.append((others[0], others[1], nn, h)); tors_par.append((2.0, np.pi, 4.6024))
    t = dict(bond_idx=np.array(bonds), bond_par=np.array(bond_par), angle_idx=np.array(angles, dtype=int).reshape(-1, 3),
             angle_par=np.array(angle_par, dtype=float).reshape(-1, 2), tors_idx=np.array(tors_idx, dtype=int).reshape(-1, 4),
             tors_par=np.array(tors_par, dtype=float).reshape(-1, 3),
             charge=np.array([q for _, _, q in atoms]), sigma=np.array([_TYPES[ty][1] for _, ty, _ in atoms]),
             epsilon=np.array([_TYPES[ty][2] for _, ty, _ in atoms]))
    # exceptions: 1-2 and 1-3 pairs excluded, 1-4 pairs scaled (Coulomb 1/1.2, LJ 1/2)
    exc, par, seen = [], [], set()
    for a, b in bonds:
        seen.add(tuple(sorted((a, b)))); exc.append((a, b)); par.append((0.0, 1.0, 0.0))
    for a, j, c in angles:
        if tuple(sorted((a, c))) not in seen:
            seen.add(tuple(sorted((a, c)))); exc.append((a, c)); par.append((0.0, 1.0, 0.0))
    for a, j, k, d in propers:
        if tuple(sorted((a, d))) not in seen:
            seen.add(tuple(sorted((a, d))))
            exc.append((a, d))
            par.append((t["charge"][a] * t["charge"][d] / 1.2, 0.5 * (t["sigma"][a] + t["sigma"][d]),
                        0.5 * np.sqrt(t["epsilon"][a] * t["epsilon"][d])))
    t["exc_idx"], t["exc_par"] = np.array(exc), np.array(par, dtype=float)
    # GB-OBC1: radii and scale factors by type, stored as the serialized form (offset radius, scaled offset radius) gives
    # them back, so that the XML round trip is exact
    orad = np.array([_TYPES[ty][3] for _, ty, _ in atoms]) - 0.009
    sr = np.array([_TYPES[ty][4] for _, ty, _ in atoms]) * orad
    t["gb_radius"], t["gb_scale"] = orad + 0.009, sr / orad
    return t, pos


def peptide_system_xml(name, seed=0, cutoff=2.0, gb=True):
    """The system of ``peptide(name, seed)`` as a serialized OpenMM System (the layout of
    ``tests._synthetic.openmm_system_xml``)."""
    t, _ = peptide(name, seed)
    return openmm_system_xml(t, cutoff=cutoff, gb=gb)
