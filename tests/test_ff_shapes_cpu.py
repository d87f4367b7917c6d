"""What tests/test_ff_shapes_gpu.py rests on, checked without a GPU: the case table of tests/_ff_shapes.py has the atom
counts, term mixes and launch plans it claims (the plan restated from pita_ff_create's byte accounting at a 163 840-byte
block limit), every base geometry is clash-free, on every case the fp32 oracle -- the same functions and tables in
float32, autograd forces -- stays within a QUARTER of what the GPU module allows the kernels, per walker, and
pita_ff_create refuses bad arguments before any device call.  The figures are printed."""
import numpy as np
import pytest
import torch

from tests import _ff_shapes as S

WPB_CLAIMED = {"co": 128, "ch2": 85, "c2h2": 64, "ch4": 51, "c2h6": 32, "cluster7": 36, "ace_nme": 21, "gly1": 13,
               "chain65": 3, "chain73": 2, "chain85": 1, "chain86": 1, "chain89": 1}


def _plan(system, lds=S.LDS_DEFAULT):
    return S.plan(*S.term_counts(S.base_system(system)[0]), lds)


def test_case_table_atoms_terms_and_plans():
    for name, n in S.N_ATOMS.items():
        t, pos = S.base_system(name)
        assert len(t["charge"]) == n and pos.shape == (n, 3), name
    for name, wpb in WPB_CLAIMED.items():
        assert _plan(name)[2] == wpb, (name, _plan(name))
        assert S.base_case(name) in S.CASES
    n = S.N_ATOMS
    # small systems: the plan is the thread count's; 3 and 5 atoms leave thread 255 without a walker, 19 atoms nine threads
    assert all(WPB_CLAIMED[k] == 256 // n[k] for k in ("co", "ch2", "c2h2", "ch4", "c2h6", "cluster7", "ace_nme", "gly1", "chain65"))
    assert 85 * n["ch2"] == 255 and 51 * n["ch4"] == 255 and 13 * n["gly1"] == 247
    # past 64 atoms the LDS sets it: fewer walkers than 256 / n
    assert [256 // n[k] for k in ("chain73", "chain85", "chain86", "chain89")] == [3, 3, 2, 2]
    assert _plan("ala2")[2] == 11 and 1 <= _plan("chain64")[2] < 4
    blob, walker, wpb = _plan("chain89")
    assert wpb == 1 and 3000 < S.LDS_DEFAULT - (blob + walker) < 5000  # about 4 KB to spare
    blob, walker, wpb = _plan(S.REFUSED)
    assert wpb == 0 and blob + walker == 169104 > S.LDS_DEFAULT
    # term mixes
    cnt = lambda name: S.term_counts(S.base_system(name)[0])[1:4]
    quads = lambda name: len({tuple(q) for q in S.base_system(name)[0]["tors_idx"].tolist()})
    assert cnt("co") == (1, 0, 0) and cnt("ch2") == (2, 1, 0) and cnt("ch4") == (4, 6, 0) and cnt("cluster7") == (0, 0, 0)
    assert cnt("c2h2")[:2] == (3, 2) and quads("c2h2") == 1 and cnt("c2h6")[:2] == (7, 12) and quads("c2h6") == 9
    assert len(S.base_system("cluster7")[0]["exc_idx"]) == 0
    assert len(S.base_system("ch4")[0]["exc_idx"]) == 10  # every pair of CH4 is an exception
    for s in S.VARIANT_SYSTEMS:
        by = {c.variant: S.case_tables(c)[0] for c in S.CASES if c.system == s}
        assert set(by) == {"base"} | {v[0] for v in S.VARIANTS}
        assert "gb_radius" not in by["gb0_all"] and "gb_radius" in by["gb1_all"]
        assert len(by["notors"]["tors_idx"]) == 0 and len(by["notors"]["angle_idx"]) > 0
        assert len(by["noangtors"]["tors_idx"]) == 0 and len(by["noangtors"]["angle_idx"]) == 0
        assert len(by["noexc"]["exc_idx"]) == 0 and len(by["noexc"]["bond_idx"]) > 0
        combos = {(p, ph) for p, ph, _ in by["per0_12"]["tors_par"].tolist()}
        assert combos == {(0.0, 0.3), (0.0, 1.1), (12.0, 0.3), (12.0, 1.1)}
        assert set(by["per0"]["tors_par"][:, 0]) == {0.0} and set(by["per12"]["tors_par"][:, 0]) == {12.0}
        assert set(by["base"]["tors_par"][:, 0]) <= {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}  # the base system is left as it was
    # batch sizes: both sides of a block, a ragged fourth block
    for c in S.CASES:
        wpb = S.case_plan(c)[2]
        bs = S.batch_sizes(wpb)
        assert wpb >= 1 and {1, wpb, wpb + 1, 3 * wpb + 1} <= set(bs) and (wpb == 1 or wpb - 1 in bs) and 0 not in bs
    # the grid-stride cases reach the second trip of the persistent-block loops, ragged
    wpb = _plan(S.GRID_STRIDE_SYSTEM)[2]
    B = S.GRID_CAP * wpb + 3
    assert S.GRID_CAP < -(-B // wpb) < 2 * S.GRID_CAP
    assert set(S.STEP_SYSTEMS) <= set(S.BASE_SYSTEMS) and {S.N_ATOMS[s] for s in S.STEP_SYSTEMS} == {2, 3, 5, 8, 19, 65, 73, 89}


def test_plan_follows_the_lds_limit():
    """The restated plan at other limits: 64 KB (a device without the opt-in) refuses chain64 and keeps ala2; a limit that
    holds everything gives 256 / n."""
    assert _plan("chain64", 65536)[2] == 0 and _plan("ala2", 65536)[2] >= 1
    for name, n in S.N_ATOMS.items():
        assert _plan(name, 1 << 30)[2] == 256 // n
    # without a single bonded term the pair table and one walker's arrays stop fitting at 114 atoms (include/pita_hip.h)
    assert S.plan(113, 0, 0, 0, True, S.LDS_DEFAULT)[2] == 1 and S.plan(114, 0, 0, 0, True, S.LDS_DEFAULT)[2] == 0


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_inputs_and_fp32_oracle(c):
    """No clash in the base geometry; the fp64 oracle finite; the fp32 oracle within a quarter of each tolerance, per walker."""
    t, pos = S.base_system(c.system)
    dmin = S.min_free_distance(t, pos)
    assert dmin >= 0.19, dmin
    r = S.reference(c)
    assert r["xd"].dtype == torch.float32 and r["xd"].shape == (S.ORACLE_WALKERS, 3 * S.N_ATOMS[c.system])
    assert torch.isfinite(r["logp64"]).all() and torch.isfinite(r["f64"]).all() and (r["f64"].norm(dim=1) > 0).all()
    e_lp, e_f = S.walker_errors(r["logp32"], r["f32"], r, torch.arange(S.ORACLE_WALKERS))
    blob, walker, wpb = S.case_plan(c)
    print(f"[ff shapes cpu {S.case_id(c)}] n {S.N_ATOMS[c.system]} terms {S.term_counts(r['tables'])[1:4]} gb {c.gb} cutoff {c.cutoff}; "
          f"plan at {S.LDS_DEFAULT} B: blob {blob} walker {walker} wpb {wpb}; min free distance {dmin:.3f} nm; max |logp| "
          f"{float(r['logp64'].abs().max()):.3g}; fp32 oracle error / allowance, worst walker: logp {float(e_lp.max()):.3f} "
          f"force {float(e_f.max()):.3f} (must be <= 0.25)")
    assert float(e_lp.max()) <= 0.25 and float(e_f.max()) <= 0.25


@pytest.mark.parametrize("system", S.VARIANT_SYSTEMS)
def test_periodicity_cases_tell_a_capped_recurrence(system):
    """If cos / sin(12 phi) were those of 6 phi, every walker of the periodicity-12 cases would leave the logp allowance:
    the cases can fail."""
    for variant in ("per12", "per0_12"):
        c = next(k for k in S.CASES if k.system == system and k.variant == variant)
        r = S.reference(c)
        t = {k: v.copy() for k, v in r["tables"].items()}
        t["tors_par"][:, 0] = np.minimum(t["tors_par"][:, 0], 6.0)
        lp, f = S.oracle_logp_force(r["xd"].double(), S.oracle_tables(t), c.cutoff)
        e_lp, e_f = S.walker_errors(lp, f, r, torch.arange(S.ORACLE_WALKERS))
        print(f"[ff shapes cpu {S.case_id(c)}] periodicity capped at 6: error / allowance, BEST walker: logp "
              f"{float(e_lp.min()):.1f} force {float(e_f.min()):.1f}")
        assert float(e_f.min()) > 10


def _step_batch(system, grid_stride=False):
    c = S.base_case(system)
    wpb = S.case_plan(c)[2]
    return c, wpb, (S.GRID_CAP * wpb + 3 if grid_stride else 3 * wpb + 1)


@pytest.mark.parametrize("system", S.STEP_SYSTEMS)
def test_fp32_oracle_descent_within_a_quarter(system):
    """O.negative_time_descent in fp32 against itself in fp64 on the inputs of the GPU module's descent test,
    deterministic and with injected noise, centring on and off, per walker."""
    c, wpb, B = _step_batch(system)
    x0, nz, _ = S.step_inputs(system, B, S.DESCENT_STEPS)
    rows = S.sample_rows(B, wpb)
    assert len(rows) <= 64
    for langevin in (False, True):
        for mean_free in (True, False):
            r64 = S.oracle_descent(c, x0[rows], nz[:, rows], S.DESCENT_STEPS, S.DESCENT_DT, langevin, mean_free)
            r32 = S.oracle_descent(c, x0[rows], nz[:, rows], S.DESCENT_STEPS, S.DESCENT_DT, langevin, mean_free, torch.float32)
            e = float(((r32.double() - r64).norm(dim=1) / r64.norm(dim=1)).max())
            print(f"[ff shapes cpu descent {system} B {B}] langevin {langevin} mean_free {mean_free}: fp32 oracle worst walker "
                  f"{e:.1e} (allowed {S.DESCENT_RTOL / 4:.1e})")
            assert torch.isfinite(r64).all() and e <= S.DESCENT_RTOL / 4


def test_oracle_mala_accepts_and_rejects():
    """At MALA_DT the fp64 oracle's first step, on the GPU module's draws, accepts and rejects on at least one system;
    the fp32 oracle follows it under the rule the GPU module applies to the kernels."""
    mixed = []
    for system in S.STEP_SYSTEMS:
        c, wpb, B = _step_batch(system)
        x0, nz, uu = S.step_inputs(system, B, S.MALA_STEPS, extra=2)
        rows = S.sample_rows(B, wpb)
        xo, acc, margin, _ = S.oracle_mala_step(c, x0[rows], nz[0][rows], uu[0][rows], S.MALA_DT)
        x32, acc32, _, _ = S.oracle_mala_step(c, x0[rows], nz[0][rows], uu[0][rows], S.MALA_DT, torch.float32)
        same = acc32 == acc
        assert bool((same | (margin.abs() < S.MALA_NEAR)).all())
        e = float((x32.double()[same] - xo[same]).norm() / xo[same].norm())
        print(f"[ff shapes cpu mala {system} B {B}] oracle accepted {int(acc.sum())} of {len(rows)}; fp32 oracle: decisions "
              f"differ on {int((~same).sum())}, rel {e:.1e} (allowed {S.MALA_RTOL / 4:.1e})")
        assert e <= S.MALA_RTOL / 4
        if 0 < int(acc.sum()) < len(rows):
            mixed.append(system)
    assert mixed


# ------------------------------------------------------------------ refusals decided from the arguments alone
def _bad(edit):
    t = {k: v.copy() for k, v in S.base_system("ace_nme")[0].items()}
    edit(t)
    return t


def _set(key, row, col, value):
    def edit(t):
        t[key][row, col] = value
    return edit


def _i_eq_j(t):
    t["exc_idx"][2, 1] = t["exc_idx"][2, 0]


REFUSALS = [
    ("periodicity_13", _set("tors_par", 3, 0, 13.0), "periodicity"),
    ("periodicity_minus_1", _set("tors_par", 0, 0, -1.0), "periodicity"),
    ("periodicity_2.5", _set("tors_par", -1, 0, 2.5), "periodicity"),
    ("exception_i_eq_j", _i_eq_j, "exception with i == j"),
    ("bond_index_12", _set("bond_idx", 1, 0, 12), "atom index out of range"),
    ("torsion_index_minus_1", _set("tors_idx", 5, 3, -1), "atom index out of range"),
    ("exception_index_12", _set("exc_idx", 0, 1, 12), "atom index out of range"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_ff_create_refuses_bad_tables_without_a_device(name, edit, message):
    """PITA_EINVAL (code -1) with a message that names the argument, on the 12-atom chain with one entry spoilt."""
    code, msg = S.raw_create(_bad(edit), 12)
    assert code == -1 and "pita_ff_create" in msg and message in msg, (code, msg)


@pytest.mark.parametrize("n", [1, 257])
def test_ff_create_refuses_atom_counts_without_a_device(n):
    t = S._empty(dict(charge=np.zeros(n), sigma=np.full(n, 0.3), epsilon=np.full(n, 0.1)))
    code, msg = S.raw_create(t, n)
    assert code == -1 and "n_atoms must be in [2,256]" in msg, (code, msg)
