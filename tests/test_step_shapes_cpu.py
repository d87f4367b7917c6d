"""What tests/test_step_shapes_gpu.py rests on, checked without a GPU: the float64 restatements of tests/_step_shapes.py
reproduce the oracle (through a closed-form backbone differentiated by torch.func), every deliberately wrong formula of
pita_fk_assemble is seen by inputs and measure, the float32 restatements behind every bound are printed, the moments'
bound holds for the kernels' own summation order, the quantile inputs meet the conditions the GPU module assumes, the
MALA cases meet the acceptance window and the cap on walkers left out, and the entry points refuse what the header says
they refuse, before any device call."""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _step_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# float64 against float64: the two sides order their operations differently (autograd of E against the assembled
# ((1+c_s) x - D - J^T x)/h, jacrev against closed forms), each rounding relative to the magnitude sums that divide the
# error; a few hundred roundings of 2^-53 at the very most
TIE_BOUND = 512 * S.U64


@pytest.fixture(scope="module")
def pa():
    from pita_amd import build as _b

    _b.build(verbose=False)
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def _say(tag, text):
    print(f"\n[step shapes cpu {tag}] {text}")


def test_tables_hold_the_edges():
    assert {1, 63, 64, 65, 128, 129, 768} <= set(S.ROWS) and {2, 8, 39, 66, 165} <= set(S.ROWS)
    assert set(S.BATCHES) == {1, 3, 4, 5, 9}
    assert len(S.ALL_FLAGS) == 16 and len(S.FK_CASES) == 2 * 16 + 10 * 2
    assert -(-S.GRID_B // 4) > S.WAVE_GRID and S.GRID_B * 65 > S.ELEM_GRID >= S.GRID_B * 2
    assert S.MOMENT_SIZES[-2] > 256 * S.MOMENTS4_GRID and S.MOMENT_SIZES[-1] > 256 * S.MOMENTS_GRID
    assert 4100 > S.ELEM_BLOCK_CAP and (256, 1, 4100) in S.MALA_CASES and 4100 in S.philox_batches(256, 1)
    assert S.GRID_B * 65 > S.ELEM_GRID  # gather_rows' and the edm kernels' second trip
    for B, chunk in S.QUANTILE_SHAPES:
        assert B >= 1 and chunk >= 1
    sizes = {hi - lo for B, chunk in S.QUANTILE_SHAPES for lo, hi in S.chunks(B, chunk)}
    assert {1, 2, 1024, 1025, 2000, 500, 952} <= sizes  # both paths, the threshold, ragged last chunks on either path
    assert [hi - lo > S.RANK_PATH_MAX for lo, hi in S.chunks(2500, 2000)] == [True, False]


# ------------------------------------------------------------------ 1. pita_fk_assemble
@pytest.mark.parametrize("parts", [False, True], ids=["dot_h", "dot_parts"])
@pytest.mark.parametrize("precondition", [False, True], ids=["plain", "precondition_beta"])
@pytest.mark.parametrize("pin", [False, True], ids=["nopin", "pin_energy"])
@pytest.mark.parametrize("D", [2, 8, 39])
def test_fk_restatement_is_the_oracle(D, pin, precondition, parts):
    """fk_restate in float64 on inputs derived by torch.func from a closed-form backbone == oracle f_debiased without the
    clamp: drift_X, drift_A, divergence_score, cross_term, dUt_dt, per walker relative to the magnitude sums."""
    worst = {}
    for t in (0.15, 0.6):
        eb, sb, tt, x = S.tie_case(D, 6, t, 9100 + D)
        a, scal = S.fk_inputs_from_backbones(eb, sb, tt, x, pin, precondition)
        flags = (precondition, precondition, pin, parts)
        got = S.fk_restate(a, flags, torch.float64, **scal)
        # the oracle differentiates E = (1-c_s)/(2h)|x|^2 - ... itself, the form in which |x|^2/h^2-sized terms cancel: its
        # own rounding is relative to the magnitudes of THAT form, which are the dot_h branch's, on either branch
        mag = S.fk_restate(a, flags[:3] + (False,), torch.float64, mag=True, **scal)
        terms = O.f_debiased(sb, eb, S.TIE_SCHED, S.TIE_GAMMA, tt, x, S.TIE_BETA, clamp_quantile=None, pin_energy=pin,
                             target_logp=S.tie_target_logp, precondition_beta=precondition)
        ref = {"drift_X": terms.drift_X, "drift_A": terms.drift_A, "divergence_score": terms.divergence_score,
               "cross_term": terms.cross_term, "dUt_dt": terms.dUt_dt}
        if pin:
            lp = S.tie_target_logp(x)
            assert bool((lp.abs() > 1e3).any()) and bool((lp.abs() < 1e3).any()), "the clamp must act on some walkers only"
        for k, e in S.rel_errors(got, ref, mag).items():
            worst[k] = max(worst.get(k, 0.0), float(S.nan_to_inf(e).max()))
    _say(f"fk tie D{D} pin={pin} precondition={precondition} {'dot_parts' if parts else 'dot_h'}",
         ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f" / {TIE_BOUND:.1e}")
    assert all(v <= TIE_BOUND for v in worst.values()), worst


def test_fk_inputs_make_every_term_visible():
    for D in S.ROWS:
        a = S.fk_inputs(D, 9)
        assert all(v.dtype == torch.float32 for v in a.values())
        assert float(a["h"][0]) == S.f32(S.H_MIN) and float(a["h"][1]) == S.f32(S.H_MAX)
        assert float((a["beta_e"] - a["beta_s"]).abs().min()) > 1e-3
        ratio = a["dhdt"].double() / a["g2"].double()
        assert 1.029 < float(ratio.min()) and float(ratio.max()) < 1.051
        lp = a["logp_target"]
        assert [float(lp[r]) for r in sorted(S.SPECIAL_LOGP)] == [S.SPECIAL_LOGP[r] for r in sorted(S.SPECIAL_LOGP)]
        size = (a["x"].double().pow(2).mean(1) / (1 + a["h"].double())).sqrt()
        assert D < 8 or (0.5 < float(size.min()) and float(size.max()) < 2.0)
    assert S.DGAMMA != 0.0 and 0.0 < S.PIN_W < 1.0 and S.PIN_DW < 0.0
    g = S.fk_inputs(65, S.GRID_B)
    assert float(g["h"].min()) == S.f32(S.H_MIN) and float(g["h"].max()) == S.f32(S.H_MAX)
    lp = g["logp_target"][9:].abs()
    assert bool((lp < 1e3).any()) and bool((lp > 1e3).any())


@pytest.mark.parametrize("c", S.FK_CASES, ids=S.fk_case_id)
def test_fk_float32_restatement_and_bound(c):
    """The yardstick behind every bound of the GPU module, printed; all of it finite, +-inf targets included."""
    D, flags = c
    r = S.fk_reference(D, 9, flags)
    assert all(bool(torch.isfinite(v).all()) for v in r["ref"].values()) and all(bool((v > 0).all()) for v in r["mag"].values())
    for k in S.FK_OUT:
        e = float(r["e32"][k].max())
        assert e <= 2e-6, (k, e)  # a float32 evaluation that is further off would say the measure is not the rounded sum
        assert r["bound"][k] == max(8 * e, 2.0 ** -22)
    _say(f"fk {S.fk_case_id(c)}", "float32 restatement, worst of 9 walkers / bound: " +
         ", ".join(f"{k} {float(r['e32'][k].max()):.1e}/{r['bound'][k]:.1e}" for k in S.FK_OUT))


@pytest.mark.parametrize("D", [2, 39, 65])
@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_fk_mutations_exceed_the_bound(mutation, D):
    """Each wrong formula, applied to the float64 restatement of the standard case (all flags on, B = 9), puts at least
    one walker of at least one output over the bound the GPU module uses; the seven that act on both branches do so
    on the dot_h branch as well."""
    a = S.fk_inputs(D, 9)
    r = S.fk_reference(D, 9, S.FLAGS_ON)
    e = S.rel_errors(S.fk_restate(a, S.FLAGS_ON, torch.float64, mutate=mutation), r["ref"], r["mag"])
    over = {k: float(S.nan_to_inf(v).max()) / r["bound"][k] for k, v in e.items() if not float(S.nan_to_inf(v).max()) <= r["bound"][k]}
    _say(f"fk mutation {mutation} D{D}", "worst walker / bound: " + ", ".join(f"{k} {v:.1e}" for k, v in over.items()))
    assert over, mutation
    if mutation != "parts_h_for_1ph":  # the other seven act on the dot_h branch as well
        fl = (True, True, True, False)
        r = S.fk_reference(D, 9, fl)
        e = S.rel_errors(S.fk_restate(a, fl, torch.float64, mutate=mutation), r["ref"], r["mag"])
        assert any(not float(S.nan_to_inf(v).max()) <= r["bound"][k] for k, v in e.items()), mutation


# ------------------------------------------------------------------ 2. energy_theta, edm_scale_input, edm_combine
@pytest.mark.parametrize("precondition", [False, True], ids=["plain", "precondition_beta"])
@pytest.mark.parametrize("D", [2, 8, 39])
def test_edm_restatement_is_the_oracle(D, precondition):
    worst = {}
    for t in (0.15, 0.6):
        eb, _, tt, x = S.tie_case(D, 6, t, 9300 + D)
        h = S.TIE_SCHED.h(tt * torch.ones(6, dtype=torch.float64))
        beta = torch.full((6,), S.TIE_BETA, dtype=torch.float64)
        c_s, c_in, c_out, c_noise = O.edm_coeffs(h)
        F = eb(c_noise, c_in[:, None] * x, beta)
        bt = beta if precondition else None
        got, mag = S.edm_restate(h, x, F, bt, torch.float64), S.edm_restate(h, x, F, bt, torch.float64, mag=True)
        ref = {"x_scaled": c_in[:, None] * x, "c_noise": c_noise, "D": O.denoiser(eb, h, x, S.TIE_BETA, precondition),
               "score": O.score(eb, h, x, S.TIE_BETA, precondition), "E": O.energy_theta(eb, h, x, S.TIE_BETA, precondition)}
        for k, e in S.rel_errors(got, ref, mag).items():
            worst[k] = max(worst.get(k, 0.0), float(S.nan_to_inf(e).max()))
    _say(f"edm tie D{D} precondition={precondition}", ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f" / {TIE_BOUND:.1e}")
    assert all(v <= TIE_BOUND for v in worst.values()), worst


@pytest.mark.parametrize("with_beta", [False, True], ids=["nobeta", "beta"])
@pytest.mark.parametrize("D", S.ROWS)
def test_edm_float32_restatement_and_bound(D, with_beta):
    r = S.edm_reference(D, 9, with_beta)
    assert all(bool(torch.isfinite(v).all()) for v in r["ref"].values()) and all(bool((v > 0).all()) for v in r["mag"].values())
    for k, e in r["e32"].items():
        assert float(e.max()) <= 2e-6, (k, float(e.max()))
    _say(f"edm D{D} beta={with_beta}", "float32 restatement, worst of 9 walkers / bound: " +
         ", ".join(f"{k} {float(e.max()):.1e}/{r['bound'][k]:.1e}" for k, e in r["e32"].items()))


# ------------------------------------------------------------------ 3. moments
@pytest.mark.parametrize("n", S.MOMENT_SIZES)
def test_moment_bound_holds_for_the_kernels_own_order(n):
    """float64 sums of the test vector in the order of a 256-thread block grid with a wave butterfly and one add per wave
    onto a non-zero start stay within moment_bound(n) of the exact sums: the bound is one of the arithmetic, not of a
    measurement; and the magnitudes span 1e-3 .. 1e3 with both signs."""
    v = S.moment_vectors(n)[0]
    a = v.abs()
    assert v.dtype == torch.float32 and float(a.min()) >= 0.99e-3 and float(a.max()) <= 1.01e3
    assert n < 64 or (float(a.min()) < 1e-2 and float(a.max()) > 1e2 and bool((v > 0).any()) and bool((v < 0).any()))
    terms, mags = S.moment_terms(v, S.OUT0[:2])
    d = v.double().numpy()
    for grid in (S.MOMENTS4_GRID, S.MOMENTS_GRID):
        threads = 256 * min(grid, -(-n // 256))
        pad = np.zeros(-(-n // threads) * threads)
        for j, vals in enumerate((d, d * d)):
            pad[:n] = vals
            per_thread = pad.reshape(-1, threads).sum(0)   # a thread's elements, in order
            waves = per_thread.reshape(-1, 64)
            o = 32
            while o:                                      # lane 0 of the xor butterfly
                waves = waves[:, :o] + waves[:, o:2 * o]
                o //= 2
            got = [0.0, 0.0]
            got[j] = S.OUT0[j]
            for wsum in waves[:, 0]:
                got[j] = got[j] + wsum
            assert S.moment_errors(terms, mags, got)[j] <= S.moment_bound(n), (n, grid, j)


# ------------------------------------------------------------------ 4. quantile clamp
@pytest.mark.parametrize("shape", S.QUANTILE_SHAPES, ids=lambda s: f"{s[0]}_{s[1]}")
def test_quantile_inputs_meet_their_conditions(shape):
    B, chunk = shape
    for kind in S.QUANTILE_KINDS:
        a = S.quantile_input(kind, B, chunk)
        assert a.shape == (B,) and a.dtype == torch.float32 and not bool(torch.isnan(a).any())
        qs = (0.25, 0.5, 0.9) if kind == "inf" else S.QUANTILES
        for q in qs:
            assert bool(torch.isfinite(S.chunk_quantiles(a, B, chunk, q)).all()), (kind, q)
            assert not bool(torch.isnan(S.quantile_reference(a, B, chunk, q)).any())
    inf = S.quantile_input("inf", B, chunk)
    for lo, hi in S.chunks(B, chunk):
        c, n = inf[lo:hi], hi - lo
        assert int((c == float("inf")).sum()) < 0.05 * n and int((c == float("-inf")).sum()) < 0.05 * n
        if n >= 50:
            assert bool((c == float("inf")).any()) and bool((c == float("-inf")).any())
            s = c.sort().values
            for q in (0.25, 0.5, 0.9):  # neither order statistic is infinite
                k = q * (n - 1)
                assert math.isfinite(float(s[math.floor(k)])) and math.isfinite(float(s[math.ceil(k)]))
    if B >= 1024:
        z = S.quantile_input("zeros", B, chunk)
        bits = z.numpy().view(np.uint32)
        assert (bits == 0).any() and (bits == 0x80000000).any() and bool((z > 0).any()) and bool((z < 0).any())
        dn = S.quantile_input("denormal", B, chunk)
        assert bool((dn != 0).any()) and float(dn.abs().max()) < 1.1754944e-38


def test_quantile_last_byte_vector():
    """Every key of the vector shares its upper three bytes; on each path there is a (chunk, q) whose two order
    statistics differ; its closed-form quantile is torch.quantile's within the GPU module's tolerance."""
    straddles = {False: 0, True: 0}
    for B, chunk in S.QUANTILE_SHAPES:
        a = S.quantile_input("lastbyte", B, chunk)
        bits = a.numpy().view(np.uint32)
        assert len(set((bits >> 8).tolist())) == 1
        for lo, hi in S.chunks(B, chunk):
            for q in S.QUANTILES:
                exact, differ = S.lastbyte_exact_quantile(hi - lo, q)
                straddles[hi - lo > S.RANK_PATH_MAX] += bool(differ)
                np.testing.assert_allclose(float(torch.quantile(a[lo:hi], q)), exact, rtol=S.QUANTILE_RTOL, atol=0)
    assert straddles[True] >= 3 and straddles[False] >= 3, straddles


# ------------------------------------------------------------------ 5. gather ids, Philox restatement
def test_gather_ids_and_philox_restatement():
    gen = torch.Generator().manual_seed(5)
    ids = S.gather_ids("resampled", 257, 260, gen)
    assert int((ids[1:] < ids[:-1]).sum()) == 1 and int(ids.min()) >= 0 and int(ids.max()) < 260
    perm = S.gather_ids("permutation", 257, 260, gen)
    assert len(set(perm.tolist())) == 257
    z3, z1 = S.philox_host(5, 7, 3), S.philox_host(5, 7, 1)
    assert z3.shape == (5, 21) and np.array_equal(z3.reshape(5, 7, 3)[:, :, 0], z1)
    # the walker key is the full 64-bit sum, the step's upper word enters the counter: neither is truncated away
    assert not np.array_equal(z1, S.philox_host(5, 7, 1, offset=S.PHILOX_OFFSET & 0xFFFFFFFF))
    assert not np.array_equal(z1, S.philox_host(5, 7, 1, step=S.PHILOX_STEP & 0xFFFFFFFF))
    big = S.philox_host(4000, 13, 3)
    assert abs(big.mean()) < 2e-2 and abs(big.std() - 1) < 2e-2
    import tests.test_hip_parity as P

    assert P._philox_normals_host is S._philox_normals_host  # moved, not copied


# ------------------------------------------------------------------ 6. MALA
@pytest.mark.parametrize("c", S.MALA_CASES, ids=S.mala_case_id)
def test_mala_cases_meet_window_and_cap(c):
    """From the float64 reference alone: 30 - 70 % accepted; at most 2 % of the walkers, and never more than 5, have a
    margin |log u - ratio| below 8 delta32 (delta32: worst error of the float32 restatement's ratio, whose terms are of
    size D/2); an accepted and a rejected walker remain; the restated ratio decides like O.mala_step on every walker
    that is compared."""
    n, d, B = c
    r = S.mala_reference(n, d, B)
    window, cap, both = S.mala_conditions(r)
    keep = ~r["left_out"]
    _say(f"mala {S.mala_case_id(c)}", f"dt {r['dt']}, accepted {int(r['acc'].sum())} of {B}, delta32 {r['delta32']:.1e}, smallest margin "
         f"{float(r['margin'].min()):.1e}, left out {int(r['left_out'].sum())}")
    assert window and cap and both
    assert r["delta32"] <= 1e-6 * max(n * d, 8), "the float32 ratio should be good to a few ulp of D/2"
    assert torch.equal(r["acc"][keep], r["acc_restated"][keep])
    np.testing.assert_allclose(r["x_new"][r["acc"]].numpy(), r["x_prop"][r["acc"]].numpy(), rtol=1e-6, atol=1e-7)


def test_adapt_reference_sides_of_the_threshold():
    up = [(t, a) for t, a in S.ADAPT_CASES if S.adapt_reference(1.0, a, t, True)[0] > 1.0]
    assert set(up) == {(100, 55), (100, 56), (100, 100), (20, 11), (4100, 2255), (4100, 2256), (7, 4)}
    assert float(np.float32(55) / np.float32(100)) > 0.55 and not 55 / 100 > 0.55  # why the count AT the threshold goes up
    assert S.adapt_reference(0.3, 54, 100, False)[0] == 0.3
    assert S.adapt_reference(0.3, 54, 100, True)[0] == 0.3 / 1.1 and S.adapt_reference(0.3, 56, 100, True)[0] == 0.3 * 1.1


# ------------------------------------------------------------------ refusals, before any device call
PTR = 4096  # non-null, aligned, never dereferenced: every call below fails a check or returns before a launch


def _fk(L, B=4, D=3, pin=(0.0, 0.0), logp=None, **null):
    names = ("x", "h", "g2", "dhdt", "D_E", "jtx_E", "dot_h", "dot_parts", "D_S", "trace_S")
    outs = ("drift_X", "drift_A", "div_bt", "cross", "dUdt", "Ut")
    p = lambda k: None if null.get(k) else PTR
    return L.pita_fk_assemble(*[p(k) for k in names], 1.0, 0.0, None, None, pin[0], pin[1], logp, *[p(k) for k in outs], B, D, None)


def test_entry_points_refuse_what_the_header_says(pa):
    L, err = pa._lib.lib(), pa._lib.last_error
    assert _fk(L, B=0) == 0 and _fk(L, B=0, x=True, Ut=True) == 0  # an empty batch launches nothing, reads nothing
    for kw in (dict(B=-1), dict(D=0), dict(D=-3), dict(pin=(0.2, 0.0)), dict(pin=(0.0, -1.0))):
        assert _fk(L, **kw) == -1 and "pita_fk_assemble" in err(), kw
    for k in ("x", "h", "g2", "dhdt", "D_E", "jtx_E", "dot_h", "D_S", "trace_S", "drift_X", "drift_A", "div_bt", "cross", "dUdt", "Ut"):
        assert _fk(L, **{k: True}) == -1 and "null" in err(), k
    for fn, args in ((L.pita_energy_theta, (PTR, PTR, PTR, None, PTR)), (L.pita_edm_scale_input, (PTR, PTR, PTR, PTR)),
                     (L.pita_edm_combine, (PTR, PTR, PTR, None, PTR, PTR))):
        assert fn(*args, 0, 3, None) == 0 and fn(*args, -1, 3, None) == -1 and fn(*args, 4, 0, None) == -1
        assert fn(None, *args[1:], 4, 3, None) == -1
    assert L.pita_edm_combine(PTR, PTR, PTR, None, None, None, 4, 3, None) == -1  # neither output
    assert L.pita_moments(PTR, 5, None, None) == -1 and L.pita_moments(PTR, -1, PTR, None) == -1
    assert L.pita_moments(None, 5, PTR, None) == -1 and L.pita_moments(None, 0, PTR, None) == 0
    assert L.pita_moments4(PTR, PTR, PTR, PTR, 5, None, None) == -1 and L.pita_moments4(PTR, PTR, PTR, PTR, -1, PTR, None) == -1
    assert L.pita_moments4(None, None, None, None, 5, PTR, None) == 0 and L.pita_moments4(PTR, PTR, PTR, PTR, 0, PTR, None) == 0
    assert L.pita_gather_rows(PTR, PTR, PTR, 4, 3, None) == -1 and "in-place" in err()
    assert L.pita_gather_rows(PTR, PTR, 2 * PTR, 0, 3, None) == 0 and L.pita_gather_rows(PTR, PTR, 2 * PTR, 4, 0, None) == -1
    for q, chunk, B in ((-0.1, 4, 8), (1.5, 4, 8), (0.5, 0, 8), (0.5, 4, -1)):
        assert L.pita_quantile_clamp(PTR, B, chunk, q, None) == -1
    assert L.pita_quantile_clamp(None, 0, 4, 0.5, None) == 0
    assert L.pita_mala_adapt(PTR, PTR, 0, 1, None, None) == -1 and L.pita_mala_adapt(None, PTR, 5, 1, None, None) == -1


def test_header_and_integration_state_the_nan_rules():
    hdr = open(os.path.join(ROOT, "include", "pita_hip.h")).read()
    fk = hdr[hdr.index("Feynman-Kac drift assembly per walker"):hdr.index("int pita_fk_assemble(")]
    qc = hdr[hdr.index("/* K11: in place"):hdr.index("int pita_quantile_clamp(")]
    assert re.search(r"NaN logp_target stays NaN", fk) and "drift_A" in fk
    assert "NaN" in qc and "above +inf" in qc and "departure from torch" in qc
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pita_quantile_clamp" in doc and "NaN" in doc[doc.index("pita_quantile_clamp"):][:600]
