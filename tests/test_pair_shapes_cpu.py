"""What tests/test_pair_shapes_gpu.py rests on, checked without a GPU: the closed forms of tests/_pair_shapes.py are
the oracle's (so their sums of magnitudes are sums of the right terms), every seeded input meets the condition it was
built for, and on every case the fp32 oracle -- the same functions on float32 inputs -- stays within a QUARTER of what
the GPU module allows the kernels, in the same per-walker measures: the tolerances leave a factor 4 over what correct
fp32 arithmetic needs on these inputs.  The figures are printed."""
import math

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _pair_shapes as S


def test_case_table_covers_every_shape_and_edge():
    for n, d in S.SHAPES:
        kinds = {c.kind for c in S.CASES if (c.n, c.d) == (n, d)}
        assert {"lj", "dw"} <= kinds, (n, d)
        wb = S.walkers_per_block(n)
        assert {1, wb, wb + 1, 3 * wb + 1} <= set(S.batch_sizes(n)) and (wb == 1 or wb - 1 in S.batch_sizes(n))
    assert {(c.n, c.d) for c in S.CASES if c.kind == "ljs"} == set(S.LJS_SHAPES)
    assert {(c.n, c.d) for c in S.CASES if c.par_name == "nonunit"} == set(S.NONUNIT_SHAPES)
    for n, d, B in S.GRID_STRIDE:  # more blocks than the grid cap: the second trip of the grid-stride loop, ragged
        nblk = -(-B // S.walkers_per_block(n))
        assert S.BLOCK_CAP < nblk < 2 * S.BLOCK_CAP
        assert {c.kind for c in S.CASES if (c.n, c.d, c.batches) == (n, d, (B,))} == {"lj", "dw"}
    assert max(n for n, _ in S.SMALL_SHAPES) == 64 and min(n for n, _ in S.LARGE_SHAPES) == 65


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_inputs_closed_forms_and_fp32_oracle(c):
    """Input condition of the case; closed form with signs = oracle to 1e-12 of the magnitude sums; fp32 oracle within
    TOL / 4 per walker."""
    r = S.reference(c)
    x, B = r["x"], r["x"].shape[0]
    assert x.dtype == torch.float32 and x.shape == (max(c.batches), c.n * c.d)
    mean = x.double().reshape(B, c.n, c.d).mean(dim=1).abs().median()
    assert mean > 0.3, "walkers must not be mean-free"
    dmin = float(S.min_pair_distance(x, c.n, c.d).min())
    if c.kind == "lj":
        assert dmin >= 0.65, dmin
        note = f"min distance {dmin:.3f}"
    elif c.kind == "ljs":
        frac = S.fraction_below_core(x, c.n, c.d)
        assert 0.05 <= frac <= 0.95, frac
        note = f"spacing {S.ljs_spacing(c.n, c.d):.3f}, {100 * frac:.1f} % of pairs below {S.RANGE_MIN}, min distance {dmin:.3f}"
    else:
        assert dmin >= 1e-3, dmin
        note = f"min distance {dmin:.2e}"
    lp, f = S.pair_sums(c.kind, x.double(), c.n, c.d, c.par, False)
    a = float(((lp - r["logp64"]).abs() / r["A"]).max())
    b = float(((f - r["f64"]).norm(dim=1) / r["Af"]).max())
    assert a <= 1e-12 and b <= 1e-12, (a, b)
    assert torch.isfinite(r["logp64"]).all() and torch.isfinite(r["f64"]).all() and (r["A"] > 0).all() and (r["Af"] > 0).all()
    assert (r["A"] >= r["logp64"].abs() * (1 - 1e-12)).all()
    e_lp, e_f = S.walker_errors(r["logp32"], r["f32"], r)
    print(f"[pair shapes cpu {S.case_id(c)}] measure {S.measure_of(c.kind, c.n)}, B {B}, {note}; closed form vs oracle {a:.1e} / {b:.1e}; fp32 oracle, worst "
          f"walker: logp {float(e_lp.max()):.1e}, force {float(e_f.max()):.1e} (allowed {S.TOL / 4:.1e}); "
          f"min |logp|/A {float((r['logp64'].abs() / r['A']).min()):.1e}")
    assert float(e_lp.max()) <= S.TOL / 4 and float(e_f.max()) <= S.TOL / 4


_DESCENTS = [(k, n, d) for n, d in S.DESCENT_SHAPES for k in ("lj", "dw")] + S.DESCENT_GRID_STRIDE


@pytest.mark.parametrize("shape", _DESCENTS, ids=lambda s: "_".join(map(str, s)))
def test_fp32_oracle_descent_within_a_quarter(shape):
    """O.negative_time_descent in fp32 against itself in fp64, deterministic and with injected noise, centring on and
    off, per walker: a quarter of the 1e-5 that
    the GPU module allows the fused descents (the figure of test_fused_descent_equals_per_step)."""
    kind, n, d = shape[:3]
    shape = shape[1:]
    B, steps = (shape[2], 2) if len(shape) == 3 else (3 * S.walkers_per_block(n) + 1, S.DESCENT_STEPS)
    par = S.LJ_PLUGIN if kind == "lj" else S.DW_DEFAULT
    x0, nz = S.descent_inputs(kind, n, d, B, steps)
    for langevin, mean_free in S.DESCENT_CONFIGS:  # the four the GPU module holds to the oracle
        r64 = S.oracle_descent(kind, x0, nz, n, d, par, steps, S.DESCENT_DT, langevin, mean_free)
        r32 = S.oracle_descent(kind, x0, nz, n, d, par, steps, S.DESCENT_DT, langevin, mean_free, torch.float32)
        e = float(S.descent_walker_errors(r32, r64).max())
        print(f"[pair shapes cpu descent {kind} {n}x{d} B {B}] langevin {langevin} mean_free {mean_free}: fp32 oracle "
              f"worst walker {e:.1e} (allowed {S.DESCENT_TOL / 4:.1e})")
        assert torch.isfinite(r64).all() and e <= S.DESCENT_TOL / 4


@pytest.mark.parametrize("dim", S.GMM_DIMS)
@pytest.mark.parametrize("K", S.GMM_KS)
def test_gmm_inputs_and_fp32_oracle(dim, K):
    """Scales unequal per component and per dimension, far rows present, and the fp32 oracle within a quarter of
    test_gmm_golden's elementwise allowances, on the far rows as on the others."""
    x, means, scales, far = S.gmm_inputs(dim, K, max(S.GMM_BS))
    assert means.abs().max() <= 40 and 0.3 <= scales.min() and scales.max() <= 3.0 and int(far.sum()) == S.GMM_FAR_ROWS
    if dim > 1:
        assert (scales[:, 0] != scales[:, 1]).all()
    if K > 1:
        assert scales[:, 0].unique().numel() == K
    assert x[far].abs().min() >= 1000 and x[~far].abs().max() < 60
    for T in S.GMM_TS:
        lp64, g64 = O.gmm_logp_force(x.double(), means.double(), scales.double(), T)
        lp32, g32 = O.gmm_logp_force(x, means, scales, T)
        tol_lp, tol_g = S.gmm_tolerances(lp64, g64)
        a = ((lp32.double() - lp64).abs() / tol_lp)
        b = ((g32.double() - g64).abs() / tol_g).max(dim=1).values
        print(f"[pair shapes cpu gmm dim {dim} K {K} T {T}] fp32 oracle error / allowance, worst row: near logp "
              f"{float(a[~far].max()):.2f} grad {float(b[~far].max()):.2f}, far logp {float(a[far].max()):.2f} grad "
              f"{float(b[far].max()):.2f} (must be <= 0.25)")
        assert torch.isfinite(lp64).all() and torch.isfinite(g64).all()
        assert float(a.max()) <= 0.25 and float(b.max()) <= 0.25


def test_gmm_grid_stride_inputs_and_fp32_oracle():
    dim, K, B = S.GMM_GRID_STRIDE
    assert B > 256 * 4096 and B % 256 != 0
    x, means, scales, far = S.gmm_inputs(dim, K, B)
    lp64, g64 = O.gmm_logp_force(x.double(), means.double(), scales.double(), 1.0)
    lp32, g32 = O.gmm_logp_force(x, means, scales, 1.0)
    tol_lp, tol_g = S.gmm_tolerances(lp64, g64)
    a, b = float(((lp32.double() - lp64).abs() / tol_lp).max()), float(((g32.double() - g64).abs() / tol_g).max())
    print(f"[pair shapes cpu gmm grid-stride] B {B}: fp32 oracle error / allowance logp {a:.2f} grad {b:.2f}")
    assert a <= 0.25 and b <= 0.25


@pytest.mark.parametrize("shape", S.ELEM_SHAPES, ids=str)
def test_elementwise_fp32_reference_within_a_quarter(shape):
    n, d = shape
    B = 3 * (256 // n) + 1
    x, dr, nz = S.elem_inputs(n, d, B)
    for rm in (True, False):
        r64 = S.em_reference(x, dr, nz, n, d, 0.05, 1.7, math.sqrt(0.05), rm)
        r32 = S.em_reference(x, dr, nz, n, d, 0.05, 1.7, math.sqrt(0.05), rm, torch.float32)
        e = float(((r32.double() - r64).abs() / (S.ELEM_ATOL + S.ELEM_RTOL * r64.abs())).max())
        print(f"[pair shapes cpu elementwise {n}x{d}] remove_mean {rm}: fp32 error / allowance {e:.2f}")
        assert e <= 0.25


def test_moment_bounds_are_one_ulp_or_four_times_fp32():
    """The allowance of pita_em_step's four sums at 1030 walkers of 129 x 1: 4 x the error of the same sums accumulated in
    float32, floored at one fp32 ulp, relative to the sums of magnitudes."""
    _, dr, nz = S.elem_inputs(129, 1, 1030)
    s64, m64 = S.moment_sums(dr, nz, 1.7, torch.float64)
    s32, _ = S.moment_sums(dr, nz, 1.7, torch.float32)
    e32 = (s32 - s64).abs() / m64
    bounds = [max(4 * float(e), S.ONE_ULP) for e in e32]
    print("[pair shapes cpu moments] fp32 accumulation error " + ", ".join(f"{float(e):.1e}" for e in e32) +
          " -> bounds " + ", ".join(f"{b:.1e}" for b in bounds))
    assert all(np.isfinite(b) and b < 1e-5 for b in bounds)
