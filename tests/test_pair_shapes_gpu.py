"""The general-shape pair-target kernels of pita_amd/csrc/energy_kernels.hip (pair_energy_n3l_kernel for n <= 64,
pair_energy_kernel for 64 < n <= 256, the two fused descents) and gmm_kernel at every dimension, against the fp64 oracle
at a fixed table of edge shapes (tests/_pair_shapes.py): the smallest rings, the antipodal half-pass of even n, idle
lanes and threads, the switch-over at 64 / 65, ragged last blocks, the second trip of the grid-stride loops, the
force == NULL path, position independence, a non-finite walker among finite ones, and the claim that the fused descents
reproduce force kernel + pita_em_step bit for bit.  Every walker of every batch is compared on its own.  What the
tolerances rest on is checked without a GPU in tests/test_pair_shapes_cpu.py.  Run on an MI355X: pytest -m gpu.  The
figures printed here are kept in profiles/pair_shapes_measured.txt."""
import math

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _pair_shapes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def _ok(pa, rc):
    assert rc == 0, (rc, pa._lib.last_error())


def _say(tag, text):
    print(f"\n[pair shapes {tag}] {text}")


# ------------------------------------------------------------------ 1. energy and force
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_logp_force_vs_oracle(pa, c):
    """Per walker: |logp - logp64| <= 2e-5 A and ||f - f64|| <= 2e-5 max(||f64||, A_f) at every batch size of the case;
    at its largest batch also force == NULL, a second call, the batch without its first walker (all bit-equal) and the
    empty batch."""
    ref = S.reference(c)
    xd = ref["x"].cuda()
    worst, bad = [0.0, 0.0, 0, 0], []
    for B in c.batches:
        xb = xd[:B].contiguous()
        rc, lp, f = S.logp_force(pa, c.kind, xb, c.n, c.d, c.par)
        _ok(pa, rc)
        e_lp, e_f = (S.nan_to_inf(e) for e in S.walker_errors(lp, f, ref, B))
        for k, e in enumerate((e_lp, e_f)):
            if float(e.max()) >= worst[k]:
                worst[k], worst[2 + k] = float(e.max()), B
            if not float(e.max()) <= S.TOL:
                bad.append((("logp", "force")[k], B, int(e.argmax()), float(e.max())))
    o_lp, o_f = S.walker_errors(ref["logp32"], ref["f32"], ref)
    _say(S.case_id(c), f"measure {S.measure_of(c.kind, c.n)}, B {','.join(map(str, c.batches))}: worst walker logp {worst[0]:.1e}@B={worst[2]} force "
         f"{worst[1]:.1e}@B={worst[3]} / tolerance {S.TOL:.0e}; fp32 oracle on the same inputs logp {float(o_lp.max()):.1e} "
         f"force {float(o_f.max()):.1e}")
    assert not bad, bad
    B = max(c.batches)
    rc, lp, f = S.logp_force(pa, c.kind, xd, c.n, c.d, c.par)
    _ok(pa, rc)
    rc, lp0, none = S.logp_force(pa, c.kind, xd, c.n, c.d, c.par, want_force=False)
    _ok(pa, rc)
    assert none is None and torch.equal(lp0, lp), "force == NULL changes logp"
    rc, lp2, f2 = S.logp_force(pa, c.kind, xd, c.n, c.d, c.par)
    _ok(pa, rc)
    assert torch.equal(lp2, lp) and torch.equal(f2, f), "second call differs"
    if B > 1:
        rc, lp3, f3 = S.logp_force(pa, c.kind, xd[1:].contiguous(), c.n, c.d, c.par)
        _ok(pa, rc)
        assert torch.equal(lp3, lp[1:]) and torch.equal(f3, f[1:]), "a walker's value depends on its place in the batch"
    rc, lp4, f4 = S.logp_force(pa, c.kind, xd[:0].contiguous(), c.n, c.d, c.par)  # empty batch: PITA_OK, nothing touched
    _ok(pa, rc)
    assert lp4.shape == (0,) and f4.shape == (0, c.n * c.d)
    rc, lp5, f5 = S.logp_force(pa, c.kind, xd, c.n, c.d, c.par, B=0, fill=7.0)  # ... also with live buffers behind it
    _ok(pa, rc)
    assert (lp5 == 7.0).all() and (f5 == 7.0).all()


@pytest.mark.parametrize("kind,n,d", [("lj", 21, 2), ("dw", 21, 2), ("lj", 85, 2), ("dw", 85, 2)])
def test_nan_walker_stays_alone(pa, kind, n, d):
    """One NaN coordinate in a walker that shares its wave with others (21 x 2: three walkers per wave; 85 x 2: walker 1
    spans waves 1 and 2, which also hold walkers 0 and 2): its logp is non-finite, every other walker bit-equal."""
    c = next(c for c in S.CASES if (c.kind, c.n, c.d) == (kind, n, d))
    x = S.reference(c)["x"].cuda()
    B = x.shape[0]
    rc, lp, f = S.logp_force(pa, kind, x, n, d, c.par)
    _ok(pa, rc)
    for w in (1, B - 1):
        xb = x.clone()
        xb[w, (n // 2) * d] = float("nan")
        rc, lpb, fb = S.logp_force(pa, kind, xb, n, d, c.par)
        _ok(pa, rc)
        keep = torch.ones(B, dtype=torch.bool, device="cuda")
        keep[w] = False
        assert not torch.isfinite(lpb[w])
        assert torch.equal(lpb[keep], lp[keep]) and torch.equal(fb[keep], f[keep]), w


# ------------------------------------------------------------------ 2. fused descents
def _descent_configs(nz):
    """(label, noise tensor or None, noise_scale, remove_mean): deterministic, injected noise, Philox; centring on / off."""
    for rm in (1, 0):
        yield f"deterministic rm={rm}", None, 0.0, rm
        yield f"injected rm={rm}", nz, 1.0, rm
        yield f"philox rm={rm}", None, 1.0, rm


def _run_descent_case(pa, kind, n, d, B, steps):
    par = S.LJ_PLUGIN if kind == "lj" else S.DW_DEFAULT
    x0, nz = S.descent_inputs(kind, n, d, B, steps)
    x0d, nzd = x0.cuda(), nz.cuda()
    dt, sq = S.DESCENT_DT, math.sqrt(2 * S.DESCENT_DT)
    seed, off, step0 = 0x5EED1234, 11, 3
    lines = []
    for label, noise, ns, rm in _descent_configs(nzd):
        xf = x0d.clone()
        _ok(pa, S.descent(pa, kind, xf, noise, n, d, par, steps, dt, ns, sq, seed, off, step0, rm))
        xs = S.per_step_descent(pa, kind, x0d.clone(), noise, n, d, par, steps, dt, ns, sq, seed, off, step0, rm)
        same = torch.equal(xf, xs)
        nbad = int((xf != xs).any(dim=1).sum())
        nonfinite = int((~torch.isfinite(xf)).any(dim=1).sum())
        assert nonfinite == 0 and not torch.equal(xf, x0d), f"{label}: {nonfinite} of {B} walkers non-finite"
        assert same, f"{kind} {n}x{d} {label}: fused descent differs from force kernel + pita_em_step in {nbad} of {B} walkers"
        if ns == 0.0 or noise is not None:
            ref = S.oracle_descent(kind, x0, nz, n, d, par, steps, dt, ns != 0.0, bool(rm))
            e = S.nan_to_inf(S.descent_walker_errors(xf, ref))
            lines.append(f"{label} {float(e.max()):.1e}")
            assert float(e.max()) <= S.DESCENT_TOL, (label, int(e.argmax()), float(e.max()))
    _say(f"descent {kind}_{n}x{d}", f"B {B}, {steps} steps: bit-equal to the per-step path in 6 configurations; worst walker "
         f"vs fp64 oracle / {S.DESCENT_TOL:.0e}: " + ", ".join(lines))


@pytest.mark.parametrize("kind", ["lj", "dw"])
@pytest.mark.parametrize("shape", S.DESCENT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fused_descent_bitwise_and_vs_oracle(pa, kind, shape):
    n, d = shape
    _run_descent_case(pa, kind, n, d, 3 * S.walkers_per_block(n) + 1, S.DESCENT_STEPS)


@pytest.mark.parametrize("kind,n,d,B", S.DESCENT_GRID_STRIDE)
def test_fused_descent_grid_stride(pa, kind, n, d, B):
    """More blocks than the 4096-block grid: the second trip of the descent kernels' loops, 2 steps (why the double well
    comes in 2-D: _pair_shapes.DESCENT_GRID_STRIDE)."""
    assert -(-B // S.walkers_per_block(n)) > S.BLOCK_CAP
    _run_descent_case(pa, kind, n, d, B, 2)


def test_descent_through_the_integrator(pa):
    """The path a user takes: WeightedSDEIntegrator.negative_time_descent with MultiDoubleWellEnergy(15, 5, 3), fused
    and per step, Philox and injected noise."""
    e = pa.MultiDoubleWellEnergy(15, 5, 3)
    S_, dt = S.DESCENT_STEPS, S.DESCENT_DT
    x0, nz = S.descent_inputs("dw", 5, 3, 3 * S.walkers_per_block(5) + 1, S_)
    x0d = x0.cuda()
    for langevin in (False, True):
        mk = lambda: pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                              end_resampling_step=1, num_negative_time_steps=S_, dt_negative_time=dt,
                                              do_langevin=langevin, seed=3)
        xf = mk().negative_time_descent(x0d, e, walker_offset=11)
        xs = mk().negative_time_descent(x0d, e, walker_offset=11, fused=False)
        assert torch.equal(xf, xs) and not torch.equal(xf, x0d)
        xf = mk().negative_time_descent(x0d, e, noise=nz.cuda())
        xs = mk().negative_time_descent(x0d, e, noise=nz.cuda(), fused=False)
        assert torch.equal(xf, xs)
        ref = S.oracle_descent("dw", x0, nz, 5, 3, S.DW_DEFAULT, S_, dt, langevin, True)
        err = float(S.descent_walker_errors(xf, ref).max())
        _say("descent integrator dw_5x3", f"langevin {langevin}: worst walker vs fp64 oracle {err:.1e} / {S.DESCENT_TOL:.0e}")
        assert err <= S.DESCENT_TOL


# ------------------------------------------------------------------ 3. the elementwise kernels the descents lean on
@pytest.mark.parametrize("shape", S.ELEM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_elementwise_vs_oracle(pa, shape):
    n, d = shape
    B = 3 * (256 // n) + 1
    x, dr, nz = S.elem_inputs(n, d, B)
    xd, drd, nzd = x.cuda(), dr.cuda(), nz.cuda()
    sq = math.sqrt(0.05)
    close = lambda got, want: np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=S.ELEM_RTOL, atol=S.ELEM_ATOL)
    for rm in (1, 0):
        xc = xd.clone()
        _ok(pa, S.em_step(pa, xc, drd, nzd, n, d, 0.05, 1.7, sq, 0, 0, 0, rm))
        close(xc, S.em_reference(x, dr, nz, n, d, 0.05, 1.7, sq, rm))
    xc = xd.clone()
    _ok(pa, pa._lib.lib().pita_remove_mean(xc.data_ptr(), B, n, d, pa._lib.stream_ptr()))
    close(xc, O.remove_mean(x.double(), n, d))
    for mean_free in (1, 0):
        out = torch.full_like(xd, float("nan"))
        _ok(pa, pa._lib.lib().pita_prior_sample(out.data_ptr(), nzd.data_ptr(), B, n, d, 2.5, 0, 0, mean_free, pa._lib.stream_ptr()))
        close(out, O.prior_from_noise(nz.double(), 2.5, n, d, mean_free=bool(mean_free)))


def test_em_step_moments_past_the_block_cap(pa):
    """stats_out of pita_em_step at 1030 walkers of 129 x 1 (one walker per block, 1024-block grid with moments: six
    blocks take a second walker) against fp64 sums of the same four moments, relative to the sums of magnitudes; bound =
    4 x the error of float32 accumulation on the CPU, floored at one fp32 ulp."""
    n, d, B = 129, 1, 1030
    x, dr, nz = S.elem_inputs(n, d, B)
    s64, m64 = S.moment_sums(dr, nz, 1.7, torch.float64)
    s32, _ = S.moment_sums(dr, nz, 1.7, torch.float32)
    e32 = (s32 - s64).abs() / m64
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    xc = x.cuda()
    _ok(pa, S.em_step(pa, xc, dr.cuda(), nz.cuda(), n, d, 0.05, 1.7, math.sqrt(0.05), 0, 0, 0, 1, stats=stats))
    err = (stats.cpu() - s64).abs() / m64
    bounds = [max(4 * float(e), S.ONE_ULP) for e in e32]
    _say("em_step moments 129x1 B 1030", ", ".join(f"{nm} {float(e):.1e}/{b:.1e} (fp32 accumulation {float(e3):.1e}, ulp {S.ONE_ULP:.1e})"
                                                     for nm, e, b, e3 in zip(("sum_drift", "sum_drift2", "sum_diffusion", "sum_diffusion2"), err, bounds, e32)))
    assert all(float(e) <= b for e, b in zip(err, bounds))
    np.testing.assert_allclose(xc.cpu().numpy(), S.em_reference(x, dr, nz, n, d, 0.05, 1.7, math.sqrt(0.05), 1).numpy(),
                               rtol=S.ELEM_RTOL, atol=S.ELEM_ATOL)


# ------------------------------------------------------------------ 4. GMM
def _gmm_check(pa, tag, x, means, scales, far, T, batches):
    """Worst element's error / allowance as [logp near, grad near, logp far, grad far] over ``batches`` (prefixes of x)."""
    lp64, g64 = O.gmm_logp_force(x.double(), means.double(), scales.double(), T)
    tol_lp, tol_g = S.gmm_tolerances(lp64, g64)
    xd, md, sd = x.cuda(), means.cuda(), scales.cuda()
    worst = [0.0, 0.0, 0.0, 0.0]
    for B in batches:
        xb = xd[:B].contiguous()
        rc, lp, g = S.gmm_call(pa, xb, md, sd, T)
        _ok(pa, rc)
        a = S.nan_to_inf((lp.cpu().double() - lp64[:B]).abs() / tol_lp[:B])
        b = S.nan_to_inf((g.cpu().double() - g64[:B]).abs() / tol_g[:B]).max(dim=1).values
        for k, (e, m) in enumerate(((a, ~far[:B]), (b, ~far[:B]), (a, far[:B]), (b, far[:B]))):
            if bool(m.any()):
                worst[k] = max(worst[k], float(e[m].max()))
        assert float(a.max()) <= 1.0, (tag, T, B, "logp row", int(a.argmax()), bool(far[int(a.argmax())]), float(a.max()))
        assert float(b.max()) <= 1.0, (tag, T, B, "grad row", int(b.argmax()), bool(far[int(b.argmax())]), float(b.max()))
        rc, lp0, none = S.gmm_call(pa, xb, md, sd, T, want_force=False)
        _ok(pa, rc)
        assert none is None and torch.equal(lp0, lp), "force == NULL changes logp"
    return worst


@pytest.mark.parametrize("dim", S.GMM_DIMS)
@pytest.mark.parametrize("K", S.GMM_KS)
def test_gmm_vs_oracle(pa, dim, K):
    """pita_gmm_logp_force at every accepted dimension, K = 1, 2, 40, 257 (the staging loop's second trip), 2048 (with
    dim = 4 the largest accepted table: 73 728 B of dynamic LDS), unequal scales, T = 1 and 2, B = 1, 255, 256, 257, rows
    near the modes and far outside; test_gmm_golden's tolerances elementwise on all of them."""
    x, means, scales, far = S.gmm_inputs(dim, K, max(S.GMM_BS))
    for T in S.GMM_TS:
        w = _gmm_check(pa, f"dim {dim} K {K}", x, means, scales, far, T, S.GMM_BS)
        _say(f"gmm dim{dim}_K{K}_T{T:g}", f"B {','.join(map(str, S.GMM_BS))}: worst element error / allowance near rows logp {w[0]:.2f} "
             f"grad {w[1]:.2f}, far rows logp {w[2]:.2f} grad {w[3]:.2f} (allowance = atol + rtol |ref|: logp {S.GMM_LOGP_ATOL:.0e} + {S.GMM_LOGP_RTOL:.0e}, grad "
             f"{S.GMM_GRAD_ATOL:.0e} + {S.GMM_GRAD_RTOL:.0e})")


def test_gmm_grid_stride(pa):
    dim, K, B = S.GMM_GRID_STRIDE
    x, means, scales, far = S.gmm_inputs(dim, K, B)
    w = _gmm_check(pa, "grid-stride", x, means, scales, far, 1.0, (B,))
    _say(f"gmm grid-stride dim{dim}_K{K}", f"B {B}: worst element error / allowance near rows logp {w[0]:.2f} grad {w[1]:.2f}, "
         f"far rows logp {w[2]:.2f} grad {w[3]:.2f}")


def test_gmm_refuses_what_it_does_not_accept(pa):
    x, means, scales, _ = S.gmm_inputs(2, 4, 16)
    xd, md, sd = x.cuda(), means.cuda(), scales.cuda()
    lp = torch.full((16,), 7.0, device="cuda")
    L, sp = pa._lib.lib(), pa._lib.stream_ptr()
    assert L.pita_gmm_logp_force(xd.data_ptr(), lp.data_ptr(), 0, 16, 5, md.data_ptr(), sd.data_ptr(), 4, 1.0, sp) == -2
    assert L.pita_gmm_logp_force(xd.data_ptr(), lp.data_ptr(), 0, 16, 2, md.data_ptr(), sd.data_ptr(), 2049, 1.0, sp) == -1
    assert L.pita_gmm_logp_force(xd.data_ptr(), lp.data_ptr(), 0, 16, 2, md.data_ptr(), sd.data_ptr(), 0, 1.0, sp) == -1
    assert L.pita_gmm_logp_force(xd.data_ptr(), lp.data_ptr(), 0, 0, 2, md.data_ptr(), sd.data_ptr(), 4, 1.0, sp) == 0
    torch.cuda.synchronize()
    assert (lp == 7.0).all()
