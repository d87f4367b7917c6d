"""The small kernels every debiased step passes through, each called directly and compared with a float64 reference at
the shapes where its mapping can go wrong (tests/_step_shapes.py): pita_fk_assemble at all 16 flag combinations, rows
from one lane to 768 components, partial / full / second blocks, the second trip of the grid-stride loop, clamped,
infinite and NaN target log-densities; pita_energy_theta, pita_edm_scale_input and pita_edm_combine on the same tables
with either output absent; pita_moments / pita_moments4 past their grid caps with null slots and the += contract;
pita_quantile_clamp at q = 0 ... 1 on both selection paths, with ties, signed zeros, denormals, infinities and a NaN;
pita_gather_rows; pita_fill_normal against the host Philox restatement and the one-stream claim of the kernels that
draw from it; the three MALA kernels against the oracle's float64 step on a quadratic target.  Every walker of every
batch is compared on its own.  What the bounds and caps rest on is checked without a GPU in
tests/test_step_shapes_cpu.py.  Run on an MI355X: pytest -m gpu.  The figures printed here are kept in
profiles/step_shapes_measured.txt."""
import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _step_shapes as S

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
    print(f"\n[step shapes {tag}] {text}")


def _cuda(a):
    return {k: v.cuda() for k, v in a.items()}


def _worst(errs, B):
    return {k: float(S.nan_to_inf(v[:B]).max()) for k, v in errs.items()}


def _line(worst, e32, bound):
    return ", ".join(f"{k} {worst[k]:.1e} (float32 restatement {float(e32[k].max()):.1e}, bound {bound[k]:.1e})" for k in worst)


# ------------------------------------------------------------------ 1. pita_fk_assemble
def _fk_check(pa, D, flags, rows, batches):
    r = S.fk_reference(D, rows, flags)
    a = _cuda(S.fk_inputs(D, rows))
    worst, bad = {k: 0.0 for k in S.FK_OUT}, []
    for B in batches:
        rc, out = S.fk_call(pa, S.prefix(a, B), flags)
        _ok(pa, rc)
        ref, mag = ({k: v[:B] for k, v in r[w].items()} for w in ("ref", "mag"))
        for k, v in _worst(S.rel_errors(out, ref, mag), B).items():
            worst[k] = max(worst[k], v)
            if not v <= r["bound"][k]:
                bad.append((k, B, v, r["bound"][k]))
    return r, a, worst, bad


@pytest.mark.parametrize("c", S.FK_CASES, ids=S.fk_case_id)
def test_fk_assemble_vs_fp64(pa, c):
    """Every output of every walker at B = 1, 3, 4, 5, 9 within max(8 x float32 restatement, 2^-22) of the float64
    restatement, relative to the magnitude sums; rows 3 .. 8 carry logp_target = +-1e3, +-5e3, +-inf (finite outputs).  At
    the largest batch also: a second call bit-equal, and B = 0 leaves NaN-filled outputs untouched."""
    D, flags = c
    r, a, worst, bad = _fk_check(pa, D, flags, 9, S.BATCHES)
    _say(f"fk {S.fk_case_id(c)}", f"flags {dict(zip(S.FLAG_NAMES, flags))}, B {','.join(map(str, S.BATCHES))}, worst walker: " +
         _line(worst, r["e32"], r["bound"]))
    assert not bad, bad
    rc, o1 = S.fk_call(pa, a, flags)
    _ok(pa, rc)
    assert all(bool(torch.isfinite(v).all()) for v in o1.values())
    rc, o2 = S.fk_call(pa, a, flags)
    _ok(pa, rc)
    assert all(torch.equal(o1[k], o2[k]) for k in S.FK_OUT), "second call differs"
    rc, o0 = S.fk_call(pa, a, flags, B=0)
    _ok(pa, rc)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in o0.values()), "B = 0 wrote something"


@pytest.mark.parametrize("flags", [S.FLAGS_ON, S.FLAGS_OFF], ids=S.flags_id)
@pytest.mark.parametrize("D", S.GRID_ROWS)
def test_fk_assemble_grid_stride(pa, D, flags):
    """4 * 8192 + 5 walkers: five waves take a second walker.  Every walker compared."""
    r, a, worst, bad = _fk_check(pa, D, flags, S.GRID_B, (S.GRID_B,))
    _say(f"fk grid-stride D{D}_{S.flags_id(flags)}", f"B {S.GRID_B}, worst walker: " + _line(worst, r["e32"], r["bound"]))
    assert not bad, bad


@pytest.mark.parametrize("parts", [False, True], ids=["dot_h", "dot_parts"])
@pytest.mark.parametrize("D", S.ALL_FLAG_ROWS)
def test_fk_assemble_nan_target(pa, D, parts):
    """One NaN logp_target among finite ones (walker 1 in the first block, walker 4 opening the second): that walker's Ut,
    dUt_dt and drift_A are NaN, as torch.clamp leaves them; its drift_X, divergence_score and cross_term stay finite and
    within bound; every other walker is bit-equal to the same batch with a finite value there."""
    flags = (True, True, True, parts)
    r = S.fk_reference(D, 9, flags)
    a = _cuda(S.fk_inputs(D, 9))
    rc, base = S.fk_call(pa, a, flags)
    _ok(pa, rc)
    for w in (1, 4):
        b = dict(a, logp_target=a["logp_target"].clone())
        b["logp_target"][w] = float("nan")
        rc, out = S.fk_call(pa, b, flags)
        _ok(pa, rc)
        keep = torch.ones(9, dtype=torch.bool, device="cuda")
        keep[w] = False
        for k in S.FK_OUT:
            assert torch.equal(out[k][keep], base[k][keep]), (k, w, "another walker changed")
        state = {k: float(out[k][w]) for k in ("Ut", "dUt_dt", "drift_A")}
        assert all(np.isnan(v) for v in state.values()), (w, state)
        e = S.rel_errors({k: out[k] for k in ("drift_X", "divergence_score", "cross_term")},
                         {k: r["ref"][k] for k in ("drift_X", "divergence_score", "cross_term")}, r["mag"])
        for k, v in e.items():
            assert bool(torch.isfinite(out[k][w]).all()) and float(v[w]) <= r["bound"][k], (k, w, float(v[w]))


# ------------------------------------------------------------------ 2. energy_theta, edm_scale_input, edm_combine
def _edm_check(pa, D, rows, batches, with_beta):
    r = S.edm_reference(D, rows, with_beta)
    h, x, F, beta = (t.cuda() for t in r["inputs"])
    worst, bad = {k: 0.0 for k in r["ref"]}, []
    for B in batches:
        bt = beta[:B].contiguous() if with_beta else None
        rcs, out = S.edm_call(pa, h[:B].contiguous(), x[:B].contiguous(), F[:B].contiguous(), bt)
        assert rcs == (0, 0, 0), (rcs, pa._lib.last_error())
        ref, mag = ({k: v[:B] for k, v in r[w].items()} for w in ("ref", "mag"))
        for k, v in _worst(S.rel_errors(out, ref, mag), B).items():
            worst[k] = max(worst[k], v)
            if not v <= r["bound"][k]:
                bad.append((k, B, v, r["bound"][k]))
    return r, (h, x, F, beta if with_beta else None), worst, bad


@pytest.mark.parametrize("with_beta", [False, True], ids=["nobeta", "beta"])
@pytest.mark.parametrize("D", S.ROWS)
def test_edm_kernels_vs_fp64(pa, D, with_beta):
    """x_scaled, c_noise (against ln(h)/8), D, score and E per walker at B = 1, 3, 4, 5, 9; pita_edm_combine with D_out
    only and with score_out only gives that output bit-equal to the call with both and leaves the absent one's
    NaN-filled buffer alone; a second call is bit-equal; B = 0 writes nothing."""
    r, (h, x, F, beta), worst, bad = _edm_check(pa, D, 9, S.BATCHES, with_beta)
    _say(f"edm D{D} beta={with_beta}", f"B {','.join(map(str, S.BATCHES))}, worst walker: " + _line(worst, r["e32"], r["bound"]))
    assert not bad, bad
    _, both = S.edm_call(pa, h, x, F, beta)
    for want, absent in ((("D",), "score"), (("score",), "D")):
        rcs, one = S.edm_call(pa, h, x, F, beta, want=want)
        assert rcs == (0, 0, 0)
        assert torch.equal(one[want[0]], both[want[0]]) and bool(torch.isnan(one[absent]).all()), want
    _, again = S.edm_call(pa, h, x, F, beta)
    assert all(torch.equal(both[k], again[k]) for k in both)
    rcs, none = S.edm_call(pa, h, x, F, beta, B=0)
    torch.cuda.synchronize()
    assert rcs == (0, 0, 0) and all(bool(torch.isnan(v).all()) for v in none.values())


@pytest.mark.parametrize("D", S.GRID_ROWS)
def test_edm_kernels_grid_stride(pa, D):
    """4 * 8192 + 5 walkers: the second trip of energy_theta's wave loop, and at D = 65 of the two elementwise kernels'
    8192 x 256-element grid.  Every walker compared, beta given; either output of combine absent."""
    r, (h, x, F, beta), worst, bad = _edm_check(pa, D, S.GRID_B, (S.GRID_B,), True)
    _say(f"edm grid-stride D{D}", f"B {S.GRID_B}, worst walker: " + _line(worst, r["e32"], r["bound"]))
    assert not bad, bad
    _, both = S.edm_call(pa, h, x, F, beta)
    for want, absent in ((("D",), "score"), (("score",), "D")):
        _, one = S.edm_call(pa, h, x, F, beta, want=want)
        assert torch.equal(one[want[0]], both[want[0]]) and bool(torch.isnan(one[absent]).all()), want


# ------------------------------------------------------------------ 3. moments
def _bits(t):
    return t.view(torch.int64)


@pytest.mark.parametrize("n", S.MOMENT_SIZES)
def test_moments_vs_exact_sums(pa, n):
    """out += (sum v, sum v^2) from a non-zero out, within n 2^-53 of the exact sums relative to the sums of magnitudes
    (the kernels accumulate in double; _step_shapes.moment_bound derives the figure); pita_moments4 with all slots, each
    single slot null and only one slot given: the null slots' words bit-unchanged, the given ones within the same bound
    (so within twice it of pita_moments); all slots null or n = 0 write nothing."""
    L, st = pa._lib.lib(), pa._lib.stream_ptr()
    vs = S.moment_vectors(n)
    vd = vs.cuda()
    bound = S.moment_bound(n)
    exact = [S.moment_terms(vs[q], S.OUT0[2 * q:2 * q + 2]) for q in range(4)]
    worst = {"moments": 0.0, "moments4": 0.0}
    single = []
    for q in range(4):
        out = torch.tensor(S.OUT0[2 * q:2 * q + 2], dtype=torch.float64, device="cuda")
        _ok(pa, L.pita_moments(vd[q].data_ptr(), n, out.data_ptr(), st))
        single.append(out.cpu())
        for j, e in enumerate(S.moment_errors(*exact[q], single[q])):
            worst["moments"] = max(worst["moments"], e)
            assert e <= bound, ("pita_moments", q, j, e, bound)
    masks = [(1, 1, 1, 1)] + [tuple(int(k != q) for k in range(4)) for q in range(4)] + [tuple(int(k == q) for k in range(4)) for q in range(4)]
    for mask in masks:
        out = torch.tensor(S.OUT0, dtype=torch.float64, device="cuda")
        before = _bits(out).clone()
        _ok(pa, L.pita_moments4(*[vd[q].data_ptr() if mask[q] else 0 for q in range(4)], n, out.data_ptr(), st))
        got = out.cpu()
        for q in range(4):
            if not mask[q]:
                assert torch.equal(_bits(out)[2 * q:2 * q + 2], before[2 * q:2 * q + 2]), (mask, q, "a null slot was written")
                continue
            for j, e in enumerate(S.moment_errors(*exact[q], got[2 * q:2 * q + 2])):
                worst["moments4"] = max(worst["moments4"], e)
                assert e <= bound, ("pita_moments4", mask, q, j, e, bound)
                assert abs(float(got[2 * q + j]) - float(single[q][j])) <= 2 * bound * exact[q][1][j]
    _say(f"moments n{n}", f"worst of 8 sums / bound n 2^-53: pita_moments {worst['moments']:.1e}/{bound:.1e}, pita_moments4 over "
         f"{len(masks)} slot masks {worst['moments4']:.1e}/{bound:.1e}")
    out = torch.tensor(S.OUT0, dtype=torch.float64, device="cuda")
    before = _bits(out).clone()
    _ok(pa, L.pita_moments4(0, 0, 0, 0, n, out.data_ptr(), st))
    _ok(pa, L.pita_moments4(*[vd[q].data_ptr() for q in range(4)], 0, out.data_ptr(), st))
    _ok(pa, L.pita_moments(vd[0].data_ptr(), 0, out.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), before)
    assert L.pita_moments(vd[0].data_ptr(), n, 0, st) == -1 and L.pita_moments4(vd[0].data_ptr(), 0, 0, 0, n, 0, st) == -1


# ------------------------------------------------------------------ 4. quantile clamp
@pytest.mark.parametrize("kind", S.QUANTILE_KINDS)
@pytest.mark.parametrize("shape", S.QUANTILE_SHAPES, ids=lambda s: f"{s[0]}_{s[1]}")
def test_quantile_clamp_vs_torch(pa, shape, kind):
    """torch.quantile + torch.clamp per chunk on the CPU at test_quantile_clamp_kernel's tolerance, q = 0, 0.25, 0.5,
    0.9, 1 (0.25, 0.5, 0.9 where the input holds infinities: there neither order statistic is infinite, shown in the CPU
    module).  The last-byte vector also against its closed-form quantile at two float32 ulps (one fmaf, or one product
    and one difference, from the exact interpolation)."""
    B, chunk = shape
    a = S.quantile_input(kind, B, chunk)
    for q in ((0.25, 0.5, 0.9) if kind == "inf" else S.QUANTILES):
        rc, got = S.quantile_call(pa, a, chunk, q)
        _ok(pa, rc)
        np.testing.assert_allclose(got.cpu().numpy(), S.quantile_reference(a, B, chunk, q).numpy(), rtol=S.QUANTILE_RTOL,
                                   atol=S.QUANTILE_ATOL, err_msg=f"{kind} q={q}")
        if kind == "lastbyte":
            g = got.cpu().double()
            for lo, hi in S.chunks(B, chunk):
                exact, _ = S.lastbyte_exact_quantile(hi - lo, q)
                want = torch.clamp(a[lo:hi].double(), max=exact)
                assert float((g[lo:hi] - want).abs().max()) <= 2 * S.LASTBYTE_ULP, (q, lo)


def test_quantile_clamp_nan_entry(pa):
    """What the kernel does with a NaN, pinned (a departure from torch, which makes the whole chunk NaN): the entry keeps
    its place and value, sorts above +inf, and the others are clamped by the quantile of that order -- the reference
    computed with +inf in its place.  A chunk whose quantile is NaN stays as it was."""
    gen = torch.Generator().manual_seed(512)
    a = torch.randn(512, generator=gen) * 10
    a[137] = float("nan")
    rc, got = S.quantile_call(pa, a, 512, 0.9)
    _ok(pa, rc)
    b = a.clone()
    b[137] = float("inf")
    want = S.quantile_reference(b, 512, 512, 0.9)
    g = got.cpu()
    assert bool(torch.isnan(g[137])) and int(torch.isnan(g).sum()) == 1
    keep = torch.arange(512) != 137
    np.testing.assert_allclose(g[keep].numpy(), want[keep].numpy(), rtol=S.QUANTILE_RTOL, atol=S.QUANTILE_ATOL)
    assert float(g[keep].max()) < float(a[keep].max()), "the clamp must have acted"
    rc, got = S.quantile_call(pa, a, 512, 1.0)  # the quantile is the NaN itself: chunk unchanged
    _ok(pa, rc)
    assert torch.equal(got.cpu()[keep], a[keep]) and bool(torch.isnan(got.cpu()[137]))


# ------------------------------------------------------------------ 5. gather_rows, fill_normal, one Philox stream
def _gather_case(pa, D, B):
    gen = torch.Generator().manual_seed(31 * D + B)
    src = torch.randn(B + 3, D, generator=gen)
    srcd = src.cuda()
    for kind in S.ID_KINDS:
        ids = S.gather_ids(kind, B, B + 3, gen)
        out = torch.full((B, D), float("nan"), device="cuda")
        _ok(pa, pa._lib.lib().pita_gather_rows(srcd.data_ptr(), ids.cuda().data_ptr(), out.data_ptr(), B, D, pa._lib.stream_ptr()))
        assert torch.equal(out.cpu(), src[ids]), (kind, D, B)
    assert pa._lib.lib().pita_gather_rows(srcd.data_ptr(), ids.cuda().data_ptr(), srcd.data_ptr(), B, D, pa._lib.stream_ptr()) == -1


@pytest.mark.parametrize("D", S.GATHER_ROWS)
def test_gather_rows_exact(pa, D):
    for B in S.GATHER_BATCHES:
        _gather_case(pa, D, B)


def test_gather_rows_grid_stride(pa):
    _gather_case(pa, *S.GATHER_GRID)


@pytest.mark.parametrize("c", S.PHILOX_CASES, ids=lambda c: f"{c[0]}x{c[1]}-B{c[2]}")
def test_fill_normal_vs_host_philox(pa, c):
    """Walker offset and step above 2^32, a ragged last block, and at 256 x 1 x 4100 the second trip of the 4096-block
    grid, at test_philox_matches_host_restatement's tolerance.  The largest case holds three draws whose 24-bit word is
    within 30 of 2^24 (walker 1492, particle 41: 2^24 - 3), where u = (k + 0.5) / 2^24 does not fit float32: before
    philox_normal4 took -2 ln u of its last 64 words from 1 - u, that normal was 4.51e-5 off (3.82396e-4 for 4.27532e-4)."""
    n, d, B = c
    rc, out = S.fill_normal(pa, B, n, d)
    _ok(pa, rc)
    want = S.philox_host(B, n, d)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)
    i = np.unravel_index(int(err.argmax()), err.shape)
    _say(f"fill_normal {n}x{d}-B{B}", f"worst element |error| {err.max():.2e} at walker {i[0]}, component {i[1]} (value {want[i]:.5e}), "
         f"elements over atol {S.PHILOX_ATOL:.0e} + rtol {S.PHILOX_RTOL:.0e} |value|: {int((err > S.PHILOX_ATOL + S.PHILOX_RTOL * np.abs(want)).sum())} of {err.size}")
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=S.PHILOX_ATOL, rtol=S.PHILOX_RTOL)


@pytest.mark.parametrize("shape", S.PHILOX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_philox_stream_everywhere(pa, shape):
    """pita_em_step, pita_prior_sample (step -1) and pita_mala_propose with noise = NULL are bit-equal to the same call
    fed pita_fill_normal's output for that (seed, offset, step); pita_mala_propose keyed by walker_ids equals the call
    keyed by the matching offset."""
    n, d = shape
    L, lib = pa._lib.lib(), pa._lib
    st = lib.stream_ptr()
    seed, off, step = S.PHILOX_SEED, S.PHILOX_OFFSET, S.PHILOX_STEP
    for B in S.philox_batches(n, d):
        gen = torch.Generator().manual_seed(17 * n + d)
        x0, dr = (torch.randn(B, n * d, generator=gen).cuda() for _ in range(2))
        rc, nz = S.fill_normal(pa, B, n, d)
        _ok(pa, rc)
        for rm in (0, 1):
            xa, xb = x0.clone(), x0.clone()
            _ok(pa, L.pita_em_step(xa.data_ptr(), dr.data_ptr(), 0, B, n, d, 0.05, 1.7, 0.05 ** 0.5, seed, off, step, rm, 0, st))
            _ok(pa, L.pita_em_step(xb.data_ptr(), dr.data_ptr(), nz.data_ptr(), B, n, d, 0.05, 1.7, 0.05 ** 0.5, 0, 0, 0, rm, 0, st))
            assert torch.equal(xa, xb) and not torch.equal(xa, x0), ("em_step", rm)
        rc, nzp = S.fill_normal(pa, B, n, d, step=-1)
        _ok(pa, rc)
        for mf in (0, 1):
            xa, xb = torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            _ok(pa, L.pita_prior_sample(xa.data_ptr(), 0, B, n, d, 2.5, seed, off, mf, st))
            _ok(pa, L.pita_prior_sample(xb.data_ptr(), nzp.data_ptr(), B, n, d, 2.5, 0, 0, mf, st))
            assert torch.equal(xa, xb) and bool(torch.isfinite(xa).all()), ("prior_sample", mf)
        dt = torch.tensor([0.3], dtype=torch.float64, device="cuda")
        ids = (torch.arange(B, dtype=torch.int64) + off).cuda()
        props = [torch.full_like(x0, float("nan")) for _ in range(3)]
        _ok(pa, L.pita_mala_propose(x0.data_ptr(), dr.data_ptr(), props[0].data_ptr(), 0, B, n, d, dt.data_ptr(), seed, off, 0, step, st))
        _ok(pa, L.pita_mala_propose(x0.data_ptr(), dr.data_ptr(), props[1].data_ptr(), nz.data_ptr(), B, n, d, dt.data_ptr(), 0, 0, 0, 0, st))
        _ok(pa, L.pita_mala_propose(x0.data_ptr(), dr.data_ptr(), props[2].data_ptr(), 0, B, n, d, dt.data_ptr(), seed, 77, ids.data_ptr(), step, st))
        assert torch.equal(props[0], props[1]) and torch.equal(props[0], props[2]) and bool(torch.isfinite(props[0]).all())


# ------------------------------------------------------------------ 6. MALA against the float64 step
@pytest.mark.parametrize("remove_mean", [0, 1], ids=["keep_mean", "remove_mean"])
@pytest.mark.parametrize("c", S.MALA_CASES, ids=S.mala_case_id)
def test_mala_kernels_vs_fp64(pa, c, remove_mean):
    """pita_mala_propose and pita_mala_accept with recorded noise and uniforms on log p = -k |x|^2 / 2 against
    O.mala_step in float64 on the float32 inputs: x_prop elementwise; the decision of every walker whose float64 margin
    |log u - ratio| is at least 8 delta32 (the CPU module caps how many are not); every walker, compared or not, equal
    to one of its two possible outcomes (old row or proposal, mean removed when asked) with the matching logp; acc_count
    = the rows that moved."""
    n, d, B = c
    L, st = pa._lib.lib(), pa._lib.stream_ptr()
    r = S.mala_reference(n, d, B)
    x, nz, u = r["x"].cuda(), r["noise"].cuda(), r["u"].cuda()
    lp64, F64 = S.quad_logp_force(r["x"].double())
    lp, F = lp64.float().cuda(), F64.float().cuda()
    dt = torch.tensor([r["dt"]], dtype=torch.float64, device="cuda")
    xp = torch.full_like(x, float("nan"))
    _ok(pa, L.pita_mala_propose(x.data_ptr(), F.data_ptr(), xp.data_ptr(), nz.data_ptr(), B, n, d, dt.data_ptr(), 0, 0, 0, 0, st))
    np.testing.assert_allclose(xp.cpu().numpy(), r["x_prop"].numpy(), rtol=S.ELEM_RTOL, atol=S.ELEM_ATOL)
    lpp64, Fp64 = S.quad_logp_force(xp.cpu().double())  # the target at the DEVICE's proposal, in float64, rounded once
    lpp, Fp = lpp64.float().cuda(), Fp64.float().cuda()
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    xc, lpc = x.clone(), lp.clone()
    _ok(pa, L.pita_mala_accept(xc.data_ptr(), lpc.data_ptr(), F.data_ptr(), xp.data_ptr(), lpp.data_ptr(), Fp.data_ptr(),
                               u.data_ptr(), B, n, d, dt.data_ptr(), 0, 0, 0, 0, remove_mean, count.data_ptr(), st))
    rm = (lambda t: O.remove_mean(t, n, d)) if remove_mean else (lambda t: t)
    stay, move = rm(r["x"].double()), rm(r["x_prop"])
    got, got_lp = xc.cpu().double(), lpc.cpu().double()
    tol = lambda ref: S.ELEM_ATOL + S.ELEM_RTOL * ref.abs()
    is_stay = ((got - stay).abs() <= tol(stay)).all(dim=1)
    is_move = ((got - move).abs() <= tol(move)).all(dim=1)
    if n == 1 and remove_mean:  # one particle: both outcomes are the zero row, the logp tells them apart
        is_move = (got_lp - r["logp_prop"]).abs() <= tol(r["logp_prop"])
        is_stay = ~is_move
    assert bool((is_stay ^ is_move).all()), ("a walker is neither its old row nor its proposal", int((~(is_stay ^ is_move)).sum()))
    lp_want = torch.where(is_move, r["logp_prop"], r["logp"])
    np.testing.assert_allclose(got_lp.numpy(), lp_want.numpy(), rtol=S.ELEM_RTOL, atol=S.ELEM_ATOL)
    keep = ~r["left_out"]
    wrong = int((is_move[keep] != r["acc"][keep]).sum())
    _say(f"mala {S.mala_case_id(c)} remove_mean={remove_mean}", f"dt {r['dt']}, moved {int(is_move.sum())} of {B} (float64 reference "
         f"{int(r['acc'].sum())}), delta32 {r['delta32']:.1e}, compared {int(keep.sum())}, decisions differing {wrong}, x_prop worst "
         f"|error| {float((xp.cpu().double() - r['x_prop']).abs().max()):.1e}")
    assert wrong == 0
    assert int(count.item()) == int(is_move.sum())


@pytest.mark.parametrize("adaptive", [0, 1])
def test_mala_adapt_rule(pa, adaptive):
    """rate = float32 quotient of the count, compared in double with 0.55; dt * 1.1 or / 1.1 in double: bit-equal, on both
    sides of the threshold and at the counts whose float32 rate is 0.55f; the count is reset."""
    L, st = pa._lib.lib(), pa._lib.stream_ptr()
    for total, acc in S.ADAPT_CASES:
        for dt0 in (0.05, 0.37):
            dt = torch.tensor([dt0], dtype=torch.float64, device="cuda")
            count = torch.tensor([acc], dtype=torch.int32, device="cuda")
            rate = torch.full((1,), float("nan"), device="cuda")
            _ok(pa, L.pita_mala_adapt(dt.data_ptr(), count.data_ptr(), total, adaptive, rate.data_ptr(), st))
            want_dt, want_rate = S.adapt_reference(dt0, acc, total, bool(adaptive))
            assert dt.item() == want_dt and np.float32(rate.item()) == want_rate and int(count.item()) == 0, (total, acc, dt0)
            count.fill_(acc)
            _ok(pa, L.pita_mala_adapt(dt.data_ptr(), count.data_ptr(), total, adaptive, 0, st))  # rate_out absent
            assert dt.item() == S.adapt_reference(want_dt, acc, total, bool(adaptive))[0]
