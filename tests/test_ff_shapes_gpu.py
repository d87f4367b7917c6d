"""The force-field kernels (ff_kernel<false>, ff_kernel<true>, ff_mala_kernel) at every launch plan pita_ff_create can
give: the systems and term mixes of tests/_ff_shapes.py -- 2 to 89 atoms, 128 walkers per block down to one, empty
tables, torsion periodicities 0 and 12 -- against the fp64 oracle, every walker on its own; the 92-atom chain refused;
results that do not depend on the plan, the batch or a NaN neighbour; the fused descent and the fused MALA chain bit for
bit against the launch-per-kernel paths, through the second trip of the persistent-block loops.  Tolerances are those
of test_forcefield_vs_oracle / test_peptide_forcefield_vs_oracle, per walker; tests/test_ff_shapes_cpu.py shows that the
fp32 oracle meets a quarter of each on the same inputs.  Run on an MI355X: pytest -m gpu -s prints the figures kept in
profiles/ff_shapes_measured.txt."""
import math

import pytest
import torch

from tests import _ff_shapes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


@pytest.fixture(scope="module")
def lds(pa):
    v, src = S.lds_limit()
    print(f"[ff shapes] per-block LDS limit {v} B, from: {src}")
    return v


def _fmt(bs):
    return ",".join(map(str, bs))


# ------------------------------------------------------------------ a, b, g: pita_ff_logp_force against the oracle
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_logp_force_vs_oracle(pa, lds, c):
    """Every case the restated plan accepts is created and evaluated; every batch size, every walker on its own; at the
    largest batch: force == NULL, a second call and the batch without its first walker give the same bits, B = 0 leaves
    live buffers alone, forces sum to zero over the atoms."""
    r = S.reference(c)
    n = S.N_ATOMS[c.system]
    blob, walker, wpb = S.case_plan(c, lds)
    assert wpb >= 1
    e = S.energy(c)
    bs = S.batch_sizes(wpb)
    worst = [(-1.0, 0), (-1.0, 0)]
    for B in bs:
        x, idx = S.case_batch(r, B)
        rc, lp, f = S.logp_force(pa, e, x.cuda())
        assert rc == 0, pa._lib.last_error()
        e_lp, e_f = S.walker_errors(lp, f, r, idx)
        worst = [max(worst[0], (float(e_lp.max()), B)), max(worst[1], (float(e_f.max()), B))]
    e32 = S.walker_errors(r["logp32"], r["f32"], r, torch.arange(S.ORACLE_WALKERS))
    print(f"[ff shapes {S.case_id(c)}] n {n} terms {S.term_counts(r['tables'])[1:4]} gb {c.gb} cutoff {c.cutoff}; plan at {lds} B: "
          f"blob {blob} walker {walker} wpb {wpb}; B {_fmt(bs)}: worst walker, error / allowance: logp {worst[0][0]:.3f}@B={worst[0][1]} "
          f"(allowance {S.LOGP_ATOL:g} + {S.LOGP_RTOL:g} |logp|) force {worst[1][0]:.3f}@B={worst[1][1]} (allowance {S.FORCE_RTOL:g} |f|); "
          f"fp32 oracle on the same inputs logp {float(e32[0].max()):.3f} force {float(e32[1].max()):.3f}")
    assert worst[0][0] <= 1.0 and worst[1][0] <= 1.0
    # lp, f: the largest batch
    xg = x.cuda()
    rc, lp0, none = S.logp_force(pa, e, xg, want_force=False)
    assert rc == 0 and none is None and torch.equal(lp0, lp)
    rc, lp2, f2 = S.logp_force(pa, e, xg)
    assert rc == 0 and torch.equal(lp2, lp) and torch.equal(f2, f)
    if B > 1:
        rc, lp1, f1 = S.logp_force(pa, e, xg[1:].contiguous())
        assert rc == 0 and torch.equal(lp1, lp[1:]) and torch.equal(f1, f[1:])
    rc, lpz, fz = S.logp_force(pa, e, xg, B=0, fill=7.0)
    torch.cuda.synchronize()
    assert rc == 0 and bool((lpz == 7.0).all()) and bool((fz == 7.0).all())
    assert abs(f.reshape(B, n, 3).sum(1)).max() < 1e-3 * f.abs().max().item()


def test_first_refused_chain_and_a_handle_after_it(pa, lds):
    """The 92-atom chain: PITA_EUNSUPPORTED (code -2) with the bytes one walker needs and the bytes the device allows, as
    the restated plan has them; a 12-atom handle created after the refusal works."""
    t, _ = S.base_system(S.REFUSED)
    blob, walker, wpb = S.plan(*S.term_counts(t), lds)
    assert wpb == 0
    with pytest.raises(pa._lib.PitaHipError) as info:
        S.energy(t, S.N_ATOMS[S.REFUSED])._native()
    print(f"[ff shapes {S.REFUSED}] plan at {lds} B: blob {blob} walker {walker} wpb 0; refused: {info.value}")
    assert info.value.code == -2 and str(blob + walker) in str(info.value) and str(lds) in str(info.value)
    c = S.base_case("ace_nme")
    r = S.reference(c)
    x, idx = S.case_batch(r, 5)
    rc, lp, f = S.logp_force(pa, S.energy(c), x.cuda())
    e_lp, e_f = S.walker_errors(lp, f, r, idx)
    assert rc == 0 and float(e_lp.max()) <= 1.0 and float(e_f.max()) <= 1.0


# ------------------------------------------------------------------ c: the plan does not show
@pytest.mark.parametrize("system", S.PLAN_SYSTEMS)
def test_plan_does_not_show_in_the_results(pa, lds, system):
    """Fewer walkers per block than 256 / n: logp, force, descent and the non-adaptive MALA chain of a walker are the same
    bits in batches of 1, 2, wpb + 1 and 7 taken at several offsets (Philox keys follow the walker: walker_offset)."""
    c = S.base_case(system)
    n = S.N_ATOMS[system]
    wpb = S.case_plan(c, lds)[2]
    assert 1 <= wpb < 256 // n
    e = S.energy(c)
    B, steps, dt = 16, 3, S.DESCENT_DT
    x = S.case_batch(S.reference(c), B)[0].cuda()

    def run(xq, lo):
        rc, lp, f = S.logp_force(pa, e, xq)
        assert rc == 0
        xd = e.fused_descent(xq.clone(), steps, dt, 1.0, math.sqrt(2 * dt), seed=5, walker_offset=lo)
        xm, lm = xq.clone(), lp.clone()
        S.fused_mala(e, xm, lm, steps, S.MALA_DT, False, None, None, 7, lo, True)
        return lp, f, xd, xm, lm

    full = run(x, 0)
    assert not torch.equal(full[2], x) and not torch.equal(full[3], x)
    for lo, cnt in ((0, 1), (5, 1), (15, 1), (0, 2), (3, 2), (14, 2), (0, wpb + 1), (4, wpb + 1), (0, 7), (3, 7), (9, 7)):
        part = run(x[lo:lo + cnt].contiguous(), lo)
        for name, a, b in zip(("logp", "force", "descent", "mala x", "mala logp"), part, full):
            assert torch.equal(a, b[lo:lo + cnt]), (name, lo, cnt)


# ------------------------------------------------------------------ d: a NaN walker stays alone
@pytest.mark.parametrize("system", S.NAN_SYSTEMS)
def test_nan_walker_stays_alone(pa, lds, system):
    """One NaN coordinate in walker 1 / in the last walker: that walker's logp is non-finite, every other walker's logp,
    force and two descent steps are the bits of the clean run."""
    c = S.base_case(system)
    wpb = S.case_plan(c, lds)[2]
    e = S.energy(c)
    B = 3 * wpb + 1
    x = S.case_batch(S.reference(c), B)[0].cuda()
    _, lp, f = S.logp_force(pa, e, x)
    xd = e.fused_descent(x.clone(), 2, S.DESCENT_DT, 0.0, 0.0, seed=0)
    assert torch.isfinite(lp).all() and torch.isfinite(f).all() and torch.isfinite(xd).all()
    for victim in (1, B - 1):
        xb = x.clone()
        xb[victim, 4] = float("nan")
        others = torch.arange(B, device=x.device) != victim
        rc, lpb, fb = S.logp_force(pa, e, xb)
        assert rc == 0 and not bool(torch.isfinite(lpb[victim]))
        assert torch.equal(lpb[others], lp[others]) and torch.equal(fb[others], f[others]), victim
        xbd = e.fused_descent(xb.clone(), 2, S.DESCENT_DT, 0.0, 0.0, seed=0)
        assert not bool(torch.isfinite(xbd[victim]).all()) and torch.equal(xbd[others], xd[others]), victim


# ------------------------------------------------------------------ e: fused descent
def _descent_case(pa, lds, system, B, steps, tag):
    c = S.base_case(system)
    wpb = S.case_plan(c, lds)[2]
    e = S.energy(c)
    x0, nz, _ = S.step_inputs(system, B, steps)
    xg, ng = x0.cuda(), nz.cuda()
    dt, sq = S.DESCENT_DT, math.sqrt(2 * S.DESCENT_DT)
    rows = S.sample_rows(B, wpb)
    worst = 0.0
    for mode in ("deterministic", "injected", "philox"):
        for rm in (True, False):
            ns = 0.0 if mode == "deterministic" else 1.0
            noise = ng if mode == "injected" else None
            xf = e.fused_descent(xg.clone(), steps, dt, ns, sq, seed=3, walker_offset=11, remove_mean=rm, noise=noise)
            xs = S.per_step_descent(pa, e, xg.clone(), noise, steps, dt, ns, sq, 3, 11, rm)
            diff = int((xf != xs).any(dim=1).sum())
            assert diff == 0, f"{mode} remove_mean {rm}: fused descent differs from force kernel + pita_em_step in {diff} of {B} walkers"
            assert torch.isfinite(xf).all() and not torch.equal(xf, xg)
            if mode != "philox":
                xo = S.oracle_descent(c, x0[rows], nz[:, rows], steps, dt, mode == "injected", rm)
                err = float(S.nan_to_inf((xf.cpu().double()[rows] - xo).norm(dim=1) / xo.norm(dim=1)).max())
                worst = max(worst, err)
    print(f"[ff shapes descent {system}{tag}] wpb {wpb} B {B} steps {steps}: six configurations bit-equal to force kernel + "
          f"pita_em_step; worst walker against the fp64 oracle {worst:.1e} / tolerance {S.DESCENT_RTOL:g} ({len(rows)} walkers)")
    assert worst <= S.DESCENT_RTOL


@pytest.mark.parametrize("system", S.STEP_SYSTEMS)
def test_fused_descent(pa, lds, system):
    wpb = S.case_plan(S.base_case(system), lds)[2]
    _descent_case(pa, lds, system, 3 * wpb + 1, S.DESCENT_STEPS, "")


def test_fused_descent_grid_stride(pa, lds):
    """More blocks than the persistent grid: the second trip of ff_kernel<true>'s block loop, ragged."""
    wpb = S.case_plan(S.base_case(S.GRID_STRIDE_SYSTEM), lds)[2]
    _descent_case(pa, lds, S.GRID_STRIDE_SYSTEM, S.GRID_CAP * wpb + 3, 2, " grid-stride")


# ------------------------------------------------------------------ f: fused MALA
def _replay_dt(rates):
    """mala_adapt_kernel's rule on the host: the same double arithmetic on the same fp32 rates."""
    dt = S.MALA_DT
    for r in rates:
        dt = dt * 1.1 if r > 0.55 else dt / 1.1
    return dt


def _mala_case(pa, lds, system, B, steps, tag, through_integrator=True):
    c = S.base_case(system)
    wpb = S.case_plan(c, lds)[2]
    e = S.energy(c)
    x0, nz, uu = S.step_inputs(system, B, steps, extra=2)
    xg, ng, ug = x0.cuda(), nz.cuda(), uu.cuda()
    lp0 = e(xg)
    assert torch.isfinite(lp0).all()
    for adaptive in (False, True):
        for inject in (False, True):
            noise, unif = (ng, ug) if inject else (None, None)
            integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                             end_resampling_step=1, post_mcmc_steps=steps, dt_negative_time=S.MALA_DT,
                                             adaptive_mcmc=adaptive, should_mean_free=True, seed=9)
            key = integ._key(2)
            xf, lf = xg.clone(), lp0.clone()
            rf, dtf = S.fused_mala(e, xf, lf, steps, S.MALA_DT, adaptive, noise, unif, key, 0, True)
            xk, lk = xg.clone(), lp0.clone()
            rk, dtk = S.per_kernel_mala(pa, e, xk, lk, steps, S.MALA_DT, adaptive, noise, unif, key, 0, True)
            print(f"[ff shapes mala {system}{tag}] wpb {wpb} B {B} adaptive {adaptive} injected {inject}: rates {rf} final dt {dtf:.6g}")
            diff = int((xf != xk).any(dim=1).sum())
            assert diff == 0, f"fused chain differs from the launch-per-kernel chain in {diff} of {B} walkers"
            assert torch.equal(lf, lk) and rf == rk and len(rf) == steps and dtf == dtk
            assert dtf == (_replay_dt(rf) if adaptive else S.MALA_DT)
            assert torch.isfinite(xf).all() and torch.isfinite(lf).all() and not torch.equal(xf, xg)
            if through_integrator:
                run = integ.metropolis_hastings_mala_adaptive if adaptive else integ.metropolis_hastings_mala
                args = (xg.clone(), e, S.MALA_DT) if adaptive else (xg.clone(), e)
                xi, ri = run(*args, return_acceptance_rate=True, fused=False, noise=noise, uniforms=unif)
                assert torch.equal(xi, xf) and ri == rf


@pytest.mark.parametrize("system", S.STEP_SYSTEMS)
def test_fused_mala_equals_per_kernel(pa, lds, system):
    """ForceFieldEnergy.fused_mala against pita_mala_propose / pita_mala_accept / pita_mala_adapt round the force kernel
    (walkers, logp, rates, final step size) and against WeightedSDEIntegrator._mala(fused=False) (walkers, rates)."""
    wpb = S.case_plan(S.base_case(system), lds)[2]
    _mala_case(pa, lds, system, 3 * wpb + 1, S.MALA_STEPS, "")


def test_fused_mala_grid_stride(pa, lds):
    """The second trip of ff_mala_kernel's block loop (it reloads the walkers, logp and the Philox key), ragged."""
    wpb = S.case_plan(S.base_case(S.GRID_STRIDE_SYSTEM), lds)[2]
    _mala_case(pa, lds, S.GRID_STRIDE_SYSTEM, S.GRID_CAP * wpb + 3, 2, " grid-stride", through_integrator=False)


def test_fused_mala_first_step_vs_oracle(pa, lds):
    """One fused step with injected draws against O.mala_step + remove_mean in fp64, under the rule and the bounds of
    test_ff_fused_mala_vs_oracle: decisions agree except where the oracle's log-ratio is within 0.1 of log u, positions
    agree to rel 1e-5 where the decisions agree.  The kernel's decision is read off the walker: nearer the centred
    proposal than the (mean-free) start.  That test's |x_out - x| > |x' - x| / 2 takes an accepted walker of two atoms for
    a rejected one: half of a two-atom move is translation, which the centring removes.  On at least one system the step
    accepts and rejects."""
    mixed = []
    for system in S.STEP_SYSTEMS:
        c = S.base_case(system)
        wpb = S.case_plan(c, lds)[2]
        B = 3 * wpb + 1
        e = S.energy(c)
        x0, nz, uu = S.step_inputs(system, B, S.MALA_STEPS, extra=2)
        rows = S.sample_rows(B, wpb)
        xf = x0.cuda()
        lf = e(xf)
        S.fused_mala(e, xf, lf, 1, S.MALA_DT, False, nz[:1].cuda(), uu[:1].cuda(), 0, 0, True)
        out = xf.cpu().double()[rows]
        xo, acc, margin, xpc = S.oracle_mala_step(c, x0[rows], nz[0][rows], uu[0][rows], S.MALA_DT)
        hip_acc = (out - xpc).norm(dim=1) < (out - x0[rows].double()).norm(dim=1)  # nearer the proposal than the start
        same = hip_acc == acc
        near = margin.abs() < S.MALA_NEAR
        err = float((out[same] - xo[same]).norm() / xo[same].norm())
        print(f"[ff shapes mala oracle {system}] wpb {wpb} B {B}: oracle accepted {int(acc.sum())} of {len(rows)}, decisions "
              f"differ on {int((~same).sum())} ({int((~same & ~near).sum())} outside the bound), rel {err:.1e} / tolerance {S.MALA_RTOL:g}")
        assert bool((same | near).all()) and bool(same.any())
        assert err < S.MALA_RTOL
        if 0 < int(acc.sum()) < len(rows):
            mixed.append(system)
    assert mixed
