"""What tests/test_mlp_shapes_gpu.py rests on, checked without a GPU: the restated oracle pieces of tests/_mlp_shapes.py
against oracle/pita_oracle.py itself, and every derived bound (see the docstring of tests/_mlp_shapes.py) finite and
below what the older MLP tests allow.  The slowest case, vmap(jacrev) of the hidden-128 x 3 net at D = 64 on 642
walkers in fp64, fp32 and perturbed fp64, takes about 7 s on 16 threads; the whole module under a minute."""
import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _mlp_shapes as S

WALKERS_PER_LEVEL = 107  # B = 642: a ragged last tile (642 = 20 * 32 + 2)


@pytest.mark.parametrize("cfg", S.CONFIGS, ids=S.cfg_id)
def test_derived_bounds_are_finite_and_below_the_older_tests(cfg):
    """max(4 * e32, 4 * perturbation change, 1.2e-7) for the backbone output and every derivative quantity, per noise
    level: finite, and below 2e-5 (forward) / 5e-5 (derivatives)."""
    _, wd, kw = S.make_net(*cfg)
    inp = S.sweep_inputs(cfg[2], WALKERS_PER_LEVEL)
    r64, r32, rp = S.reference_sets(wd, kw, inp)
    bounds = S.derive_bounds(r64, r32, rp, S.level_masks(inp["x"].shape[0]))
    for name, rows in bounds.items():
        print(f"[mlp shapes bounds {S.cfg_id(cfg)}] {name}: " +
              ", ".join(f"h={h:g} {b:.1e} (e32 {e:.1e}, floor {f:.1e})" for h, (b, e, f) in zip(S.LEVELS, rows)))
        for h, (b, e, f) in zip(S.LEVELS, rows):
            assert np.isfinite(b) and np.isfinite(e) and np.isfinite(f), (name, h)
            assert b < S.cap_of(name), (name, h, b)
            assert torch.isfinite(r64[name]).all() and float(r64[name].abs().max()) > 0, name


def test_restated_forward_is_the_oracle():
    """embed + mlp_tail is O.mlp_forward (same operations: equal to fp64 rounding); with the angle formed in fp32 it
    equals O.mlp_forward (fp64) at small angles up to the fp32 rounding of the angle, bounded by the change under an
    embedding perturbation of one fp32 ulp of an angle of 1 rad (2^-23)."""
    for cfg in S.CONFIGS[:6]:
        _, wd, kw = S.make_net(*cfg)
        D = cfg[2]
        gen = torch.Generator().manual_seed(D)
        B = 96
        x = (torch.rand(B, D, generator=gen) * 2 - 1).float().double() * 0.04  # |25 x| <= 1 rad
        t = (torch.rand(B, generator=gen) * 2 - 1).float().double()
        beta = torch.rand(B, generator=gen).float().double()
        want = O.mlp_forward(wd, t, x, beta, **kw)
        assert S.rel(S.forward_restated(wd, kw, t, x, beta), want) < 1e-14
        got = S.forward_restated(wd, kw, t, x, beta, angle32=True)
        delta = S.emb_delta(B, D, kw) * (2.0**-23 / S.PERTURB)
        floor = 4 * S.rel(S.forward_restated(wd, kw, t, x, beta, delta=delta), want)
        e = S.rel(got, want)
        print(f"[mlp shapes restated {S.cfg_id(cfg)}] fp32-angle restatement vs fp64 oracle {e:.1e} (bound {floor:.1e})")
        assert 0 < e <= floor < 1e-5


@pytest.mark.parametrize("cfg", S.LARGE_ANGLE_CONFIGS, ids=S.cfg_id)
def test_large_angle_restatement_and_fp32_oracle(cfg):
    """At |x| up to 400 and t, beta up to 50 the fp32 reference rounds the angle to fp32 before the sine; against the
    fp64 restatement OF THAT fp32 ANGLE it stays within the derived bound, which is below 2e-5.  Against the plain fp64
    oracle (angle in fp64) it does not: that comparison would measure the rounding of the inputs' products."""
    _, wd, kw = S.make_net(*cfg)
    x, t, beta = S.large_angle_inputs(cfg[2], 640)
    r64, r32, rp = S.large_angle_references(wd, kw, x, t, beta)
    e32, floor = S.rel(r32, r64), 4 * S.rel(rp, r64)
    bound = max(4 * e32, floor, S.ONE_ULP)
    plain = S.rel(O.mlp_forward(wd, t.double(), x.double(), beta.double(), **kw), r64)
    print(f"[mlp shapes large angles {S.cfg_id(cfg)}] fp32 oracle {e32:.1e}, floor {floor:.1e}, bound {bound:.1e}; "
          f"fp64-angle oracle differs by {plain:.1e}")
    assert np.isfinite(bound) and e32 <= bound < S.CAP_FORWARD
    assert plain > 10 * e32  # the reason for the restatement


def _fp64_table(n_steps, beta, gamma=4 / 3):
    """The step table from the oracle's own schedule in fp64 (layout of include/pita_hip.h)."""
    from pita_amd import _lib

    sched, gam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(gamma)
    times = torch.linspace(1.0, 0.0, n_steps + 1)[:-1].double()
    tab = torch.zeros(n_steps, _lib.STEP_STRIDE, dtype=torch.float64)
    for k, t in enumerate(times):
        h, g = sched.h(t), sched.g(t)
        c_s, c_in, c_out, c_noise = O.edm_coeffs(h)
        for col, v in ((_lib.ST_CS, c_s), (_lib.ST_CIN, c_in), (_lib.ST_COUT, c_out), (_lib.ST_CNOISE, c_noise),
                       (_lib.ST_H, h), (_lib.ST_G2, g**2), (_lib.ST_GAMMA, gam.gamma(t)), (_lib.ST_DT, 1.0 / n_steps),
                       (_lib.ST_NOISE_SCALE, g), (_lib.ST_SQRT_DT, np.sqrt(1.0 / n_steps)), (_lib.ST_BETA, beta)):
            tab[k, col] = float(v)
    return tab


@pytest.mark.parametrize("remove_mean", [True, False])
def test_oracle_sampler_loop_is_the_oracle_integrator(remove_mean):
    """oracle_sampler_loop on an fp64 step table equals O.integrate_sde driven by O.f_not_debiased (2 x 3-D particles,
    5 steps, injected noise); the host's fp32 table equals the fp64 one to the fp32 rounding of the schedule."""
    _, wd, kw = S.make_net(64, 2, 6, True)
    bb = S.backbone(wd, kw)
    N, B, n, d, beta = 5, 37, 2, 3, 1.3
    x0, noise = S.sampler_inputs(6, n, d, B, N)
    tab = _fp64_table(N, beta)
    got, stats = S.oracle_sampler_loop(bb, tab, x0, noise, n, d, remove_mean)
    sched, gam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    cfg = O.IntegratorConfig(num_integration_steps=N, end_resampling_step=N, should_mean_free=remove_mean)
    ref = O.integrate_sde(cfg, x0.double(), lambda t, xc: O.f_not_debiased(bb, sched, gam, t, xc, beta), sched.g,
                          lambda i, shp: noise[i].double(), n, d, record=True)
    assert S.rel(got, ref["x"]) < 1e-12
    assert S.rel(stats[:, 0], ref["drift_X"].sum(dim=(1, 2))) < 1e-10
    assert S.rel(stats[:, 1], (ref["drift_X"] ** 2).sum(dim=(1, 2))) < 1e-12
    t32 = S.step_table(N, beta=beta).double()
    used = [c for c in range(11)]
    err = ((t32[:, used] - tab[:, used]).abs() / tab[:, used].abs().clamp_min(1e-30)).max()
    # sigma(t) = (a + t b)^7 and h = sigma^2 in fp32: each rounding of the base comes back 14-fold, 6e-8 * 14 * (a few)
    assert float(err) < 5e-6, float(err)


@pytest.mark.parametrize("case", S.SAMPLER_CASES, ids=lambda c: f"h{c[0]}_d{c[1]}_{c[2]}x{c[3]}")
def test_sampler_bounds_are_finite_and_below_the_older_tests(case):
    """The fused sampler's bound on the final walkers and on the four per-step sums, from the fp32 and the perturbed
    oracle loop: finite and below 2e-5 (what test_mlp_fused_sampler_particles allows)."""
    hidden, D, n, d = case
    _, wd, kw = S.make_net(hidden, 2, D, True)
    tab = S.step_table(5, beta=1.3)
    x0, noise = S.sampler_inputs(D, n, d, 107, 5)
    for rm in (True, False):
        r64, r32, rp = S.sampler_reference_sets(wd, kw, tab, x0, noise, n, d, rm)
        e32, floor = S.rel(r32["x"], r64["x"]), 4 * S.rel(rp["x"], r64["x"])
        bound = max(4 * e32, floor, S.ONE_ULP)
        print(f"[mlp shapes sampler bounds h{hidden} D={D} remove_mean={rm}] walkers {bound:.1e} (e32 {e32:.1e}, floor {floor:.1e})")
        assert np.isfinite(bound) and bound < S.CAP_FORWARD
        assert torch.isfinite(r64["stats"]).all()
        steps = S.stats_steps(n, rm, 5)
        sb = S.stats_bounds(r64["stats"], r32["stats"], rp["stats"], 107 * D, steps)
        print(f"[mlp shapes sampler bounds h{hidden} D={D} remove_mean={rm}] sums: " +
              ", ".join(f"{nm} {b:.1e} (e32 {e:.1e}, floor {f:.1e})" for nm, (b, e, f) in zip(S.STATS_NAMES, sb)))
        for k, (b, e, f) in enumerate(sb):
            assert np.isfinite(b) and b < S.STATS_CAPS[k], (S.STATS_NAMES[k], rm, b)
