"""The debiased Feynman-Kac regime on the MLP backbones (MyMLP / MyMLPTemperature): the forward-mode derivative kernels
of csrc/mlp_jac_kernel.hip (pita_mlp_jacobian, pita_mlp_jvp) against the fp64 oracle's autograd / vmap(jacrev), every
SDETerms field of VEReverseSDE(debias_inference=True) against O.f_debiased, the integrator end to end, and the kernel's
determinism and batch independence.  Run on an MI355X: pytest -m gpu."""
import copy

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests._mlp_shapes import _oracle_derivs  # fp64 D, F, J_x D, dD/dh by vmap(jacrev); shared with test_mlp_shapes_*

pytestmark = pytest.mark.gpu
T = torch.tensor


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def _net(kind, golden):
    """(HIP module, fp64 state dict, oracle kwargs) of the three configurations under test."""
    from pita_amd import mlp

    if kind == "gmm":  # MyMLP 128 x 3, emb 128, D = 2 (config C1)
        net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
        net.load_state_dict({k[2:]: T(v) for k, v in golden("mlp_gmm_fwd.npz").items() if k.startswith("w.")})
        kw = dict(emb_size=128, hidden_layers=3)
    elif kind == "temp":  # MyMLPTemperature 64 x 2, emb 64, D = 3
        net = mlp.MyMLPTemperature(hidden_size=64, hidden_layers=2, emb_size=64, out_dim=3, input_dim=3)
        net.load_state_dict({k[2:]: T(v) for k, v in golden("mlp_temp_fwd.npz").items() if k.startswith("w.")})
        kw = dict(emb_size=64, hidden_layers=2, temperature_conditioned=True)
    else:  # hidden 32, D = 6: emb_size/2 = 16, the general embedding path (no weight stream)
        torch.manual_seed(61)
        net = mlp.MyMLPTemperature(hidden_size=32, hidden_layers=2, emb_size=32, out_dim=6, input_dim=6)
        kw = dict(emb_size=32, hidden_layers=2, temperature_conditioned=True)
    wd = {k: v.double() for k, v in net.state_dict().items()}
    return net, wd, kw


@pytest.mark.parametrize("kind", ["gmm", "temp", "h32"])
def test_mlp_jacobian_vs_oracle(pa, golden, kind):
    """jvp (unit / dense vx, vh, both; dot_out, diag_acc), jacobian_trace and vjp (cot = x and dense; dot_h, dot_parts)
    against autograd of the fp64 oracle at several h, small ones included; D against ScoreNet.denoiser."""
    net, wd, kw = _net(kind, golden)
    D = net.input_dim
    bb = lambda cn, xs, b: O.mlp_forward(wd, cn, xs, b, **kw)
    gen = torch.Generator().manual_seed(5 + D)
    hs = [1e-3, 1e-2, 0.3, 4.0, 70.0]
    B = 20 * len(hs)
    h = torch.tensor(hs)[torch.arange(B) % len(hs)]
    x = (torch.randn(B, D, generator=gen) * (1 + h.sqrt())[:, None]).float()
    beta = (torch.rand(B, generator=gen) + 0.5).float()
    vx = torch.randn(B, D, generator=gen).float()
    vh = torch.randn(B, generator=gen).float()
    cot = torch.randn(B, D, generator=gen).float()
    Do, Fo, J, dDdh = _oracle_derivs(bb, h.double(), x.double(), beta.double())
    hc, xc, bc = h.cuda(), x.cuda(), beta.cuda()
    c_s, c_in, c_out, _ = O.edm_coeffs(h.double())
    errs = {}

    def check(name, got, want, bound=5e-5):  # per noise level: the magnitudes differ by orders between them
        for i, hv in enumerate(hs):
            sel = (torch.arange(B) % len(hs)) == i
            e = rel(got.detach().cpu()[sel], want[sel])
            errs[name] = max(errs.get(name, 0.0), e)
            assert e < bound, (kind, name, hv, e)

    # D itself: the oracle, and the production wrapper (pita_edm_scale_input + pita_mlp_forward + pita_edm_combine)
    tr, Dk = net.jacobian_trace(hc, xc, bc, want_denoiser=True)
    check("D", Dk, Do)
    assert rel(Dk, pa.ScoreNet(net).denoiser(hc, xc, bc)) < 1e-6
    check("trace", tr, torch.diagonal(J, dim1=1, dim2=2).sum(-1))
    assert torch.equal(net.jacobian_trace(hc, xc, bc), tr)
    # jvp: unit directions with the in-kernel reductions, dense vx, vh, both
    diag = torch.zeros(B, device="cuda")
    dots = torch.zeros(B, D, device="cuda")
    for k in range(D):
        out, dout = net.jvp(hc, xc, bc, direction=k, dot_out=dots, dot_col=k, diag_acc=diag)
        check("jvp_unit", dout, J[:, :, k])
        if k == 0:
            check("jvp_primal", out, Do)
    check("jvp_dot_out", dots, torch.einsum("bi,bik->bk", x.double(), J))
    check("jvp_diag_acc", diag, torch.diagonal(J, dim1=1, dim2=2).sum(-1))
    vxd, vhd = vx.double(), vh.double()
    _, d1 = net.jvp(hc, xc, bc, vx=vx.cuda())
    check("jvp_dense", d1, torch.einsum("bij,bj->bi", J, vxd))
    dot_h1 = torch.zeros(B, device="cuda")
    _, d2 = net.jvp(hc, xc, bc, vh=vh.cuda(), dot_out=dot_h1)
    check("jvp_vh", d2, dDdh * vhd[:, None])
    check("jvp_vh_dot", dot_h1, (x.double() * dDdh).sum(-1) * vhd)
    _, d3 = net.jvp(hc, xc, bc, vx=vx.cuda(), vh=vh.cuda())
    check("jvp_both", d3, torch.einsum("bij,bj->bi", J, vxd) + dDdh * vhd[:, None])
    # vjp: cot = x (what grad_x E_theta needs) and a dense cotangent, with dot_h and the split dot_parts
    for cname, cv in (("x", None), ("dense", cot)):
        cvd = x.double() if cv is None else cv.double()
        Dv, vj, dh, parts = net.vjp(hc, xc, bc, cot=None if cv is None else cv.cuda(), want_dot_h=True, want_h_parts=True)
        check("vjp_D", Dv, Do)
        check(f"vjp_{cname}", vj, torch.einsum("bi,bik->bk", cvd, J))
        dho = (cvd * dDdh).sum(-1)
        check(f"dot_h_{cname}", dh, dho)
        check(f"parts0_{cname}", parts[:, 0], c_out * (cvd * Fo).sum(-1))
        check(f"parts1_{cname}", parts[:, 1], dho + c_s**2 * (cvd * x.double()).sum(-1))
    print(f"[mlp jacobian {kind}] max rel err per noise level: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))


def _sde_pair(pa, golden, case, pb=False):
    """(VEReverseSDE with MLP score AND energy nets, oracle backbones fp64 / fp32, beta, D, geometry)."""
    from pita_amd import mlp
    from pita_amd.energy_net import EnergyNet

    if case == "gmm":
        s_net, wd_s, kw = _net("gmm", golden)
        torch.manual_seed(17)
        e_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
        beta, D, n, d = 1.0, 2, 1, 2
    else:  # 2 particles x 3-D, mean-free, temperature-conditioned
        torch.manual_seed(23)
        s_net = mlp.MyMLPTemperature(hidden_size=64, hidden_layers=2, emb_size=64, out_dim=6, input_dim=6)
        e_net = copy.deepcopy(s_net)
        with torch.no_grad():
            for p in e_net.parameters():
                p.mul_(0.9)
        kw = dict(emb_size=64, hidden_layers=2, temperature_conditioned=True)
        beta, D, n, d = 1.25, 6, 2, 3
    ws = {k: v.double() for k, v in s_net.state_dict().items()}
    we = {k: v.double() for k, v in e_net.state_dict().items()}
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(s_net, precondition_beta=pb),
                          energy_net=EnergyNet(e_net, precondition_beta=pb), debias_inference=True)
    mk = lambda w, dt: (lambda cn, xs, b: O.mlp_forward({k: v.to(dt) for k, v in w.items()}, cn, xs, b, **kw))
    return sde, (mk(ws, torch.float64), mk(we, torch.float64)), (mk(ws, torch.float32), mk(we, torch.float32)), beta, D, n, d


@pytest.mark.parametrize("case,pb", [("gmm", False), ("particles", False), ("particles", True)])
def test_debiased_terms_on_mlp_backbones_vs_oracle(pa, golden, case, pb):
    """VEReverseSDE(debias_inference=True) with MLP score and energy nets: every SDETerms field against O.f_debiased
    (autograd / vmap(jacrev) in fp64) at t in {0.15, 0.6, 0.95}, bounds of the AD2_cat test; EnergyNet.forward against
    autograd of O.energy_theta.  The fp32 oracle's own error against fp64 is printed beside the kernel's."""
    sde, (bs64, be64), (bs32, be32), beta, D, n, d = _sde_pair(pa, golden, case, pb)
    osched, ogam = O.Elucidating(0.01, 80.0, 7), O.GammaConstant(4 / 3)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    gen = torch.Generator().manual_seed(40 + D)
    B = 96
    for tv in (0.15, 0.6, 0.95):
        scale = 1.0 + 30.0 * tv
        x = torch.randn(B, D, generator=gen) * scale
        if n > 1:
            x = O.remove_mean(x, n, d)
        terms = sde.f(torch.tensor(tv), x.cuda(), beta, gam, None, None, resampling_interval=1)
        ref = O.f_debiased(bs64, be64, osched, ogam, torch.tensor(tv, dtype=torch.float64), x.double(), beta,
                           precondition_beta=pb)
        r32 = O.f_debiased(bs32, be32, osched, ogam, torch.tensor(tv, dtype=torch.float32), x.float(), beta,
                           precondition_beta=pb)
        e, e32 = rel(terms.drift_X, ref.drift_X), rel(r32.drift_X, ref.drift_X)
        msg = [f"drift_X {e:.1e} (fp32 oracle {e32:.1e})"]
        assert e < 2e-4, (case, pb, tv, e)
        for nm in ("divergence_score", "cross_term", "dUt_dt", "drift_A"):
            want = getattr(ref, nm).numpy()
            got = getattr(terms, nm).cpu().numpy()
            msg.append(f"{nm} {rel(got, want):.1e} (fp32 oracle {rel(getattr(r32, nm), want):.1e})")
            np.testing.assert_allclose(got, want, rtol=3e-3, atol=3e-3 * float(np.abs(want).mean()),
                                       err_msg=f"{case} {pb} {tv} {nm}")
        print(f"[debiased {case} pb={pb} t={tv}] " + ", ".join(msg))
        if not pb:  # grad_x E_theta through the module interface (energy_net.py:51-62)
            ht = osched.h(torch.full((B,), tv, dtype=torch.float64))
            xg = x.double().requires_grad_(True)
            (gE,) = torch.autograd.grad(O.energy_theta(be64, ht, xg, beta).sum(), xg)
            got = sde.energy_net(ht.float().cuda(), x.cuda(), beta)
            assert rel(got, gE) < 2e-4, (case, tv, rel(got, gE))


def _gmm_setup(pa, golden, dtype=torch.float64):
    sde, (bs64, be64), (bs32, be32), beta, D, n, d = _sde_pair(pa, golden, "gmm")
    osched, ogam = O.Elucidating(0.01, 80.0, 7), O.GammaConstant(4 / 3)
    bs, be = (bs64, be64) if dtype == torch.float64 else (bs32, be32)
    drift = lambda t, xc: O.f_debiased(bs, be, osched, ogam, t, xc, beta)
    return sde, drift, osched


def test_debiased_integration_on_gmm_vs_oracle(pa, golden):
    """integrate_sde in the debiased regime on the GMM target with the MLP nets, injected noise, 256 walkers x 20 steps
    without resampling: walkers and log-weights against O.integrate_sde driven by O.f_debiased.  Twenty Euler-Maruyama
    steps down to h = 1e-4 amplify any rounding difference by orders of magnitude over the last ten steps (the fp32
    oracle itself ends 1e-1 away from the fp64 one), so every step is held to the fp32 oracle's own deviation from
    fp64: at most 10x that, floored at 2e-5."""
    sde, drift, osched = _gmm_setup(pa, golden)
    _, drift32, _ = _gmm_setup(pa, golden, torch.float32)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    N, B = 20, 256
    gen = torch.Generator().manual_seed(77)
    x1 = torch.randn(B, 2, generator=gen) * 40.0
    noise = torch.randn(N, B, 2, generator=gen)
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                     resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0,
                                     should_mean_free=False)
    x, logw, uniq, _, _ = integ.integrate_sde(x1.cuda(), pa.GMM(), gam, inverse_temperature=1.0, noise=noise.cuda())
    assert torch.isfinite(x).all() and torch.isfinite(logw).all()
    cfg = O.IntegratorConfig(num_integration_steps=N, end_resampling_step=N, should_mean_free=False)
    ref = O.integrate_sde(cfg, x1.double(), drift, osched.g, lambda i, shp: noise[i].double(), 1, 2)
    r32 = O.integrate_sde(cfg, x1.float(), drift32, osched.g, lambda i, shp: noise[i].float(), 1, 2)
    for k in range(N):
        e, e32 = rel(logw[k], ref["logweights"][k]), rel(r32["logweights"][k], ref["logweights"][k])
        print(f"[debiased gmm 256 x {N}] step {k:2d} log-weights rel {e:.1e} (fp32 oracle {e32:.1e})")
        assert e <= max(10 * e32, 2e-5), (k, e, e32)
    ex, ex32 = rel(x, ref["x"]), rel(r32["x"], ref["x"])
    print(f"[debiased gmm 256 x {N}] final walkers rel {ex:.1e} (fp32 oracle {ex32:.1e})")
    assert ex <= max(10 * ex32, 2e-5)


def test_debiased_resampling_ids_and_mala_on_gmm(pa, golden):
    """Resampling every step over 10 steps with fixed uniforms: at every event, from the oracle's walkers, the ids the
    HIP drift and systematic resampling give equal the oracle's (uniform_fn) -- a different id only where the uniform
    grid point lies between the oracle's and the kernel's cumulative weight (fp32 rounding of the weights); then the
    integrator itself over the same steps with a short MALA tail: finite results."""
    from pita_amd.utils import sample_cat_sys

    sde, drift, osched = _gmm_setup(pa, golden)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    N, B = 10, 256
    gen = torch.Generator().manual_seed(78)
    x1 = torch.randn(B, 2, generator=gen) * 40.0
    noise = torch.randn(N, B, 2, generator=gen)
    us = [float(u) for u in torch.rand(N, generator=gen, dtype=torch.float64)]
    times = torch.linspace(1.0, 0.0, N + 1)[:-1]
    dt = 1.0 / N
    x = x1.double()
    flips = 0
    for s in range(N):
        t = times[s].double()
        ref = drift(t, x)
        got = sde.f(times[s], x.float().cuda(), 1.0, gam, None, None, resampling_interval=1)
        a_ref, a_got = ref.drift_A * dt, (got.drift_A.double() * dt).cpu()
        ids_ref = O.sample_cat_sys(a_ref, us[s])
        ids_got = sample_cat_sys(B, a_got.float().cuda(), us[s])[0].cpu().numpy()
        bad = np.nonzero(ids_ref != ids_got)[0]
        if len(bad):
            u = (torch.tensor([us[s]], dtype=torch.float64) + torch.arange(B) / B) % 1.0
            cr = torch.cumsum(torch.clip(torch.softmax(a_ref, -1), 1e-6, 1.0), -1)
            cg = torch.cumsum(torch.clip(torch.softmax(a_got, -1), 1e-6, 1.0), -1)
            for j in bad:  # the boundary between the two chosen parents: u_j sits between the two cumulative weights
                k = int(min(ids_ref[j], ids_got[j]))
                lo, hi = sorted((float(cr[k]), float(cg[k])))
                assert lo - 1e-6 <= float(u[j]) <= hi + 1e-6, (s, j, float(u[j]), lo, hi)
            flips += len(bad)
        g_fn = osched.g(t * torch.ones(B, dtype=torch.float64))
        x = x + (ref.drift_X * dt + g_fn[:, None] * noise[s].double() * np.sqrt(dt))
        x = x[torch.from_numpy(ids_ref)]
    print(f"[debiased gmm resampling] {N} events x {B} walkers, ids differing at the grid: {flips}")
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                     resampling_interval=1, num_negative_time_steps=0, post_mcmc_steps=5,
                                     should_mean_free=False)
    xf, logw, uniq, _, acc = integ.integrate_sde(x1.cuda(), pa.GMM(), gam, inverse_temperature=1.0, noise=noise.cuda(),
                                                 resample_u=us)
    assert torch.isfinite(xf).all() and torch.isfinite(logw).all() and len(uniq) == N
    assert all(np.isfinite(float(a)) for a in acc)


def test_mlp_jacobian_determinism_and_batch_independence(pa, golden):
    """A 65 536-walker pita_mlp_jacobian twice: bit-identical; slices of 1, 33 and 4 097 walkers at several offsets:
    bit-equal to the full batch; unsupported configurations raise PitaHipError."""
    from pita_amd import mlp

    for kind in ("gmm", "h32"):
        net, _, _ = _net(kind, golden)
        D = net.input_dim
        gen = torch.Generator().manual_seed(9)
        B = 65536
        h = (10.0 ** (torch.rand(B, generator=gen) * 5 - 3)).cuda()
        x = (torch.randn(B, D, generator=gen) * 5).cuda()
        beta = (torch.rand(B, generator=gen) + 0.5).cuda()
        want = dict(want_denoiser=True, want_trace=True, want_vjp=True, want_dot_h=True, want_h_parts=True)
        a = net.jacobian(h, x, beta, **want)
        b = net.jacobian(h, x, beta, **want)
        for k in a:
            assert torch.equal(a[k], b[k]), (kind, k)
            assert torch.isfinite(a[k]).all(), (kind, k)
        for m in (1, 33, 4097):
            for off in (0, 31, 1000, B - m):
                s = net.jacobian(h[off:off + m], x[off:off + m], beta[off:off + m], **want)
                for k in a:
                    assert torch.equal(s[k], a[k][off:off + m]), (kind, k, m, off)
    x = torch.randn(8, 3).cuda()
    h = torch.rand(8).cuda() + 0.1
    bad = mlp.MyMLP(hidden_size=32, hidden_layers=1, emb_size=32, out_dim=2, input_dim=3)
    with pytest.raises(pa._lib.PitaHipError):
        bad.jacobian_trace(h, x, 1.0)
    with pytest.raises(pa._lib.PitaHipError):
        bad.jvp(h, x, 1.0, direction=0)
    big = mlp.MyMLP(hidden_size=32, hidden_layers=1, emb_size=32, out_dim=65, input_dim=65)
    with pytest.raises(pa._lib.PitaHipError):
        big.vjp(h, torch.randn(8, 65).cuda(), 1.0)
