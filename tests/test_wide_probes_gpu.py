"""pita_egnn_wide_trace_probes / EGNN_dynamics_AD2_cat.jacobian_trace_estimate: the Hutchinson estimate of trace(J_x D)
of the EDM denoiser around the wide EGNN backbone from (walker, probe) work items, pita_rademacher_probes, and the
``divergence="hutchinson"`` regime of VEReverseSDE / WeightedSDEIntegrator built on them.  Run on an MI355X: pytest -m gpu.

Fixtures as tests/test_wide_trace_gpu.py: the two golden 22-atom nets with their 12 walkers (a batch of B walkers is rows
``arange(B) % 12``), a seeded 33-atom net (two waves per item on the matrix pipe) and a seeded 5-atom net (vector pipe
only).  The fp64 oracle is vmap(jacrev) of O.denoiser around O.egnn_ad2_cat_forward, computed once per module.  The item
counts (B * K) of the exactness cases wrap the grid-stride loops on 256 compute units: 1 024 one-wave items (22 atoms),
512 two-wave items (33 atoms)."""
import copy

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _probes as P

pytestmark = pytest.mark.gpu

T = torch.tensor
NETS = {"h64": dict(L=5, tanh=True, att=True), "h48": dict(L=2, tanh=False, att=False)}
KEY = dict(seed=0x5EED0123456789, walker_offset=0, step=7)


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def oracle_jacobian(wd, h, x, beta, n, **kw):
    """(J_x D [B, nd, nd], D [B, nd]) of the fp64 oracle (utils.py:30-51 differentiates the same function)."""
    from torch.func import jacrev, vmap

    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, n, 3, **kw)
    one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
    J = vmap(jacrev(one, argnums=1))(h.double(), x.double(), beta.double())
    return J.numpy(), O.denoiser(bb, h.double(), x.double(), beta.double()).numpy()


def _case(net, n, x, h, beta, **kw):
    wd = {k: v.detach().double() for k, v in net.state_dict().items()}
    J, D = oracle_jacobian(wd, h, x, beta, n, **kw)
    return dict(net=net, n=n, x=x, h=h, beta=beta, J64=J, D64=D, trace64=np.einsum("bii->b", J))


@pytest.fixture(scope="module")
def cases(pa, golden):
    """tag -> module, walkers and the fp64 oracle Jacobian on them (computed once, never modified)."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    out = {}
    for tag, c in NETS.items():
        g = golden(f"egnn_ad2cat_{tag}_fwd.npz")
        w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
        net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=w["egnn.embedding.weight"].shape[0], n_layers=c["L"], tanh=c["tanh"],
                                    attention=c["att"], condition_beta=True)
        net.load_state_dict(w)
        out[tag] = _case(net, 22, T(g["x"]), T(g["h"]), T(g["beta"]), n_layers=c["L"], tanh=c["tanh"], attention=c["att"])
    torch.manual_seed(33)  # the 33-atom net and walkers of test_wide_trace_gpu.py::test_vector_pipe_shape_33_atoms
    net = EGNN_dynamics_AD2_cat(33, 3, hidden_nf=64, n_layers=2, condition_beta=True)
    gen = torch.Generator().manual_seed(34)
    x = O.remove_mean(torch.randn(3, 99, generator=gen), 33, 3)
    out["n33"] = _case(net, 33, x, T([0.05, 0.7, 9.0]), T([1.0, 1.25, 0.8]), n_layers=2, tanh=True, attention=True)
    torch.manual_seed(5)
    h0 = torch.nn.functional.one_hot(T([0, 1, 1, 3, 4])).float()
    net = EGNN_dynamics_AD2_cat(5, 3, hidden_nf=64, n_layers=2, condition_beta=True, h_initial=h0)
    gen = torch.Generator().manual_seed(6)
    x = O.remove_mean(torch.randn(2, 15, generator=gen), 5, 3)
    out["n5"] = _case(net, 5, x, T([0.3, 4.0]), T([1.0, 0.9]), n_layers=2, tanh=True, attention=True, h_initial=h0)
    return out


def batch(c, B, first=0):
    rows = (first + torch.arange(B)) % c["x"].shape[0]
    return rows, c["h"][rows].cuda(), c["x"][rows].cuda(), c["beta"][rows].cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------- 1. the draw
def test_rademacher_draw(pa):
    from pita_amd.utils import rademacher_probes

    key = dict(seed=KEY["seed"], step=KEY["step"])
    v = rademacher_probes(5, 22, 3, 3, walker_offset=0, **key)
    assert v.shape == (3, 5, 66) and v.dtype == torch.float32
    assert bool((v.abs() == 1.0).all())
    assert np.array_equal(v.cpu().numpy(), P.rademacher_probes(5, 22, 3, 3, walker_offset=0, **key))
    big = rademacher_probes(8, 22, 3, 3, walker_offset=0, **key)
    assert torch.equal(big[:, 3:8], rademacher_probes(5, 22, 3, 3, walker_offset=3, **key))  # keyed by global walker
    assert not torch.equal(v, rademacher_probes(5, 22, 3, 3, seed=KEY["seed"] + 1, step=KEY["step"]))
    assert not torch.equal(v, rademacher_probes(5, 22, 3, 3, seed=KEY["seed"], step=KEY["step"] + 1))
    assert not torch.equal(v[0], v[1]) and not torch.equal(v[1], v[2])
    far = dict(seed=2**64 - 3, walker_offset=2**40 + 5, step=2**33 + 1)  # every counter word's high part in use
    assert np.array_equal(rademacher_probes(2, 22, 3, 2, **far).cpu().numpy(), P.rademacher_probes(2, 22, 3, 2, **far))
    many = rademacher_probes(8, 22, 3, 256, **key).double()
    assert bool((many.abs() == 1.0).all())
    mean, count = float(many.mean()), many.numel()
    print(f"[probes/draw] mean over {count} signs {mean:+.3e}, 5 / sqrt(count) = {5 / count ** 0.5:.3e}")
    assert abs(mean) <= 5 / count ** 0.5
    assert rademacher_probes(0, 22, 3, 3).shape == (3, 0, 66)
    with pytest.raises(pa._lib.PitaHipError):
        rademacher_probes(2, 22, 3, 257)


# ------------------------------------------------------------------------------------ 2. per-item exactness, injected probes
EXACT = [("h64", 1, 1), ("h64", 6, 4), ("h64", 5, 256), ("h48", 1, 1), ("h48", 6, 4), ("h48", 5, 256), ("n33", 3, 200),
         ("n5", 2, 3)]


@pytest.mark.parametrize("tag,B,K", EXACT)
def test_per_probe_against_the_fp64_quadratic_forms(pa, cases, tag, B, K):
    """per_probe[k, b] against the fp64 v_k^T J_b v_k with the forward-mode tolerance of
    test_hip_parity.py::test_egnn_ad2cat_forward_mode_vs_oracle_jacobian applied to what is being summed: rtol 5e-5,
    atol 5e-5 (sum_i |(J v)_i| + 1), both from the oracle; the estimate is the fp32 mean of per_probe, D the D of
    jacobian_trace, bit for bit."""
    from pita_amd.utils import rademacher_probes

    c = cases[tag]
    net, n = c["net"], c["n"]
    rows, h, x, beta = batch(c, B)
    assert bool(net.jvp_uses_matrix_pipe("cuda:0")) == (n != 5)
    V = rademacher_probes(B, n, 3, K, **KEY)
    est, D, per = net.jacobian_trace_estimate(h, x, beta, K, probes=V, want_denoiser=True, want_per_probe=True)
    assert est.shape == (B,) and D.shape == (B, 3 * n) and per.shape == (K, B)
    q64, l1 = P.quadratic_forms(c["J64"][rows.numpy()], V.cpu().numpy())
    got = per.cpu().numpy().astype(np.float64)
    bound = 5e-5 * np.abs(q64) + 5e-5 * (l1 + 1.0)
    worst = float((np.abs(got - q64) / bound).max())
    print(f"[probes/exact/{tag}/B={B}/K={K}] max |per_probe - fp64| = {np.abs(got - q64).max():.3e}, "
          f"largest error / bound = {worst:.3f} (mean |q| {np.abs(q64).mean():.3e}, mean sum|Jv| {l1.mean():.3e})")
    assert worst <= 1.0
    assert np.array_equal(est.cpu().numpy().view(np.int32), P.fp32_mean(per.cpu().numpy()).view(np.int32))
    _, D_exact = net.jacobian_trace(h, x, beta, want_denoiser=True)
    assert torch.equal(bits(D), bits(D_exact))
    e2, none, none2 = net.jacobian_trace_estimate(h, x, beta, K, probes=V)  # the estimate alone: same bits
    assert none is None and none2 is None and torch.equal(bits(e2), bits(est))


# ------------------------------------------------------------------------------------------ 3. same item, same tangent
@pytest.mark.parametrize("tag", list(NETS))
def test_per_probe_is_the_dot_product_with_jvps_tangent(pa, cases, tag):
    """<v_k, dout_k> in fp64 from jvp(vx=v_k)'s dout against per_probe[k, b]: within (n d - 1) 2^-24 sum_i |dout_i|, the
    rounding bound of an fp32 sum of n d exact terms (v = +-1: the products are exact)."""
    from pita_amd.utils import rademacher_probes

    c = cases[tag]
    net = c["net"]
    B, K = 6, 4
    _, h, x, beta = batch(c, B)
    V = rademacher_probes(B, 22, 3, K, **KEY)
    _, _, per = net.jacobian_trace_estimate(h, x, beta, K, probes=V, want_per_probe=True)
    for k in range(K):
        _, dout = net.jvp(h, x, beta, vx=V[k], want_primal=False)
        d64, v64 = dout.double().cpu().numpy(), V[k].double().cpu().numpy()
        want, bound = (d64 * v64).sum(-1), 65 * 2.0 ** -24 * np.abs(d64).sum(-1)
        err = np.abs(per[k].double().cpu().numpy() - want)
        print(f"[probes/jvp/{tag}] probe {k}: max err / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (k, err, bound)


# ---------------------------------------------------------------------------------------------------- 4. drawn = injected
@pytest.mark.parametrize("tag", ["h64", "h48", "n33", "n5"])
def test_drawn_probes_have_the_bits_of_injected_ones(pa, cases, tag):
    from pita_amd.utils import rademacher_probes

    c = cases[tag]
    net, n = c["net"], c["n"]
    K = 5
    key = dict(seed=KEY["seed"], step=KEY["step"])
    _, h, x, beta = batch(c, 17)
    drawn = net.jacobian_trace_estimate(h, x, beta, K, walker_offset=0, want_denoiser=True, want_per_probe=True, **key)
    V = rademacher_probes(17, n, 3, K, walker_offset=0, **key)
    fed = net.jacobian_trace_estimate(h, x, beta, K, probes=V, want_denoiser=True, want_per_probe=True)
    for a, b in zip(drawn, fed):
        assert torch.equal(bits(a), bits(b))
    # a walker's bits depend neither on B nor on its row: global walkers 5 .. 10 as a batch of their own
    _, h6, x6, b6 = batch(c, 6, first=5)
    est6, D6, per6 = net.jacobian_trace_estimate(h6, x6, b6, K, walker_offset=5, want_denoiser=True, want_per_probe=True,
                                                 **key)
    assert torch.equal(bits(est6), bits(drawn[0][5:11]))
    assert torch.equal(bits(D6), bits(drawn[1][5:11]))
    assert torch.equal(bits(per6), bits(drawn[2][:, 5:11]))


# ------------------------------------------------------------------------------------------ 5. unbiased, derived bound
@pytest.mark.parametrize("tag", list(NETS))
def test_estimate_is_unbiased_within_the_rademacher_bound(pa, cases, tag):
    """K = 256 drawn probes on the 12 golden walkers: |estimate - trace64| <= 5 sigma_b / sqrt(256) + the fp tolerance of
    test_wide_trace_gpu.py::test_against_the_fp64_oracle, sigma_b^2 = 1/2 sum_{i != j} (J_ij + J_ji)^2 from the oracle
    (a correct kernel exceeds 5 standard errors with probability ~6e-7 per walker).  At K = 4 the estimate must differ
    from the exact trace somewhere: it is an estimate, not the trace under another name."""
    c = cases[tag]
    net = c["net"]
    _, h, x, beta = batch(c, 12)
    est, _, per = net.jacobian_trace_estimate(h, x, beta, 256, want_per_probe=True, **KEY)
    want, sigma = c["trace64"], P.rademacher_sigma(c["J64"])
    fp = 5e-5 * np.abs(want) + 5e-5 * (float(np.abs(want).mean()) + 1.0)
    bound = 5.0 * sigma / 16.0 + fp
    err = np.abs(est.cpu().numpy().astype(np.float64) - want)
    se = per.double().std(0, unbiased=True).cpu().numpy() / 16.0
    print(f"[probes/unbiased/{tag}] |est - trace64| / bound per walker: {np.array2string(err / bound, precision=3)}; "
          f"measured standard error {np.array2string(se, precision=3)} vs sigma_b / 16 {np.array2string(sigma / 16, precision=3)}")
    assert (err <= bound).all(), (err / bound, per.cpu().numpy())
    est4, _, _ = net.jacobian_trace_estimate(h, x, beta, 4, **KEY)
    trace, _ = net.jacobian_trace(h, x, beta)
    assert not torch.equal(est4, trace)


# --------------------------------------------------------------------------------------------------------------- 6. repair
@pytest.mark.parametrize("tag", list(NETS))
def test_out_of_range_items_are_repaired_by_the_vector_pipe(pa, cases, tag, monkeypatch):
    """As test_wide_trace_gpu.py's test of the same name: beta[1] = 1e7 drives walker 1 out of the f16 range; its K items
    and its D row come from the vector-pipe kernel (the bits under PITA_WIDE_NO_MFMA), every other walker keeps its bits."""
    c = cases[tag]
    net = c["net"]
    B, K = 6, 4
    _, h, x, beta = batch(c, B)
    assert net.jvp_uses_matrix_pipe("cuda:0")
    call = lambda b: net.jacobian_trace_estimate(h, x, b, K, want_denoiser=True, want_per_probe=True, **KEY)
    est, D, per = call(beta)
    hot = beta.clone()
    hot[1] = 1.0e7
    est_hot, D_hot, per_hot = call(hot)
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        assert not net.jvp_uses_matrix_pipe("cuda:0")
        est_vec, D_vec, per_vec = call(hot)
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    assert torch.equal(bits(per_hot[:, 1]), bits(per_vec[:, 1]))
    assert torch.equal(bits(D_hot[1]), bits(D_vec[1]))
    assert torch.equal(bits(est_hot[1:2]), bits(est_vec[1:2]))
    keep = torch.arange(B) != 1
    assert torch.equal(bits(per_hot[:, keep]), bits(per[:, keep]))
    assert torch.equal(bits(D_hot[keep]), bits(D[keep])) and torch.equal(bits(est_hot[keep]), bits(est[keep]))


# ----------------------------------------------------------------------------------------------------------- 7. edge cases
def test_empty_batch_and_too_many_drawn_probes(pa, cases):
    c = cases["h64"]
    net = c["net"]
    _, h, x, beta = batch(c, 0)
    est, D, per = net.jacobian_trace_estimate(h, x, beta, 3, want_denoiser=True, want_per_probe=True)
    assert est.shape == (0,) and D.shape == (0, 66) and per.shape == (3, 0)
    _, h, x, beta = batch(c, 2)
    with pytest.raises(pa._lib.PitaHipError):
        net.jacobian_trace_estimate(h, x, beta, 257)  # the drawn path's counter tag holds 256 probes
    with pytest.raises(pa._lib.PitaHipError):
        net.jacobian_trace_estimate(h, x, beta, 0)
    V = torch.ones(257, 2, 66, device="cuda")  # injected probes carry no such limit
    assert net.jacobian_trace_estimate(h, x, beta, 257, probes=V)[0].shape == (2,)


# ------------------------------------------------------------------------------------------ 8. through the SDE, wide backbone
@pytest.mark.parametrize("gamma", [1.0, 4 / 3])
def test_sde_takes_the_estimator_in_one_call(pa, cases, monkeypatch, gamma):
    """VEReverseSDE(divergence="hutchinson", n_probes=4).f on the h64 net as score and energy net at t = 0.15 (the step
    time of test_wide_trace_gpu.py::test_debiased_sde_runs_through_the_single_call).  divergence_score is
    div b = (trace - n d) g^2 / (2 h) WITHOUT the annealing factor (sdes.py:222-227 and pita_fk_assemble multiply it in
    when they form drift_A), so the estimator moves the field by (est - trace) g^2 / (2 h): at gamma = 1 that is the
    gamma (est - trace) g^2 / (2 h) of the estimator's specification to the letter, at gamma = 4/3 it pins that the field
    itself carries no gamma."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
    from pita_amd.energy_net import EnergyNet

    net = cases["h64"]["net"]
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    mk = lambda **kw: pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net),
                                      energy_net=EnergyNet(copy.deepcopy(net)), debias_inference=True, **kw)
    exact, hutch = mk(), mk(divergence="hutchinson", n_probes=4)
    gam = pa.ConstantAnnealingFactorSchedule(gamma)
    gen = torch.Generator().manual_seed(12)
    x = O.remove_mean(torch.randn(5, 66, generator=gen), 22, 3).cuda()
    t = torch.tensor(0.15)
    key = (KEY["seed"], 11, 3)
    calls, exact_calls = [], []
    real, real_exact = EGNN_dynamics_AD2_cat.jacobian_trace_estimate, EGNN_dynamics_AD2_cat.jacobian_trace

    def spy(self, *a, **kw):
        calls.append((self, a[3], kw.get("seed"), kw.get("walker_offset"), kw.get("step")))
        return real(self, *a, **kw)

    def spy_exact(self, *a, **kw):
        exact_calls.append(self)
        return real_exact(self, *a, **kw)

    monkeypatch.setattr(EGNN_dynamics_AD2_cat, "jacobian_trace_estimate", spy)
    monkeypatch.setattr(EGNN_dynamics_AD2_cat, "jacobian_trace", spy_exact)
    f = lambda sde, **kw: sde.f(t.cuda(), x, 1.25, gam, None, None, resampling_interval=1, **kw)
    one = f(hutch, probe_key=key)
    assert calls == [(net, 4, key[0], key[1], key[2])] and exact_calls == []
    ref = f(exact)
    assert len(calls) == 1 and exact_calls == [net]
    for name in ("drift_X", "cross_term", "dUt_dt"):
        assert torch.equal(bits(getattr(one, name)), bits(getattr(ref, name))), name
    assert bool(torch.isfinite(one.drift_A).all())
    ht = sched.h(t.reshape(1)).expand(5).contiguous().cuda()
    beta = torch.full((5,), 1.25, device="cuda")
    est = real(net, ht, x, beta, 4, seed=key[0], walker_offset=key[1], step=key[2])[0].double().cpu().numpy()
    trace = real_exact(net, ht, x, beta)[0].double().cpu().numpy()
    h64, g2 = float(sched.h(t.reshape(1))[0]), float(sched.g(t.reshape(1)).pow(2)[0])
    shift = (est - trace) * g2 / (2.0 * h64)
    got, base = one.divergence_score.double().cpu().numpy(), ref.divergence_score.double().cpu().numpy()
    print(f"[probes/sde/gamma={gamma:.3f}] est - trace {np.array2string(est - trace, precision=4)}; divergence_score moved by "
          f"{np.array2string(got - base, precision=4)}, expected {np.array2string(shift, precision=4)}")
    assert np.abs(shift).max() > 0
    np.testing.assert_allclose(got, base + shift, rtol=1e-5)
    again = f(hutch, probe_key=key)
    for name in ("drift_X", "drift_A", "divergence_score", "cross_term", "dUt_dt"):
        assert torch.equal(bits(getattr(again, name)), bits(getattr(one, name))), name
    other = f(hutch, probe_key=(key[0], key[1], key[2] + 1))
    assert not torch.equal(other.divergence_score, one.divergence_score)
    assert torch.equal(bits(other.drift_X), bits(one.drift_X))


# ------------------------------------------------------------------------------------------ 9. through the SDE, generic fallback
def test_sde_generic_fallback_on_the_hidden32_egnn(pa, golden):
    """Backbones without jacobian_trace_estimate (here the hidden-32 EGNN at 13 particles, golden weights): probes from
    rademacher_probes, K jvp(vx=v_k) launches, the mean of <v_k, dD_k> in the trace's place.  divergence_score against
    the one assembled from the fp64 oracle's v_k^T J v_k for the same probes, by the standard
    test_hip_parity.py::test_debiased_terms_other_systems_vs_oracle sets for this field on this backbone: the rel-L2
    distance from the fp64 oracle may be at most 4 x that of the oracle's own float32 arithmetic (floored by the median
    over the step's fields)."""
    from torch.func import jacrev, vmap

    from pita_amd.energy_net import EnergyNet
    from pita_amd.utils import rademacher_probes

    n, d, B, K = 13, 3, 3, 2
    w = golden("egnn_weights_trainedlike.npz")
    net = pa.EGNN_dynamics(n, d, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True,
                           condition_temperature=True, agg="sum")
    net.load_state_dict({k: T(v) for k, v in w.items()})
    assert not hasattr(net, "jacobian_trace_estimate")
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True, divergence="hutchinson", n_probes=K)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    key = (KEY["seed"], 4, 2)
    V = rademacher_probes(B, n, d, K, seed=key[0], walker_offset=key[1], step=key[2]).cpu().numpy()
    gen = torch.Generator().manual_seed(113)
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
                             / max(np.linalg.norm(np.asarray(b, dtype=np.float64)), 1e-30))
    for tv in (0.15, 0.6):
        hv = float(sched.h(torch.tensor(tv)))
        x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + hv ** 0.5), n, d)
        terms = sde.f(torch.tensor(tv).cuda(), x.cuda(), 1.25, gam, None, None, resampling_interval=1, clamp_chunk=B,
                      probe_key=key)
        refs = {}
        for dt in (torch.float64, torch.float32):
            wt = {k: T(v).to(dt) for k, v in w.items()}
            bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, n, d)
            r = O.f_debiased(bb, bb, osched, ogam, torch.tensor(tv, dtype=dt), x.to(dt), 1.25)
            tb = torch.full((B,), tv, dtype=dt)
            ht, g2 = osched.h(tb), osched.g(tb).pow(2)
            one = lambda h1, x1: O.denoiser(bb, h1[None], x1[None], 1.25)[0]
            J = vmap(jacrev(one, argnums=1))(ht, x.to(dt))
            Vt = T(V).to(dt)
            q = torch.einsum("kbi,bij,kbj->kb", Vt, J, Vt).mean(0)
            r.divergence_score = (q - n * d) / ht * g2 / 2  # the trace of the score's Jacobian, estimated
            refs[dt] = r
        names = ("drift_X", "divergence_score", "cross_term", "dUt_dt")
        e_refs = {nm: rel(getattr(refs[torch.float32], nm), getattr(refs[torch.float64], nm)) for nm in names}
        typical = float(np.median(list(e_refs.values())))
        e_hip = rel(terms.divergence_score.cpu(), refs[torch.float64].divergence_score)
        print(f"[probes/fallback] t = {tv}: divergence_score HIP vs fp64 {e_hip:.2e}, fp32 reference arithmetic vs fp64 "
              f"{e_refs['divergence_score']:.2e} (median over the fields {typical:.2e})")
        assert e_hip <= 4 * max(e_refs["divergence_score"], typical), (tv, e_hip, e_refs)
        assert bool(torch.isfinite(terms.drift_A).all())


# -------------------------------------------------------------------------------------------------------- 10. the integrator
class _Geometry:  # what WeightedSDEIntegrator reads from the target when nothing evaluates it
    n_particles, n_spatial_dim = 22, 3


def test_integrator_is_repeatable_and_leaves_the_exact_regime_alone(pa, cases):
    """integrate_sde on the h64 net, 8 walkers, 3 steps, the Euler-Maruyama noise injected so that the seed reaches the run
    through the probes' Philox stream alone.  Resampling at every step: exact, estimator, estimator, exact again -- the
    estimator runs repeat every bit, the exact runs around them too.  This integrator returns the log-weights AFTER a
    step's resampling has reset them, so with an event at every step they are identically zero; that the estimator's
    noise reaches the log-weights, and changes with the seed, is therefore checked on a second run of the same set-up
    that resamples every other step (rows 0 and 2 carry weights)."""
    from pita_amd.energy_net import EnergyNet

    net = cases["h64"]["net"]
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    gen = torch.Generator().manual_seed(21)
    x1 = (O.remove_mean(torch.randn(8, 66, generator=gen), 22, 3) * 80.0).cuda()
    noise = torch.randn(3, 8, 66, generator=gen).cuda()

    def run(seed, interval, **kw):
        sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                              debias_inference=True, **kw)
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=3, start_resampling_step=0, end_resampling_step=3,
                                         resampling_interval=interval, num_negative_time_steps=0, post_mcmc_steps=0,
                                         batch_size=8, seed=seed)
        x, logw, _, _, _ = integ.integrate_sde(x1, _Geometry(), gam, inverse_temperature=1.0, noise=noise,
                                               resample_u=[0.3, 0.6, 0.9])
        return x, logw

    est = dict(divergence="hutchinson", n_probes=4)
    for interval in (1, 2):
        xe0, we0 = run(3, interval)
        xa, wa = run(3, interval, **est)
        xb, wb = run(3, interval, **est)
        xe1, we1 = run(3, interval)
        assert torch.equal(bits(xa), bits(xb)) and torch.equal(bits(wa), bits(wb)), interval
        assert torch.equal(bits(xe0), bits(xe1)) and torch.equal(bits(we0), bits(we1)), interval
        assert wa.shape == we0.shape == (3, 8) and bool(torch.isfinite(wa).all()) and bool(torch.isfinite(xa).all())
    assert bool((wa[1] == 0).all()) and bool((wa[0] != 0).any()) and bool((wa[2] != 0).any())
    assert not torch.equal(wa[0], we0[0])  # the estimator's noise is in the log-weights
    xc, wc = run(4, 2, **est)
    assert not torch.equal(wc[0], wa[0])  # another seed: other probes
    xe2, we2 = run(4, 2)
    assert torch.equal(bits(we2), bits(we0)) and torch.equal(bits(xe2), bits(xe0))  # ... which the exact regime never draws
