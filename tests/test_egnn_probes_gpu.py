"""pita_egnn_trace_probes / EGNN_dynamics.trace_probes: the Hutchinson estimate of trace(J_x D) on the hidden-32 EGNN with
the probes of a launch sharing one primal evaluation (the multi-direction kernels of the exact trace, probes in the place
of unit vectors), and ``VEReverseSDE(divergence="hutchinson", shared_primal=True)`` built on it.  Run on an MI355X:
pytest -m gpu.

The fp64 truth is vmap(jacrev) of O.denoiser around O.egnn_forward, computed once per system (module fixture, never
modified) together with the same Jacobian in the oracle's float32 arithmetic.  Walkers: the golden LJ13 / DW4 / LJ55
forward walkers (a batch of B walkers is rows ``arange(B) % rows``), seeded ones for 22 particles and the variants.
Shapes are the smallest that reach every group and launch edge: G walkers per wave (13x3: 2, 4x2: 8, else 1) against
B = 1, G, G + 1 and a few groups; K_launch probes per launch (3; 55x3: 1) against K below, at, one above and several
launches with a short last one."""
import copy

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _probes as P

pytestmark = pytest.mark.gpu

T = torch.tensor
KEY = dict(seed=0x5EED0123456789, walker_offset=0, step=7)
PRECISIONS = ["f16x2", "bf16x3", "f32"]  # handle precision 2, 1, 0
KW = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True, agg="sum")


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def bits(t):
    return t.contiguous().view(torch.int32)


def _jacobians(wd, h, x, beta, n, d, **kw):
    """(J64, J32): J_x D per walker from the fp64 oracle and from the same oracle in float32."""
    from torch.func import jacrev, vmap

    out = []
    for dt in (torch.float64, torch.float32):
        w = {k: v.to(dt) for k, v in wd.items()}
        bb = lambda cn, xs, b: O.egnn_forward(w, cn, xs, b, n, d, **kw)
        if beta is None:
            one = lambda hh, xx: O.denoiser(lambda cn, xs, b: bb(cn, xs, None), hh[None], xx[None], 1.0)[0]
            J = vmap(jacrev(one, argnums=1))(h.to(dt), x.to(dt))
        else:
            one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
            J = vmap(jacrev(one, argnums=1))(h.to(dt), x.to(dt), beta.to(dt))
        out.append(J.double().numpy())
    return out


class Case:
    """One particle system / network variant: module factory per precision, walkers and the oracle Jacobians."""

    def __init__(self, make, wd, n, d, x, h, beta, **okw):
        self.make, self.n, self.d, self.x, self.h, self.beta = make, n, d, x, h, beta
        self.J64, self.J32 = _jacobians(wd, h, x, beta, n, d, **okw)
        self.trace64 = np.einsum("bii->b", self.J64)
        self._nets = {}

    def net(self, precision):
        if precision not in self._nets:
            self._nets[precision] = self.make(precision)
        return self._nets[precision]

    def batch(self, B, first=0):
        rows = (first + torch.arange(B)) % self.x.shape[0]
        beta = None if self.beta is None else self.beta[rows].cuda()
        return rows, self.h[rows].cuda(), self.x[rows].cuda(), beta


@pytest.fixture(scope="module")
def cases(pa, golden):
    from pita_amd import egnn

    w = {k: T(v) for k, v in golden("egnn_weights_trainedlike.npz").items()}

    def temp_net(n, d, weights=w, **kw):
        def make(precision):
            net = pa.EGNN_dynamics(n, d, condition_temperature=True, precision=precision, **{**KW, **kw})
            net.load_state_dict({k: v for k, v in weights.items() if k in net.state_dict()})
            return net
        return make

    out = {}
    for tag, n, d, rows in (("lj13", 13, 3, 24), ("dw4", 4, 2, 9), ("lj55", 55, 3, 2)):
        g = golden({"lj13": "egnn_lj13_fwd.npz", "dw4": "egnn_dw4_fwd.npz", "lj55": "egnn_lj55_fwd.npz"}[tag])
        out[tag] = Case(temp_net(n, d), w, n, d, T(g["x"])[:rows], T(g["h"])[:rows], T(g["beta"])[:rows])
    gen = torch.Generator().manual_seed(22)
    h22 = T([0.3, 2.5])
    x22 = O.remove_mean(torch.randn(2, 66, generator=gen) * (1 + h22.sqrt())[:, None], 22, 3)
    out["n22"] = Case(temp_net(22, 3), w, 22, 3, x22, h22, T([1.0, 1.25]))
    # variants at 13x3 on three of the golden walkers (one small, one middling, one large h)
    g = golden("egnn_lj13_fwd.npz")
    order = np.argsort(g["h"])
    pick = [int(order[1]), int(order[len(order) // 2]), int(order[-2])]
    x3, h3, b3 = T(g["x"])[pick], T(g["h"])[pick], T(g["beta"])[pick]
    out["no_attention"] = Case(temp_net(13, 3, attention=False), w, 13, 3, x3, h3, b3, attention=False)
    out["no_tanh"] = Case(temp_net(13, 3, tanh=False), w, 13, 3, x3, h3, b3, tanh=False)
    out["correct"] = Case(temp_net(13, 3, feature_layout="correct"), w, 13, 3, x3, h3, b3, feature_layout="correct")
    # time-only (egnn.py): the golden weights with the embedding cut to its time column
    wt = dict(w)
    wt["egnn.embedding.weight"] = w["egnn.embedding.weight"][:, :1].clone()
    wt["egnn.embedding_out.weight"] = w["egnn.embedding_out.weight"][:1].clone()
    wt["egnn.embedding_out.bias"] = w["egnn.embedding_out.bias"][:1].clone()

    def make_time_only(precision):
        net = egnn.EGNN_dynamics(13, 3, precision=precision, **KW)
        net.load_state_dict(wt)
        return net

    out["time_only"] = Case(make_time_only, wt, 13, 3, x3, h3, None)
    return out


def _ratio(got, q64, l1):
    bound = 5e-5 * np.abs(q64) + 5e-5 * (l1 + 1.0)
    return float((np.abs(np.asarray(got, dtype=np.float64) - q64) / bound).max())


def _check_call(c, net, B, K, V, label):
    """One call with injected probes V [K, B, nd] against the fp64 quadratic forms; returns per_probe."""
    rows, h, x, beta = c.batch(B)
    est, D, per = net.trace_probes(h, x, beta, K, probes=V, want_denoiser=True, want_per_probe=True)
    assert est.shape == (B,) and D.shape == (B, c.n * c.d) and per.shape == (K, B)
    Vn = V.cpu().numpy()
    q64, l1 = P.quadratic_forms(c.J64[rows.numpy()], Vn)
    q32, _ = P.quadratic_forms(c.J32[rows.numpy()], Vn)
    jv = np.empty((K, B))
    for k in range(K):  # the K-launch path's numbers for the same probes
        _, dout = net.jvp(h, x, beta, vx=V[k], want_primal=False)
        jv[k] = (dout.double().cpu().numpy() * Vn[k].astype(np.float64)).sum(-1)
    worst = _ratio(per.cpu().numpy(), q64, l1)
    print(f"[egnn-probes/{label}/B={B}/K={K}] largest error / bound: trace_probes {worst:.3f}, <v, jvp dout> "
          f"{_ratio(jv, q64, l1):.3f}, fp32 oracle {_ratio(q32, q64, l1):.3f} (mean |q| {np.abs(q64).mean():.3e})")
    assert worst <= 1.0
    assert np.array_equal(est.cpu().numpy().view(np.int32), P.fp32_mean(per.cpu().numpy()).view(np.int32))
    _, D_exact = net.jacobian_trace(h, x, beta, want_denoiser=True)
    assert torch.equal(bits(D), bits(D_exact))
    e2, none, none2 = net.trace_probes(h, x, beta, K, probes=V)  # the estimate alone (handle-owned q): same bits
    assert none is None and none2 is None and torch.equal(bits(e2), bits(est))
    return per


# ---------------------------------------------------------------------------------------- 1. per probe against fp64
SHAPES = {"lj13": ([1, 2, 3, 9], [1, 3, 4, 7]), "dw4": ([1, 8, 9], [2, 5]), "n22": ([2], [4]), "lj55": ([2], [2])}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", list(SHAPES))
def test_per_probe_against_the_fp64_quadratic_forms(pa, cases, tag, precision):
    """per_probe[k, b] against the fp64 v_k^T J_b v_k with the project's forward-mode tolerance as
    test_wide_probes_gpu.py::test_per_probe_against_the_fp64_quadratic_forms applies it: 5e-5 |q| + 5e-5 (sum_i |(J v)_i|
    + 1), both from the oracle; the estimate is the fp32 mean of per_probe, D the D of jacobian_trace, bit for bit."""
    from pita_amd.utils import rademacher_probes

    c = cases[tag]
    net = c.net(precision)
    assert net.precision == {"f16x2": 2, "bf16x3": 1, "f32": 0}[precision]
    for B in SHAPES[tag][0]:
        for K in SHAPES[tag][1]:
            V = rademacher_probes(B, c.n, c.d, K, **KEY)
            _check_call(c, net, B, K, V, f"{tag}/{precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["no_attention", "no_tanh", "time_only", "correct"])
def test_per_probe_network_variants(pa, cases, tag, precision):
    from pita_amd.utils import rademacher_probes

    c = cases[tag]
    V = rademacher_probes(3, 13, 3, 4, **KEY)
    _check_call(c, c.net(precision), 3, 4, V, f"{tag}/{precision}")


# ------------------------------------------------------------------------------------ 2. probes that are not signs
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gaussian_probes_meet_the_same_bound(pa, cases, precision):
    """Gaussian values in every probe entry: a read-out that assumed v^2 = 1 (c_s n d in the place of c_s |v|^2) or a
    seed that took the sign alone would miss the fp64 quadratic form by far more than the bound."""
    c = cases["lj13"]
    gen = torch.Generator().manual_seed(77)
    V = torch.randn(3, 3, 39, generator=gen).cuda()
    _check_call(c, c.net(precision), 3, 3, V, f"gaussian/{precision}")


# ---------------------------------------------------------------------------------------------- 3. drawn = injected
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["lj13", "dw4", "lj55"])
def test_drawn_probes_have_the_bits_of_injected_ones(pa, cases, tag, precision):
    from pita_amd.utils import rademacher_probes

    c = cases[tag]
    net = c.net(precision)
    K = 5
    key = dict(seed=KEY["seed"], step=KEY["step"])
    call = lambda B, first=0, K=K, **kw: net.trace_probes(*c.batch(B, first)[1:], K, want_denoiser=True,
                                                          want_per_probe=True, **kw)
    drawn = call(17, walker_offset=0, **key)
    V = rademacher_probes(17, c.n, c.d, K, walker_offset=0, **key)
    fed = call(17, probes=V)
    for a, b in zip(drawn, fed):
        assert torch.equal(bits(a), bits(b))
    # a walker's bits depend neither on B nor on its row: global walkers 5 .. 10 as a batch of their own
    est6, D6, per6 = call(6, first=5, walker_offset=5, **key)
    assert torch.equal(bits(est6), bits(drawn[0][5:11]))
    assert torch.equal(bits(D6), bits(drawn[1][5:11]))
    assert torch.equal(bits(per6), bits(drawn[2][:, 5:11]))
    # ... nor on how many probes the call carries or the launch slot a probe lands in
    _, D4, per4 = call(17, K=4, walker_offset=0, **key)
    assert torch.equal(bits(per4), bits(drawn[2][:4])) and torch.equal(bits(D4), bits(drawn[1]))


# ------------------------------------------------------------------------------------------------------ 4. unbiased
@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_estimate_is_unbiased_within_the_rademacher_bound(pa, cases, precision):
    """K = 256 drawn probes on 12 golden LJ13 walkers: |estimate - trace64| <= 5 sigma_b / sqrt(256) + the fp tolerance of
    the exact trace, sigma_b^2 = 1/2 sum_{i != j} (J_ij + J_ji)^2 from the oracle (a correct kernel exceeds 5 standard
    errors with probability ~6e-7 per walker).  At K = 4 the estimate must differ from the exact trace somewhere."""
    c = cases["lj13"]
    net = c.net(precision)
    _, h, x, beta = c.batch(12)
    est, _, per = net.trace_probes(h, x, beta, 256, want_per_probe=True, **KEY)
    want, sigma = c.trace64[:12], P.rademacher_sigma(c.J64[:12])
    fp = 5e-5 * np.abs(want) + 5e-5 * (float(np.abs(want).mean()) + 1.0)
    bound = 5.0 * sigma / 16.0 + fp
    err = np.abs(est.cpu().numpy().astype(np.float64) - want)
    se = per.double().std(0, unbiased=True).cpu().numpy() / 16.0
    print(f"[egnn-probes/unbiased/{precision}] |est - trace64| / bound per walker: {np.array2string(err / bound, precision=3)}; "
          f"measured standard error {np.array2string(se, precision=3)} vs sigma_b / 16 {np.array2string(sigma / 16, precision=3)}")
    assert (err <= bound).all(), (err / bound)
    est4, _, _ = net.trace_probes(h, x, beta, 4, **KEY)
    trace = net.jacobian_trace(h, x, beta)
    assert not torch.equal(est4, trace)


# -------------------------------------------------------------------------------------------------- 5. range repair
def test_out_of_range_walkers_are_repaired_by_the_bf16_kernel(pa, cases):
    """Walkers with pair distances of 10^3 (test_hip_parity.py::test_jacobian_trace_out_of_range_walkers_fall_back_to_bf16)
    leave the f16 range: the f16 kernel marks them and the bf16x3 kernel recomputes exactly those -- they get the bits of a
    precision-1 handle's call, their neighbours (one of them shares a wave's walker group with an out-of-range walker)
    keep the bits they have in a call without them."""
    c = cases["lj13"]
    nf, nb = c.net("f16x2"), c.net("bf16x3")
    gen = torch.Generator().manual_seed(5)
    B, K = 11, 4
    far = torch.zeros(B, dtype=torch.bool)
    far[[4, 7, 8]] = True  # 4: second walker of a group, 7 / 8: end of one group and start of the next
    x = torch.randn(B, 39, generator=gen)
    x[far] *= 2000.0
    x = O.remove_mean(x, 13, 3).cuda()
    h, b = torch.full((B,), 0.02).cuda(), torch.ones(B).cuda()
    call = lambda net, rows: net.trace_probes(h[rows], x[rows], b[rows], K, want_denoiser=True, want_per_probe=True,
                                              seed=KEY["seed"], step=KEY["step"], walker_offset=0)
    every = torch.arange(B)
    ef, Df, pf = call(nf, every)
    eb, Db, pb = call(nb, every)
    assert bool(torch.isfinite(ef).all()) and bool(torch.isfinite(Df).all()) and bool(torch.isfinite(pf).all())
    assert torch.equal(bits(pf[:, far]), bits(pb[:, far])) and torch.equal(bits(ef[far]), bits(eb[far]))
    assert torch.equal(bits(Df[far]), bits(Db[far]))
    near = ~far
    # (that a precision-2 handle runs arithmetic of its own where nothing is out of range: the golden walkers)
    _, hg, xg, bg = c.batch(12)
    pg = [net.trace_probes(hg, xg, bg, K, want_per_probe=True, **KEY)[2] for net in (nf, nb)]
    assert not torch.equal(pg[0], pg[1])
    # the neighbours alone, probes injected so that every walker keeps its own: same bits
    from pita_amd.utils import rademacher_probes

    V = rademacher_probes(B, 13, 3, K, seed=KEY["seed"], step=KEY["step"], walker_offset=0)
    en, Dn, pn = nf.trace_probes(h[near], x[near], b[near], K, probes=V[:, near].contiguous(), want_denoiser=True,
                                 want_per_probe=True)
    assert torch.equal(bits(pn), bits(pf[:, near])) and torch.equal(bits(en), bits(ef[near]))
    assert torch.equal(bits(Dn), bits(Df[near]))


# ----------------------------------------------------------------------------------------------------------- 6. edges
def test_empty_batch_probe_limits_and_unsupported_systems(pa, cases):
    c = cases["lj13"]
    net = c.net("f16x2")
    _, h, x, beta = c.batch(0)
    est, D, per = net.trace_probes(h, x, beta, 3, want_denoiser=True, want_per_probe=True)
    assert est.shape == (0,) and D.shape == (0, 39) and per.shape == (3, 0)
    _, h, x, beta = c.batch(2)
    with pytest.raises(pa._lib.PitaHipError):
        net.trace_probes(h, x, beta, 257)  # the drawn path's counter tag holds 256 probes
    with pytest.raises(pa._lib.PitaHipError):
        net.trace_probes(h, x, beta, 0)
    V = torch.ones(257, 2, 39, device="cuda")  # injected probes carry no such limit
    assert net.trace_probes(h, x, beta, 257, probes=V)[0].shape == (2,)
    with pytest.raises(ValueError):
        net.trace_probes(h, x, beta, 3, probes=V)
    torch.manual_seed(5)
    odd = pa.EGNN_dynamics(5, 3, condition_temperature=True, **KW)  # no multi-direction kernel for 5 particles
    assert odd.trace_probes(torch.ones(2).cuda(), torch.randn(2, 15).cuda(), torch.ones(2).cuda(), 3) is None


# ------------------------------------------------------------------------------------------------ 7. through the SDE
def test_sde_takes_trace_probes_under_shared_primal(pa, golden, monkeypatch):
    """The set-up of test_wide_probes_gpu.py::test_sde_generic_fallback_on_the_hidden32_egnn with shared_primal=True:
    divergence_score against the one assembled from the fp64 oracle's v_k^T J v_k for the same probes by that test's own
    standard (rel-L2 distance from fp64 at most 4 x max(the fp32 oracle's, the median over the step's fields));
    drift_X, cross_term and dUt_dt by the standard of test_hip_parity.py::test_debiased_terms_other_systems_vs_oracle
    (the same rule per field).  One trace_probes call and no jvp call per f; with the default False trace_probes is
    never called."""
    from torch.func import jacrev, vmap

    from pita_amd.egnn_temp_conditioned import EGNN_dynamics
    from pita_amd.energy_net import EnergyNet
    from pita_amd.utils import rademacher_probes

    n, d, B, K = 13, 3, 3, 2
    w = golden("egnn_weights_trainedlike.npz")
    net = pa.EGNN_dynamics(n, d, condition_temperature=True, **KW)
    net.load_state_dict({k: T(v) for k, v in w.items()})
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    mk = lambda **kw: pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net),
                                      energy_net=EnergyNet(copy.deepcopy(net)), debias_inference=True,
                                      divergence="hutchinson", n_probes=K, **kw)
    sde, plain = mk(shared_primal=True), mk()
    calls, jvps = [], []
    real, real_jvp = EGNN_dynamics.trace_probes, EGNN_dynamics.jvp

    def spy(self, *a, **kw):
        calls.append((self, a[3], kw.get("seed"), kw.get("walker_offset"), kw.get("step")))
        return real(self, *a, **kw)

    def spy_jvp(self, *a, **kw):
        jvps.append(self)
        return real_jvp(self, *a, **kw)

    monkeypatch.setattr(EGNN_dynamics, "trace_probes", spy)
    monkeypatch.setattr(EGNN_dynamics, "jvp", spy_jvp)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    key = (KEY["seed"], 4, 2)
    V = rademacher_probes(B, n, d, K, seed=key[0], walker_offset=key[1], step=key[2]).cpu().numpy()
    gen = torch.Generator().manual_seed(113)
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
                             / max(np.linalg.norm(np.asarray(b, dtype=np.float64)), 1e-30))
    for tv in (0.15, 0.6):
        hv = float(sched.h(torch.tensor(tv)))
        x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + hv ** 0.5), n, d)
        f = lambda s, k=key: s.f(torch.tensor(tv).cuda(), x.cuda(), 1.25, gam, None, None, resampling_interval=1,
                                 clamp_chunk=B, probe_key=k)
        del calls[:], jvps[:]
        terms = f(sde)
        assert calls == [(net, K, key[0], key[1], key[2])] and jvps == []
        f(plain)
        assert len(calls) == 1 and len(jvps) == K  # the default: the K-launch path, trace_probes never called
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
        for nm in names:
            e_hip = rel(getattr(terms, nm).cpu(), getattr(refs[torch.float64], nm))
            print(f"[egnn-probes/sde] t = {tv}: {nm:16s} HIP vs fp64 {e_hip:.2e}, fp32 reference arithmetic vs fp64 "
                  f"{e_refs[nm]:.2e} (median over the fields {typical:.2e})")
            assert e_hip <= 4 * max(e_refs[nm], typical), (tv, nm, e_hip, e_refs)
        assert bool(torch.isfinite(terms.drift_A).all())
        again = f(sde)
        for nm in names + ("drift_A",):
            assert torch.equal(bits(getattr(again, nm)), bits(getattr(terms, nm))), nm
        other = f(sde, (key[0], key[1], key[2] + 1))
        assert not torch.equal(other.divergence_score, terms.divergence_score)
        assert torch.equal(bits(other.drift_X), bits(terms.drift_X))


# ---------------------------------------------------------------------------------------------------- 8. the integrator
class _Geometry:  # what WeightedSDEIntegrator reads from the target when nothing evaluates it
    n_particles, n_spatial_dim = 13, 3


def test_integrator_is_repeatable_and_leaves_the_exact_regime_alone(pa, cases):
    """integrate_sde on the golden LJ13 net, 8 walkers, 3 steps, an event every other step, the Euler-Maruyama noise
    injected so that the seed reaches the run through the probes' Philox stream alone: exact, estimator, estimator, exact
    again -- the estimator runs repeat every bit, the exact runs around them too; another seed changes the log-weights of
    the estimator and nothing of the exact regime."""
    from pita_amd.energy_net import EnergyNet

    net = cases["lj13"].net("f16x2")
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    gen = torch.Generator().manual_seed(21)
    x1 = (O.remove_mean(torch.randn(8, 39, generator=gen), 13, 3) * 80.0).cuda()
    noise = torch.randn(3, 8, 39, generator=gen).cuda()

    def run(seed, **kw):
        sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                              debias_inference=True, **kw)
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=3, start_resampling_step=0, end_resampling_step=3,
                                         resampling_interval=2, num_negative_time_steps=0, post_mcmc_steps=0,
                                         batch_size=8, seed=seed)
        x, logw, _, _, _ = integ.integrate_sde(x1, _Geometry(), gam, inverse_temperature=1.0, noise=noise,
                                               resample_u=[0.3, 0.6, 0.9])
        return x, logw

    est = dict(divergence="hutchinson", n_probes=4, shared_primal=True)
    xe0, we0 = run(3)
    xa, wa = run(3, **est)
    xb, wb = run(3, **est)
    xe1, we1 = run(3)
    assert torch.equal(bits(xa), bits(xb)) and torch.equal(bits(wa), bits(wb))
    assert torch.equal(bits(xe0), bits(xe1)) and torch.equal(bits(we0), bits(we1))
    assert wa.shape == we0.shape == (3, 8) and bool(torch.isfinite(wa).all()) and bool(torch.isfinite(xa).all())
    assert not torch.equal(wa[0], we0[0])  # the estimator's noise is in the log-weights
    xc, wc = run(4, **est)
    assert not torch.equal(wc[0], wa[0])  # another seed: other probes
    xe2, we2 = run(4)
    assert torch.equal(bits(we2), bits(we0)) and torch.equal(bits(xe2), bits(xe0))  # ... which the exact regime never draws
