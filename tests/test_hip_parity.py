"""GPU parity tests: the HIP path (through the C ABI / pita_amd façade) against the CPU oracle
and the golden vectors produced by the reference.  Run on an MI355X: pytest -m gpu.

Tolerances (fp32, stated per test): target energies rel 1e-5 (logp) / rel-L2 1e-5 (force) on
physical configurations; EGNN backbone rel-L2 2e-5 vs the fp32 reference and within 4x the
reference's own fp32-vs-fp64 error; per-step drift rel-L2 1e-4 at identical inputs; integer
index work (resampling ids) exact except where a uniform falls within fp32 rounding of a bin
edge (counted, must be < 0.5 %, always off by one).
"""
import os

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = torch.tensor


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def cu(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).cuda()


# ------------------------------------------------------------------------------- energies
@pytest.mark.parametrize("n", [13, 55])
def test_lj_golden(pa, golden, n):
    g = golden(f"lj{n}_logp_force.npz")
    nphys = int(g["n_cold"]) + int(g["n_warm"])
    x = cu(g["x"])
    for Tk in (1.0, 2.0, 4.0):
        e = pa.LennardJonesEnergy(3 * n, n, 3, temperature=Tk)
        lp = e(x)
        lp2, f = e(x, return_force=True)
        assert torch.equal(lp, lp2)
        np.testing.assert_allclose(lp.cpu().numpy()[:nphys], g[f"logp_T{Tk}"][:nphys], rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(lp.cpu().numpy()[nphys:], g[f"logp_T{Tk}"][nphys:], rtol=2e-5)  # |E| ~ 1e6+
        assert rel(f[:nphys], g[f"force_T{Tk}"][:nphys]) < 1e-5
        assert rel(f[nphys:], g[f"force_T{Tk}"][nphys:]) < 1e-4
    e = pa.LennardJonesEnergy(3 * n, n, 3, temperature=1.0, energy_factor=0.5)
    lp, f = e(x, return_force=True)
    np.testing.assert_allclose(lp.cpu().numpy()[:nphys], g["logp_ef0.5"][:nphys], rtol=1e-5, atol=2e-5)
    assert rel(f[:nphys], g["force_ef0.5"][:nphys]) < 1e-5


def test_lj13_ring_instantiation_golden(pa, golden, monkeypatch):
    """The lane-per-particle instantiation of the LJ13 target (Ring<13, 3>: a walker on a DPP row of 16 lanes, four
    walkers per wave; PITA_LJ13_RING=1 -- the round-4 experiment of DESIGN 4.2, slower than the lane-per-walker kernels at
    every batch size and therefore not the route) against the same reference goldens, ragged batch sizes included."""
    g = golden("lj13_logp_force.npz")
    nphys = int(g["n_cold"]) + int(g["n_warm"])
    x = cu(g["x"])
    e = pa.LennardJonesEnergy(39, 13, 3)
    lp0, f0 = e(x, return_force=True)
    monkeypatch.setenv("PITA_LJ13_RING", "1")
    lp, f = e(x, return_force=True)
    assert not torch.equal(f, f0)  # a different kernel really ran
    np.testing.assert_allclose(lp.cpu().numpy()[:nphys], g["logp_T1.0"][:nphys], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(lp.cpu().numpy()[nphys:], g["logp_T1.0"][nphys:], rtol=2e-5)
    assert rel(f[:nphys], g["force_T1.0"][:nphys]) < 1e-5 and rel(f[nphys:], g["force_T1.0"][nphys:]) < 1e-4
    for n in (1, 3, 4, 5, 63):
        lpn, fn = e(x[:n].contiguous(), return_force=True)
        assert torch.equal(lpn, lp[:n]) and torch.equal(fn, f[:n]), n
    big = x[:nphys].repeat(720, 1)[:40001].contiguous()  # more groups than resident waves: the prefetching loop
    lpb, fb = e(big, return_force=True)
    idx = (torch.arange(40001) % nphys).cuda()
    assert torch.equal(lpb, lp[idx]) and torch.equal(fb, f[idx])


def test_lj13_against_reference_held_energy2(pa, golden):
    """A12 against reference-held code only: ``energy2`` of sampling/sample_lj13.py:24-30 executed as shipped in
    make_golden.py (torch.pdist, no distance eps; force by autograd).  The HIP kernel with the bgflow eps of 1e-6 is
    within 2e-4 of it (the eps term); with dist_eps = 0 it is the same function: rel 1e-5 like the other goldens."""
    g = golden("lj13_logp_force.npz")
    nphys = int(g["n_cold"]) + int(g["n_warm"])
    x = cu(g["x"])
    lp, f = pa.LennardJonesEnergy(39, 13, 3)(x, return_force=True)
    np.testing.assert_allclose(lp.cpu().numpy(), g["energy2_logp_f32"], rtol=2e-4)
    assert rel(f[:nphys], g["energy2_force_f32"][:nphys]) < 2e-4
    e0 = pa.LennardJonesEnergy(39, 13, 3)
    e0.dist_eps = 0.0
    lp0, f0 = e0(x, return_force=True)
    np.testing.assert_allclose(lp0.cpu().numpy()[:nphys], g["energy2_logp_f64"][:nphys], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(lp0.cpu().numpy()[nphys:], g["energy2_logp_f64"][nphys:], rtol=2e-5)
    assert rel(f0[:nphys], g["energy2_force_f64"][:nphys]) < 1e-5
    assert rel(f0[nphys:], g["energy2_force_f64"][nphys:]) < 1e-4


def test_lj_smooth_core_golden(pa, golden):
    """LennardJonesEnergy(smooth=True): cubic core below r = 0.65, against the reference's log-density and autograd force
    (walkers with and without pairs inside the core), for LJ13 and, against the oracle, LJ55 / ragged batches."""
    g = golden("lj13_smooth_logp_force.npz")
    coef, r0 = pa.lennardjones_energy.smooth_core_coefficients()
    np.testing.assert_array_equal(coef, g["spline_c0"])
    assert np.float32(r0) == g["spline_x0"][0]
    x = cu(g["x"])
    for Tk, ef in ((1.0, 1.0), (2.0, 0.5)):
        e = pa.LennardJonesEnergy(39, 13, 3, temperature=Tk, energy_factor=ef, smooth=True)
        lp = e(x)
        lp2, f = e(x, return_force=True)
        assert torch.equal(lp, lp2)
        np.testing.assert_allclose(lp.cpu().numpy(), g[f"logp_T{Tk}_ef{ef}"], rtol=1e-5, atol=2e-5)
        assert rel(f, g[f"force_T{Tk}_ef{ef}"]) < 1e-5
        assert e.fused_descent(x.clone(), 1, 1e-3, 0.0, 1.0) is None  # fused loops know the plain curve only
    gen = torch.Generator().manual_seed(11)
    for n, B in ((13, 1), (13, 21), (55, 37)):
        xo = torch.randn(B, 3 * n, generator=gen) * 0.5 + torch.linspace(-1.5, 1.5, 3 * n)[None]
        lp_o, f_o = O.lj_smooth_logp_force(xo, n, 3, temperature=1.5)
        e = pa.LennardJonesEnergy(3 * n, n, 3, temperature=1.5, smooth=True)
        lp, f = e(xo.cuda(), return_force=True)
        np.testing.assert_allclose(lp.cpu().numpy(), lp_o.numpy(), rtol=2e-5)
        assert rel(f, f_o) < 2e-5


def test_lj_vs_oracle_random_and_edges(pa):
    gen = torch.Generator().manual_seed(3)
    for n, B in ((13, 1000), (13, 1), (13, 19), (13, 20), (55, 37)):
        x = torch.randn(B, 3 * n, generator=gen) * 0.6 + torch.linspace(-2, 2, 3 * n)[None]
        lp_o, f_o = O.lj_logp_force(x.double(), n, 3, temperature=1.5)
        e = pa.LennardJonesEnergy(3 * n, n, 3, temperature=1.5)
        lp, f = e(x.cuda(), return_force=True)
        np.testing.assert_allclose(lp.cpu().numpy(), lp_o.numpy(), rtol=2e-5)
        assert rel(f, f_o) < 2e-5
    e = pa.LennardJonesEnergy(39, 13, 3)
    lp, f = e(torch.empty(0, 39).cuda(), return_force=True)  # empty batch
    assert lp.shape == (0,) and f.shape == (0, 39)
    with pytest.raises(pa._lib.PitaHipError):
        e(torch.zeros(4, 39))  # CPU tensor: no fallback, must fail loudly


def test_lj13_large_batch_streaming_kernel(pa, monkeypatch):
    """Beyond 262 144 walkers pita_lj_logp_force runs persistent blocks that keep the next tile's coordinates in flight
    (lj13_stream_kernel): same tile arithmetic as the plain one-lane-per-walker kernel -> bit-identical to it
    (PITA_LJ13_NO_STREAM=1 selects the plain kernel), ragged last tile included, and equal to the oracle."""
    gen = torch.Generator().manual_seed(8)
    B = 262144 + 300 + 77
    x = (torch.randn(B, 39, generator=gen) * 0.6 + torch.linspace(-2, 2, 39)[None]).cuda()
    e = pa.LennardJonesEnergy(39, 13, 3, temperature=1.5)
    lp, f = e(x, return_force=True)
    monkeypatch.setenv("PITA_LJ13_NO_STREAM", "1")
    lp0, f0 = e(x, return_force=True)
    monkeypatch.delenv("PITA_LJ13_NO_STREAM")
    assert torch.equal(lp, lp0) and torch.equal(f, f0)
    assert torch.equal(e(x), lp)  # force == NULL path
    idx = torch.cat([torch.arange(0, B, 4099), torch.arange(B - 400, B, 7)])
    lp_o, f_o = O.lj_logp_force(x[idx.cuda()].cpu().double(), 13, 3, temperature=1.5)
    np.testing.assert_allclose(lp[idx.cuda()].cpu().numpy(), lp_o.numpy(), rtol=2e-5)
    assert rel(f[idx.cuda()], f_o) < 2e-5


@pytest.mark.parametrize("name", ["lj55", "dw4"])
def test_ring_kernels_edge_cases(pa, name):
    """Ring kernels (compile-time particle count, lane = particle): empty batch, one walker, batches that leave the last
    wave group ragged (DW4: 16 walkers per wave), determinism, translation invariance of the pair part, zero net force,
    the energy_factor / temperature / (LJ) non-unit rm variants against the oracle, and a walker with a non-finite
    coordinate that must not disturb its neighbours in the same wave."""
    gen = torch.Generator().manual_seed(21)
    if name == "lj55":
        n, d = 55, 3
        mk = lambda **kw: pa.LennardJonesEnergy(165, 55, 3, **kw)
        orc = lambda x, T=1.0, ef=1.0: O.lj_logp_force(x, 55, 3, temperature=T, energy_factor=ef)
        base = torch.randn(1, 165, generator=gen) * 0.9 + torch.linspace(-2.5, 2.5, 165)[None]
    else:
        n, d = 4, 2
        mk = lambda **kw: pa.MultiDoubleWellEnergy(**kw)
        orc = lambda x, T=1.0, ef=1.0: O.dw4_logp_force(x, temperature=T)
        base = torch.tensor([[2.0, 2.0, -2.0, 2.0, -2.0, -2.0, 2.0, -2.0]])
    D = n * d
    e = mk()
    lp, f = e(torch.empty(0, D).cuda(), return_force=True)
    assert lp.shape == (0,) and f.shape == (0, D)
    for B in (1, 2, 15, 16, 17, 63, 65, 1000):
        x = base + 0.25 * torch.randn(B, D, generator=gen)
        lp, f = e(x.cuda(), return_force=True)
        lp2, f2 = e(x.cuda(), return_force=True)
        assert torch.equal(lp, lp2) and torch.equal(f, f2) and torch.equal(e(x.cuda()), lp)
        lpo, fo = orc(x.double())
        np.testing.assert_allclose(lp.cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=2e-5)
        assert rel(f, fo) < 2e-5
        # a walker's value does not depend on where it sits in the batch / wave group
        if B > 2:
            lp3, f3 = e(x[1:].contiguous().cuda(), return_force=True)
            assert torch.equal(lp3, lp[1:]) and torch.equal(f3, f[1:])
        fsum = f.reshape(B, n, d).sum(1).abs().max().item()
        if name == "dw4":
            assert fsum < 1e-4 * max(1.0, f.abs().max().item())  # pair forces cancel exactly up to rounding
    x = (base + 0.2 * torch.randn(40, D, generator=gen)).cuda()
    for T, ef in ((2.5, 1.0), (0.7, 0.5)):
        kw = dict(temperature=T) if name == "dw4" else dict(temperature=T, energy_factor=ef)
        lp, f = mk(**kw)(x, return_force=True)
        lpo, fo = orc(x.cpu().double(), T, ef)
        np.testing.assert_allclose(lp.cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=2e-5)
        assert rel(f, fo) < 2e-5
    if name == "lj55":  # non-unit rm / eps / oscillator scale through the C ABI (the plug-in class always passes 1)
        lp = torch.empty(40, device="cuda")
        f = torch.empty_like(x)
        pa._lib.check(pa._lib.lib().pita_lj_logp_force(x.data_ptr(), lp.data_ptr(), f.data_ptr(), 40, 55, 3, 1.7, 0.8, 1e-6, 0.7, 1.1,
                                                       0.5, pa._lib.stream_ptr()), "pita_lj_logp_force")
        lpo, fo = O.lj_logp_force(x.cpu().double(), 55, 3, temperature=1.7, energy_factor=0.8, eps=0.7, rm=1.1, osc_scale=0.5)
        np.testing.assert_allclose(lp.cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=2e-5)
        assert rel(f, fo) < 2e-5
    xb = x.clone()
    xb[17, 3] = float("nan")
    lpb, fb = e(xb, return_force=True)
    lp, f = e(x, return_force=True)
    keep = torch.ones(40, dtype=torch.bool, device="cuda")
    keep[17] = False
    assert torch.equal(lpb[keep], lp[keep]) and torch.equal(fb[keep], f[keep]) and not torch.isfinite(lpb[17])


def test_dw4_vs_oracle(pa):
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(513, 8, generator=gen) * 2.5
    lp_o, f_o = O.dw4_logp_force(x.double(), temperature=2.0)
    e = pa.MultiDoubleWellEnergy(temperature=2.0)
    lp, f = e(x.cuda(), return_force=True)
    np.testing.assert_allclose(lp.cpu().numpy(), lp_o.numpy(), rtol=1e-5, atol=1e-5)
    assert rel(f, f_o) < 1e-5


def test_gmm_golden(pa, golden):
    g = golden("gmm40.npz")
    x = cu(g["x"])
    for Tk in (1.0, 2.0):
        e = pa.GMM(temperature=Tk)
        np.testing.assert_array_equal(e.locs.cpu().numpy(), g["means"])
        np.testing.assert_allclose(e(x).cpu().numpy(), g[f"logp_T{Tk}"], rtol=3e-6, atol=3e-5)
    lp, grad = pa.GMM()(x, return_force=True)
    np.testing.assert_allclose(grad.cpu().numpy(), g["grad_T1.0"], rtol=3e-5, atol=2e-5)


def _guarded_targets(pa):
    """(target, x [17, D] on cuda:0) of the three classes that took the device guard with the HipTarget mix-in."""
    gen = torch.Generator().manual_seed(17)
    lj = torch.tensor(np.load(os.path.join(ROOT, "tests", "golden", "lj13_logp_force.npz"))["x"][:17])
    return [(pa.LennardJonesEnergy(39, 13, 3), lj.float().cuda(0)),
            (pa.MultiDoubleWellEnergy(), (torch.randn(17, 8, generator=gen) * 2.5).cuda(0)),
            (pa.GMM(device="cuda:0"), ((torch.rand(17, 2, generator=gen) - 0.5) * 90).cuda(0))]


def test_targets_under_device_guard_equal_bare_calls(pa):
    """__call__ of LennardJonesEnergy, MultiDoubleWellEnergy and GMM under ``torch.cuda.device(x.device)`` gives the bits
    of the bare call (with one device nothing else is observable), B = 17."""
    for e, x in _guarded_targets(pa):
        lp, f = e(x, return_force=True)
        with torch.cuda.device(x.device):
            lp_g, f_g = e(x, return_force=True)
        assert torch.isfinite(lp).all() and torch.isfinite(f).all(), type(e).__name__
        assert torch.equal(lp, lp_g) and torch.equal(f, f_g), type(e).__name__


def test_targets_follow_the_tensors_device_not_the_current_one(pa):
    """With another device current, a target evaluates on its tensor's device: same bits, outputs on that device."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices: with one, the current device is always the tensor's")
    for e, x in _guarded_targets(pa):
        lp, f = e(x, return_force=True)
        with torch.cuda.device(1):
            lp_o, f_o = e(x, return_force=True)
        assert lp_o.device == x.device and f_o.device == x.device
        assert torch.equal(lp, lp_o) and torch.equal(f, f_o), type(e).__name__


# ------------------------------------------------------------------------------- EGNN
def make_net(pa, n, d, weights, temp=True, **kw):
    if temp:
        net = pa.EGNN_dynamics(n, d, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                               condition_time=True, condition_temperature=True, agg="sum", **kw)
    else:
        from pita_amd import egnn

        net = egnn.EGNN_dynamics(n, d, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                                 condition_time=True, agg="sum")
    net.load_state_dict({k: T(v) for k, v in weights.items()})
    return net


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("name", ["lj13", "dw4", "lj55"])
@pytest.mark.parametrize("tag,wfile", [("init", "egnn_weights_seed12345.npz"), ("trained", "egnn_weights_trainedlike.npz")])
def test_egnn_golden(pa, golden, name, tag, wfile, precision):
    """All dense-layer arithmetic modes (f32 MFMA; bf16 matrix pipe with exact 3-way split; f16 matrix pipe with 2-way
    round-to-nearest split) must be fp32-accurate: within 4x the reference's own fp32-vs-fp64 error."""
    g = golden(f"egnn_{name}_fwd.npz")
    w = golden(wfile)
    n, d = int(g["n"]), int(g["d"])
    net = make_net(pa, n, d, w, precision=precision)
    print(f"[{name}/{tag}/{precision}]", end=" ")
    x, h, beta = cu(g["x"]), cu(g["h"]), cu(g["beta"])
    c_s, c_in, c_out, c_noise = O.edm_coeffs(T(g["h"]))
    F = net(c_noise.cuda(), (c_in[:, None] * T(g["x"])).cuda(), beta)
    # the reference's own fp32 error, measured against the fp64 oracle on the same inputs
    wd = {k: T(v) for k, v in w.items()}
    F64 = O.egnn_forward(wd, c_noise.double(), (c_in[:, None] * T(g["x"])).double(), T(g["beta"]).double(), n, d)
    err_ref = rel(g[f"F_{tag}"], F64)
    err_hip = rel(F, F64)
    print(f"err_hip_vs_fp64={err_hip:.3e} err_ref_vs_fp64={err_ref:.3e}")
    assert err_hip < max(4 * err_ref, 2e-6), (err_hip, err_ref)
    assert rel(F, g[f"F_{tag}"]) < max(2e-5, 6 * err_ref)
    sn = pa.ScoreNet(net)
    assert rel(sn.denoiser(h, x, beta), g[f"D_{tag}"]) < 2e-6
    sc = sn(h, x, beta).cpu().numpy()
    for hv in np.unique(g["h"]):
        m = g["h"] == hv
        tol = 1e-4 if hv > 0.05 else 5e-3  # (D - x)/h amplifies fp32 rounding by 1/h
        assert rel(sc[m], g[f"score_{tag}"][m]) < tol, hv


@pytest.mark.parametrize("tag,L,tanh,att", [("h64", 5, True, True), ("h48", 2, False, False)])
def test_egnn_ad2cat_golden(pa, golden, tag, L, tanh, att):
    """EGNN_dynamics_AD2_cat through pita_egnn_wide_eval (22 atoms: the matrix-pipe kernel; hidden 64 x 5 layers and a
    hidden-48 net that exercises the padding): backbone output within 4x the reference's own fp32-vs-fp64 error, denoiser
    and score through ScoreNet's fused EDM path, batch edges, and the per-step sampler path of the integrator against
    the oracle."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    g = golden(f"egnn_ad2cat_{tag}_fwd.npz")
    w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
    H = w["egnn.embedding.weight"].shape[0]
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=H, n_layers=L, tanh=tanh, attention=att, condition_beta=True)
    net.load_state_dict(w)
    x, h, beta = cu(g["x"]), cu(g["h"]), cu(g["beta"])
    c_s, c_in, c_out, c_noise = O.edm_coeffs(T(g["h"]))
    F = net(c_noise.cuda(), (c_in[:, None] * T(g["x"])).cuda(), beta)
    wd = {k: v.double() for k, v in w.items()}
    F64 = O.egnn_ad2_cat_forward(wd, c_noise.double(), (c_in[:, None] * T(g["x"])).double(), T(g["beta"]).double(), 22, 3,
                                 n_layers=L, tanh=tanh, attention=att)
    err_ref, err_hip = rel(g["F"], F64), rel(F, F64)
    print(f"[ad2cat/{tag}] err_hip_vs_fp64={err_hip:.3e} err_ref_vs_fp64={err_ref:.3e}")
    assert err_hip < max(4 * err_ref, 2e-6), (err_hip, err_ref)
    assert rel(F, g["F"]) < max(2e-5, 6 * err_ref)
    assert net.uses_matrix_pipe("cuda:0")
    sn = pa.ScoreNet(net)
    assert rel(sn.denoiser(h, x, beta), g["D"]) < 2e-6
    sc = sn(h, x, beta).cpu().numpy()
    for hv in np.unique(g["h"]):
        m = g["h"] == hv
        assert rel(sc[m], g["score"][m]) < (1e-4 if hv > 0.05 else 5e-3), hv
    # batch edges: empty, one walker, more walkers than resident waves; a walker's value does not depend on the batch
    assert net(c_noise[:0].cuda(), x[:0], beta[:0]).shape == (0, 66)
    one = net(c_noise[:1].cuda(), (c_in[:1, None] * T(g["x"][:1])).cuda(), beta[:1])
    assert torch.equal(one, F[:1])
    reps = 700
    big = net(c_noise.repeat(reps).cuda(), (c_in[:, None] * T(g["x"])).repeat(reps, 1).cuda(), beta.repeat(reps))
    assert torch.equal(big[-12:], F) and torch.equal(big[:12], F)
    with pytest.raises(pa._lib.PitaHipError):
        net(c_noise, T(g["x"]), T(g["beta"]))  # CPU tensors: no fallback
    if not tanh:
        return  # without the tanh bound these scaled-up coordinate heads diverge from the prior's scale (in the oracle too)
    # the integrator's per-step path (ScoreNet's fused EDM evaluation + pita_em_step) against the oracle, 6 steps
    N, B = 6, 12
    sched, gam = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7), pa.ConstantAnnealingFactorSchedule(1.0)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=sn, debias_inference=False)
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                     resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0)
    gen = torch.Generator().manual_seed(4)
    x1 = O.remove_mean(torch.randn(B, 66, generator=gen) * 60.0, 22, 3)
    noise = torch.randn(N, B, 66, generator=gen)

    class Geo:  # what the integrator reads off an energy function
        n_particles, n_spatial_dim, is_molecule = 22, 3, True

    xh, *_ = integ.integrate_sde(x1.cuda(), Geo(), gam, inverse_temperature=1.3, noise=noise.cuda())
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(w, cn, xs, b, 22, 3, n_layers=L, tanh=tanh, attention=att)
    osched, ogam = O.Elucidating(0.01, 80.0, 7), O.GammaConstant(1.0)
    ref = O.integrate_sde(O.IntegratorConfig(num_integration_steps=N, end_resampling_step=N), x1,
                          lambda t, xc: O.f_not_debiased(bb, osched, ogam, t, xc, 1.3), osched.g, lambda i, shp: noise[i],
                          22, 3)["x"]
    assert torch.isfinite(ref).all() and rel(xh, ref) < 1e-4


@pytest.mark.parametrize("tag,L,tanh,att", [("h64", 5, True, True), ("h48", 2, False, False)])
def test_egnn_ad2cat_forward_mode_vs_oracle_jacobian(pa, golden, tag, L, tanh, att, monkeypatch):
    """pita_egnn_wide_jvp (forward mode through EGNN_dynamics_AD2_cat, hidden 64 x 5 and the padded hidden-48 net; 22 atoms:
    the matrix-pipe kernel egnn_wide64_jvp_kernel with the vector-pipe kernel as its out-of-range repair) on the
    inputs of the reference golden: the denoiser, J_x D e_k for unit directions, J_x D v for a dense direction, dD/dh, the
    in-kernel reductions <x, dD> and the diagonal accumulator -- against vmap(jacrev) of the fp64 oracle (the reference's
    utils.py:30-51 on its own module), rel 5e-5 like the h32 kernels."""
    from torch.func import jacrev, vmap

    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    g = golden(f"egnn_ad2cat_{tag}_fwd.npz")
    w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
    H = w["egnn.embedding.weight"].shape[0]
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=H, n_layers=L, tanh=tanh, attention=att, condition_beta=True)
    net.load_state_dict(w)
    sel = np.arange(0, g["x"].shape[0], 2)[:6]
    x, h, beta = T(g["x"][sel]), T(g["h"][sel]), T(g["beta"][sel])
    B = x.shape[0]
    wd = {k: v.double() for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, 22, 3, n_layers=L, tanh=tanh, attention=att)
    one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
    Jx = vmap(jacrev(one, argnums=1))(h.double(), x.double(), beta.double())      # [B, 66, 66]
    Jh = vmap(jacrev(one, argnums=0))(h.double(), x.double(), beta.double())      # [B, 66]
    D64 = O.denoiser(bb, h.double(), x.double(), beta.double())
    xc, hc, bc = x.cuda(), h.cuda(), beta.cuda()
    acc = torch.zeros(B, device="cuda")
    jtx = torch.empty(B, 66, device="cuda")
    for k in range(66):
        out, dout = net.jvp(hc, xc, bc, direction=k, want_primal=(k == 0), want_tangent=(k % 13 == 0), dot_out=jtx, dot_col=k,
                            diag_acc=acc)
        if k == 0:
            assert rel(out, D64) < 2e-6
            assert rel(out, net.edm(1, hc, xc, bc)) < 2e-6
        if dout is not None:
            assert rel(dout, Jx[:, :, k]) < 5e-5, k
    scale = float(Jx.diagonal(dim1=1, dim2=2).sum(-1).abs().mean()) + 1.0
    np.testing.assert_allclose(acc.cpu().numpy(), Jx.diagonal(dim1=1, dim2=2).sum(-1).numpy(), rtol=5e-5, atol=5e-5 * scale)
    assert rel(jtx, torch.einsum("bq,bqk->bk", x.double(), Jx)) < 5e-5
    # h direction and a dense position direction in one launch
    gen = torch.Generator().manual_seed(9)
    vx, vh = torch.randn(B, 66, generator=gen), torch.rand(B, generator=gen) + 0.5
    dot = torch.empty(B, device="cuda")
    _, dout = net.jvp(hc, xc, bc, vx=vx.cuda(), vh=vh.cuda(), want_primal=False, dot_out=dot)
    want = torch.einsum("bqk,bk->bq", Jx, vx.double()) + Jh * vh.double()[:, None]
    assert rel(dout, want) < 5e-5
    np.testing.assert_allclose(dot.cpu().numpy(), (x.double() * want).sum(-1).numpy(), rtol=2e-4,
                               atol=2e-4 * float((x.double() * want).sum(-1).abs().mean()))
    _, dh = net.jvp(hc, xc, bc, direction=-1, vh=torch.ones(B).cuda(), want_primal=False)
    assert rel(dh, Jh) < 5e-5
    # the two kernels behind pita_egnn_wide_jvp: the matrix-pipe kernel (22 atoms; f16 two-piece split) served the calls
    # above; the fp32 vector-pipe kernel alone (PITA_WIDE_NO_MFMA) agrees to rounding, and takes over -- bit for bit --
    # exactly the walkers whose activations leave the f16 range (beta = 1e7), their neighbours untouched
    assert net.uses_matrix_pipe("cuda:0")
    _, dm = net.jvp(hc, xc, bc, direction=7, want_primal=False)
    bhot = bc.clone()
    bhot[1] = 1.0e7
    _, dm_hot = net.jvp(hc, xc, bhot, direction=7, want_primal=False)
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        _, dv = net.jvp(hc, xc, bc, direction=7, want_primal=False)
        _, dv_hot = net.jvp(hc, xc, bhot, direction=7, want_primal=False)
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    assert rel(dm, dv) < 5e-6 and not torch.equal(dm, dv)
    assert torch.equal(dm_hot[1].view(torch.int32), dv_hot[1].view(torch.int32))
    keep = torch.arange(B) != 1
    assert torch.equal(dm_hot[keep], dm[keep])
    # batch edges: empty batch; more walkers than resident waves give the same bits per walker
    assert net.jvp(hc[:0], xc[:0], bc[:0], direction=3)[1].shape == (0, 66)
    reps = 400
    _, big = net.jvp(hc.repeat(reps), xc.repeat(reps, 1), bc.repeat(reps), direction=5, want_primal=False)
    _, small = net.jvp(hc, xc, bc, direction=5, want_primal=False)
    assert torch.equal(big[:B], small) and torch.equal(big[-B:], small)


@pytest.mark.parametrize("tag,L,tanh,att", [("h64", 5, True, True), ("h48", 2, False, False), ("h64", 5, True, False)])
def test_egnn_ad2cat_reverse_mode_vs_oracle_jacobian(pa, golden, tag, L, tanh, att):
    """pita_egnn_wide_vjp (reverse mode through EGNN_dynamics_AD2_cat: ONE launch for J_x D^T cot and <cot, dD/dh>)
    against vmap(jacrev) of the fp64 oracle on the inputs of the reference golden -- cot = x (what grad_x E_theta needs,
    energy_net.py:51-62) and a dense cotangent --, against the forward-mode launches it replaces, and through
    EnergyNet.forward against autograd of the oracle's E_theta; rel 5e-5 like the h32 reverse-mode kernel."""
    from torch.func import jacrev, vmap

    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
    from pita_amd.energy_net import EnergyNet

    g = golden(f"egnn_ad2cat_{tag}_fwd.npz")
    w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
    H = w["egnn.embedding.weight"].shape[0]
    if not att:  # the gate's parameters are absent from an attention=False module
        w = {k: v for k, v in w.items() if "att_mlp" not in k}
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=H, n_layers=L, tanh=tanh, attention=att, condition_beta=True)
    net.load_state_dict(w)
    sel = np.arange(0, g["x"].shape[0], 2)[:6]
    x, h, beta = T(g["x"][sel]), T(g["h"][sel]), T(g["beta"][sel])
    B = x.shape[0]
    wd = {k: v.double() for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, 22, 3, n_layers=L, tanh=tanh, attention=att)
    one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
    Jx = vmap(jacrev(one, argnums=1))(h.double(), x.double(), beta.double())      # [B, 66, 66]
    Jh = vmap(jacrev(one, argnums=0))(h.double(), x.double(), beta.double())      # [B, 66]
    D64 = O.denoiser(bb, h.double(), x.double(), beta.double())
    xc, hc, bc = x.cuda(), h.cuda(), beta.cuda()
    gen = torch.Generator().manual_seed(11)
    for name, cot in (("x", None), ("dense", torch.randn(B, 66, generator=gen))):
        c64 = (x if cot is None else cot).double()
        D, vj, dh = net.vjp(hc, xc, bc, cot=None if cot is None else cot.cuda(), want_dot_h=True)
        assert rel(D, D64) < 2e-6, name
        assert rel(vj, torch.einsum("bq,bqk->bk", c64, Jx)) < 5e-5, (name, rel(vj, torch.einsum("bq,bqk->bk", c64, Jx)))
        want_h = (c64 * Jh).sum(-1)
        np.testing.assert_allclose(dh.cpu().numpy(), want_h.numpy(), rtol=2e-4, atol=2e-4 * float(want_h.abs().mean()))
        _, vj2 = net.vjp(hc, xc, bc, cot=None if cot is None else cot.cuda(), want_primal=False)  # x-only sweep
        assert rel(vj2, vj) < 1e-6
    # the forward-mode launches it replaces
    jtx = torch.empty(B, 66, device="cuda")
    for k in range(66):
        net.jvp(hc, xc, bc, direction=k, want_primal=False, want_tangent=False, dot_out=jtx, dot_col=k)
    _, vj = net.vjp(hc, xc, bc)
    assert rel(vj, jtx) < 2e-5
    # grad_x E_theta through the plug-in class
    en = EnergyNet(net)
    xr = x.double().requires_grad_(True)
    gref = torch.autograd.grad(O.energy_theta(bb, h.double(), xr, beta.double()).sum(), xr)[0]
    assert rel(en(hc, xc, bc), gref) < 5e-5
    # batch edges: empty batch; more walkers than resident waves give the same bits per walker
    assert net.vjp(hc[:0], xc[:0], bc[:0])[1].shape == (0, 66)
    reps = 400
    _, big = net.vjp(hc.repeat(reps), xc.repeat(reps, 1), bc.repeat(reps), want_primal=False)
    assert torch.equal(big[:B], vj) and torch.equal(big[-B:], vj)


def test_debiased_regime_on_the_ad2cat_backbone_vs_oracle(pa, golden):
    """VEReverseSDE(debias_inference=True) -- the reference default (model/energytemp.yaml:78) -- with the
    alanine-dipeptide backbone EGNN_dynamics_AD2_cat for the score AND the energy net (sdes.py:151-239 on
    egnn_dynamics_ad2_cat.py:11-203): every SDETerms field against the fp64 oracle's autograd / vmap(jacrev), and
    EnergyNet.forward (grad_x E_theta) against autograd."""
    import copy

    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
    from pita_amd.energy_net import EnergyNet

    g = golden("egnn_ad2cat_h64_fwd.npz")
    w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=64, n_layers=5, tanh=True, attention=True, condition_beta=True)
    net.load_state_dict(w)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    en = EnergyNet(copy.deepcopy(net))
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=en, debias_inference=True)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    wd = {k: v.double() for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, 22, 3, n_layers=5, tanh=True, attention=True)
    osched, ogam = O.Elucidating(0.01, 80.0, 7), O.GammaConstant(4 / 3)
    gen = torch.Generator().manual_seed(12)
    B = 5
    for tv, scale in ((0.15, 1.0), (0.6, 8.0)):
        x = O.remove_mean(torch.randn(B, 66, generator=gen) * scale, 22, 3)
        terms = sde.f(torch.tensor(tv).cuda(), x.cuda(), 1.25, gam, None, None, resampling_interval=1)
        ref = O.f_debiased(bb, bb, osched, ogam, torch.tensor(tv, dtype=torch.float64), x.double(), 1.25)
        assert rel(terms.drift_X, ref.drift_X) < 2e-4, tv
        for nm in ("divergence_score", "cross_term", "dUt_dt", "drift_A"):
            want = getattr(ref, nm).numpy()
            np.testing.assert_allclose(getattr(terms, nm).cpu().numpy(), want, rtol=3e-3,
                                       atol=3e-3 * float(np.abs(want).mean()), err_msg=f"{tv} {nm}")
        # grad_x E_theta through the module interface (energy_net.py:51-62)
        ht = osched.h(torch.full((B,), tv, dtype=torch.float64))
        xg = x.double().requires_grad_(True)
        (gE,) = torch.autograd.grad(O.energy_theta(bb, ht, xg, 1.25).sum(), xg)
        got = en(ht.float().cuda(), x.cuda(), 1.25)
        assert rel(got, gE) < 2e-4, tv


def test_egnn_ad2cat_fused_sampler(pa, golden, monkeypatch):
    """pita_egnn_wide_sampler_run (all steps of the not-debiased SDE in one launch on EGNN_dynamics_AD2_cat, hidden 64 x 5,
    22 atoms): against the launch-per-step path of the integrator (ScoreNet's fused EDM evaluation + pita_em_step: the
    same arithmetic up to the EDM coefficients, which the fused kernel takes from the host's step table), with the
    sampler's own Philox noise and with injected noise; per-step moments equal to the per-step path's; bitwise
    independent of how the steps are cut into launches and of how the walkers are sharded; the vector-pipe kernel alone
    (PITA_WIDE_NO_MFMA) within fp32 rounding; walkers whose activations leave the f16 range come back from the repair
    pass with exactly the vector-pipe kernel's values, their neighbours untouched, every walker's moments counted once."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    g = golden("egnn_ad2cat_h64_fwd.npz")
    w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=64, n_layers=5, tanh=True, attention=True, condition_beta=True)
    net.load_state_dict(w)
    sched, gam = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7), pa.ConstantAnnealingFactorSchedule(4 / 3)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), debias_inference=False)
    N, B = 8, 41  # ragged: ten groups of four walkers + one

    class Geo:
        n_particles, n_spatial_dim, is_molecule = 22, 3, True

    gen = torch.Generator().manual_seed(21)
    x1 = O.remove_mean(torch.randn(B, 66, generator=gen) * 60.0, 22, 3).cuda()
    noise = torch.randn(N, B, 66, generator=gen).cuda()
    mk = lambda **kw: pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0,
                                               end_resampling_step=N, resampling_interval=-1, num_negative_time_steps=0,
                                               post_mcmc_steps=0, seed=5, **kw)
    for nz in (None, noise):
        xf, _, _, tf, _ = mk().integrate_sde(x1, Geo(), gam, inverse_temperature=1.3, noise=nz)
        xs, _, _, ts, _ = mk(record_terms=True).integrate_sde(x1, Geo(), gam, inverse_temperature=1.3, noise=nz)
        assert torch.isfinite(xf).all() and rel(xf, xs) < 2e-5, rel(xf, xs)
        assert len(tf) == N and len(ts) == N
        for k in range(N):  # device-reduced moments of the fused launch == statistics of the per-step tensors
            assert abs(float(tf[k].drift_X.std()) - float(ts[k].drift_X.std())) < 2e-5 * float(ts[k].drift_X.std())
    # the C entry point directly: chunking and sharding invariance, bit for bit
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, N + 1)[:-1], 1.0 / N, 1.0, 1.3).cuda()
    # (walkers inside the f16 range: a walker the repair pass takes over is computed on the vector pipe for the steps of
    # THAT launch, so across a cut it would agree only to the two kernels' rounding difference, checked further down)
    x3 = (x1 * 0.05).contiguous()
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(0.3, 0.0, N + 1)[:-1], 0.3 / N, 1.0, 1.3).cuda()
    st = torch.zeros(N, 4, dtype=torch.float64, device="cuda")
    whole = net.sampler_run(x3.clone(), tab, N, seed=9, stats_out=st)
    for cut in (1, 3, 7):
        parts = x3.clone()
        net.sampler_run(parts, tab[:cut].contiguous(), cut, seed=9)
        net.sampler_run(parts, tab[cut:].contiguous(), N - cut, seed=9, step0=cut)
        assert torch.equal(whole, parts), cut
    lo, hi = x3[:17].clone(), x3[17:].clone()
    net.sampler_run(lo, tab, N, seed=9)
    net.sampler_run(hi, tab, N, seed=9, walker_offset=17)
    assert torch.equal(whole, torch.cat([lo, hi]))
    assert float(whole.reshape(B, 22, 3).mean(1).abs().max()) < 2e-4  # remove_mean every step
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        stv = torch.zeros(N, 4, dtype=torch.float64, device="cuda")
        vec = net.sampler_run(x3.clone(), tab, N, seed=9, stats_out=stv)
        vparts = x3.clone()
        net.sampler_run(vparts, tab[:3].contiguous(), 3, seed=9)
        net.sampler_run(vparts, tab[3:].contiguous(), N - 3, seed=9, step0=3)
        assert torch.equal(vec, vparts)
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    assert rel(whole, vec) < 1e-5 and not torch.equal(whole, vec)
    np.testing.assert_allclose(st.cpu().numpy()[:, [1, 3]], stv.cpu().numpy()[:, [1, 3]], rtol=1e-5)
    # out-of-range walkers (pair distances ~1e4: edge pre-activations beyond the f16 range from the first layer on)
    x2 = x1.clone()
    hot = torch.tensor([2, 3, 20, 40])
    x2[hot.cuda()] *= 400.0
    tab2 = pa.sde_integration.build_step_table(sched, gam, torch.linspace(0.05, 0.0, N + 1)[:-1], 0.05 / N, 1.0, 1.3).cuda()
    sa, sb = (torch.zeros(N, 4, dtype=torch.float64, device="cuda") for _ in range(2))
    a = net.sampler_run(x2.clone(), tab2, N, seed=9, stats_out=sa)
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        b = net.sampler_run(x2.clone(), tab2, N, seed=9, stats_out=sb)
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    assert torch.isfinite(b[hot]).all(), "the vector-pipe kernel handles this range in fp32"
    assert torch.equal(a[hot], b[hot])
    keep = torch.ones(B, dtype=torch.bool)
    keep[hot] = False
    plain = net.sampler_run(x2[keep.cuda()].clone(), tab2, N, seed=9)  # (Philox keys follow the position in the batch)
    assert plain.shape[0] == B - 4 and rel(a[keep], b[keep]) < 1e-5
    sah, sbh = sa.cpu().numpy(), sb.cpu().numpy()
    np.testing.assert_allclose(sah[:, [1, 3]], sbh[:, [1, 3]], rtol=1e-5)


def test_egnn_aldp_golden(pa, golden):
    """``pita_amd.egnn_aldp.EGNN_dynamics`` (egnn_aldp.py:8-197 on the wide-backbone kernels) against the reference
    module's output: class defaults at 22 atoms (hidden 64 x 4 layers, no gate, no tanh: the matrix-pipe kernel) and a
    33-atom hidden-32 net with gate and tanh; beta is ignored unless the net is temperature conditioned."""
    from pita_amd.egnn_aldp import EGNN_dynamics

    g = golden("egnn_aldp_fwd.npz")
    for tag, n, kw in (("n22", 22, dict(n_layers=4, tanh=False, attention=False)),
                       ("n33", 33, dict(n_layers=2, tanh=True, attention=True))):
        w = {k[len(f"w_{tag}."):]: T(v) for k, v in g.items() if k.startswith(f"w_{tag}.")}
        H = w["egnn.embedding.weight"].shape[0]
        net = EGNN_dynamics(n, 3, hidden_nf=H, condition_temperature=True, **kw)
        net.load_state_dict(w)
        x, t, beta = cu(g[f"x_{tag}"]), cu(g[f"t_{tag}"]), cu(g[f"beta_{tag}"])
        F = net(t, x, beta)
        wd = {k: v.double() for k, v in w.items()}
        F64 = O.egnn_ad2_cat_forward(wd, T(g[f"t_{tag}"]).double(), T(g[f"x_{tag}"]).double(), T(g[f"beta_{tag}"]).double(),
                                     n, 3, h_initial=O.egnn_aldp_h_initial(n).double(), **kw)
        err_ref, err_hip = rel(g[f"F_{tag}"], F64), rel(F, F64)
        print(f"[egnn_aldp/{tag}] err_hip_vs_fp64={err_hip:.3e} err_ref_vs_fp64={err_ref:.3e}")
        assert err_hip < max(4 * err_ref, 2e-6) and rel(F, g[f"F_{tag}"]) < max(2e-5, 6 * err_ref)
        if H == 64:
            assert net.uses_matrix_pipe("cuda:0")
        if n == 22:  # forward mode through this class too (no gate, no tanh: the other instantiation of the JVP kernels)
            from torch.func import jacrev, vmap

            hq = torch.tensor([0.05, 0.7, 3.0, 40.0])
            xq = T(g[f"x_{tag}"][:4]) * (1 + hq.sqrt())[:, None]
            bq = T(g[f"beta_{tag}"][:4])
            bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, n, 3, h_initial=O.egnn_aldp_h_initial(n).double(), **kw)
            one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
            J = vmap(jacrev(one, argnums=1))(hq.double(), xq.double(), bq.double())
            acc = torch.zeros(4, device="cuda")
            for k in (0, 17, 40, 65):
                _, dk = net.jvp(hq.cuda(), xq.cuda(), bq.cuda(), direction=k, want_primal=False, diag_acc=acc)
                assert rel(dk, J[:, :, k]) < 5e-5, k
            want = sum(J[:, k, k] for k in (0, 17, 40, 65))
            np.testing.assert_allclose(acc.cpu().numpy(), want.numpy(), rtol=5e-5, atol=5e-5 * float(want.abs().mean() + 1))
    plain = EGNN_dynamics(22, 3)  # not temperature conditioned: beta is accepted and ignored, like the reference's forward
    xs = cu(g["x_n22"])
    assert torch.equal(plain(cu(g["t_n22"]), xs, cu(g["beta_n22"])), plain(cu(g["t_n22"]), xs, None))


def test_default_regime_end_to_end_on_the_ad2cat_backbone(pa, golden):
    """integrate_sde with the reference's default regime on the alanine-dipeptide backbone end to end: debiased drift
    (forward-mode launches), an event after every step, two clamp chunks, resample_at_end (EnergyNet.forward_energy on
    the wide net) -- against the oracle's integrator on the same noise and uniforms: parent counts, log-weights and
    walkers after 3 steps."""
    import copy

    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
    from pita_amd.energy_net import EnergyNet

    g = golden("egnn_ad2cat_h64_fwd.npz")
    w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=64, n_layers=5, tanh=True, attention=True, condition_beta=True)
    net.load_state_dict(w)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    N, B, chunk = 3, 4, 2
    gen = torch.Generator().manual_seed(31)
    x1 = O.remove_mean(torch.randn(B, 66, generator=gen) * 2.0, 22, 3)
    noise = torch.randn(N, B, 66, generator=gen)
    us = [0.21, 0.77, 0.48]

    class Target:  # a cheap analytic target with the energy-function interface (harmonic well)
        n_particles, n_spatial_dim, is_molecule = 22, 3, True

        def __call__(self, x, return_force=False):
            lp = -0.5 * (x * x).sum(-1)
            return (lp, -x) if return_force else lp

    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=2,
                                     resampling_interval=1, num_negative_time_steps=0, post_mcmc_steps=0, batch_size=chunk,
                                     resample_at_end=True, time_range=0.3)
    x, logw, uniq, terms, _ = integ.integrate_sde(x1.cuda(), Target(), gam, inverse_temperature=1.25, noise=noise.cuda(),
                                                  resample_u=us)
    wd = {k: v.double() for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, 22, 3, n_layers=5, tanh=True, attention=True)
    osched, ogam = O.Elucidating(0.01, 80.0, 7), O.GammaConstant(4 / 3)
    cfg = O.IntegratorConfig(num_integration_steps=N, start_resampling_step=0, end_resampling_step=2, resampling_interval=1,
                             batch_size=chunk, time_range=0.3)
    drift = lambda t, xc: O.f_debiased(bb, bb, osched, ogam, t, xc, 1.25)
    ref = O.integrate_sde(cfg, x1.double(), drift, osched.g, lambda i, shp: noise[i // 2][(i % 2) * chunk:(i % 2 + 1) * chunk].double(),
                          22, 3, uniform_fn=lambda s_: us[s_])
    t_end = torch.linspace(0.3, 0.0, N + 1)[:-1][2].double()
    xr, a_next, nu = O.resample_at_end(ref["x"], ref["logweights"][-1], t_end, lambda xx: -0.5 * (xx * xx).sum(-1),
                                       lambda tb, xx: O.energy_theta(bb, osched.h(tb), xx, 1.25), 4 / 3, us[2])
    assert uniq[:N] == ref["num_unique"] and uniq[N] == nu
    np.testing.assert_allclose(logw[:N].cpu().numpy(), ref["logweights"].numpy(), rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(logw[N].cpu().numpy(), a_next.numpy(), rtol=2e-3, atol=2e-3 * float(a_next.abs().mean()))
    assert rel(x, xr) < 2e-3
    assert len(terms) == N


@pytest.mark.parametrize("n", [13, 22, 33, 42, 55])
def test_egnn_ad2cat_other_particle_counts(pa, n, monkeypatch):
    """Every instantiation of the matrix-pipe kernel -- the particle counts EGNN_dynamics_AD2_cat knows node features for
    (alanine di- / tri- / tetra-peptide, LJ13, LJ55) x attention gate on / off x tanh head on / off: seeded
    reference-style weights, backbone output against the fp64 oracle (fp32-level error) and against the vector-pipe
    kernel, ragged batch (partial last group)."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    gen = torch.Generator().manual_seed(n)
    B = 9
    x = O.remove_mean(torch.randn(B, n * 3, generator=gen) * 1.5, n, 3)
    t = torch.rand(B, generator=gen) - 0.5
    beta = torch.rand(B, generator=gen) + 0.5
    for att in (True, False):
        for tanh in (True, False):
            torch.manual_seed(100 + n)
            net = EGNN_dynamics_AD2_cat(n, 3, hidden_nf=64, n_layers=3, tanh=tanh, attention=att, condition_beta=True)
            with torch.no_grad():
                for prm in net.parameters():  # trained-like magnitudes: the fresh coordinate head (gain 1e-3) hides errors
                    if prm.dim() == 2 and prm.shape[0] == 1 and prm.shape[1] == 64:
                        prm.mul_(200.0 if tanh else 20.0)
            w = {k: v.detach().clone() for k, v in net.state_dict().items()}
            assert net.uses_matrix_pipe("cuda:0")
            F = net(t.cuda(), x.cuda(), beta.cuda())
            kw = dict(n_layers=3, tanh=tanh, attention=att)
            F64 = O.egnn_ad2_cat_forward({k: v.double() for k, v in w.items()}, t.double(), x.double(), beta.double(), n, 3, **kw)
            F32 = O.egnn_ad2_cat_forward(w, t, x, beta, n, 3, **kw)
            err_hip, err_ref = rel(F, F64), rel(F32, F64)
            print(f"[ad2cat n={n} att={att} tanh={tanh}] err_hip_vs_fp64={err_hip:.3e} err_fp32_oracle_vs_fp64={err_ref:.3e}")
            assert torch.isfinite(F64).all() and float(F64.abs().max()) > 1e-3, float(F64.abs().max())
            assert err_hip < max(4 * err_ref, 2e-6), (att, tanh, err_hip, err_ref)
            monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
            Fv = net(t.cuda(), x.cuda(), beta.cuda())
            monkeypatch.delenv("PITA_WIDE_NO_MFMA")
            assert rel(Fv, F64) < max(4 * err_ref, 2e-6) and rel(F, Fv) < max(8 * err_ref, 2e-6), (rel(F, Fv), err_ref)
            assert torch.equal(net(t[:5].cuda(), x[:5].cuda(), beta[:5].cuda()), F[:5])


def test_egnn_ad2cat_other_sizes_golden(pa, golden):
    """33 and 42 atoms (tri- / tetra-alanine) against the REFERENCE module's output (egnn_ad2cat_sizes.npz): hidden 32
    padded to the matrix-pipe kernel's 64, static node features from the module's own tables."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    g = golden("egnn_ad2cat_sizes.npz")
    for n in (33, 42):
        w = {k[len(f"w{n}."):]: T(v) for k, v in g.items() if k.startswith(f"w{n}.")}
        net = EGNN_dynamics_AD2_cat(n, 3, hidden_nf=32, n_layers=2, condition_beta=True)
        net.load_state_dict(w)
        F = net(cu(g[f"t_{n}"]), cu(g[f"x_{n}"]), cu(g[f"beta_{n}"]))
        F64 = O.egnn_ad2_cat_forward({k: v.double() for k, v in w.items()}, T(g[f"t_{n}"]).double(), T(g[f"x_{n}"]).double(),
                                     T(g[f"beta_{n}"]).double(), n, 3, n_layers=2)
        err_ref, err_hip = rel(g[f"F_{n}"], F64), rel(F, F64)
        print(f"[ad2cat sizes n={n}] err_hip_vs_fp64={err_hip:.3e} err_ref_vs_fp64={err_ref:.3e}")
        assert net.uses_matrix_pipe("cuda:0") and err_hip < max(4 * err_ref, 2e-6), (n, err_hip, err_ref)
        assert rel(F, g[f"F_{n}"]) < max(2e-5, 6 * err_ref)


def test_egnn_ad2cat_matrix_pipe_vs_vector_pipe(pa, golden, monkeypatch):
    """The two kernels behind pita_egnn_wide_eval on the same inputs: the matrix-pipe kernel (f16 two-piece split) agrees
    with the vector-pipe kernel (fp32 FMA chains) to fp32 rounding in all three modes and at ragged batch sizes (1 .. 9
    walkers: partial groups of 4); walkers whose activations leave the f16 range come back from the vector-pipe repair
    pass with exactly its values, their neighbours in the batch untouched."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    g = golden("egnn_ad2cat_h64_fwd.npz")
    w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=64, n_layers=5, tanh=True, attention=True, condition_beta=True)
    net.load_state_dict(w)
    gen = torch.Generator().manual_seed(11)
    B = 37
    x = (torch.randn(B, 66, generator=gen) * 2.0).cuda()
    h = (torch.rand(B, generator=gen) * 4.0 + 0.05).cuda()
    beta = (torch.rand(B, generator=gen) + 0.5).cuda()

    def both(fn):
        a = fn()
        monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
        try:
            assert not net.uses_matrix_pipe("cuda:0")
            b = fn()
        finally:
            monkeypatch.delenv("PITA_WIDE_NO_MFMA")
        assert net.uses_matrix_pipe("cuda:0")
        return a, b

    for what in (0, 1, 2):
        fn = (lambda: net(h, x, beta)) if what == 0 else (lambda: net.edm(what, h, x, beta))
        a, b = both(fn)
        assert torch.isfinite(a).all() and rel(a, b) < 2e-6, (what, rel(a, b))
    full = net(h, x, beta)
    for n in (1, 2, 3, 4, 5, 9):
        assert torch.equal(net(h[:n], x[:n], beta[:n]), full[:n]), n
    # out-of-range walkers: beta = 1e7 drives the node features beyond 65504 in the first dense layer
    hot = torch.tensor([3, 4, 17, 36])
    beta2 = beta.clone()
    beta2[hot.cuda()] = 1.0e7
    a, b = both(lambda: net(h, x, beta2))
    assert torch.equal(a[hot].view(torch.int32), b[hot].view(torch.int32))  # bitwise (holds for non-finite values too)
    assert torch.isfinite(a[hot]).all(), "the vector-pipe kernel handles this range in fp32"
    keep = torch.ones(B, dtype=torch.bool)
    keep[hot] = False
    assert torch.equal(a[keep], full[keep])


def test_f16x2_out_of_range_walkers_are_recomputed_on_the_bf16_path(pa, golden):
    """precision="f16x2" has a range limit (SiLU outputs beyond 65504 overflow f16).  The launch wrapper follows the f16
    kernel with a repair launch of the bf16x3 kernel that recomputes exactly the walker groups whose results are
    non-finite: far-out walkers (where the reference's fp32 arithmetic is still finite) must come out equal to the
    bf16x3 result, ordinary walkers must keep their f16x2 result, and the per-step moments must count every walker once."""
    w = golden("egnn_weights_trainedlike.npz")
    nf, nb = make_net(pa, 13, 3, w, precision="f16x2"), make_net(pa, 13, 3, w, precision="bf16x3")
    gen = torch.Generator().manual_seed(77)
    B = 70  # ten 7-walker groups: 0-4 ordinary, 5-9 far out (pair distances ~1e3: edge pre-activations ~1e5)
    x = torch.randn(B, 39, generator=gen)
    x[35:] *= 1000.0
    x = O.remove_mean(x, 13, 3).cuda()
    t, b = torch.full((B,), -0.3).cuda(), torch.full((B,), 1.0).cuda()
    Ff, Fb = nf(t, x, b), nb(t, x, b)
    assert torch.isfinite(Ff).all() and torch.isfinite(Fb).all()
    assert torch.equal(Ff[35:], Fb[35:])                      # recomputed by the bf16x3 kernel
    assert not torch.equal(Ff[:35], Fb[:35]) and rel(Ff[:35], Fb[:35]) < 1e-6   # untouched f16x2 results
    ref = O.egnn_forward({k: T(v) for k, v in w.items()}, t.cpu().double(), x.cpu().double(), b.cpu().double(), 13, 3)
    assert rel(Ff, ref) < 2e-5
    # fused sampler, with the per-step moments the integrator asks for
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    N = 5
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(0.2, 0.0, N + 1)[:-1], 0.2 / N, 1.0, 1.0).cuda()
    sf, sb = (torch.zeros(N, 4, dtype=torch.float64, device="cuda") for _ in range(2))
    df, db = torch.empty_like(x), torch.empty_like(x)
    xf = nf.sampler_run(x.clone(), tab, N, seed=3, stats_out=sf, drift_out=df)
    xb = nb.sampler_run(x.clone(), tab, N, seed=3, stats_out=sb, drift_out=db)
    assert torch.isfinite(xf).all()
    assert torch.equal(xf[35:], xb[35:]) and torch.equal(df[35:], db[35:])
    assert not torch.equal(xf[:35], xb[:35]) and rel(xf[:35], xb[:35]) < 1e-5
    sfh, sbh = sf.cpu().numpy(), sb.cpu().numpy()   # every walker counted exactly once
    np.testing.assert_allclose(sfh[:, [1, 3]], sbh[:, [1, 3]], rtol=1e-6)
    # plain sums of mean-free drifts cancel to ~0: compare on the scale of the summands (fp32 lane partials, B*39 terms)
    scale = np.sqrt(sbh[:, [1, 3]] * B * 39)
    assert (np.abs(sfh[:, [0, 2]] - sbh[:, [0, 2]]) < 1e-6 * scale).all()
    # the same ordinary walkers alone: their result does not depend on who else is in the batch
    xa = nf.sampler_run(x[:35].clone(), tab, N, seed=3)
    assert torch.equal(xa, xf[:35])


def test_egnn_notemp_and_layouts(pa, golden):
    g = golden("egnn_notemp_lj13_fwd.npz")
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    net = make_net(pa, 13, 3, w, temp=False)
    out = net(cu(g["t"]), cu(g["x"]))
    assert rel(out, g["out"]) < 1e-4  # fresh-init velocities are ~1e-4 |x| (cancellation)
    # feature_layout="correct": (t, beta) on every node == oracle with the un-quirked features
    w2 = golden("egnn_weights_trainedlike.npz")
    netc = make_net(pa, 13, 3, w2, feature_layout="correct")
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(9, 39, generator=gen)
    t, b = torch.randn(9, generator=gen), torch.rand(9, generator=gen) + 0.5
    out = netc(t.cuda(), x.cuda(), b.cuda())
    ref = O.egnn_forward({k: T(v) for k, v in w2.items()}, t, x, b, 13, 3, feature_layout="correct")
    assert rel(out, ref) < 2e-5
    assert abs(out.reshape(9, 13, 3).mean(1)).max() < 1e-5  # mean-free output
    # with the "correct" layout the network is permutation equivariant (the reference's quirk breaks this)
    perm = torch.randperm(13, generator=gen)
    xp = x.reshape(9, 13, 3)[:, perm].reshape(9, 39)
    outp = netc(t.cuda(), xp.cuda(), b.cuda())
    assert rel(outp, out.reshape(9, 13, 3)[:, perm.cuda()].reshape(9, 39)) < 2e-5


@pytest.mark.parametrize("B", [1, 6, 7, 8, 100, 1001])
def test_egnn_batch_edges(pa, golden, B):
    """ragged batches: B not a multiple of the 7-walker wave group, single walker, etc."""
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, 13, 3, w)
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, 39, generator=gen) * 1.2
    t = torch.randn(B, generator=gen) * 0.5
    b = torch.rand(B, generator=gen) * 2 + 0.5
    ref = O.egnn_forward({k: T(v) for k, v in w.items()}, t, x, b, 13, 3)
    out = net(t.cuda(), x.cuda(), b.cuda())
    assert rel(out, ref) < 2e-5


# config C1 (GMM target, MLP score net) against the reference's run: first-step drift, final walkers after 100 steps, fused
# sampler vs the per-step path.  Measured on MI355X 3.8e-10 / 1.7e-7 / 2.6e-8 (profiles/r05_parity_measured.txt); the
# bounds are 4 x that, floored at one fp32 rounding
_C1_BOUNDS = (1.2e-7, 7e-7, 1.2e-7)


# ------------------------------------------------------------------------------- MLP
def test_mlp_golden(pa, golden):
    from pita_amd import mlp

    g = golden("mlp_gmm_fwd.npz")
    net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
    net.load_state_dict({k[2:]: T(v) for k, v in g.items() if k.startswith("w.")})
    x, h = T(g["x"]), T(g["h"])
    c_s, c_in, c_out, c_noise = O.edm_coeffs(h)
    F = net(c_noise.cuda(), (c_in[:, None] * x).cuda(), torch.ones(64).cuda())
    assert rel(F, g["F"]) < 2e-5
    sc = pa.ScoreNet(net)(h.cuda(), x.cuda(), 1.0).cpu().numpy()
    big = g["h"] > 1e-2
    assert rel(sc[big], g["score"][big]) < 2e-4
    g2 = golden("mlp_temp_fwd.npz")
    net2 = mlp.MyMLPTemperature(hidden_size=64, hidden_layers=2, emb_size=64, out_dim=3, input_dim=3)
    net2.load_state_dict({k[2:]: T(v) for k, v in g2.items() if k.startswith("w.")})
    y = net2(cu(g2["t"]), cu(g2["x"]), cu(g2["beta"]))
    assert rel(y, g2["out"]) < 2e-5
    # ragged batch / plug-in path through the integrator (config C1: GMM target, MLP score net)
    gt = golden("em_traj_gmm_mlp.npz")
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), debias_inference=False)
    N = int(gt["N"])
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                     resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0,
                                     should_mean_free=False, record_terms=True)
    xf, logw, uniq, terms, acc = integ.integrate_sde(cu(gt["x1"]), pa.GMM(), pa.ConstantAnnealingFactorSchedule(1.0),
                                                     inverse_temperature=1.0, noise=cu(gt["noise"]))
    # measured on MI355X (printed; profiles/r05_parity_measured.txt): bounds are 4 x the measured deviations
    print(f"[c1/gmm] first-step drift rel-L2 vs reference {rel(terms[0].drift_X, gt['drift_X'][0]):.2e}, final walkers after "
          f"{N} steps {rel(xf, gt['x_final']):.2e}")
    assert rel(terms[0].drift_X, gt["drift_X"][0]) < _C1_BOUNDS[0]
    assert rel(xf, gt["x_final"]) < _C1_BOUNDS[1]
    # the fused MLP sampler (pita_mlp_sampler_run: all steps in one launch) against the per-step path and the golden
    integ.record_terms = False
    xfu, *_ = integ.integrate_sde(cu(gt["x1"]), pa.GMM(), pa.ConstantAnnealingFactorSchedule(1.0),
                                  inverse_temperature=1.0, noise=cu(gt["noise"]))
    print(f"[c1/gmm] fused sampler vs per-step path {rel(xfu, xf):.2e}, vs reference {rel(xfu, gt['x_final']):.2e}")
    assert rel(xfu, xf) < _C1_BOUNDS[2] and rel(xfu, gt["x_final"]) < _C1_BOUNDS[1]


@pytest.mark.parametrize("pb", [False, True])
def test_scorenet_wrapper_kernels(pa, golden, pb):
    """ScoreNet around a backbone without a fused EDM kernel (the HIP MLP): pita_edm_scale_input + backbone +
    pita_edm_combine against the oracle, with and without beta preconditioning (score_net.py:21-43)."""
    from pita_amd import mlp

    g2 = golden("mlp_temp_fwd.npz")
    w2 = {k[2:]: T(v) for k, v in g2.items() if k.startswith("w.")}
    net = mlp.MyMLPTemperature(hidden_size=64, hidden_layers=2, emb_size=64, out_dim=3, input_dim=3)
    net.load_state_dict(w2)
    bb = lambda cn, xs, b: O.mlp_forward(w2, cn, xs, b, emb_size=64, hidden_layers=2, temperature_conditioned=True)
    gen = torch.Generator().manual_seed(8)
    B = 517
    h = torch.tensor([0.01, 0.3, 2.0, 40.0, 900.0])[torch.arange(B) % 5]
    x = torch.randn(B, 3, generator=gen) * (1 + h.sqrt())[:, None]
    beta = torch.rand(B, generator=gen) + 0.5
    sn = pa.ScoreNet(net, precondition_beta=pb)
    Dh, sh = sn.denoiser(h.cuda(), x.cuda(), beta.cuda(), return_score=True)
    Do = O.denoiser(bb, h, x, beta, precondition_beta=pb)
    so = O.score(bb, h, x, beta, precondition_beta=pb)
    assert rel(Dh, Do) < 2e-5 and rel(sh, so) < 2e-4
    assert rel(sn(h.cuda(), x.cuda(), beta.cuda()), so) < 2e-4
    assert torch.equal(sn.denoiser(h.cuda(), x.cuda(), beta.cuda()), Dh)
    assert rel(sn(h.cuda(), x.cuda(), 1.3), O.score(bb, h, x, 1.3, precondition_beta=pb)) < 2e-4  # scalar beta


def test_mlp_fused_sampler_particles(pa):
    """pita_mlp_sampler_run on a particle system (2 x 3-D, mean removal, temperature-conditioned MLP): Philox noise and
    injected noise, ragged batch, against the per-step path (pita_mlp_forward + ScoreNet + pita_em_step)."""
    from types import SimpleNamespace

    from pita_amd import mlp

    torch.manual_seed(3)
    net = mlp.MyMLPTemperature(hidden_size=64, hidden_layers=2, emb_size=64, out_dim=6, input_dim=6)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), debias_inference=False)
    geom = SimpleNamespace(n_particles=2, n_spatial_dim=3, is_molecule=True)
    N, B = 9, 333
    gen = torch.Generator().manual_seed(1)
    x1 = O.remove_mean(torch.randn(B, 6, generator=gen) * 5, 2, 3).cuda()
    nz = torch.randn(N, B, 6, generator=gen).cuda()
    mk = lambda rec: pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0,
                                              end_resampling_step=N, resampling_interval=-1, num_negative_time_steps=0,
                                              post_mcmc_steps=0, record_terms=rec, seed=21)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    for noise in (nz, None):
        xa, *_ = mk(False).integrate_sde(x1, geom, gam, inverse_temperature=1.3, noise=noise)
        xb, *_ = mk(True).integrate_sde(x1, geom, gam, inverse_temperature=1.3, noise=noise)
        assert rel(xa, xb) < 2e-5
        assert abs(xa.reshape(B, 2, 3).mean(1)).max() < 1e-4 and not torch.equal(xa, x1)


# ------------------------------------------------------------------------------- sampler
def lj13_stack(pa, golden, **kw):
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, 13, 3, w).cuda()
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=None, debias_inference=False)
    return sde, sched, net


# final walkers, first drift, worst drift along the run, fused vs per-step: measured 1.7e-7 / 1.0e-8 / 3.3e-7 / 1.7e-7
_TRAJ20_BOUNDS = (6.8e-7, 1.2e-7, 1.4e-6, 6.8e-7)


def test_traj_golden_fused_and_stepwise(pa, golden):
    g = golden("em_traj_lj13_nodebias.npz")
    sde, sched, net = lj13_stack(pa, golden)
    N = int(g["N"])
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    e = pa.LennardJonesEnergy(39, 13, 3)
    noise = cu(g["noise"])
    outs = {}
    for rec in (False, True):
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0,
                                         end_resampling_step=N, resampling_interval=-1, num_negative_time_steps=0,
                                         post_mcmc_steps=0, batch_size=16, record_terms=rec)
        x, logw, uniq, terms, acc = integ.integrate_sde(cu(g["x1"]), e, gam, inverse_temperature=1.0, noise=noise)
        outs[rec] = x
        # measured on MI355X (printed; profiles/r05_parity_measured.txt); bounds 4 x measured
        print(f"[traj20/{'per-step' if rec else 'fused'}] final walkers vs the reference's rel-L2 {rel(x, g['x_final']):.2e}")
        assert rel(x, g["x_final"]) < _TRAJ20_BOUNDS[0]
        assert logw.shape == (N, 32) and float(logw.abs().max()) == 0 and uniq == [32] * N and acc == []
        if rec:
            assert len(terms) == N
            worst = max(rel(terms[k].drift_X, g["drift_X"][k]) for k in range(N))
            print(f"[traj20/per-step] drift at identical inputs (step 0) {rel(terms[0].drift_X, g['drift_X'][0]):.2e}, worst step "
                  f"along the run {worst:.2e}")
            assert rel(terms[0].drift_X, g["drift_X"][0]) < _TRAJ20_BOUNDS[1]  # per-step drift at identical inputs
            assert worst < _TRAJ20_BOUNDS[2]
    print(f"[traj20] fused launch vs per-step launches {rel(outs[False], outs[True]):.2e}")
    assert rel(outs[False], outs[True]) < _TRAJ20_BOUNDS[3]  # fused launch == per-step launches
    # drift_out of the fused kernel, one step from the golden state
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, N + 1)[:-1], 1.0 / N, 1.0, 1.0)
    x = cu(g["x1"]).clone()
    drift = torch.empty_like(x)
    net.sampler_run(x, tab[:1].cuda().contiguous(), 1, noise=noise[:1].contiguous(), drift_out=drift)
    assert rel(drift, g["drift_X"][0]) < 1e-4


def pcg_noise(seed, N, B, D):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((N, B, D), dtype=np.float32)


_TRUTH_1000 = {}


def _truth_1000(g, w, n, noise_h, at):
    N = int(g["N"])
    wd = {k: T(v).double() for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_forward(wd, cn, xs, b, n, 3)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    nz64 = T(noise_h).double()
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(16, nthreads))
    try:
        out = O.integrate_sde(O.IntegratorConfig(num_integration_steps=N, end_resampling_step=N), T(g["x1"]).double(),
                              lambda t, xc: O.f_not_debiased(bb, osched, ogam, t, xc, 1.0), osched.g, lambda i, shp: nz64[i],
                              n, 3, record=True)
    finally:
        torch.set_num_threads(nthreads)
    return [g["x1"].astype(np.float64)] + [out["traj"][a - 1].numpy() for a in at[1:]]


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("n", [13, 55])
def test_traj_1000_steps_golden(pa, golden, precision, n):
    """Parity at the metric's own trajectory length: the reference's integrate_sde, LJ13, N = 1 000 (experiment/lj13.yaml),
    fixed PCG64 noise, walkers recorded every 100 steps.  The fused HIP sampler fed the same noise must stay as close
    to fp64 arithmetic as the fp32 reference does -- err(HIP, fp64 oracle) <= 4 x err(reference, fp64 oracle) -- at every
    checkpoint, through the small-h end (h -> 2.5e-3) where score = (D - x)/h amplifies rounding 400x."""
    g = golden(f"em_traj_lj{n}_1000.npz")  # LJ55: config C5's system, 4 walkers, checkpoints every 250 steps
    D = 3 * n
    w = golden("egnn_weights_trainedlike.npz")
    N, B = int(g["N"]), int(g["B"])
    noise_h = pcg_noise(int(g["seed"]), N, B, D)
    at = [int(a) for a in g["at"]] + [N]
    want = list(g["x_at"]) + [g["x_final"]]
    # fp64 oracle on the same noise (once per system: shared by the three arithmetic modes; 16 threads -- these small ops
    # only lose time on the 256 hardware threads of the GPU box's host)
    if n not in _TRUTH_1000:
        _TRUTH_1000[n] = _truth_1000(g, w, n, noise_h, at)
    truth = _TRUTH_1000[n]
    # HIP: ten launches of 100 steps (bitwise equal to one launch of 1 000, tested elsewhere), walkers read in between
    net = make_net(pa, n, 3, w, precision=precision).cuda()
    sched, gam = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7), pa.ConstantAnnealingFactorSchedule(4 / 3)
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, N + 1)[:-1], 1.0 / N, 1.0, 1.0).cuda()
    noise = cu(noise_h)
    x = cu(g["x1"]).clone()
    got = [x.cpu().numpy()]
    every = at[1] - at[0]
    for s0 in range(0, N, every):
        net.sampler_run(x, tab[s0:s0 + every].contiguous(), every, noise=noise[s0:s0 + every].contiguous(), step0=s0,
                        remove_mean=True, n_particles=n, n_dim=3)
        got.append(x.cpu().numpy())
    for k, a in enumerate(at):
        e_ref, e_hip = rel(want[k], truth[k]), rel(got[k], truth[k])
        print(f"[traj1000/lj{n}/{precision}] step {a:4d}: HIP vs fp64 {e_hip:.2e}, reference vs fp64 {e_ref:.2e}, HIP vs reference {rel(got[k], want[k]):.2e}")
        assert e_hip <= 4 * e_ref, (a, e_hip, e_ref)
    # the whole trajectory through the integrator front end in one launch gives the same walkers
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), debias_inference=False)
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                     resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0)
    xi, *_ = integ.integrate_sde(cu(g["x1"]), pa.LennardJonesEnergy(D, n, 3), gam, inverse_temperature=1.0, noise=noise)
    assert torch.equal(xi, x)


def test_sampler_sharding_invariance_and_determinism(pa, golden):
    """Philox noise is keyed by the global walker index: integrating two half batches with the
    right walker_offset reproduces the full batch bit for bit; reruns are bitwise identical."""
    sde, sched, net = lj13_stack(pa, golden)
    N, B = 12, 4096 + 5
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, N + 1)[:-1], 1.0 / N, 1.0, 1.0).cuda()
    prior = pa.Prior(scale=69.28, n_particles=13, spatial_dim=3, seed=5)
    x0 = prior.sample(B)
    assert abs(x0.reshape(B, 13, 3).mean(1)).max() < 1e-4
    a = net.sampler_run(x0.clone(), tab, N, seed=11)
    b = net.sampler_run(x0.clone(), tab, N, seed=11)
    assert torch.equal(a, b)
    h = 2003
    c0 = net.sampler_run(x0[:h].clone(), tab, N, seed=11, walker_offset=0)
    c1 = net.sampler_run(x0[h:].clone(), tab, N, seed=11, walker_offset=h)
    assert torch.equal(torch.cat([c0, c1]), a)
    # chunking the steps over launches is also exact (step0 keys the noise)
    d = net.sampler_run(x0.clone(), tab[:5].contiguous(), 5, seed=11, step0=0)
    d = net.sampler_run(d, tab[5:].contiguous(), N - 5, seed=11, step0=5)
    assert torch.equal(d, a)
    assert abs(a.reshape(B, 13, 3).mean(1)).max() < 1e-4 and torch.isfinite(a).all()
    assert not torch.equal(net.sampler_run(x0.clone(), tab, N, seed=12), a)


def test_philox_normals(pa):
    out = torch.empty(200000, 39, device="cuda")
    pa._lib.check(pa._lib.lib().pita_fill_normal(out.data_ptr(), 200000, 13, 3, 42, 0, 7, pa._lib.stream_ptr()))
    v = out.double()
    assert abs(v.mean().item()) < 2e-3 and abs(v.std().item() - 1) < 2e-3
    assert abs((v**4).mean().item() - 3) < 3e-2  # kurtosis
    assert abs(torch.corrcoef(v[:, :4].T)[0, 1].item()) < 1e-2


from tests._step_shapes import _philox_normals_host  # noqa: E402  (shared with tests/test_step_shapes_gpu.py)


def test_philox_matches_host_restatement(pa):
    """The in-kernel generator is exactly the documented counter layout (walker, step, particle) -> 3 normals."""
    B, off, step, seed = 1000, (1 << 33) + 5, (3 << 32) + 9, 0x1234567890ABCDEF
    out = torch.empty(B, 39, device="cuda")
    pa._lib.check(pa._lib.lib().pita_fill_normal(out.data_ptr(), B, 13, 3, seed, off, step, pa._lib.stream_ptr()))
    want = _philox_normals_host(seed, off + np.arange(B), step, np.arange(13)).reshape(B, 39)
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=2e-5, rtol=1e-5)


def test_elementwise_vs_oracle(pa, golden):
    g = golden("prior.npz")
    for n, d in ((13, 3), (4, 2)):
        nz = cu(g[f"noise_{n}"])
        p = pa.Prior(scale=float(g["scale"]), n_particles=n, spatial_dim=d)
        np.testing.assert_allclose(p.sample(16, noise=nz).cpu().numpy(), g[f"sample_{n}"], rtol=1e-6, atol=2e-5)
        np.testing.assert_allclose(pa.data_utils.remove_mean(nz, n, d).cpu().numpy(), g[f"remove_mean_{n}"],
                                   rtol=1e-6, atol=1e-6)
    gen = torch.Generator().manual_seed(1)
    x, dr, nz = (torch.randn(777, 39, generator=gen) for _ in range(3))
    xo = O.remove_mean(x + (dr * 0.05 + (1.7 * nz) * np.sqrt(0.05)), 13, 3)
    xc, drc, nzc = x.cuda().clone(), dr.cuda(), nz.cuda()  # keep the device copies alive across the async call
    L = pa._lib.lib()
    pa._lib.check(L.pita_em_step(xc.data_ptr(), drc.data_ptr(), nzc.data_ptr(), 777, 13, 3, 0.05, 1.7,
                                 float(np.sqrt(0.05)), 0, 0, 0, 1, 0, pa._lib.stream_ptr()))
    np.testing.assert_allclose(xc.cpu().numpy(), xo.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", ["normal", "ties", "peaked", "neginf", "huge", "big"])
def test_resample_golden(pa, golden, case):
    g = golden("resample_sys.npz")
    logits = cu(g[f"logits_{case}"])
    ids, _ = pa.utils.sample_cat_sys(logits.shape[0], logits, u=float(g[f"u_{case}"][0]))
    ids = ids.cpu().numpy()
    want = g[f"ids_{case}"]
    bad = ids != want
    print(f"[resample/{case}] {int(bad.sum())} of {len(ids)} ids differ from the reference's")
    # index work is exact except where a uniform lies within fp32 rounding of a bin edge: the reference's softmax sums
    # its exponentials in the vector-lane order of the host CPU, which no other summation reproduces bit for bit
    assert bad.sum() <= max(2, len(ids) // 2000) and (np.abs(ids[bad] - want[bad]) <= 1).all(), (bad.sum(), len(ids))
    assert (np.diff(ids) >= 0).sum() >= len(ids) - 2  # sorted up to the single wrap of (u0 + k/B) mod 1
    x = torch.arange(logits.shape[0] * 3, dtype=torch.float32, device="cuda").reshape(-1, 3)
    got = pa.utils.gather_rows(x, torch.as_tensor(want).cuda())
    assert torch.equal(got, x[torch.as_tensor(want).cuda()])


def test_count_runs_kernel_equals_np_unique(pa):
    """pita_count_runs (round 6: the distinct-parent count of a resampling event in ONE launch instead of roll + != + cast +
    sum + clamp) against len(np.unique(ids)) -- sde_integration.py:295 -- on reference-shaped id vectors: constant, strictly
    increasing, runs that wrap around the end, and the kernel's own ids at 1, 2, 1 000, 65 536 and 262 144 walkers."""
    from pita_amd.sde_integration import _count_distinct, _host_counts
    from pita_amd.utils import sample_cat_sys

    gen = torch.Generator().manual_seed(3)
    cases = [torch.zeros(17, dtype=torch.int64), torch.arange(9), torch.tensor([3, 3, 4, 7, 7, 0, 0, 3]),
             torch.tensor([5, 5, 5, 1, 1, 5]), torch.zeros(1, dtype=torch.int64), torch.arange(5000)]
    cases = [c.cuda() for c in cases]
    for B in (1, 2, 1000, 65536, 262144):
        for spread in (0.1, 3.0, 30.0):
            logits = (torch.randn(B, generator=gen) * spread).cuda()
            for u0 in (0.0, 0.37, 0.999):
                cases.append(sample_cat_sys(B, logits, torch.tensor([u0], dtype=torch.float64))[0])
    counts = [_count_distinct(c) for c in cases]
    assert all(c.is_cuda and c.dim() == 0 and c.dtype == torch.int64 for c in counts)
    assert _host_counts(list(counts)) == [len(np.unique(c.cpu().numpy())) for c in cases]


def test_resample_global_batch_of_config_c5(pa):
    """262 144 walkers (config C5's global batch): ids against the oracle, sortedness, every id a valid walker; the
    multi-block passes are timed (printed) so the cost of a global resampling event is on record."""
    B = 262144
    gen = torch.Generator().manual_seed(9)
    logits = torch.randn(B, generator=gen)
    u0 = 0.7312345678901234
    want = O.sample_cat_sys(logits, u0)
    lg = logits.cuda()
    ids, _ = pa.utils.sample_cat_sys(B, lg, u=u0)
    got = ids.cpu().numpy()
    bad = got != want
    print(f"[resample/C5] {int(bad.sum())} of {B} ids differ from the fp32 oracle's (all by one)")
    # At this size the reference's own fp32 softmax denominator (a vector-lane sum of 262 144 terms) is off by ~1e-7
    # relative, a few percent of one walker's weight by the end of the cumulative sum: ids shift by one for ~10 % of
    # the walkers, depending on the host CPU's lane count.  Exactness is therefore checked against the same arithmetic
    # carried out with exact (double) sums -- which the kernel must reproduce bit for bit -- and the fp32 oracle
    # bounds the deviation: never more than one position.
    assert (np.abs(got - want) <= 1).all()
    l64 = logits.numpy().astype(np.float32)
    e = np.exp((l64 - l64.max()).astype(np.float64)).astype(np.float32)
    sm = np.float32(e.astype(np.float64).sum())
    w = np.clip(e / sm, np.float32(1e-6), np.float32(1.0)).astype(np.float32)
    bins = np.cumsum(w.astype(np.float64)).astype(np.float32)
    u = (u0 + (np.arange(B, dtype=np.float32) * np.float32(1.0 / B)).astype(np.float64)) % 1.0
    exact = np.minimum(np.searchsorted(bins.astype(np.float64), u, side="left"), B - 1)
    nbad = int((got != exact).sum())
    print(f"[resample/C5] {nbad} of {B} ids differ from the double-sum restatement")
    assert nbad <= 2
    assert got.min() >= 0 and got.max() < B and (np.diff(got) >= 0).sum() >= B - 2
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        pa.utils.sample_cat_sys(B, lg, u=u0)
    e1.record()
    torch.cuda.synchronize()
    print(f"[resample/C5] {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per global resampling event at {B} walkers")


@pytest.mark.parametrize("n", [13, 55])
def test_post_processing_golden(pa, golden, n):
    """The reference's negative-time descent, Langevin descent, MALA and adaptive MALA (recorded noise and uniforms) on the
    LJ13 and LJ55 targets: the fused chains (lj13 kernels / ring kernels) reproduce walkers and acceptance rates."""
    g = golden(f"post_lj{n}.npz")
    dtm = float(g["dt_mala"])
    e = pa.LennardJonesEnergy(3 * n, n, 3)
    mk = lambda **kw: pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                               end_resampling_step=1, **kw)
    x0 = cu(g["x0"])
    xd = mk(num_negative_time_steps=25, dt_negative_time=1e-4).negative_time_descent(x0, e)
    assert rel(xd, g["x_descent"]) < 1e-5
    xl = mk(num_negative_time_steps=10, dt_negative_time=1e-4, do_langevin=True).negative_time_descent(
        x0, e, noise=cu(g["langevin_noise"]))
    assert rel(xl, g["x_langevin"]) < 1e-5
    xm, acc = mk(post_mcmc_steps=6, dt_negative_time=dtm).metropolis_hastings_mala(
        x0, e, return_acceptance_rate=True, noise=cu(g["mala_noise"]), uniforms=cu(g["mala_u"]))
    np.testing.assert_allclose(acc, g["mala_acc"], atol=1e-7)
    assert rel(xm, g["x_mala"]) < 1e-5
    xa, acc = mk(post_mcmc_steps=6, dt_negative_time=dtm, adaptive_mcmc=True).metropolis_hastings_mala_adaptive(
        x0, e, dt_init=dtm, return_acceptance_rate=True, noise=cu(g["mala_adaptive_noise"]),
        uniforms=cu(g["mala_adaptive_u"]))
    np.testing.assert_allclose(acc, g["mala_adaptive_acc"], atol=1e-7)
    assert rel(xa, g["x_mala_adaptive"]) < 1e-5


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("B,steps", [(777, 6), (128, 3), (5, 4), (65536, 5), (70001, 3)])
def test_fused_mala_equals_per_step(pa, golden, B, steps, adaptive):
    """pita_lj_mala (all steps, both target evaluations per step, accept / reject and step-size adaptation in fused
    launches) == the launch-per-kernel chain, bit for bit: walkers, acceptance rates, with Philox and with injected noise
    / uniforms, with and without centring, ragged and full blocks, with a walker that is set aside (quirk Q7), and with
    more tiles than blocks in the grid (70 001 walkers: a block then takes several tiles per launch)."""
    g = golden("post_lj13.npz")
    e = pa.LennardJonesEnergy(39, 13, 3)
    gen = torch.Generator().manual_seed(B + steps)
    base = T(g["x0"])
    x0 = base[torch.arange(B) % base.shape[0]] + 0.02 * torch.randn(B, 39, generator=gen)
    x0 = O.remove_mean(x0, 13, 3).cuda()
    for mean_free in (True, False):
        for inject in (False, True):
            if inject and B > 1000:
                continue
            kw = {}
            if inject:
                kw = dict(noise=torch.randn(steps, B, 39, generator=gen).cuda(),
                          uniforms=torch.rand(steps, B, generator=gen).cuda())
            outs = []
            for fused in (True, False):
                integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                                 end_resampling_step=1, post_mcmc_steps=steps, dt_negative_time=3e-4,
                                                 adaptive_mcmc=adaptive, should_mean_free=mean_free, seed=9)
                if adaptive:
                    outs.append(integ.metropolis_hastings_mala_adaptive(x0.clone(), e, dt_init=3e-4,
                                                                        return_acceptance_rate=True, fused=fused, **kw))
                else:
                    outs.append(integ.metropolis_hastings_mala(x0.clone(), e, return_acceptance_rate=True, fused=fused, **kw))
            assert torch.equal(outs[0][0], outs[1][0]), (mean_free, inject)
            assert outs[0][1] == outs[1][1] and len(outs[0][1]) == steps
            if B >= 100:
                assert 0.0 < max(outs[0][1]) and min(outs[0][1]) < 1.0  # a chain that actually accepts and rejects
    if B == 777:  # a non-finite walker in the middle: Philox keys follow the original indices in both paths
        xb = x0.clone()
        xb[300, 0] = float("inf")  # log p is not finite: the walker is set aside and re-appended last
        outs = []
        for fused in (True, False):
            integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                             end_resampling_step=1, post_mcmc_steps=steps, dt_negative_time=3e-4,
                                             adaptive_mcmc=adaptive, seed=9)
            fn = integ.metropolis_hastings_mala_adaptive if adaptive else integ.metropolis_hastings_mala
            akw = dict(dt_init=3e-4) if adaptive else {}
            outs.append(fn(xb.clone(), e, return_acceptance_rate=True, fused=fused, **akw))
        assert torch.equal(outs[0][0][:-1], outs[1][0][:-1]) and outs[0][1] == outs[1][1]
        assert integ._last_mala_valid == B - 1 and torch.isinf(outs[0][0][-1, 0]) and torch.isinf(outs[1][0][-1, 0])


def _ring_target(pa, name, B, gen):
    """LJ55 / DW4 target with B jittered near-equilibrium walkers (chains that accept and reject)."""
    if name == "lj55":
        e, n, d = pa.LennardJonesEnergy(165, 55, 3), 55, 3
        r = 3
        grid = np.stack(np.meshgrid(*[np.arange(-r, r + 1)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        pts = grid[np.argsort((grid**2).sum(-1), kind="stable")[:55]] * 1.09
        base = torch.tensor(pts, dtype=torch.float32).reshape(1, 165)
        x0 = base + 0.03 * torch.randn(B, 165, generator=gen)
    else:
        e, n, d = pa.MultiDoubleWellEnergy(temperature=1.0), 4, 2
        base = torch.tensor([[2.0, 2.0], [-2.0, 2.0], [-2.0, -2.0], [2.0, -2.0]]).reshape(1, 8)
        x0 = base + 0.3 * torch.randn(B, 8, generator=gen)
    return e, n, d, O.remove_mean(x0, n, d).cuda()


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("name,B,steps,dt", [("lj55", 301, 5, 2e-4), ("lj55", 3, 4, 2e-4), ("lj55", 10007, 3, 2e-4),
                                             ("dw4", 1000, 6, 0.05), ("dw4", 37, 4, 0.05), ("dw4", 65536, 3, 0.05),
                                             ("dw4", 700001, 3, 0.05)])
def test_fused_ring_mala_equals_per_step(pa, name, B, steps, dt, adaptive):
    """pita_lj_mala (LJ55) / pita_dw_mala (DW4): the ring-kernel chains == the launch-per-kernel chain, bit for bit --
    walkers, acceptance rates; Philox and injected noise / uniforms; with and without centring; ragged wave groups; a
    batch beyond one residency of the grid (LJ55 10 007 walkers = 10 007 wave groups > 8 192 resident waves; DW4 700 001
    walkers), where a wave takes several groups per launch."""
    gen = torch.Generator().manual_seed(B + steps)
    e, n, d, x0 = _ring_target(pa, name, B, gen)
    D = n * d
    for mean_free in (True, False):
        for inject in (False, True):
            if inject and B * D > 2_000_000:
                continue
            kw = {}
            if inject:
                kw = dict(noise=torch.randn(steps, B, D, generator=gen).cuda(), uniforms=torch.rand(steps, B, generator=gen).cuda())
            outs = []
            for fused in (True, False):
                integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                                 end_resampling_step=1, post_mcmc_steps=steps, dt_negative_time=dt,
                                                 adaptive_mcmc=adaptive, should_mean_free=mean_free, seed=9)
                if adaptive:
                    outs.append(integ.metropolis_hastings_mala_adaptive(x0.clone(), e, dt_init=dt, return_acceptance_rate=True,
                                                                        fused=fused, **kw))
                else:
                    outs.append(integ.metropolis_hastings_mala(x0.clone(), e, return_acceptance_rate=True, fused=fused, **kw))
            assert torch.equal(outs[0][0], outs[1][0]), (mean_free, inject)
            assert outs[0][1] == outs[1][1] and len(outs[0][1]) == steps
            assert torch.isfinite(outs[0][0]).all()
            if B >= 100:
                assert 0.0 < max(outs[0][1]) and min(outs[0][1]) < 1.0, outs[0][1]  # a chain that accepts and rejects
    if B in (301, 1000):  # a non-finite walker in the middle is set aside: Philox keys follow the ORIGINAL indices
        xb = x0.clone()
        xb[B // 3, 1] = float("inf")
        outs = []
        for fused in (True, False):
            integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                             end_resampling_step=1, post_mcmc_steps=steps, dt_negative_time=dt,
                                             adaptive_mcmc=adaptive, seed=9)
            fn = integ.metropolis_hastings_mala_adaptive if adaptive else integ.metropolis_hastings_mala
            akw = dict(dt_init=dt) if adaptive else {}
            outs.append(fn(xb.clone(), e, return_acceptance_rate=True, fused=fused, **akw))
        assert torch.equal(outs[0][0][:-1], outs[1][0][:-1]) and outs[0][1] == outs[1][1]
        assert integ._last_mala_valid == B - 1 and torch.isinf(outs[0][0][-1, 1]) and torch.isinf(outs[1][0][-1, 1])
    # the chain follows the oracle's MALA step (fp32 rounding may flip an accept decision whose log-ratio is within 1e-5)
    if B <= 1000:
        steps_o = 2
        noise = torch.randn(steps_o, B, D, generator=gen)
        us = torch.rand(steps_o, B, generator=gen)
        integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                         post_mcmc_steps=steps_o, dt_negative_time=dt, should_mean_free=True)
        out, rates = integ.metropolis_hastings_mala(x0.clone(), e, return_acceptance_rate=True, noise=noise.cuda(),
                                                    uniforms=us.cuda())
        lf = (lambda xx: O.lj_logp_force(xx, 55, 3)) if name == "lj55" else (lambda xx: O.dw4_logp_force(xx))
        xv = x0.cpu().double()
        lp = lf(xv)[0]
        for k in range(steps_o):
            xv, lp, acc = O.mala_step(xv, lp, lf, dt, noise[k].double(), torch.log(us[k].double()))
            xv = O.remove_mean(xv, n, d)
        same = (out.cpu().double() - xv).abs().amax(dim=1) < 1e-4
        assert same.float().mean() > 0.99, float(same.float().mean())


def _mala_target(pa, golden, name, B, gen):
    """(target, n, d, MALA step size, B near-equilibrium walkers) of the three targets with a fused pair-target chain."""
    if name != "lj13":
        e, n, d, x0 = _ring_target(pa, name, B, gen)
        return e, n, d, (2e-4 if name == "lj55" else 0.05), x0
    base = T(golden("post_lj13.npz")["x0"])
    x0 = O.remove_mean(base[torch.arange(B) % base.shape[0]] + 0.02 * torch.randn(B, 39, generator=gen), 13, 3).cuda()
    return pa.LennardJonesEnergy(39, 13, 3), 13, 3, 3e-4, x0


@pytest.mark.parametrize("name", ["lj13", "lj55", "dw4"])
def test_fused_adaptive_mala_barrier_timeout_falls_back(pa, golden, name):
    """The adaptive fused chain on a device that is NOT idle (the condition its former per-step grid barrier could not
    tolerate): while a second stream holds tens of milliseconds of matmuls, the chain on the current stream -- through
    the integrator and through the C ABI -- still equals the launch-per-kernel chain computed on the idle device, bit
    for bit, with finite rates and step size, and the integrator has no rerun protocol left to count."""
    steps, (e, n, d, dt, x0) = 4, _mala_target(pa, golden, name, 2000, torch.Generator().manual_seed(5))
    mk = lambda: pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                          post_mcmc_steps=steps, dt_negative_time=dt, adaptive_mcmc=True, seed=3)
    want = mk().metropolis_hastings_mala_adaptive(x0.clone(), e, dt_init=dt, return_acceptance_rate=True, fused=False)
    lp, xc, rates = e(x0), x0.clone(), torch.zeros(steps, device="cuda")
    dt_dev = torch.tensor([dt], device="cuda", dtype=torch.float64)
    a, side, integ = torch.randn(8192, 8192, device="cuda"), torch.cuda.Stream(), mk()
    a @ a  # (the library's first-call set-up is not part of the queued work)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(6):
            a @ a
    got = integ.metropolis_hastings_mala_adaptive(x0.clone(), e, dt_init=dt, return_acceptance_rate=True)
    assert e.fused_mala(xc, lp, steps, dt_dev, True, x0.shape[0], seed=mk()._key(2), remove_mean=e.is_molecule,
                        rates_out=rates) is not None
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and not any("fallback" in k for k in vars(integ))
    assert torch.equal(xc, want[0]) and rates.tolist() == want[1] and torch.isfinite(rates).all() and torch.isfinite(dt_dev).all()


@pytest.mark.parametrize("name,B", [("lj13", 300), ("lj55", 37), ("dw4", 300)])
def test_fused_adaptive_mala_final_step_size(pa, golden, name, B):
    """The step size an adaptive fused chain leaves in dt_dev == the float64 replay of the adaptation rule over the rates
    it returns (the same IEEE operations) == the dt_dev the launch-per-kernel loop (pita_mala_adapt) leaves, bit for bit."""
    steps, key, (e, n, d, dt, x0) = 6, 7, _mala_target(pa, golden, name, B, torch.Generator().manual_seed(B))
    new = lambda: (x0.clone(), e(x0), torch.tensor([dt], device="cuda", dtype=torch.float64), torch.zeros(steps, device="cuda"))
    x, lp, dt_dev, rates = new()
    assert e.fused_mala(x, lp, steps, dt_dev, True, B, seed=key, rates_out=rates) is not None
    replay = dt
    for r in rates.tolist():  # mala_adapt_kernel's rule in float64
        replay = replay * 1.1 if r > 0.55 else replay / 1.1
    assert dt_dev.item() == replay
    L, st, check = pa._lib.lib(), pa._lib.stream_ptr(x0.device), pa._lib.check
    (xk, lpk, dtk, rk), xp, count = new(), torch.empty_like(x), torch.zeros(1, device="cuda", dtype=torch.int32)
    for i in range(steps):
        _, F = e(xk, return_force=True)
        check(L.pita_mala_propose(xk.data_ptr(), F.data_ptr(), xp.data_ptr(), 0, B, n, d, dtk.data_ptr(), key, 0, 0, i, st))
        lpp, Fp = e(xp, return_force=True)
        check(L.pita_mala_accept(xk.data_ptr(), lpk.data_ptr(), F.data_ptr(), xp.data_ptr(), lpp.data_ptr(), Fp.data_ptr(), 0,
                                 B, n, d, dtk.data_ptr(), key, 0, 0, i, 1, count.data_ptr(), st))
        check(L.pita_mala_adapt(dtk.data_ptr(), count.data_ptr(), B, 1, rk[i:].data_ptr(), st))
    assert torch.equal(dtk, dt_dev) and torch.equal(rk, rates) and torch.equal(xk, x) and torch.equal(lpk, lp)


@pytest.mark.parametrize("adaptive", [False, True])
def test_fused_ring_mala_step_index_past_the_lds_counters(pa, adaptive):
    """520 steps of DW4 on ragged quad groups: the smallest chain whose step index passes the ring kernel's 512 per-block
    LDS counters (later steps are counted in global memory); walkers and all 520 rates equal the launch-per-kernel chain."""
    steps, outs = 520, []
    e, n, d, x0 = _ring_target(pa, "dw4", 37, torch.Generator().manual_seed(steps))
    for fused in (True, False):
        integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                         post_mcmc_steps=steps, dt_negative_time=0.05, adaptive_mcmc=adaptive, seed=9)
        fn = integ.metropolis_hastings_mala_adaptive if adaptive else integ.metropolis_hastings_mala
        outs.append(fn(x0.clone(), e, return_acceptance_rate=True, fused=fused, **(dict(dt_init=0.05) if adaptive else {})))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and len(outs[0][1]) == steps
    assert max(outs[0][1][512:]) > 0.0, "the steps past the LDS counters must count too"


def test_mala_sets_non_finite_walkers_aside(pa, golden):
    """Quirk Q7 (sde_integration.py:366-369,400): walkers whose target log-density is not finite are taken out before
    the chain and re-appended AFTER the valid ones (order not preserved); the chain itself runs on the valid rows with
    the acceptance rate computed over them."""
    g = golden("post_lj13.npz")
    e = pa.LennardJonesEnergy(39, 13, 3)
    x0 = torch.as_tensor(g["x0"], dtype=torch.float32)
    B = x0.shape[0]
    bad = torch.tensor([1, 7, B - 1])
    x = x0.clone()
    x[bad[0]] = float("nan")
    x[bad[1], 5] = float("inf")
    x[bad[2]] = torch.arange(39, dtype=torch.float32) * 3e19  # squared distances overflow -> logp = -inf
    keep = torch.ones(B, dtype=torch.bool)
    keep[bad] = False
    nv = int(keep.sum())
    steps, dt = 4, 4e-4
    gen = torch.Generator().manual_seed(9)
    noise = torch.randn(steps, nv, 39, generator=gen)
    us = torch.rand(steps, nv, generator=gen)
    integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                     post_mcmc_steps=steps, dt_negative_time=dt)
    out, rates = integ.metropolis_hastings_mala(x.cuda(), e, return_acceptance_rate=True, noise=noise.cuda(),
                                                uniforms=us.cuda())
    assert out.shape == x.shape and len(rates) == steps
    tail = out[nv:].cpu()
    assert torch.isnan(tail[0]).all() and torch.isinf(tail[1, 5]) and torch.equal(tail[2], x[bad[2]])
    lf = lambda xx: O.lj_logp_force(xx, 13, 3)
    xv = x0[keep].clone()
    lp = O.lj_logp(xv, 13, 3)
    want_rates = []
    for k in range(steps):
        xv, lp, acc = O.mala_step(xv, lp, lf, dt, noise[k], torch.log(us[k]))
        xv = O.remove_mean(xv, 13, 3)
        want_rates.append(float(acc.float().mean()))
    np.testing.assert_allclose(rates, want_rates, atol=1e-7)
    assert rel(out[:nv], xv) < 1e-5


@pytest.mark.parametrize("target", ["lj13", "lj13_ragged", "lj55", "dw4", "ff22", "ff22_gb"])
@pytest.mark.parametrize("langevin", [False, True])
def test_fused_descent_equals_per_step(pa, golden, target, langevin):
    """pita_lj_descent / pita_dw_descent / (round 6) pita_ff_descent keep the walkers in LDS for all steps; they must
    reproduce the per-step path (force kernel + pita_em_step) bit for bit, with injected and with Philox noise, and follow
    the oracle.  ff22: the table-driven force field on the synthetic 22-atom peptide (cutoff + reaction field; _gb: with the
    GB-OBC1 solvent), 4 099 walkers = the C4 shard plus a ragged last block."""
    gen = torch.Generator().manual_seed(7)
    if target.startswith("ff22"):
        from pita_amd.alp_energy import ForceFieldEnergy

        tabs, pos = _synthetic_peptide()
        if target.endswith("gb"):
            rng = np.random.default_rng(3)
            tabs["gb_radius"] = rng.choice([0.12, 0.13, 0.15, 0.155, 0.17], 22)
            tabs["gb_scale"] = rng.choice([0.72, 0.79, 0.85], 22)
        ff_t = {k: torch.as_tensor(v) for k, v in tabs.items()}
        ff_t = {k: (v.long() if "idx" in k else v.double()) for k, v in ff_t.items()}
        scale, n, d = 0.1640, 22, 3
        e = ForceFieldEnergy(tabs, n_particles=22, temperature=300.0, data_normalization_factor=scale, cutoff=0.45)
        x0 = ((torch.tensor(pos.reshape(-1), dtype=torch.float32)[None] + 0.004 * torch.randn(4099, 66, generator=gen)) / scale).cuda()
        lf = lambda x: O.ff_logp_force(x.double(), ff_t, e.kT, scale, 0.45)
    elif target.startswith("lj13"):
        e, n, d = pa.LennardJonesEnergy(39, 13, 3), 13, 3
        x0 = cu(golden("post_lj13.npz")["x0"])
        x0 = x0.repeat(9, 1)[: (577 if target.endswith("ragged") else 512)]
        x0 = x0 + 0.01 * torch.randn(x0.shape, generator=gen).cuda()
        lf = lambda x: O.lj_logp_force(x, 13, 3)
    elif target == "lj55":
        e, n, d = pa.LennardJonesEnergy(165, 55, 3), 55, 3
        g = golden("lj55_logp_force.npz")
        x0 = cu(g["x"][: int(g["n_cold"])]).repeat(3, 1)[:37]
        lf = lambda x: O.lj_logp_force(x, 55, 3)
    else:
        e, n, d = pa.MultiDoubleWellEnergy(8, 4, 2), 4, 2
        x0 = (torch.randn(1000, 8, generator=gen) * 1.5).cuda()
        lf = lambda x: O.dw4_logp_force(x, 4, 2)
    S, dt = 12, 1e-4
    if target.startswith("ff22"):
        S, dt = 6, 1e-7  # forces of a stiff molecule are ~1e4 in model units
    mk = lambda: pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                          end_resampling_step=1, num_negative_time_steps=S, dt_negative_time=dt,
                                          do_langevin=langevin, seed=3)
    xf = mk().negative_time_descent(x0, e, walker_offset=11)
    xs = mk().negative_time_descent(x0, e, walker_offset=11, fused=False)
    assert torch.equal(xf, xs)
    assert not torch.equal(xf, x0)
    nz = torch.randn(S, x0.shape[0], n * d, generator=gen)
    xf = mk().negative_time_descent(x0, e, noise=nz.cuda())
    xs = mk().negative_time_descent(x0, e, noise=nz.cuda(), fused=False)
    assert torch.equal(xf, xs)
    if target.startswith("ff22"):  # the fp64 oracle on a sample of the walkers
        sel = torch.arange(0, x0.shape[0], 173)
        xo = O.negative_time_descent(x0.cpu()[sel], lf, S, dt, n, d, do_langevin=langevin, noise_fn=lambda k, s: nz[k][sel])
        assert rel(xf[sel.cuda()], xo) < 1e-5
        return
    xo = O.negative_time_descent(x0.cpu(), lf, S, dt, n, d, do_langevin=langevin, noise_fn=lambda k, s: nz[k])
    assert rel(xf, xo) < 1e-5


# ------------------------------------------------------------------------------- full size (BASELINE configs)
def test_full_size_lj13_properties(pa, golden):
    """LJ13 @ 65 536 walkers (config C3): size-independent properties of the force kernel and of
    the sampler -- force is the gradient of logp (directional finite difference in fp64 oracle on a
    sample), translation invariance of logp's pair part, permutation equivariance, mean-free."""
    B = 65536
    gen = torch.Generator().manual_seed(123)
    base = T(golden("lj13_logp_force.npz")["x"][:48])
    x = (base[torch.randint(0, 48, (B,), generator=gen)] + 0.03 * torch.randn(B, 39, generator=gen)).cuda()
    e = pa.LennardJonesEnergy(39, 13, 3)
    lp, f = e(x, return_force=True)
    assert torch.isfinite(lp).all() and torch.isfinite(f).all()
    idx = torch.randint(0, B, (256,), generator=gen)
    lpo, fo = O.lj_logp_force(x[idx.cuda()].cpu().double(), 13, 3)
    np.testing.assert_allclose(lp[idx.cuda()].cpu().numpy(), lpo.numpy(), rtol=1e-5)
    assert rel(f[idx.cuda()], fo) < 1e-5
    # total force on the centre of mass is zero (pair forces cancel, oscillator is mean-free)
    assert abs(f.reshape(B, 13, 3).sum(1)).max() < 2e-2
    # permutation of particles permutes forces and keeps logp
    perm = torch.randperm(13, generator=gen)
    xp = x.reshape(B, 13, 3)[:, perm.cuda()].reshape(B, 39).contiguous()
    lpp, fp = e(xp, return_force=True)
    np.testing.assert_allclose(lpp.cpu().numpy(), lp.cpu().numpy(), rtol=2e-5, atol=3e-5)
    assert rel(fp, f.reshape(B, 13, 3)[:, perm.cuda()].reshape(B, 39)) < 1e-5
    # the fused sampler at the metric's batch: one step of all 65 536 walkers, a sample of them against the oracle
    _one_step_vs_oracle(pa, golden, 13, 3, B, 0.05)


def _one_step_vs_oracle(pa, golden, n, d, B, sigma_min, subset=24, seed=0):
    """One fused sampler step at full batch; a random subset of walkers is re-computed by the oracle."""
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, n, d, w)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=sigma_min, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    N = 50
    k0 = 37  # a mid-trajectory step (h ~ 1e2)
    times = torch.linspace(1.0, 0.0, N + 1)[:-1]
    tab = pa.sde_integration.build_step_table(sched, gam, times, 1.0 / N, 1.0, 1.0)
    gen = torch.Generator().manual_seed(seed)
    h_k = float(tab[k0, pa._lib.ST_H])
    x0 = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1.0 + h_k) ** 0.5, n, d)
    noise = torch.randn(1, B, n * d, generator=gen)
    x = x0.cuda().clone()
    drift = torch.empty_like(x)
    net.sampler_run(x, tab[k0:k0 + 1].cuda().contiguous(), 1, noise=noise.cuda(), drift_out=drift)
    assert torch.isfinite(x).all()
    assert abs(x.reshape(B, n, d).mean(1)).max() < 1e-4 * (1 + x.abs().max().item())
    idx = torch.randint(0, B, (subset,), generator=gen)
    wt = {k: T(v) for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, n, d)
    osched, ogam = O.Elucidating(sigma_min, 80.0, 7), O.GammaConstant(4 / 3)
    t = times[k0]
    terms = O.f_not_debiased(bb, osched, ogam, t, x0[idx], 1.0)
    tb = t * torch.ones(subset)
    xo = x0[idx] + (terms.drift_X * (1.0 / N) + (osched.g(tb)[:, None] * noise[0, idx]) * np.sqrt(1.0 / N))
    xo = O.remove_mean(xo, n, d)
    assert rel(drift[idx.cuda()], terms.drift_X) < 1e-4
    assert rel(x[idx.cuda()], xo) < 1e-5
    return net, tab, x


def test_full_size_dw4_config(pa, golden):
    """BASELINE config C2: DW4 (4 particles x 2D), EGNN score net, 65 536 walkers."""
    B = 65536
    net, tab, x = _one_step_vs_oracle(pa, golden, 4, 2, B, 0.01)
    e = pa.MultiDoubleWellEnergy()
    lp, f = e(x, return_force=True)
    assert torch.isfinite(lp).all() and torch.isfinite(f).all()
    idx = torch.arange(0, B, 997)
    lpo, fo = O.dw4_logp_force(x[idx.cuda()].cpu().double())
    np.testing.assert_allclose(lp[idx.cuda()].cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=2e-4)
    assert rel(f[idx.cuda()], fo) < 2e-5
    assert abs(f.reshape(B, 4, 2).sum(1)).max() < 1e-2 * f.abs().max().item()  # no net force on the centre of mass


def test_full_size_lj55_config(pa, golden):
    """BASELINE config C5 per-GPU shard: LJ55 (55 x 3D), EGNN score net, 32 768 walkers."""
    B = 32768
    net, tab, x = _one_step_vs_oracle(pa, golden, 55, 3, B, 0.05, subset=6)
    g = golden("lj55_logp_force.npz")
    base = T(g["x"][:48])
    gen = torch.Generator().manual_seed(9)
    xe = (base[torch.randint(0, 48, (B,), generator=gen)] + 0.02 * torch.randn(B, 165, generator=gen)).cuda()
    e = pa.LennardJonesEnergy(165, 55, 3)
    lp, f = e(xe, return_force=True)
    idx = torch.arange(0, B, 4099)
    lpo, fo = O.lj_logp_force(xe[idx.cuda()].cpu().double(), 55, 3)
    np.testing.assert_allclose(lp[idx.cuda()].cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=1e-3)
    assert rel(f[idx.cuda()], fo) < 2e-5


def test_full_size_aldp_shape(pa, golden):
    """BASELINE config C4 per-GPU shard: 22 atoms x 3D (alanine dipeptide), EGNN score net, 4 096 walkers, and a ragged
    batch that leaves the last group partly filled; multi-step launch == the same steps one launch at a time."""
    for B in (4096, 4099):
        net, tab, x = _one_step_vs_oracle(pa, golden, 22, 3, B, 0.01, subset=12, seed=B)
    xa = x.clone()
    net.sampler_run(xa, tab[10:16].cuda().contiguous(), 6, seed=5, step0=10)
    xb = x.clone()
    for k in range(10, 16):
        net.sampler_run(xb, tab[k:k + 1].cuda().contiguous(), 1, seed=5, step0=k)
    assert torch.equal(xa, xb)


def test_time_only_egnn_sampler(pa, golden):
    """The time-only EGNN (egnn.py: in_node_nf = 1, no temperature conditioning) through the fused sampler: fused ==
    step-by-step recording path, and one step against the oracle."""
    g = golden("egnn_notemp_lj13_fwd.npz")
    net = make_net(pa, 13, 3, {k[2:]: v for k, v in g.items() if k.startswith("w.")}, temp=False)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), debias_inference=False)
    N, B = 6, 37
    gen = torch.Generator().manual_seed(4)
    x1 = O.remove_mean(torch.randn(B, 39, generator=gen) * 4, 13, 3).cuda()
    nz = torch.randn(N, B, 39, generator=gen).cuda()
    mk = lambda rec: pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0,
                                              end_resampling_step=N, resampling_interval=-1, num_negative_time_steps=0,
                                              post_mcmc_steps=0, record_terms=rec)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    e = pa.LennardJonesEnergy(39, 13, 3)
    xa, *_ = mk(False).integrate_sde(x1, e, gam, noise=nz)
    xb, *_ = mk(True).integrate_sde(x1, e, gam, noise=nz)
    assert rel(xa, xb) < 2e-5 and not torch.equal(xa, x1)


# ------------------------------------------------------------------------------- debiased regime (section 8(f) N1)
def test_jvp_vs_oracle(pa, golden):
    """pita_egnn_jvp against torch.func.jvp of the fp64 oracle denoiser: x-directions, the h-direction, mixed."""
    from torch.func import jvp

    w = golden("egnn_weights_trainedlike.npz")
    wt = {k: T(v).double() for k, v in w.items()}
    for n, d, B in ((13, 3, 23), (4, 2, 40)):
        net = make_net(pa, n, d, w)
        gen = torch.Generator().manual_seed(n)
        h = torch.tensor([0.01, 0.3, 2.0, 40.0, 900.0])[torch.arange(B) % 5]
        x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + h.sqrt())[:, None], n, d)
        beta = torch.rand(B, generator=gen) + 0.7
        vx = torch.randn(B, n * d, generator=gen)
        vh = torch.randn(B, generator=gen) * h
        bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, n, d)
        fn = lambda hh, xx: O.denoiser(bb, hh, xx, beta.double())
        for tag, (tx, th) in {"x": (vx, torch.zeros(B)), "h": (torch.zeros(B, n * d), vh), "xh": (vx, vh)}.items():
            Dref, dref = jvp(fn, (h.double(), x.double()), (th.double(), tx.double()))
            Dh, dDh = net.jvp(h.cuda(), x.cuda(), beta.cuda(), vx=tx.cuda(), vh=th.cuda())
            assert rel(Dh, Dref) < 2e-6, tag
            assert rel(dDh, dref) < 2e-5, (tag, rel(dDh, dref))
        # unit directions
        for k in (0, n * d - 1, 5):
            e = torch.zeros(B, n * d)
            e[:, k] = 1
            _, dref = jvp(fn, (h.double(), x.double()), (torch.zeros(B).double(), e.double()))
            _, dk = net.jvp(h.cuda(), x.cuda(), beta.cuda(), direction=k, want_primal=False)
            assert rel(dk, dref) < 2e-5, k


def test_jacobian_trace_multi_direction(pa, golden):
    """pita_egnn_div_accumulate (K unit directions per launch, shared primal) == the trace assembled from single-direction
    JVP launches, and == the trace of the fp64 oracle Jacobian (the reference's vmap(jacrev), utils.py:30-51)."""
    from torch.func import jacrev, vmap

    w = golden("egnn_weights_trainedlike.npz")
    wt = {k: T(v).double() for k, v in w.items()}
    for n, d, B in ((13, 3, 23), (4, 2, 41), (13, 3, 1), (13, 3, 300)):
        net = make_net(pa, n, d, w)
        gen = torch.Generator().manual_seed(3 * n + B)
        h = torch.tensor([0.01, 0.3, 2.0, 40.0, 900.0])[torch.arange(B) % 5]
        x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + h.sqrt())[:, None], n, d)
        beta = torch.rand(B, generator=gen) + 0.7
        tr, den = net.jacobian_trace(h.cuda(), x.cuda(), beta.cuda(), want_denoiser=True)
        assert torch.equal(tr, net.jacobian_trace(h.cuda(), x.cuda(), beta.cuda()))
        assert rel(den, net.edm(1, h.cuda(), x.cuda(), beta.cuda())) < 1e-6
        acc = torch.zeros(B, device="cuda")
        for k in range(n * d):
            net.jvp(h.cuda(), x.cuda(), beta.cuda(), direction=k, want_primal=False, want_tangent=False, diag_acc=acc)
        scale = float(acc.abs().mean()) + 1.0
        np.testing.assert_allclose(tr.cpu().numpy(), acc.cpu().numpy(), rtol=2e-5, atol=2e-5 * scale)
        if B <= 41:
            bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, n, d)
            one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
            J = vmap(jacrev(one, argnums=1))(h.double(), x.double(), beta.double())
            want = torch.diagonal(J, dim1=1, dim2=2).sum(-1)
            np.testing.assert_allclose(tr.cpu().numpy(), want.numpy(), rtol=5e-5, atol=5e-5 * scale)


@pytest.mark.parametrize("n,B", [(13, 40003), (22, 4099), (55, 1031)])
def test_jacobian_trace_large_batches_block_shared_stream(pa, golden, n, B):
    """At production batch sizes every block of the block-shared tangent kernel sweeps MANY walker groups: the LDS ring
    wraps thousands of times, the parked results are flushed every 32 groups, the last group of a wave's quota is ragged.
    The trace must still equal the one assembled from single-direction forward-mode launches, walker by walker."""
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, n, 3, w)
    gen = torch.Generator().manual_seed(n + B)
    h = torch.tensor([0.01, 0.3, 2.0, 40.0, 900.0])[torch.arange(B) % 5].cuda()
    x = O.remove_mean(torch.randn(B, n * 3, generator=gen) * (1 + h.cpu().sqrt())[:, None], n, 3).cuda()
    beta = (torch.rand(B, generator=gen) + 0.7).cuda()
    tr = net.jacobian_trace(h, x, beta)
    assert torch.equal(tr, net.jacobian_trace(h, x, beta))  # same bits on a second call (cache reuse)
    acc = torch.zeros(B, device="cuda")
    for k in range(n * 3):
        net.jvp(h, x, beta, direction=k, want_primal=False, want_tangent=False, diag_acc=acc)
    scale = float(acc.abs().mean()) + 1.0
    np.testing.assert_allclose(tr.cpu().numpy(), acc.cpu().numpy(), rtol=2e-5, atol=2e-5 * scale)


@pytest.mark.parametrize("variant", ["no_attention", "no_tanh", "layers2", "layers4", "layers5"])
def test_jacobian_trace_network_variants(pa, golden, variant):
    """The cached / block-shared trace path for the network options the kernels branch on (gate off, tanh off, fewer and
    more layers than the reference configs' three): equal to the trace assembled from single-direction forward-mode
    launches, for a batch with several walker groups per block."""
    w = {k: T(v) for k, v in golden("egnn_weights_trainedlike.npz").items()}
    kw = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True,
              condition_temperature=True, agg="sum")
    if variant == "no_attention":
        kw["attention"] = False
    elif variant == "no_tanh":
        kw["tanh"] = False
    elif variant == "layers2":
        kw["n_layers"] = 2
    elif variant == "layers4":
        kw["n_layers"] = 4
    elif variant == "layers5":  # deeper than the block-shared kernel's LDS budget: the wave-owned tangent kernel takes over
        kw["n_layers"] = 5
    net = pa.EGNN_dynamics(13, 3, **kw)
    sd = net.state_dict()
    gen = torch.Generator().manual_seed(17)
    for k in sd:  # reuse the trained-like tensors where the shapes agree, seeded noise elsewhere (extra layer)
        src = w.get(k, w.get(k.replace("gcl_3", "gcl_1")))
        sd[k] = src.clone() if src is not None and src.shape == sd[k].shape else 0.2 * torch.randn(sd[k].shape, generator=gen)
    net.load_state_dict(sd)
    B = 3001
    h = torch.tensor([0.05, 0.8, 12.0])[torch.arange(B) % 3].cuda()
    x = O.remove_mean(torch.randn(B, 39, generator=gen) * (1 + h.cpu().sqrt())[:, None], 13, 3).cuda()
    beta = (torch.rand(B, generator=gen) + 0.7).cuda()
    tr = net.jacobian_trace(h, x, beta)
    acc = torch.zeros(B, device="cuda")
    for k in range(39):
        net.jvp(h, x, beta, direction=k, want_primal=False, want_tangent=False, diag_acc=acc)
    scale = float(acc.abs().mean()) + 1.0
    assert torch.isfinite(tr).all()
    np.testing.assert_allclose(tr.cpu().numpy(), acc.cpu().numpy(), rtol=2e-5, atol=2e-5 * scale)


@pytest.mark.parametrize("n,d,want16,want32", [(13, 3, 2889, 252), (55, 3, 132012, 18144), (4, 2, 105.75, 4.125),
                                                  (22, 3, 13338, 1449)])
def test_div_work_of_default_handles(pa, n, d, want16, want32):
    """pita_egnn_div_work prices the debiased leg's roofline (bench.py): for the default h32 x 3 handles (f16x2, primal-cache
    path) it counts the matrix instructions per walker of one full trace.  The counts depend on the plan
    pita_egnn_jacobian_trace takes, not on the batch or the device."""
    import ctypes

    net = pa.EGNN_dynamics(n, d, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True,
                           condition_temperature=True, agg="sum", precision="f16x2")
    a, b = ctypes.c_double(), ctypes.c_double()
    pa._lib.check(pa._lib.lib().pita_egnn_div_work(net._native(torch.device("cuda", 0)), ctypes.byref(a), ctypes.byref(b)),
                  "pita_egnn_div_work")
    assert (a.value, b.value) == (want16, want32)


def test_jacobian_trace_22_atoms_four_layers(pa, golden):
    """22 atoms x 4 layers: the sweep's piece sequence exceeds the block-shared kernel's table, so the wave-owned
    tangent kernel must take over (a silent overflow would give garbage)."""
    w = {k: T(v) for k, v in golden("egnn_weights_trainedlike.npz").items()}
    net = pa.EGNN_dynamics(22, 3, hidden_nf=32, n_layers=4, recurrent=True, tanh=True, attention=True, condition_time=True,
                           condition_temperature=True, agg="sum")
    sd = net.state_dict()
    gen = torch.Generator().manual_seed(23)
    for k in sd:
        src = w.get(k, w.get(k.replace("gcl_3", "gcl_1")))
        sd[k] = src.clone() if src is not None and src.shape == sd[k].shape else 0.2 * torch.randn(sd[k].shape, generator=gen)
    net.load_state_dict(sd)
    B = 1501
    h = torch.tensor([0.05, 0.8, 12.0])[torch.arange(B) % 3].cuda()
    x = O.remove_mean(torch.randn(B, 66, generator=gen) * (1 + h.cpu().sqrt())[:, None], 22, 3).cuda()
    beta = (torch.rand(B, generator=gen) + 0.7).cuda()
    tr = net.jacobian_trace(h, x, beta)
    acc = torch.zeros(B, device="cuda")
    for k in range(66):
        net.jvp(h, x, beta, direction=k, want_primal=False, want_tangent=False, diag_acc=acc)
    scale = float(acc.abs().mean()) + 1.0
    np.testing.assert_allclose(tr.cpu().numpy(), acc.cpu().numpy(), rtol=2e-5, atol=2e-5 * scale)


@pytest.mark.parametrize("n_layers", [2, 4])
def test_jacobian_trace_lj55_block_shared_layer_counts(pa, golden, n_layers):
    """55 particles on the block-shared tangent kernel (two column tiles, 8 waves x 1 direction, the per-ITEM piece table)
    with fewer and more layers than the reference configs' three: the item sequence, the ring and the table sizes all
    depend on the depth.  Equal to the trace assembled from single-direction forward-mode launches."""
    w = {k: T(v) for k, v in golden("egnn_weights_trainedlike.npz").items()}
    net = pa.EGNN_dynamics(55, 3, hidden_nf=32, n_layers=n_layers, recurrent=True, tanh=True, attention=True,
                           condition_time=True, condition_temperature=True, agg="sum")
    sd = net.state_dict()
    gen = torch.Generator().manual_seed(31 + n_layers)
    for k in sd:
        src = w.get(k, w.get(k.replace("gcl_3", "gcl_1")))
        sd[k] = src.clone() if src is not None and src.shape == sd[k].shape else 0.2 * torch.randn(sd[k].shape, generator=gen)
    net.load_state_dict(sd)
    B = 301
    h = torch.tensor([0.05, 0.8, 12.0])[torch.arange(B) % 3].cuda()
    x = O.remove_mean(torch.randn(B, 165, generator=gen) * (1 + h.cpu().sqrt())[:, None], 55, 3).cuda()
    beta = (torch.rand(B, generator=gen) + 0.7).cuda()
    tr = net.jacobian_trace(h, x, beta)
    acc = torch.zeros(B, device="cuda")
    for k in range(165):
        net.jvp(h, x, beta, direction=k, want_primal=False, want_tangent=False, diag_acc=acc)
    scale = float(acc.abs().mean()) + 1.0
    assert torch.isfinite(tr).all()
    np.testing.assert_allclose(tr.cpu().numpy(), acc.cpu().numpy(), rtol=2e-5, atol=2e-5 * scale)


def test_jacobian_trace_in_cache_chunks(golden):
    """A batch whose primal cache exceeds PITA_DIV_CACHE_GB is processed in chunks of walkers; the result does not
    depend on the chunking (the budget is read once per process, so this runs in a child process)."""
    import subprocess
    import sys

    code = """
import os, sys, numpy as np, torch
sys.path.insert(0, %r)
import pita_amd as pa
w = dict(np.load(os.path.join(%r, "tests", "golden", "egnn_weights_trainedlike.npz")))
net = pa.EGNN_dynamics(13, 3, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                       condition_time=True, condition_temperature=True, agg="sum")
net.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
B = 5003
gen = torch.Generator().manual_seed(1)
from pita_amd.data_utils import remove_mean
x = remove_mean(torch.randn(B, 39, generator=gen).cuda() * 2.0, 13, 3)
h = torch.full((B,), 1.5).cuda(); b = torch.ones(B).cuda()
tr = net.jacobian_trace(h, x, b)
torch.save(tr.cpu(), sys.argv[1])
""" % (ROOT, ROOT)
    import tempfile

    outs = []
    with tempfile.TemporaryDirectory() as td:
        for gb in ("0.3", "24"):
            env = dict(os.environ, PITA_DIV_CACHE_GB=gb)
            path = os.path.join(td, f"tr_{gb}.pt")
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env)
            assert r.returncode == 0, r.stderr[-2000:]
            outs.append(torch.load(path))
    assert torch.isfinite(outs[0]).all()
    # chunking changes the wave quotas (which walkers share a tile), not the per-walker arithmetic
    assert torch.equal(outs[0], outs[1])


def test_jacobian_trace_survives_a_cache_the_device_cannot_hold():
    """With an unlimited budget 1.7 million LJ13 walkers would need a 306 GB primal cache: the allocation fails, smaller
    chunks are tried until one fits, and the walkers' traces are the ones a small batch gives (child process: the budget
    is read once)."""
    import subprocess
    import sys

    code = """
import os, sys, numpy as np, torch
sys.path.insert(0, %r)
import pita_amd as pa
from pita_amd.data_utils import remove_mean
w = dict(np.load(os.path.join(%r, "tests", "golden", "egnn_weights_trainedlike.npz")))
net = pa.EGNN_dynamics(13, 3, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                       condition_time=True, condition_temperature=True, agg="sum")
net.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
B = 1700000
x = remove_mean(torch.randn(B, 39, generator=torch.Generator().manual_seed(2)).cuda() * 2.0, 13, 3)
h = torch.full((B,), 1.5).cuda(); b = torch.ones(B).cuda()
tr = net.jacobian_trace(h, x, b)
small = net.jacobian_trace(h[:3001], x[:3001], b[:3001])
tail = net.jacobian_trace(h[-2000:], x[-2000:], b[-2000:])
assert torch.isfinite(tr).all()
assert torch.equal(tr[:3001], small) and torch.equal(tr[-2000:], tail)
print("ok")
""" % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PITA_DIV_CACHE_GB="100000"))
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_jacobian_trace_out_of_range_walkers_fall_back_to_bf16(pa, golden):
    """The f16 divergence kernel marks walkers whose trace term is non-finite (operands beyond the f16 range) and the
    bf16x3 kernel recomputes exactly those: far-out walkers must equal the pure bf16x3 result, ordinary walkers keep
    the f16 kernel's, the denoiser by-product follows the same rule, and nothing is counted twice."""
    w = golden("egnn_weights_trainedlike.npz")
    nf, nb = make_net(pa, 13, 3, w, precision="f16x2"), make_net(pa, 13, 3, w, precision="bf16x3")
    gen = torch.Generator().manual_seed(5)
    B = 40
    x = torch.randn(B, 39, generator=gen)
    x[20:] *= 2000.0
    x = O.remove_mean(x, 13, 3).cuda()
    h, b = torch.full((B,), 0.02).cuda(), torch.ones(B).cuda()
    tf, df = nf.jacobian_trace(h, x, b, want_denoiser=True)
    tb, db = nb.jacobian_trace(h, x, b, want_denoiser=True)
    assert torch.isfinite(tf).all() and torch.isfinite(df).all()
    assert torch.equal(tf[20:], tb[20:]) and torch.equal(df[20:], db[20:])
    assert not torch.equal(tf[:20], tb[:20])
    np.testing.assert_allclose(tf[:20].cpu().numpy(), tb[:20].cpu().numpy(), rtol=2e-5, atol=2e-5)
    assert rel(df[:20], db[:20]) < 1e-6


def _walker_variant(pa, w, variant):
    kw = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True,
              condition_temperature=True, agg="sum")
    kw.update({"no_attention": dict(attention=False), "no_tanh": dict(tanh=False), "layers2": dict(n_layers=2),
               "layers4": dict(n_layers=4), "default": {}}[variant])
    net = pa.EGNN_dynamics(13, 3, **kw)
    sd = net.state_dict()
    gen = torch.Generator().manual_seed(17)
    for k in sd:
        src = w.get(k, w.get(k.replace("gcl_3", "gcl_1")))
        sd[k] = T(src).clone() if src is not None and tuple(src.shape) == tuple(sd[k].shape) else 0.2 * torch.randn(sd[k].shape, generator=gen)
    net.load_state_dict(sd)
    return net


def test_handles_of_different_depth_share_kernels(pa, golden):
    """The dynamic-LDS limit of a kernel is state of (device, kernel function): two live handles that share the
    instantiations (same particle system and switches) but need different sizes -- 4 layers and 2 layers of per-layer
    vectors -- must not lower each other's limit.  The deeper handle runs, then the shallower one configures the same
    kernels smaller, then the deeper one again: same bits as before, on every entry point that opts in to LDS."""
    w = golden("egnn_weights_trainedlike.npz")
    deep, shallow = _walker_variant(pa, w, "layers4"), _walker_variant(pa, w, "layers2")
    B = 29
    gen = torch.Generator().manual_seed(5)
    h = torch.tensor([0.01, 0.3, 2.0, 40.0])[torch.arange(B) % 4].cuda()
    x = O.remove_mean(torch.randn(B, 39, generator=gen) * 1.5, 13, 3).cuda()
    beta = (torch.rand(B, generator=gen) + 0.7).cuda()

    def everything(net):
        out = [net(0.125 * torch.log(h), x / (1 + h).sqrt()[:, None], beta)]
        out += list(net.vjp(h, x, beta, want_dot_h=True))
        out += list(net.jvp(h, x, beta, direction=3))
        out += list(net.jacobian_trace(h, x, beta, want_denoiser=True))
        return [o for o in out if o is not None]

    first = everything(deep)
    small = everything(shallow)
    again = everything(deep)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert all(bool(torch.isfinite(o).all()) for o in first + small)
    assert all(torch.equal(a, b) for a, b in zip(small, everything(shallow)))


def test_default_path_full_batch_rerun(pa, golden):
    """Bitwise run-to-run soak of every kernel a default run of the library executes, at the FULL batch of the metric.
    Why: round 5 met a rare run-to-run difference in a kernel built from hipcc's packed fp32 instructions (v_pk_mul_f32 /
    v_pk_fma_f32 with an SGPR-pair source and op_sel; profiles/r05_walker_packed_fp32_hazard.txt -- that kernel no longer
    ships).  It needed 8 192 walkers to show 2-4 differing results, and the same instruction form is in the objects that
    DO ship (tests/test_kernel_resources.py::test_packed_fp32_exposure_of_shipped_kernels lists the counts), so the
    determinism contract of DESIGN 2 / 6 (W-GPU = 1-GPU bit for bit) is checked here where the fault would show:
    * the headline fused sampler, 65 536 LJ13 walkers x 200 Philox steps, twice;
    * the debiased drift -- cache writer, three block-shared tangent launches, reverse-mode launch, pita_fk_assemble --
      at 65 536 walkers, four reruns of every output (trace, denoisers, J^T x, <x, dD/dh> split, all SDETerms fields);
    * the LJ55 fused sampler at the C5 shard (32 768 walkers x 20 steps), twice;
    * the fused MLP sampler, 65 536 walkers x 100 steps, twice."""
    import time

    from pita_amd import mlp

    t_start = time.time()
    B = 65536
    sde, sched, gam = _long_stack(pa, golden)
    net = sde.score_net.model
    scale = float((sched.h(torch.tensor(1.0)) / gam.gamma(torch.tensor(1.0))) ** 0.5)
    x0 = pa.Prior(scale=scale, n_particles=13, spatial_dim=3, seed=5).sample(B)
    N = 200
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, N + 1)[:-1], 1.0 / N, 1.0, 1.0).cuda()
    a = net.sampler_run(x0.clone(), tab, N, seed=11)
    b = net.sampler_run(x0.clone(), tab, N, seed=11)
    assert torch.isfinite(a).all() and not torch.equal(a, x0)
    nd = int((a != b).any(1).sum())
    assert nd == 0, f"fused LJ13 sampler: {nd} of {B} walkers differ between two identical runs"
    # debiased drift on mid-trajectory walkers (the sampler's own state after 120 of the 200 steps: h ~ 1)
    xm = net.sampler_run(x0.clone(), tab[:120].contiguous(), 120, seed=11)
    t = torch.tensor(float(1.0 - 120 / N))
    ht = torch.full((B,), float(sched.h(t.reshape(1))[0]), device="cuda")
    beta = torch.ones(B, device="cuda")
    lj = pa.LennardJonesEnergy(39, 13, 3)

    def drift():
        out = list(net.jacobian_trace(ht, xm, beta, want_denoiser=True))
        out += [o for o in sde.energy_net.net.vjp(ht, xm, beta, want_dot_h=True, want_h_parts=True) if o is not None]
        terms = sde.f(t, xm, 1.0, gam, None, lj, resampling_interval=1, clamp_chunk=512)
        out += [terms.drift_X, terms.drift_A, terms.divergence_score, terms.cross_term, terms.dUt_dt]
        return [o.clone() for o in out]

    first = drift()
    assert all(bool(torch.isfinite(o).all()) for o in first)
    names = ["trace", "D_S", "D_E", "JTx", "dot_h", "h_parts", "drift_X", "drift_A", "div", "cross", "dUt_dt"]
    for rerun in range(4):
        for nm, u, v in zip(names, first, drift()):
            nd = int((u != v).reshape(B, -1).any(1).sum())
            assert nd == 0, f"debiased drift rerun {rerun}: {nm} differs for {nd} of {B} walkers"
    # the reference's own batch (num_eval_samples = 2 048, lj13.yaml:32): the small-batch mappings -- two walkers per wave in
    # the sampler and (round 6) in the reverse-mode kernel -- through the same drift, four reruns
    Bs = 2048
    xs_, hs_, bs_ = xm[:Bs].contiguous(), ht[:Bs].contiguous(), beta[:Bs].contiguous()

    def drift_small():
        out = list(net.jacobian_trace(hs_, xs_, bs_, want_denoiser=True))
        out += [o for o in sde.energy_net.net.vjp(hs_, xs_, bs_, want_dot_h=True, want_h_parts=True) if o is not None]
        return [o.clone() for o in out]

    first_s = drift_small()
    # (another reverse-mode instantiation runs here: same values to fp32 rounding, DESIGN 2 "determinism")
    assert rel(first_s[3], first[3][:Bs]) < 2e-6 and rel(first_s[0], first[0][:Bs]) < 2e-6
    for rerun in range(4):
        for nm, u, v in zip(names, first_s, drift_small()):
            assert torch.equal(u, v), f"small-batch drift rerun {rerun}: {nm} differs"
    a = net.sampler_run(x0[:Bs].clone(), tab, N, seed=11)
    assert torch.equal(a, net.sampler_run(x0[:Bs].clone(), tab, N, seed=11))
    # LJ55 at the C5 shard
    net55 = make_net(pa, 55, 3, golden("egnn_weights_trainedlike.npz"))
    B55, N55 = 32768, 20
    x55 = pa.Prior(scale=scale, n_particles=55, spatial_dim=3, seed=6).sample(B55)
    tab55 = pa.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, N55 + 1)[:-1], 1.0 / N55, 1.0, 1.0).cuda()
    a = net55.sampler_run(x55.clone(), tab55, N55, seed=3)
    nd = int((a != net55.sampler_run(x55.clone(), tab55, N55, seed=3)).any(1).sum())
    assert torch.isfinite(a).all() and nd == 0, f"fused LJ55 sampler: {nd} of {B55} walkers differ"
    # fused MLP sampler (config C1's backbone at the metric's batch)
    torch.manual_seed(3)
    mnet = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2).cuda()
    xg = (torch.randn(B, 2, generator=torch.Generator().manual_seed(8)) * 40).cuda()
    tabm = pa.sde_integration.build_step_table(sched, pa.ConstantAnnealingFactorSchedule(1.0),
                                               torch.linspace(1.0, 0.0, 101)[:-1], 0.01, 1.0, 1.0).cuda()
    a = mnet.sampler_run(xg.clone(), tabm, 100, seed=9, remove_mean=False)
    nd = int((a != mnet.sampler_run(xg.clone(), tabm, 100, seed=9, remove_mean=False)).any(1).sum())
    assert torch.isfinite(a).all() and nd == 0, f"fused MLP sampler: {nd} of {B} walkers differ"
    print(f"\n[rerun soak] {time.time() - t_start:.1f} s")


@pytest.mark.parametrize("n,B", [(22, 9), (55, 3)])
def test_derivative_kernels_other_shapes(pa, golden, n, B):
    """The 22-atom (alanine dipeptide, config C4) and LJ55 (C5) instantiations of the forward-mode, reverse-mode and
    multi-direction divergence kernels against the fp64 oracle (same weights: the EGNN does not depend on n)."""
    from torch.func import jvp

    d = 3
    w = golden("egnn_weights_trainedlike.npz")
    wt = {k: T(v).double() for k, v in w.items()}
    net = make_net(pa, n, d, w)
    gen = torch.Generator().manual_seed(n)
    h = torch.tensor([0.05, 1.0, 30.0])[torch.arange(B) % 3]
    x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + h.sqrt())[:, None], n, d)
    beta = torch.rand(B, generator=gen) + 0.7
    bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, n, d)
    fn = lambda hh, xx: O.denoiser(bb, hh, xx, beta.double())
    vx, cot = torch.randn(B, n * d, generator=gen), torch.randn(B, n * d, generator=gen)
    Dref, dref = jvp(fn, (h.double(), x.double()), (torch.zeros(B).double(), vx.double()))
    Dh, dDh = net.jvp(h.cuda(), x.cuda(), beta.cuda(), vx=vx.cuda())
    assert rel(Dh, Dref) < 2e-6 and rel(dDh, dref) < 2e-5
    xd = x.double().requires_grad_(True)
    (gref,) = torch.autograd.grad((fn(h.double(), xd) * cot.double()).sum(), xd)
    Dv, vj = net.vjp(h.cuda(), x.cuda(), beta.cuda(), cot=cot.cuda())
    assert rel(Dv, Dref) < 2e-6 and rel(vj, gref) < 2e-5
    tr = net.jacobian_trace(h.cuda(), x.cuda(), beta.cuda())
    acc = torch.zeros(B, device="cuda")
    for k in range(n * d):
        net.jvp(h.cuda(), x.cuda(), beta.cuda(), direction=k, want_primal=False, want_tangent=False, diag_acc=acc)
    np.testing.assert_allclose(tr.cpu().numpy(), acc.cpu().numpy(), rtol=2e-5, atol=2e-5 * (float(acc.abs().mean()) + 1))


def test_vjp_vs_oracle(pa, golden):
    """pita_egnn_vjp (reverse mode, one launch) against torch.autograd of the fp64 oracle denoiser: the default
    cotangent x (what grad_x E_theta needs) and a random one; ragged batches that leave tiles partly filled; and
    consistency with the forward-mode kernel: <cot, J v> == <J^T cot, v>."""
    w = golden("egnn_weights_trainedlike.npz")
    wt = {k: T(v).double() for k, v in w.items()}
    for n, d, B in ((13, 3, 23), (4, 2, 41), (13, 3, 7), (13, 3, 1)):
        net = make_net(pa, n, d, w)
        gen = torch.Generator().manual_seed(n + B)
        h = torch.tensor([0.01, 0.3, 2.0, 40.0, 900.0])[torch.arange(B) % 5]
        x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + h.sqrt())[:, None], n, d)
        beta = torch.rand(B, generator=gen) + 0.7
        cot = torch.randn(B, n * d, generator=gen)
        bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, n, d)
        for tag, c in (("x", None), ("random", cot)):
            xd = x.double().requires_grad_(True)
            Dref = O.denoiser(bb, h.double(), xd, beta.double())
            cc = (x if c is None else c).double()
            (gref,) = torch.autograd.grad((Dref * cc).sum(), xd)
            Dh, vj = net.vjp(h.cuda(), x.cuda(), beta.cuda(), cot=None if c is None else c.cuda())
            assert rel(Dh, Dref.detach()) < 2e-6, (n, B, tag)
            assert rel(vj, gref) < 2e-5, (n, B, tag, rel(vj, gref))
        # EnergyNet.forward = grad_x E_theta (energy_net.py:51-62: autograd in the reference, one VJP launch here)
        from pita_amd.energy_net import EnergyNet

        xd = x.double().requires_grad_(True)
        (gE,) = torch.autograd.grad(O.energy_theta(bb, h.double(), xd, beta.double()).sum(), xd)
        assert rel(EnergyNet(net).forward(h.cuda(), x.cuda(), beta.cuda()), gE) < 5e-5, (n, B)
        v = torch.randn(B, n * d, generator=gen)
        _, Jv = net.jvp(h.cuda(), x.cuda(), beta.cuda(), vx=v.cuda(), want_primal=False)
        _, JTc = net.vjp(h.cuda(), x.cuda(), beta.cuda(), cot=cot.cuda(), want_primal=False)
        assert torch.equal(JTc, net.vjp(h.cuda(), x.cuda(), beta.cuda(), cot=cot.cuda(), want_primal=False)[1])  # reproducible
        lhs, rhs = (cot.cuda() * Jv).sum(1), (JTc * v.cuda()).sum(1)
        np.testing.assert_allclose(lhs.cpu().numpy(), rhs.cpu().numpy(), rtol=2e-4, atol=2e-4 * float(lhs.abs().mean()))
        # <cot, dD/dh> from the reverse sweep (time feature, c_in scaling, explicit c_s / c_out) against autograd of the
        # fp64 oracle through h and against the forward-mode kernel's h direction
        for tag, c in (("x", None), ("random", cot)):
            hd = h.double().requires_grad_(True)
            cc = (x if c is None else c).double()
            (gh,) = torch.autograd.grad((O.denoiser(bb, hd, x.double(), beta.double()) * cc).sum(), hd)
            _, vj2, dh = net.vjp(h.cuda(), x.cuda(), beta.cuda(), cot=None if c is None else c.cuda(), want_dot_h=True)
            np.testing.assert_allclose(dh.cpu().numpy(), gh.numpy(), rtol=5e-5, atol=5e-5 * float(gh.abs().mean()),
                                       err_msg=f"{n} {B} {tag}")
            if c is None:
                dj = torch.empty(B, device="cuda")
                net.jvp(h.cuda(), x.cuda(), beta.cuda(), direction=-1, vh=torch.ones(B).cuda(), want_primal=False,
                        want_tangent=False, dot_out=dj)
                np.testing.assert_allclose(dh.cpu().numpy(), dj.cpu().numpy(), rtol=1e-4,
                                           atol=1e-4 * float(dj.abs().mean()))
            # the split of the same derivative (dot_parts): c_out <cot, F> and <cot, d(c_out F)/dh>, against the fp64
            # oracle's backbone output; together with the closed-form c_s'(h) <cot, x> share they are dot_h again
            _, vj3, dh3, parts = net.vjp(h.cuda(), x.cuda(), beta.cuda(), cot=None if c is None else c.cuda(),
                                         want_dot_h=True, want_h_parts=True)
            assert torch.equal(vj3, vj2) and torch.equal(dh3, dh)
            hd = h.double().requires_grad_(True)
            c_s, c_in, c_out, c_noise = O.edm_coeffs(hd)
            s1 = c_out * (bb(c_noise, c_in[:, None] * x.double(), beta.double()) * cc).sum(1)
            (s2,) = torch.autograd.grad(s1.sum(), hd)
            np.testing.assert_allclose(parts[:, 0].cpu().numpy(), s1.detach().numpy(), rtol=2e-5,
                                       atol=2e-5 * float(s1.detach().abs().mean()), err_msg=f"{n} {B} {tag}")
            np.testing.assert_allclose(parts[:, 1].cpu().numpy(), s2.numpy(), rtol=5e-5, atol=5e-5 * float(s2.abs().mean()),
                                       err_msg=f"{n} {B} {tag}")
            whole = parts[:, 1].cpu().double() - (x.double() * cc).sum(1) / (1 + h.double()) ** 2
            np.testing.assert_allclose(dh.cpu().numpy(), whole.numpy(), rtol=1e-5, atol=1e-5 * float(whole.abs().mean()))


def test_vjp_f16_edge_gemms_and_marked_walker_repair(pa, golden):
    """pita_egnn_vjp runs its four per-edge primal GEMMs on the f16 two-piece path (precision-2 handles) and hands the
    walkers whose activations leave the f16 range to the bf16x3 instantiation: the two paths agree to fp32 rounding; a
    walker with beta = 1e7 comes out finite and bit-equal to a bf16x3-only handle's result; its neighbours keep the
    f16 path's bits; ragged groups (7 walkers per wave) around the marked walker are untouched."""
    w = golden("egnn_weights_trainedlike.npz")
    n, d, B = 13, 3, 45
    net = make_net(pa, n, d, w)
    net_b = make_net(pa, n, d, w, precision="bf16x3")  # handle whose reverse-mode launch is the bf16x3 kernel alone
    gen = torch.Generator().manual_seed(77)
    h = torch.tensor([0.01, 0.3, 2.0, 40.0, 900.0])[torch.arange(B) % 5].cuda()
    x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + h.cpu().sqrt())[:, None], n, d).cuda()
    beta = (torch.rand(B, generator=gen) + 0.7).cuda()
    D0, v0, dh0 = net.vjp(h, x, beta, want_dot_h=True)
    assert torch.isfinite(v0).all() and torch.isfinite(dh0).all()
    hot = beta.clone()
    hot[17] = 1.0e7
    D1, v1, dh1 = net.vjp(h, x, hot, want_dot_h=True)
    keep = torch.arange(B) != 17
    assert torch.equal(v1[keep], v0[keep]) and torch.equal(dh1[keep], dh0[keep]) and torch.equal(D1[keep], D0[keep])
    Db, vb, dhb = net_b.vjp(h, x, beta, want_dot_h=True)
    assert rel(v0, vb) < 5e-6 and not torch.equal(v0, vb)
    np.testing.assert_allclose(dh0.cpu().numpy(), dhb.cpu().numpy(), rtol=2e-5, atol=2e-5 * float(dhb.abs().mean()))
    Dh, vh, dhh = net_b.vjp(h, x, hot, want_dot_h=True)
    assert torch.equal(v1[17].view(torch.int32), vh[17].view(torch.int32))
    assert torch.equal(dh1[17:18].view(torch.int32), dhh[17:18].view(torch.int32))
    assert torch.equal(D1[17].view(torch.int32), Dh[17].view(torch.int32))


@pytest.mark.parametrize("variant", ["no_attention", "no_tanh", "layers2"])
def test_vjp_network_variants(pa, golden, variant):
    """The reverse-mode kernel's run-time instantiation (gate off, tanh off, two layers; the compile-time path covers
    the reference configuration): J^T cot and the h-derivative against torch.autograd of the fp64 oracle."""
    w = {k: T(v) for k, v in golden("egnn_weights_trainedlike.npz").items()}
    kw = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True,
              condition_temperature=True, agg="sum")
    if variant == "no_attention":
        kw["attention"] = False
    elif variant == "no_tanh":
        kw["tanh"] = False
    else:
        kw["n_layers"] = 2
    net = pa.EGNN_dynamics(13, 3, **kw)
    sd = net.state_dict()
    gen = torch.Generator().manual_seed(29)
    for k in sd:
        src = w.get(k)
        sd[k] = src.clone() if src is not None and src.shape == sd[k].shape else 0.2 * torch.randn(sd[k].shape, generator=gen)
    net.load_state_dict(sd)
    wt = {k: v.double() for k, v in sd.items()}
    B = 19
    h = torch.tensor([0.05, 0.8, 12.0])[torch.arange(B) % 3]
    x = O.remove_mean(torch.randn(B, 39, generator=gen) * (1 + h.sqrt())[:, None], 13, 3)
    beta = torch.rand(B, generator=gen) + 0.7
    cot = torch.randn(B, 39, generator=gen)
    bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, 13, 3, n_layers=kw["n_layers"], tanh=kw["tanh"],
                                          attention=kw["attention"])
    xd, hd = x.double().requires_grad_(True), h.double().requires_grad_(True)
    Dref = O.denoiser(bb, hd, xd, beta.double())
    gx, gh = torch.autograd.grad((Dref * cot.double()).sum(), (xd, hd))
    for want_h in (False, True):
        out = net.vjp(h.cuda(), x.cuda(), beta.cuda(), cot=cot.cuda(), want_dot_h=want_h)
        assert rel(out[0], Dref.detach()) < 2e-6 and rel(out[1], gx) < 2e-5, (variant, want_h, rel(out[1], gx))
        if want_h:
            np.testing.assert_allclose(out[2].cpu().numpy(), gh.numpy(), rtol=5e-5, atol=5e-5 * float(gh.abs().mean()))


# drift_X, weight-drift terms, final walkers, log-weights: measured 6.4e-8 / 2.0e-7 / 7.3e-7 / 3.8e-6
_DEBIAS8_BOUNDS = (2.6e-7, 8e-7, 3e-6, 1.6e-5)


def test_debiased_terms_and_trajectory_golden(pa, golden):
    """Feynman-Kac drift terms at identical inputs and the 8-step weighted trajectory with resampling, against the
    reference run stored in em_traj_lj13_debias.npz (autograd + vmap(jacrev) there, HIP JVPs here)."""
    import copy

    g = golden("em_traj_lj13_debias.npz")
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, 13, 3, w)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    from pita_amd.energy_net import EnergyNet

    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    x1 = cu(g["x1"])
    terms = sde.f(torch.tensor(1.0).cuda(), x1, 1.0, gam, None, None, resampling_interval=2)
    # deviations from the reference's fp32 values at identical inputs: measured on MI355X (printed;
    # profiles/r05_parity_measured.txt), bounds 4 x measured
    dev = {nm: float(np.abs(getattr(terms, nm).cpu().numpy() - g[nm][0]).max() / np.abs(g[nm][0]).mean())
           for nm in ("divergence_score", "cross_term", "dUt_dt", "drift_A")}
    print(f"[debias8] first step, max |HIP - reference| / mean |reference|: drift_X rel-L2 {rel(terms.drift_X, g['drift_X'][0]):.2e}, "
          + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    assert rel(terms.drift_X, g["drift_X"][0]) < _DEBIAS8_BOUNDS[0]
    assert all(v < _DEBIAS8_BOUNDS[1] for v in dev.values()), dev
    N = int(g["N"])
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=1, end_resampling_step=7,
                                     resampling_interval=2, num_negative_time_steps=0, post_mcmc_steps=0, batch_size=12)
    e = pa.LennardJonesEnergy(39, 13, 3)
    x, logw, uniq, _, _ = integ.integrate_sde(x1, e, gam, inverse_temperature=1.0, noise=cu(g["noise"]),
                                              resample_u=[float(u[0]) for u in g["u"]])
    assert uniq == list(g["num_unique"])
    d_lw = float(np.abs(logw.cpu().numpy() - g["logweights"]).max() / np.abs(g["logweights"]).mean())
    print(f"[debias8] after {N} steps: walkers rel-L2 {rel(x, g['x_final']):.2e}, log-weights max dev / mean {d_lw:.2e}")
    assert rel(x, g["x_final"]) < _DEBIAS8_BOUNDS[2] and d_lw < _DEBIAS8_BOUNDS[3]
    # whole-batch evaluation with a per-chunk clamp == one call per chunk (the reference's loop)
    xa = pa.Prior(scale=3.0, n_particles=13, spatial_dim=3, seed=4).sample(24)
    t = torch.tensor(0.4).cuda()
    whole = sde.f(t, xa, 1.0, gam, None, None, clamp_chunk=8)
    parts = [sde.f(t, xa[lo:lo + 8], 1.0, gam, None, None) for lo in range(0, 24, 8)]
    # (not bitwise: the reverse-mode kernel's partner sums depend on where a walker sits in its wave's column tiles)
    np.testing.assert_allclose(whole.drift_A.cpu().numpy(), torch.cat([p_.drift_A for p_ in parts]).cpu().numpy(),
                               rtol=2e-5, atol=2e-4)
    assert rel(whole.drift_X, torch.cat([p_.drift_X for p_ in parts])) < 2e-6


def _replay_reference_term_logging(sde_terms):
    """The reference caller's exact access pattern on integrate_sde's 4th return value
    (energytemp_module.py:938-945 / 1061-1068 loop + _log_sde_term :1132-1143), minus the plotting."""
    from dataclasses import fields

    logged = {}
    for term in fields(pa_SDETerms()):
        if term.name == "drift_X" or term.name == "drift_A" or getattr(sde_terms[0], term.name) is None:
            continue
        mean = torch.stack([getattr(sde_terms[i], term.name).mean() for i in range(len(sde_terms))])
        std = torch.stack([getattr(sde_terms[i], term.name).std() for i in range(len(sde_terms))])
        logged[term.name] = (mean.cpu().numpy(), std.cpu().numpy())
    return logged


def pa_SDETerms():
    import pita_amd

    return pita_amd.SDETerms


def test_sde_terms_default_return_serves_the_reference_caller(pa, golden):
    """Default (record_terms=False) integrate_sde returns N indexable SDETerms whose fields answer .mean()/.std():
    the reference's unchanged logging loop runs on them and reproduces the statistics of the reference's own
    per-step tensors (goldens), in both regimes."""
    import copy

    # ---- not-debiased: `diffusion` is the only logged field (drift_X / drift_A are skipped by the caller)
    g = golden("em_traj_lj13_nodebias.npz")
    sde, sched, net = lj13_stack(pa, golden)
    N = int(g["N"])
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    e = pa.LennardJonesEnergy(39, 13, 3)
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                     resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0)
    _, _, _, terms, _ = integ.integrate_sde(cu(g["x1"]), e, gam, inverse_temperature=1.0, noise=cu(g["noise"]))
    assert len(terms) == N and terms[0].divergence_score is None
    logged = _replay_reference_term_logging(terms)
    assert set(logged) == {"diffusion"}
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, N + 1)[:-1], 1.0 / N, 1.0, 1.0)
    dif = tab[:, pa._lib.ST_NOISE_SCALE][:, None, None] * torch.tensor(g["noise"])  # sdes.py:250
    np.testing.assert_allclose(logged["diffusion"][0], dif.mean(dim=(1, 2)).numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(logged["diffusion"][1], dif.reshape(N, -1).std(dim=1).numpy(), rtol=1e-5)
    dX = torch.tensor(g["drift_X"])
    got = np.array([[float(t.drift_X.mean()), float(t.drift_X.std())] for t in terms])
    # atol: means are sums of mean-free drifts (~1e-6 relative cancellation residue)
    np.testing.assert_allclose(got[:, 1], dX.reshape(N, -1).std(dim=1).numpy(), rtol=3e-3)
    np.testing.assert_allclose(got[:, 0], dX.mean(dim=(1, 2)).numpy(), atol=1e-3 * float(dX.abs().max()))
    assert all(t.drift_A.numel() == 32 and float(t.drift_A.mean()) == 0.0 for t in terms)
    # same statistics from the per-step launch path (pita_em_step stats_out): a foreign backbone takes this route
    integ2 = pa.WeightedSDEIntegrator(sde=pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(_Foreign(net)),
                                                          debias_inference=False),
                                      num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                      resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0)
    _, _, _, terms2, _ = integ2.integrate_sde(cu(g["x1"]), e, gam, inverse_temperature=1.0, noise=cu(g["noise"]))
    got2 = np.array([[float(t.diffusion.mean()), float(t.diffusion.std()), float(t.drift_X.std())] for t in terms2])
    np.testing.assert_allclose(got2[:, 1], logged["diffusion"][1], rtol=1e-6)
    np.testing.assert_allclose(got2[:, 2], got[:, 1], rtol=1e-4)

    # ---- debiased: divergence_score / cross_term / dUt_dt / diffusion are logged
    g = golden("em_traj_lj13_debias.npz")
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, 13, 3, w)
    from pita_amd.energy_net import EnergyNet

    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    N = int(g["N"])
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=1, end_resampling_step=7,
                                     resampling_interval=2, num_negative_time_steps=0, post_mcmc_steps=0, batch_size=12)
    _, _, _, terms, _ = integ.integrate_sde(cu(g["x1"]), e, gam, inverse_temperature=1.0, noise=cu(g["noise"]),
                                            resample_u=[float(u[0]) for u in g["u"]])
    assert len(terms) == N
    logged = _replay_reference_term_logging(terms)
    assert set(logged) == {"divergence_score", "cross_term", "dUt_dt", "diffusion"}
    for name in ("divergence_score", "cross_term", "dUt_dt"):
        ref = torch.tensor(g[name])  # [N, B] of the reference run
        # step 0 lies before start_resampling_step: the walkers are frozen there and the HIP integrator does not
        # evaluate the drift terms (documented: their statistics are NaN); compare the steps that move walkers
        assert np.isnan(logged[name][0][0])
        np.testing.assert_allclose(logged[name][0][1:], ref.mean(dim=1).numpy()[1:], rtol=2e-2, atol=5e-2)
        np.testing.assert_allclose(logged[name][1][1:], ref.std(dim=1).numpy()[1:], rtol=2e-2, atol=5e-2)
    dA = np.array([float(t.drift_A.mean()) for t in terms])
    np.testing.assert_allclose(dA[1:], torch.tensor(g["drift_A"]).mean(dim=1).numpy()[1:], rtol=2e-2, atol=5e-2)


class _Foreign(torch.nn.Module):
    """A backbone the integrator cannot fuse (no sampler_run / edm): only forward(t, x, beta)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, t, x, beta):
        return self.net.forward(t, x, beta)


_VARIANT_BOUNDS = (8.5e-7, 8e-6)  # drift_X, weight-drift terms: measured <= 2.1e-7 / <= 2.0e-6 over the six (variant, t) cases


@pytest.mark.parametrize("name,pin,pb,sch", [("pin", True, False, "elucidating"), ("pb", False, True, "elucidating"),
                                             ("pinpb_geo", True, True, "geometric")])
def test_debiased_variants_golden(pa, golden, name, pin, pb, sch):
    """pin_energy (the target log-density enters the drift terms every step, energy_net.py:43-48), precondition_beta on
    both nets, dh/dt from the schedule (Geometric), d gamma/dt != 0 (Linear annealing): VEReverseSDE.f on the HIP path
    against the reference's own output (debias_variants_lj13.npz)."""
    import copy

    from pita_amd.energy_net import EnergyNet

    g = golden("debias_variants_lj13.npz")
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, 13, 3, w)
    sched = (pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7) if sch == "elucidating"
             else pa.GeometricNoiseSchedule(sigma_min=0.05, sigma_max=20.0))
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net, precondition_beta=pb),
                          energy_net=EnergyNet(copy.deepcopy(net), precondition_beta=pb), pin_energy=pin,
                          debias_inference=True)
    gam = pa.LinearAnnealingFactorSchedule(annealing_factor=1.5, annealing_factor_start=1.0)
    e = pa.LennardJonesEnergy(39, 13, 3)
    x, beta = cu(g["x"]), float(g["beta"])
    np.testing.assert_allclose(e(x).cpu().numpy(), g["pin_logp"], rtol=2e-5)
    for ti, tv in enumerate(g["t"]):
        terms = sde.f(torch.tensor(float(tv)).cuda(), x, beta, gam, None, e, resampling_interval=1)
        key = f"{name}_t{ti}_"
        # measured on MI355X (printed; profiles/r05_parity_measured.txt), bounds 4 x the largest measured deviation
        dev = {nm: float(np.abs(getattr(terms, nm).cpu().numpy() - g[key + nm]).max() / np.abs(g[key + nm]).max())
               for nm in ("drift_A", "divergence_score", "cross_term", "dUt_dt")}
        print(f"[variants/{name}] t = {float(tv):.2f}: drift_X rel-L2 {rel(terms.drift_X, g[key + 'drift_X']):.2e}, max |HIP - "
              "reference| / max |reference|: " + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
        assert rel(terms.drift_X, g[key + "drift_X"]) < _VARIANT_BOUNDS[0], key
        assert all(v < _VARIANT_BOUNDS[1] for v in dev.values()), (key, dev)
    if pin:
        with pytest.raises(ValueError):
            sde.f(torch.tensor(0.5).cuda(), x, beta, gam, None, None)  # pinning needs the target


@pytest.mark.parametrize("n,d,B", [(4, 2, 9), (22, 3, 5), (55, 3, 3)])
def test_debiased_terms_other_systems_vs_oracle(pa, golden, n, d, B):
    """VEReverseSDE.f in the debiased regime for DW4, the 22-atom system and LJ55 (configs C2, C4, C5): every SDETerms
    field against the fp64 oracle (autograd + vmap(jacrev), sdes.py:151-239), with DIFFERENT weights in the score and the
    energy net so that no term can borrow from the other network."""
    import copy

    from pita_amd.energy_net import EnergyNet

    w = golden("egnn_weights_trainedlike.npz")
    net_s = make_net(pa, n, d, w)
    gen = torch.Generator().manual_seed(100 + n)
    we = {k: T(v) * (1.0 + 0.05 * torch.randn(T(v).shape, generator=gen)) for k, v in w.items()}
    net_e = pa.EGNN_dynamics(n, d, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                             condition_time=True, condition_temperature=True, agg="sum")
    net_e.load_state_dict(we)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.LinearAnnealingFactorSchedule(annealing_factor=1.5, annealing_factor_start=1.0)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net_s), energy_net=EnergyNet(net_e),
                          debias_inference=True)
    ws = {k: T(v).double() for k, v in w.items()}
    wed = {k: v.double() for k, v in we.items()}
    bs = lambda cn, xs, b: O.egnn_forward(ws, cn, xs, b, n, d)
    be = lambda cn, xs, b: O.egnn_forward(wed, cn, xs, b, n, d)
    ws32, we32 = {k: T(v) for k, v in w.items()}, {k: v.float() for k, v in we.items()}
    bs32 = lambda cn, xs, b: O.egnn_forward(ws32, cn, xs, b, n, d)
    be32 = lambda cn, xs, b: O.egnn_forward(we32, cn, xs, b, n, d)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaLinear(1.5, 1.0)
    for tv in (0.15, 0.6):
        hv = float(sched.h(torch.tensor(tv)))
        x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + hv ** 0.5), n, d)
        terms = sde.f(torch.tensor(tv).cuda(), x.cuda(), 1.25, gam, None, None, resampling_interval=1, clamp_chunk=B)
        ref = O.f_debiased(bs, be, osched, ogam, torch.tensor(tv, dtype=torch.float64), x.double(), 1.25)
        # the same standard as LJ13's: the oracle in float32 is the reference's arithmetic (op for op), its distance from
        # the float64 oracle the reference's own error; the HIP terms may be at most 4 x as far (floor: one fp32 rounding
        # of a sum of n * d terms)
        r32 = O.f_debiased(bs32, be32, osched, ogam, torch.tensor(tv), x, 1.25)
        names = ("drift_X", "drift_A", "divergence_score", "cross_term", "dUt_dt")
        e_refs = {nm: rel(getattr(r32, nm), getattr(ref, nm)) for nm in names}
        typical = float(np.median(list(e_refs.values())))  # 3 .. 9 walkers: one term's fp32 error can be lucky-small
        for nm in names:
            e_hip, e_ref = rel(getattr(terms, nm), getattr(ref, nm)), e_refs[nm]
            print(f"[other/{n}x{d}] t = {tv}: {nm:16s} HIP vs fp64 {e_hip:.2e}, fp32 reference arithmetic vs fp64 {e_ref:.2e}")
            assert e_hip <= 4 * max(e_ref, typical), (n, tv, nm, e_hip, e_ref, typical)


def test_debiased_resample_at_end_golden(pa, golden):
    """experiment/lj13.yaml settings: inference chunks of 6 (per-chunk quantile clamp inside one set of launches) and
    resample_at_end=True (sde_integration.py:158-183), against the reference run em_traj_lj13_debias_end.npz."""
    import copy

    from pita_amd.energy_net import EnergyNet

    g = golden("em_traj_lj13_debias_end.npz")
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, 13, 3, w)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    N = int(g["N"])
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=6,
                                     resampling_interval=3, num_negative_time_steps=0, post_mcmc_steps=0, batch_size=6,
                                     resample_at_end=True)
    x, logw, uniq, _, _ = integ.integrate_sde(cu(g["x1"]), pa.LennardJonesEnergy(39, 13, 3), gam, inverse_temperature=1.0,
                                              noise=cu(g["noise"]), resample_u=[float(u[0]) for u in g["u"]])
    assert uniq == list(g["num_unique"])
    assert logw.shape == (N + 1, 12)
    # deviations from the reference's fp32 run, measured on MI355X (printed; profiles/r05_parity_measured.txt); bounds 4 x
    lw, want = logw.cpu().numpy(), g["logweights"]
    d_run = float(np.abs(lw[:N] - want[:N]).max() / max(np.abs(want[:N]).mean(), 1e-30))
    d_end = float(np.abs(lw[N] - want[N]).max() / np.abs(want[N]).mean())
    print(f"[debias_end] running log-weights max |HIP - reference| / mean |reference| {d_run:.2e}, end-of-trajectory "
          f"log-weights {d_end:.2e}, final walkers rel-L2 {rel(x, g['x_final']):.2e}")
    assert d_run < _END_BOUNDS[0] and d_end < _END_BOUNDS[1] and rel(x, g["x_final"]) < _END_BOUNDS[2]


# measured 8.4e-6 / 2.3e-7 / 1.8e-6
_END_BOUNDS = (3.4e-5, 1e-6, 7.2e-6)


def _long_stack(pa, golden, weights="egnn_weights_trainedlike.npz"):
    import copy

    from pita_amd.energy_net import EnergyNet

    w = golden(weights)
    net = make_net(pa, 13, 3, w)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    return sde, sched, pa.ConstantAnnealingFactorSchedule(4 / 3)


_LONG = {"trainedlike": ("em_traj_lj13_debias_long.npz", "egnn_weights_trainedlike.npz"),
         "init": ("em_traj_lj13_debias_long_init.npz", "egnn_weights_seed12345.npz")}
_TERMS = ("drift_A", "divergence_score", "cross_term", "dUt_dt")


def _long_terms_truth(g, w):
    """fp64 oracle on the ten recorded walker sets of a long fixture (the walkers ENTERING steps 0, 20, ..., 180, which the
    reference's own fp32 terms of those steps were computed from): {term: [10, B]} per inference chunk of 32."""
    w64 = {k: T(v).double() for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_forward(w64, cn, xs, b, 13, 3)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    N, B, chunk = (int(g[k]) for k in ("N", "B", "chunk"))
    times = torch.linspace(1.0, 0.0, N + 1)[:-1]
    out = {nm: [] for nm in _TERMS}
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(nthreads, 16))
    try:
        for k, s in enumerate(g["at"]):
            x = T(g["x_at"][k]).double()
            parts = [O.f_debiased(bb, bb, osched, ogam, times[int(s)].double(), x[lo:lo + chunk], 1.0)
                     for lo in range(0, B, chunk)]
            for nm in _TERMS:
                out[nm].append(torch.cat([getattr(p_, nm) for p_ in parts]).numpy())
    finally:
        torch.set_num_threads(nthreads)
    return {nm: np.stack(v) for nm, v in out.items()}


@pytest.mark.parametrize("which", ["trainedlike", "init"])
def test_debiased_default_regime_long_golden(pa, golden, monkeypatch, which):
    """PITA's DEFAULT regime at the LJ13 experiment's settings over a real horizon, against the reference's own run
    (em_traj_lj13_debias_long.npz; configs/experiment/lj13.yaml:24-42, model/energytemp.yaml:64-85): debiased drift,
    a resampling event after EVERY step of the window [0, 160), two inference chunks of 32 (per-chunk 0.9-quantile
    clamp), resample_at_end, 5 adaptive MALA steps; N = 200, B = 64, the fixture's PCG64 noise and uniforms.

    (1) The weight-drift terms to the standard of the headline kernel: on the ten recorded walker sets the fp64 oracle is
        the truth, and err(HIP, fp64) <= 4 x err(reference fp32, fp64) for every term of every set (both printed).
    (2) Through WeightedSDEIntegrator.integrate_sde:
      * the parent ids of all 161 events, event by event.  A differing id must be a +-1 neighbour with the event's
        uniform within fp32 rounding of the bin edge (counted; at most 2 % of the events may have one), and the
        reference's ids are then fed forward so the run stays on the recorded trajectory and EVERY later event is still
        compared exactly;
      * the weight-drift terms of all 200 steps, the walkers entering steps 0, 20, ..., 180, the end-of-trajectory
        log-weights and the final walkers, bounded at 4 x the deviation measured on MI355X (printed).
    (3) ``init`` (seed-12345 initialisation weights; em_traj_lj13_debias_long_init.npz): the run does not collapse -- log p
        after the end-of-trajectory event is -505 .. -755 -- so from the reference's recorded pre-event walkers the
        event's walkers (x_post_end) are reproduced EXACTLY, and the accept MASK of each of the five MALA steps at
        dt = 1e-5 (mixed decisions) and the acceptance rates at 4e-4 (all rejected) equal the reference's."""
    from tests._long_fixture import ids_mismatch_is_bin_edge_tie, long_fixture_draws

    import pita_amd.sde_integration as si

    init = which == "init"
    g = golden(_LONG[which][0])
    N, B, chunk, end, n_mala = (int(g[k]) for k in ("N", "B", "chunk", "end", "n_mala"))
    noise, mala_noise, mala_u, us = long_fixture_draws(g)
    sde, sched, gam = _long_stack(pa, golden, _LONG[which][1])
    energy = pa.LennardJonesEnergy(39, 13, 3)
    times = torch.linspace(1.0, 0.0, N + 1)[:-1]

    # (1) per-term accuracy against fp64 on the recorded walker sets
    truth = _long_terms_truth(g, golden(_LONG[which][1]))
    for k, s in enumerate(g["at"]):
        terms = sde.f(times[int(s)], cu(g["x_at"][k]), 1.0, gam, None, energy, 1, clamp_chunk=chunk)
        for nm in _TERMS:
            e_ref, e_hip = rel(g[nm][int(s)], truth[nm][k]), rel(getattr(terms, nm), truth[nm][k])
            print(f"[long/{which}] step {int(s):3d} {nm:16s}: HIP vs fp64 {e_hip:.2e}, reference vs fp64 {e_ref:.2e}")
            assert e_hip <= 4 * e_ref, (int(s), nm, e_hip, e_ref)

    # (2) the whole run through the integrator
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=end,
                                     resampling_interval=1, num_negative_time_steps=0, post_mcmc_steps=n_mala,
                                     adaptive_mcmc=True, dt_negative_time=float(g["dt_mala"]), batch_size=chunk,
                                     resample_at_end=True)
    events, seen = [], {"x": [], "terms": []}
    real_cat, real_f = si.sample_cat_sys, sde.f

    def forced_cat(bs, logits, u=None):
        ids, nu = real_cat(bs, logits, u)
        k = len(events)
        want = torch.as_tensor(g["ids"][k].astype(np.int64), device=ids.device)
        same = bool(torch.equal(ids, want))
        if not same:
            assert ids_mismatch_is_bin_edge_tie(logits.cpu().numpy(), float(us[k]), ids.cpu().numpy(), g["ids"][k]), \
                f"event {k}: ids differ from the reference's by more than a bin-edge tie"
        events.append(same)
        return want, nu

    def rec_f(t, x, *a, **k):
        if len(seen["terms"]) % 20 == 0:
            seen["x"].append(x.clone())
        terms = real_f(t, x, *a, **k)
        seen["terms"].append(terms)
        return terms

    monkeypatch.setattr(si, "sample_cat_sys", forced_cat)
    sde.f = rec_f
    try:
        x, logw, uniq, _, acc = integ.integrate_sde(cu(g["x1"]), energy, gam, inverse_temperature=1.0,
                                                    noise=cu(noise), resample_u=[float(u) for u in us],
                                                    mala_noise=cu(mala_noise), mala_uniforms=cu(mala_u))
    finally:
        sde.f = real_f
    assert len(events) == end + 1 and len(seen["terms"]) == N
    n_tie = sum(1 for e in events if not e)
    assert n_tie <= max(1, (end + 1) // 50), f"{n_tie} of {end + 1} events needed the bin-edge allowance"
    # deviations from the reference's own fp32 run along the trajectory: measured on MI355X (printed), bounds 4 x that
    bound_terms, bound_x = _LONG_BOUNDS[which]
    worst, worst_at = {nm: 0.0 for nm in _TERMS}, {nm: 0 for nm in _TERMS}
    for s in range(N):
        for nm in _TERMS:
            want = g[nm][s]
            dev_ = float(np.abs(getattr(seen["terms"][s], nm).cpu().numpy() - want).max() / np.abs(want).mean())
            if dev_ > worst[nm]:
                worst[nm], worst_at[nm] = dev_, s
    worst_x = max(rel(seen["x"][k], g["x_at"][k]) for k in range(len(g["at"])))
    print(f"[long/{which}] along the run, max |HIP - reference| / mean |reference| per term: "
          + ", ".join(f"{nm} {v:.2e} (step {worst_at[nm]})" for nm, v in worst.items())
          + f"; walkers entering the recorded steps {worst_x:.2e}, final walkers {rel(x, g['x_final']):.2e}, "
          f"{n_tie} bin-edge ties")
    for nm in _TERMS:
        assert worst[nm] < bound_terms, (nm, worst[nm])
    assert worst_x < bound_x
    assert logw.shape == (N + 1, B)
    np.testing.assert_array_equal(logw[:N].cpu().numpy(), 0.0)  # an event (or the closed window) resets a every step
    np.testing.assert_allclose(logw[N].cpu().numpy(), g["logweights"][N], rtol=2e-4)
    assert uniq == list(g["num_unique"])  # the fed-forward ids are the reference's
    assert len(acc) == n_mala
    if not init:
        assert rel(x, g["x_final"]) < bound_x
        # log p ~ -1e10 .. -1e21 on the collapsed final walkers: the 5 accept decisions per walker are signs of rounding
        # differences, so only the shape of the result is pinned here (the init fixture pins the decisions)
        assert all(0.0 <= r <= 1.0 for r in acc)
        return
    assert acc == [float(r) for r in g["mala_acc"]]
    assert rel(x, g["x_final"]) < bound_x

    # (3) the end-of-trajectory event and the chain from the reference's recorded pre-event walkers.  Walkers frozen
    # (start_resampling_step = N, :278-280) and not re-centred, so the event sees the recorded walkers bit for bit.
    captured = []
    integ2 = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=N, end_resampling_step=end,
                                      resampling_interval=1, num_negative_time_steps=0, post_mcmc_steps=n_mala,
                                      adaptive_mcmc=True, dt_negative_time=float(g["dt_mala"]), batch_size=chunk,
                                      resample_at_end=True, should_mean_free=False)
    real_mala = integ2.metropolis_hastings_mala_adaptive

    def rec_mala(xm, *a, **k):
        captured.append(xm.clone())
        return real_mala(xm, *a, **k)

    integ2.metropolis_hastings_mala_adaptive = rec_mala
    events.clear()
    events.extend([True] * end)  # forced_cat's event counter: the end-of-trajectory event is number `end`
    x2, logw2, uniq2, _, acc2 = integ2.integrate_sde(cu(g["x_pre_end"]), energy, gam, inverse_temperature=1.0,
                                                     resample_u=[float(us[end])], mala_noise=cu(mala_noise),
                                                     mala_uniforms=cu(mala_u))
    assert events[end], "the end-of-trajectory event's parent ids differ from the reference's"
    np.testing.assert_array_equal(captured[0].cpu().numpy(), g["x_post_end"])
    np.testing.assert_allclose(energy(captured[0]).cpu().numpy(), g["logp_post_end"], rtol=5e-6)
    np.testing.assert_allclose(logw2[N].cpu().numpy(), g["logweights"][N], rtol=2e-4)
    assert acc2 == [float(r) for r in g["mala_acc"]] and rel(x2, g["x_final"]) < 1e-6
    # the accept mask of every step: the chain re-run with 1 .. 5 steps (deterministic in its draws); an accepted
    # proposal moved the walker by ~sqrt(dt), a rejected one only by the re-centring's rounding
    prev = captured[0]
    for k in range(1, n_mala + 1):
        integ2.post_mcmc_steps = k
        xk, rk = real_mala(captured[0].clone(), energy, dt_init=float(g["dt_mala"]), return_acceptance_rate=True,
                           noise=cu(mala_noise), uniforms=cu(mala_u))
        moved = (xk - prev).abs().amax(1).cpu().numpy() > 1e-3 * float(g["dt_mala"]) ** 0.5
        np.testing.assert_array_equal(moved, g["mala_accept"][k - 1], err_msg=f"accept mask of MALA step {k - 1}")
        assert rel(xk, g["x_mala"][k]) < 1e-6 and rk == [float(r) for r in g["mala_acc"][:k]]
        prev = xk
    integ2.post_mcmc_steps = n_mala
    xa, ra = real_mala(captured[0].clone(), energy, dt_init=float(g["dt_mala_alt"]), return_acceptance_rate=True,
                       noise=cu(mala_noise), uniforms=cu(mala_u))
    assert ra == [float(r) for r in g["mala_acc_alt"]] and rel(xa, g["x_final_alt"]) < 1e-6


# bounds of part (2) above: 4 x the deviations measured on MI355X (profiles/r05_parity_measured.txt) -- (terms, walkers).
# Measured: trained-like 3.3e-6 (divergence, step 199) / 2.2e-7; init 7.4e-4 (dU/dt, step 197: there the REFERENCE's fp32
# dU/dt is the less accurate of the two -- at step 180 it is 4.0e-5 from fp64, the HIP value 1.5e-6) / 2.4e-7
_LONG_BOUNDS = {"trainedlike": (1.4e-5, 9e-7), "init": (3e-3, 1e-6)}


def test_debiased_default_regime_long_free_run(pa, golden):
    """The same run WITHOUT feeding the reference's ids forward: after the first bin-edge tie two correct samplers are on
    different trajectories, so the comparison is statistical -- the trace of distinct parents per event and the final
    interatomic-distance distribution against the reference's, bounded by the sampler's own spread over resampling
    uniforms."""
    from tests._long_fixture import long_fixture_draws

    g = golden("em_traj_lj13_debias_long.npz")
    N, B, chunk, end = (int(g[k]) for k in ("N", "B", "chunk", "end"))
    noise, _, _, us = long_fixture_draws(g)
    sde, sched, gam = _long_stack(pa, golden)

    def run(u):
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0,
                                         end_resampling_step=end, resampling_interval=1, num_negative_time_steps=0,
                                         post_mcmc_steps=0, batch_size=chunk, resample_at_end=False)
        x, _, uniq, _, _ = integ.integrate_sde(cu(g["x1"]), pa.LennardJonesEnergy(39, 13, 3), gam,
                                               inverse_temperature=1.0, noise=cu(noise), resample_u=[float(v) for v in u])
        v = x.reshape(B, 13, 3)
        d = torch.cdist(v, v)[:, torch.triu(torch.ones(13, 13, dtype=torch.bool), 1)].reshape(-1).cpu().numpy()
        return np.asarray(uniq[:end], dtype=np.float64), d

    uq, d = run(us)
    ref_uq = g["num_unique"][:end].astype(np.float64)
    vr = g["x_pre_end"].reshape(B, 13, 3)
    ref_d = np.linalg.norm(vr[:, :, None] - vr[:, None], axis=-1)[:, np.triu(np.ones((13, 13), dtype=bool), 1)].reshape(-1)
    others = [run(np.random.default_rng(100 + i).random(end + 1)) for i in range(3)]
    spread_uq = max(abs(o[0].mean() - uq.mean()) for o in others)
    spread_d = max(O.w2_1d(o[1], d) for o in others)
    assert abs(uq.mean() - ref_uq.mean()) <= max(2 * spread_uq, 0.5), (uq.mean(), ref_uq.mean(), spread_uq)
    assert O.w2_1d(d, ref_d) <= 2 * spread_d + 1e-3, (O.w2_1d(d, ref_d), spread_d)


def test_default_regime_at_metric_batch(pa, golden):
    """The LJ13 experiment's settings at the METRIC'S batch (65 536 walkers, inference chunks of 512, debiased, an event
    after every step of the window, resample_at_end, 5 adaptive MALA steps at dt = 1e-13) for 20 steps: size-independent
    properties -- every walker finite, the log-weights zero after every event and outside the window, the number of
    distinct parents in [1, B] and below B whenever weights differ, the end-of-trajectory log-weights clamped at their
    0.9 quantile (a tenth of them equal the maximum), centre of mass zero."""
    sde, sched, gam = _long_stack(pa, golden)
    B, N, end = 65536, 20, 16
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=end,
                                     resampling_interval=1, num_negative_time_steps=0, post_mcmc_steps=5,
                                     adaptive_mcmc=True, dt_negative_time=1e-13, batch_size=512, resample_at_end=True,
                                     seed=11)
    scale = float((sched.h(torch.tensor(1.0)) / gam.gamma(torch.tensor(1.0))) ** 0.5)
    x1 = pa.Prior(scale=scale, n_particles=13, spatial_dim=3, seed=5).sample(B)
    x, logw, uniq, terms, acc = integ.integrate_sde(x1, pa.LennardJonesEnergy(39, 13, 3), gam, inverse_temperature=1.0)
    assert x.shape == (B, 39) and bool(torch.isfinite(x).all())
    assert logw.shape == (N + 1, B) and len(uniq) == N + 1 and len(terms) == N and len(acc) == 5
    assert bool((logw[:N] == 0).all())
    assert all(1 <= u <= B for u in uniq) and all(u < B for u in uniq[:end]) and all(u == B for u in uniq[end:N])
    fin = logw[N]
    assert bool(torch.isfinite(fin).all())
    # clamped at the 0.9 quantile (sde_integration.py:179): the top tenth of the walkers sits AT the maximum
    assert int((fin == fin.max()).sum()) >= int(0.1 * (B - 1))
    assert float(x.reshape(B, 13, 3).mean(1).abs().max()) < 1e-4
    for t in terms:  # device-reduced statistics of every step answer the reference's logging calls
        assert np.isfinite(float(t.drift_A.mean())) and np.isfinite(float(t.divergence_score.std()))


@pytest.mark.parametrize("n,chunk", [(12, 12), (1000, 1000), (65536, 512), (65536, 65536), (777, 100), (5, 1), (4096, 1024), (4100, 1025)])
def test_quantile_clamp_kernel(pa, n, chunk):
    """K11 against torch.quantile (CPU) per chunk: exact order statistics, torch's lerp."""
    gen = torch.Generator().manual_seed(n + chunk)
    a = torch.randn(n, generator=gen) * 10
    a[::7] = a[0]  # ties
    want = a.clone()
    for lo in range(0, n, chunk):
        c = want[lo:lo + chunk]
        want[lo:lo + chunk] = torch.clamp(c, max=torch.quantile(c, 0.9))
    got = a.cuda().clone()
    pa._lib.check(pa._lib.lib().pita_quantile_clamp(got.data_ptr(), n, chunk, 0.9, pa._lib.stream_ptr()))
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-6)


from tests._synthetic import synthetic_peptide as _synthetic_peptide  # noqa: E402


@pytest.mark.parametrize("gb", [False, True])
@pytest.mark.parametrize("cutoff", [None, 0.45])
def test_forcefield_vs_oracle(pa, cutoff, gb):
    """K4 (parity unpinned): HIP force field vs the oracle's restatement of the same OpenMM functional forms, with
    autograd forces, on a synthetic 22-atom topology; 16 384 walkers (config C4 batch) spot-checked.  gb: with the
    GB-OBC1 implicit solvent + ACE surface area of implicit/obc1.xml (radii / scale factors of amber magnitude)."""
    from pita_amd.alp_energy import ForceFieldEnergy

    tabs, pos = _synthetic_peptide()
    if gb:
        rng = np.random.default_rng(3)
        tabs["gb_radius"] = rng.choice([0.12, 0.13, 0.15, 0.155, 0.17], 22)
        tabs["gb_scale"] = rng.choice([0.72, 0.79, 0.85], 22)
    ff_t = {k: torch.as_tensor(v) for k, v in tabs.items()}
    ff_t = {k: (v.long() if "idx" in k else v.float()) for k, v in ff_t.items()}
    scale = 0.1640
    gen = torch.Generator().manual_seed(5)
    B = 16384
    x = (torch.tensor(pos.reshape(-1), dtype=torch.float32)[None] + 0.004 * torch.randn(B, 66, generator=gen)) / scale
    e = ForceFieldEnergy(tabs, n_particles=22, temperature=300.0, data_normalization_factor=scale, cutoff=cutoff)
    lp, f = e(x.cuda(), return_force=True)
    assert torch.equal(lp, e(x.cuda()))
    assert torch.isfinite(lp).all() and torch.isfinite(f).all()
    idx = torch.arange(0, B, 257)
    lpo, fo = O.ff_logp_force(x[idx].double(), {k: v.double() if v.is_floating_point() else v for k, v in ff_t.items()},
                              e.kT, scale, cutoff)
    np.testing.assert_allclose(lp[idx.cuda()].cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=2e-3)
    assert rel(f[idx.cuda()], fo) < 5e-5
    assert abs(f.reshape(B, 22, 3).sum(1)).max() < 1e-3 * f.abs().max().item()  # translation invariance
    # the torsion angle enters through an angle-addition recurrence over its (integer) periodicity: anything else is refused
    bad = {k: np.array(v, copy=True) for k, v in tabs.items()}
    bad["tors_par"][0, 0] = 2.5
    with pytest.raises(pa._lib.PitaHipError, match="periodicity"):
        ForceFieldEnergy(bad, n_particles=22, temperature=300.0, data_normalization_factor=scale, cutoff=cutoff)(x[:4].cuda())


def test_alp_energy_from_system_xml_vs_oracle(pa, golden):
    """A14 boundary: ``ALPEnergy(..., system_xml=)`` (reference constructor names, alp_energy.py:41-59) on the committed
    serialized-System fixture == the oracle's restatement of OpenMM's functional forms on the same tables (bonded,
    nonbonded with reaction field, GB-OBC1), in chunks of ``energy_batch_size`` like alp_energy.py:127-145.
    Parity with OpenMM itself stays unpinned (no OpenMM, no amber14 tables in the reference tree)."""
    from pita_amd.alp_energy import ALPEnergy
    from tests._synthetic import synthetic_peptide_gb

    path = os.path.join(ROOT, "tests", "golden", "synthetic_peptide22_system.xml")
    tabs, pos = synthetic_peptide_gb(22)
    scale, B = 0.1640, 1000
    e = ALPEnergy(data_path=None, pdb_filename="A_capped.pdb", dimensionality=66, n_particles=22, temperature=300.0,
                  data_normalization_factor=scale, energy_batch_size=300, system_xml=path)
    gen = torch.Generator().manual_seed(6)
    x = (torch.tensor(pos.reshape(-1), dtype=torch.float32)[None] + 0.004 * torch.randn(B, 66, generator=gen)) / scale
    lp, f = e(x.cuda(), return_force=True)
    assert lp.shape == (B,) and f.shape == (B, 66) and torch.equal(lp, e(x.cuda()))
    e1 = ALPEnergy(dimensionality=66, n_particles=22, temperature=300.0, data_normalization_factor=scale, system_xml=path)
    assert torch.equal(e1(x.cuda()), lp)  # chunking does not change a walker's value
    ff_t = {k: torch.as_tensor(v) for k, v in tabs.items()}
    ff_t = {k: (v.long() if "idx" in k else v.double()) for k, v in ff_t.items()}
    idx = torch.arange(0, B, 37)
    lpo, fo = O.ff_logp_force(x[idx].double(), ff_t, e.kT, scale, 2.0)
    np.testing.assert_allclose(lp[idx.cuda()].cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=2e-3)
    assert rel(f[idx.cuda()], fo) < 5e-5
    # should_normalize=False: the samples are taken as nanometres (maybe_unnormalize is the identity)
    e2 = ALPEnergy(dimensionality=66, n_particles=22, temperature=300.0, data_normalization_factor=scale,
                   should_normalize=False, system_xml=path)
    np.testing.assert_allclose(e2((x * scale).cuda()).cpu().numpy(), lp.cpu().numpy(), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("N", [40, 1000])
def test_final_histograms_match_oracle_sampler(pa, golden, N):
    """Distribution-level parity of the whole sampler with its OWN noise (Philox): the final interatomic-distance and
    energy histograms of the HIP run must be as close to an oracle run (torch noise, fp32 CPU) as two oracle runs with
    different seeds are to each other (1-D Wasserstein-2; 4x margin).  LJ13, EGNN h32x3, from the prior, 40 steps and
    the metric's own 1 000 steps (experiment/lj13.yaml; ~1 min of oracle time per seed)."""
    w = golden("egnn_weights_trainedlike.npz")
    wt = {k: T(v) for k, v in w.items()}
    B = 1024
    bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, 13, 3)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    cfg = O.IntegratorConfig(num_integration_steps=N, start_resampling_step=0, end_resampling_step=N, resampling_interval=-1)
    scale = 80.0 / np.sqrt(4 / 3)
    iu = np.triu_indices(13, 1)

    def stats(x):
        x = x.detach().cpu().float()
        d = (x.reshape(-1, 13, 1, 3) - x.reshape(-1, 1, 13, 3)).norm(dim=-1)[:, iu[0], iu[1]].reshape(-1).numpy()
        le = np.log10(-O.lj_logp(x, 13, 3).numpy())  # energies span 8 decades with these weights: compare in log
        return d, le

    ref = []
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(16, nthreads))  # small ops: more threads only add overhead on a 256-thread host
    for seed in (1, 2):
        gen = torch.Generator().manual_seed(seed)
        x1 = O.remove_mean(torch.randn(B, 39, generator=gen) * scale, 13, 3)
        out = O.integrate_sde(cfg, x1, lambda t, xc: O.f_not_debiased(bb, osched, ogam, t, xc, 1.0), osched.g,
                              lambda i, shp: torch.randn(shp, generator=gen), 13, 3)
        ref.append(stats(out["x"]))
    torch.set_num_threads(nthreads)
    net = make_net(pa, 13, 3, w)
    sde = pa.VEReverseSDE(noise_schedule=pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7),
                          score_net=pa.ScoreNet(net), debias_inference=False)
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                     resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0, seed=77)
    x1 = pa.Prior(scale=scale, n_particles=13, spatial_dim=3, seed=5).sample(B)
    x, _, _, _, _ = integ.integrate_sde(x1, pa.LennardJonesEnergy(39, 13, 3), pa.ConstantAnnealingFactorSchedule(4 / 3),
                                        inverse_temperature=1.0)
    got = stats(x)
    from pita_amd import metrics

    for k, name in enumerate(("interatomic distance", "log10 energy")):
        seed_to_seed = O.w2_1d(ref[0][k], ref[1][k])
        # the product's own metric (pita_amd.metrics, device sort) measures the HIP run; the oracle's W2 checks it
        w2 = lambda a, b: np.sqrt(metrics._w_1d(torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda(), 2))
        assert abs(w2(got[k], ref[0][k]) - O.w2_1d(got[k], ref[0][k])) < 1e-6 * (1 + seed_to_seed)
        hip_to_ref = max(w2(got[k], ref[0][k]), w2(got[k], ref[1][k]))
        assert hip_to_ref < 4 * seed_to_seed + 1e-3 * float(np.abs(ref[0][k]).mean()), (name, hip_to_ref, seed_to_seed)
        # the reference's figure view of the same comparison (base_molecule_energy_function.py:160-254): 100-bin densities on
        # the edges of oracle run 0 (device histogram kernel); bin-wise L1 (total-variation-like, in [0, 2]) of the HIP run
        # against an oracle run within 4x the oracle's own seed-to-seed L1
        edges = np.histogram_bin_edges(ref[0][k].astype(np.float32), bins=100)
        dens = lambda a: metrics._density(metrics.histogram(torch.as_tensor(a, dtype=torch.float32).cuda(), edges), edges)
        l1 = lambda a, b: float((np.abs(dens(a) - dens(b)) * np.diff(edges.astype(np.float64))).sum())
        l1_seed, l1_hip = l1(ref[0][k], ref[1][k]), max(l1(got[k], ref[0][k]), l1(got[k], ref[1][k]))
        print(f"\n{name}: W2 HIP-vs-oracle {hip_to_ref:.4g} (oracle seed to seed {seed_to_seed:.4g}); 100-bin L1 {l1_hip:.4g} (seed to seed {l1_seed:.4g})")
        assert l1_hip < 4 * l1_seed + 0.02, (name, l1_hip, l1_seed)


def test_histogram_kernel_and_reference_sample_histograms(pa):
    """pita_histogram against numpy.histogram, count for count -- uniform edges from a data range (what matplotlib's
    `hist(bins=100)` builds), values exactly on edges, out-of-range values, NaNs, a sample much larger than the grid --
    and pita_amd.metrics.sample_histograms against the reference's own construction of the two 100-bin density pairs
    (base_molecule_energy_function.py:160-254: distance bins from the test set; energies over (min - 10, max + 10))."""
    from pita_amd import metrics

    rng = np.random.default_rng(3)
    for n, nb in ((1, 1), (1000, 7), (300_000, 100), (5_000_000, 1024)):
        v = rng.normal(2.0, 1.5, n).astype(np.float32)
        edges = np.histogram_bin_edges(v, bins=nb)
        v2 = np.concatenate([v, edges[: min(nb + 1, 50)], [np.nan, np.inf, -np.inf, edges[0] - 1.0, edges[-1] + 1.0]]).astype(np.float32)
        want = np.histogram(v2[np.isfinite(v2)], bins=edges)[0]
        got = metrics.histogram(torch.from_numpy(v2).cuda(), edges).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, nb, np.abs(got - want).max())
    # non-uniform edges (the explicit `bins=` call of the reference's second histogram takes any ascending edges)
    edges = np.sort(rng.uniform(-3, 8, 65)).astype(np.float32)
    v = rng.normal(2.0, 3.0, 200_000).astype(np.float32)
    assert np.array_equal(metrics.histogram(torch.from_numpy(v).cuda(), edges).cpu().numpy(), np.histogram(v, bins=edges)[0])
    with pytest.raises(pa._lib.PitaHipError):
        metrics.histogram(torch.zeros(4).cuda(), np.linspace(0, 1, 1026))  # more bins than the kernel's LDS copy holds
    # the reference's figure numbers on LJ13 configurations
    energy = pa.LennardJonesEnergy(39, 13, 3)
    gen = torch.Generator().manual_seed(4)
    base = O.remove_mean(torch.randn(1, 39, generator=gen) * 0.9, 13, 3)
    test_set = O.remove_mean(base + 0.08 * torch.randn(5000, 39, generator=gen), 13, 3).cuda()
    samples = O.remove_mean(base + 0.10 * torch.randn(3000, 39, generator=gen), 13, 3).cuda()
    h = metrics.sample_histograms(energy, samples, test_set)
    dt, ds = energy.interatomic_dist(test_set).cpu().numpy().reshape(-1), energy.interatomic_dist(samples).cpu().numpy().reshape(-1)
    wt, bins = np.histogram(dt, bins=100, density=True)
    ws, _ = np.histogram(ds, bins=bins, density=True)
    assert np.array_equal(h["dist_edges"], bins) and np.allclose(h["dist_test"], wt, rtol=0, atol=0) and np.allclose(h["dist_samples"], ws, rtol=0, atol=0)
    et, es = -energy(test_set).cpu().numpy(), -energy(samples).cpu().numpy()
    rngE = (float(et.min()) - 10, float(et.max()) + 10)
    wt, bins = np.histogram(et, bins=100, density=True, range=rngE)
    ws, _ = np.histogram(es, bins=bins, density=True, range=rngE)
    assert np.array_equal(h["energy_edges"], bins) and np.array_equal(h["energy_test"], wt) and np.array_equal(h["energy_samples"], ws)
    assert abs(float((h["dist_test"] * np.diff(h["dist_edges"])).sum()) - 1.0) < 1e-12


def test_checkpoint_to_samples_to_metrics_round_trip(pa, golden, tmp_path):
    """Edges of the path on real artefact layouts: a Lightning-layout checkpoint with raw and EMA
    shadow parameters (energytemp_module.py:94-111, ema.py:6-80) -> io.load_reference_checkpoint -> HIP sampler ->
    samples_temperature_*.pt (:1040-1041) -> reload -> energy W1/W2 and interatomic-distance W2 (:1157-1191,
    distribution_distances.py:13-33) on HIP energies, checked against the oracle's sorted-sample W2."""
    import copy

    from pita_amd import io, metrics
    from pita_amd.energy_net import EnergyNet

    w_raw = golden("egnn_weights_seed12345.npz")       # "raw" training weights
    w_ema = golden("egnn_weights_trainedlike.npz")     # what the EMA shadow holds
    src = make_net(pa, 13, 3, w_raw)
    names = [n for n, p_ in src.named_parameters() if p_.requires_grad]
    state = {"score_net.model.model." + k: T(v) for k, v in w_raw.items()}
    state.update({"energy_net.model.net." + k: T(v) for k, v in w_raw.items()})
    for pre in ("score_net", "energy_net"):
        state.update({f"{pre}.shadow_params.{i}": T(w_ema[n]) for i, n in enumerate(names)})
        state[f"{pre}.num_updates"] = torch.tensor(1234)
    state["h_theta." + next(iter(w_raw))] = T(next(iter(w_raw.values())))
    ckpt = tmp_path / "last.ckpt"
    torch.save({"state_dict": state, "epoch": 3, "hyper_parameters": {"ema_decay": 0.999}}, ckpt)

    torch.manual_seed(99)  # the nets start from unrelated weights: everything must come from the file
    mk = lambda: pa.EGNN_dynamics(13, 3, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                                  condition_time=True, condition_temperature=True, agg="sum")
    sn, en = pa.ScoreNet(mk()), EnergyNet(mk())
    rep = io.load_reference_checkpoint(str(ckpt), sn, en, use_ema=True)
    assert rep["ema"] == ["score_net.shadow_params", "energy_net.shadow_params"] and not rep["missing"]
    assert rep["layout"] == ["score_net.model.model", "energy_net.model.net"]
    for k, v in sn.model.state_dict().items():
        want = w_ema[k] if k in names else w_raw[k]
        assert np.array_equal(v.cpu().numpy(), want), k

    # sample with the loaded nets; the same run from nets built directly from the EMA weights must agree bitwise
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    e = pa.LennardJonesEnergy(39, 13, 3)
    N, B = 30, 2048
    x1 = pa.Prior(scale=80.0 / np.sqrt(4 / 3), n_particles=13, spatial_dim=3, seed=11).sample(B)

    def sample(score_net):
        sde = pa.VEReverseSDE(noise_schedule=sched, score_net=score_net, energy_net=en, debias_inference=False)
        integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                         resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0, seed=5)
        return integ.integrate_sde(x1, e, gam, inverse_temperature=1.0)[0]

    xa = sample(sn)
    direct = make_net(pa, 13, 3, {k: (w_ema[k] if k in names else w_raw[k]) for k in w_raw})
    assert torch.equal(xa, sample(pa.ScoreNet(direct)))
    path = tmp_path / "samples_temperature_3.0.pt"
    io.save_samples(xa, str(path))
    xb = io.load_samples(str(path))
    assert xb.is_cuda and torch.equal(xa, xb)

    # metrics against a second sample set (different Philox seed) through the product's functions, oracle W2 as checker
    x2 = pa.Prior(scale=80.0 / np.sqrt(4 / 3), n_particles=13, spatial_dim=3, seed=12).sample(B)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=sn, energy_net=en, debias_inference=False)
    xc = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N,
                                  resampling_interval=-1, num_negative_time_steps=0, post_mcmc_steps=0,
                                  seed=6).integrate_sde(x2, e, gam, inverse_temperature=1.0)[0]
    ea, ec = -e(xb), -e(xc)   # energies (the reference logs -log p)
    # these untrained-net samples have enormous energies; compare on a monotone transform so W2 is well conditioned
    la, lc = torch.log10(ea.clamp_min(1.0)), torch.log10(ec.clamp_min(1.0))
    d = metrics.energy_distances(la, lc, prefix="test")
    assert abs(d["test/energy_w2"] - O.w2_1d(lc.cpu().numpy(), la.cpu().numpy())) < 1e-9
    assert d["test/energy_w1"] <= d["test/energy_w2"] + 1e-12 and d["test/num_cropped"] == 0
    dw2 = metrics.interatomic_w2(e, xb, xc)
    iu = np.triu_indices(13, 1)
    dist = lambda x: (x.reshape(-1, 13, 1, 3) - x.reshape(-1, 1, 13, 3)).norm(dim=-1)[:, iu[0], iu[1]].reshape(-1)
    assert abs(dw2 - O.w2_1d(dist(xc.cpu()).numpy(), dist(xb.cpu()).numpy())) < 1e-5 * (1 + dw2)


def test_not_debiased_resample_at_end(pa, golden):
    """resample_at_end in the not-debiased regime (sde_integration.py:158-183 with a = 0): weights
    log p_target(x) + gamma E_theta(h(t_end), x), 0.9-quantile clamp, systematic resampling -- against the oracle."""
    import copy

    from pita_amd.energy_net import EnergyNet

    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, 13, 3, w)
    N, B, end, interval = 10, 24, 8, 4
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=False)
    gen = torch.Generator().manual_seed(123)
    x1 = O.remove_mean(torch.randn(B, 39, generator=gen) * 3, 13, 3)
    noise = torch.randn(N, B, 39, generator=gen)
    events = [s for s in range(0, end) if (s + 1) % interval == 0]
    us = {s: float(torch.rand(1, generator=gen, dtype=torch.float64)) for s in events}
    u_end = float(torch.rand(1, generator=gen, dtype=torch.float64))
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=end,
                                     resampling_interval=interval, num_negative_time_steps=0, post_mcmc_steps=0,
                                     resample_at_end=True)
    x, logw, uniq, _, _ = integ.integrate_sde(x1.cuda(), pa.LennardJonesEnergy(39, 13, 3), gam, inverse_temperature=1.0,
                                              noise=noise.cuda(), resample_u=[us[s] for s in events] + [u_end])
    wt = {k: T(v) for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, 13, 3)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    cfg = O.IntegratorConfig(num_integration_steps=N, start_resampling_step=0, end_resampling_step=end,
                             resampling_interval=interval)
    ref = O.integrate_sde(cfg, x1, lambda t, xc: O.f_not_debiased(bb, osched, ogam, t, xc, 1.0), osched.g,
                          lambda i, shp: noise[i], 13, 3, uniform_fn=lambda s: us[s])
    t_end = torch.linspace(1.0, 0.0, N + 1)[:-1][end]
    xe, a_next, nu = O.resample_at_end(ref["x"], torch.zeros(B), t_end, lambda xx: O.lj_logp(xx, 13, 3),
                                       lambda tb, xx: O.energy_theta(bb, osched.h(tb), xx, 1.0), 4 / 3, u_end)
    assert logw.shape == (N + 1, B) and uniq == ref["num_unique"] + [nu]
    # x differs by the rounding accumulated over 10 steps; r^-12 amplifies it 12-fold in the weights
    np.testing.assert_allclose(logw[N].cpu().numpy(), a_next.numpy(), rtol=3e-3)
    assert rel(x, xe) < 2e-4


@pytest.mark.parametrize("start,end,interval", [(0, 12, -1), (3, 12, -1), (2, 9, 3), (0, 12, 1), (5, 7, 2)])
def test_integrator_window_and_resampling_semantics(pa, golden, start, end, interval):
    """A2 gates (sde_integration.py:278-297): walkers frozen before start_resampling_step, resampling events only
    inside the window when (step+1) % interval == 0; not-debiased weights are zero so every event resamples with
    uniform weights.  Same noise and uniforms on both sides -> trajectories agree to fp32 rounding."""
    w = golden("egnn_weights_trainedlike.npz")
    net = make_net(pa, 13, 3, w)
    N, B = 12, 21
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), debias_inference=False)
    gen = torch.Generator().manual_seed(start * 100 + end * 10 + interval + 50)
    x1 = O.remove_mean(torch.randn(B, 39, generator=gen) * 3, 13, 3)
    noise = torch.randn(N, B, 39, generator=gen)
    us = {s: float(torch.rand(1, generator=gen, dtype=torch.float64)) for s in range(N)}
    events = [] if interval == -1 else [s for s in range(start, min(end, N)) if (s + 1) % interval == 0]
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=N, start_resampling_step=start,
                                     end_resampling_step=end, resampling_interval=interval, num_negative_time_steps=0,
                                     post_mcmc_steps=0)
    e = pa.LennardJonesEnergy(39, 13, 3)
    x, logw, uniq, _, _ = integ.integrate_sde(x1.cuda(), e, gam, inverse_temperature=1.0, noise=noise.cuda(),
                                              resample_u=[us[s] for s in events])
    wt = {k: T(v) for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, 13, 3)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    cfg = O.IntegratorConfig(num_integration_steps=N, start_resampling_step=start, end_resampling_step=end,
                             resampling_interval=interval)
    ref = O.integrate_sde(cfg, x1, lambda t, xc: O.f_not_debiased(bb, osched, ogam, t, xc, 1.0), osched.g,
                          lambda i, shp: noise[i], 13, 3, uniform_fn=lambda s: us[s])
    assert rel(x, ref["x"]) < 2e-4
    assert uniq == ref["num_unique"]
    assert float(logw.abs().max()) == 0.0 and logw.shape == (N, B)
