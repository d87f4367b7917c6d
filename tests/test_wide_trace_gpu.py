"""pita_egnn_wide_jacobian_trace / EGNN_dynamics_AD2_cat.jacobian_trace: trace(J_x D) of the EDM denoiser around the wide
EGNN backbone, and D itself, from ONE call whose work items are (walker, unit direction) pairs.  The contract is bitwise:
every item is computed exactly as the single-direction launch ``jvp(direction=k, diag_acc=acc)`` computes it and the
reduction adds the diagonal entries in direction order from +0, so the call has the bits of the n*d launches it replaces
(and therefore their error against the fp64 oracle: the bounds below are those of
test_hip_parity.py::test_egnn_ad2cat_forward_mode_vs_oracle_jacobian, no new tolerance).  Run on an MI355X: pytest -m gpu.

Shapes: 22 atoms (the matrix-pipe kernel, 66 directions) at B = 1, 6 and 17 -- 17 walkers are 1 122 items, more than the
1 024 waves one launch holds on 256 compute units, so the grid-stride loop wraps --, and 33 atoms (vector-pipe kernel for
all items, 99 directions) at B = 3."""
import numpy as np
import pytest
import torch

from oracle import pita_oracle as O

pytestmark = pytest.mark.gpu

T = torch.tensor
NETS = {"h64": dict(L=5, tanh=True, att=True), "h48": dict(L=2, tanh=False, att=False)}
BATCHES = (1, 6, 17)


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


def direction_loop(net, h, x, beta, D):
    """The launches the single call replaces, as VEReverseSDE._denoiser_jacobian_terms issues them for the trace."""
    acc = torch.zeros(x.shape[0], device="cuda")
    den = None
    for k in range(D):
        out, _ = net.jvp(h, x, beta, direction=k, want_primal=(k == 0), want_tangent=False, diag_acc=acc)
        den = out if k == 0 else den
    return acc, den


def oracle_trace(wd, h, x, beta, n, **kw):
    """(trace J_x D, D) of the fp64 oracle: vmap(jacrev) of O.denoiser around O.egnn_ad2_cat_forward (utils.py:30-51)."""
    from torch.func import jacrev, vmap

    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, n, 3, **kw)
    one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
    Jx = vmap(jacrev(one, argnums=1))(h.double(), x.double(), beta.double())
    return Jx.diagonal(dim1=1, dim2=2).sum(-1), O.denoiser(bb, h.double(), x.double(), beta.double())


@pytest.fixture(scope="module")
def cases(pa, golden):
    """Per golden net: the module, the golden's 12 walkers and the fp64 oracle on them (computed once, never modified);
    a batch of B walkers is rows ``arange(B) % 12`` of it."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    out = {}
    for tag, c in NETS.items():
        g = golden(f"egnn_ad2cat_{tag}_fwd.npz")
        w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
        net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=w["egnn.embedding.weight"].shape[0], n_layers=c["L"], tanh=c["tanh"],
                                    attention=c["att"], condition_beta=True)
        net.load_state_dict(w)
        x, h, beta = T(g["x"]), T(g["h"]), T(g["beta"])
        tr64, D64 = oracle_trace({k: v.double() for k, v in w.items()}, h, x, beta, 22, n_layers=c["L"], tanh=c["tanh"],
                                 attention=c["att"])
        out[tag] = dict(net=net, x=x, h=h, beta=beta, trace64=tr64, D64=D64)
    return out


def batch(c, B):
    rows = torch.arange(B) % c["x"].shape[0]
    return rows, c["h"][rows].cuda(), c["x"][rows].cuda(), c["beta"][rows].cuda()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("tag", list(NETS))
def test_single_call_has_the_bits_of_the_direction_loop(cases, tag, B):
    c = cases[tag]
    net = c["net"]
    _, h, x, beta = batch(c, B)
    assert net.uses_matrix_pipe("cuda:0")
    trace, D = net.jacobian_trace(h, x, beta, want_denoiser=True)
    acc, den = direction_loop(net, h, x, beta, 66)
    assert trace.shape == (B,) and D.shape == (B, 66)
    assert torch.equal(trace, acc), (trace - acc).abs().max()
    assert torch.equal(D, den)
    t2, none = net.jacobian_trace(h, x, beta)  # the trace alone: same bits, no denoiser
    assert none is None and torch.equal(t2, trace)


@pytest.mark.parametrize("tag", list(NETS))
def test_empty_batch(cases, tag):
    c = cases[tag]
    _, h, x, beta = batch(c, 0)
    trace, D = c["net"].jacobian_trace(h, x, beta, want_denoiser=True)
    assert trace.shape == (0,) and D.shape == (0, 66)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("tag", list(NETS))
def test_against_the_fp64_oracle(cases, tag, B):
    c = cases[tag]
    rows, h, x, beta = batch(c, B)
    trace, D = c["net"].jacobian_trace(h, x, beta, want_denoiser=True)
    want = c["trace64"][rows].numpy()
    scale = float(np.abs(want).mean()) + 1.0
    print(f"[wide trace/{tag}/B={B}] max |trace - fp64| = {np.abs(trace.cpu().numpy() - want).max():.3e} "
          f"(mean |trace| {scale - 1.0:.3e}), denoiser rel {rel(D, c['D64'][rows]):.3e}")
    np.testing.assert_allclose(trace.cpu().numpy(), want, rtol=5e-5, atol=5e-5 * scale)
    assert rel(D, c["D64"][rows]) < 2e-6


@pytest.mark.parametrize("tag", list(NETS))
def test_out_of_range_items_are_repaired_by_the_vector_pipe(cases, tag, monkeypatch):
    """beta[1] = 1e7 drives walker 1's activations out of the f16 range: its items come from the fp32 vector-pipe kernel
    (bit for bit the trace under PITA_WIDE_NO_MFMA), every other walker keeps the matrix-pipe kernel's bits."""
    c = cases[tag]
    net = c["net"]
    B = 6
    _, h, x, beta = batch(c, B)
    assert net.uses_matrix_pipe("cuda:0")
    trace, D = net.jacobian_trace(h, x, beta, want_denoiser=True)
    hot = beta.clone()
    hot[1] = 1.0e7
    trace_hot, D_hot = net.jacobian_trace(h, x, hot, want_denoiser=True)
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        assert not net.uses_matrix_pipe("cuda:0")
        trace_vec, D_vec = net.jacobian_trace(h, x, hot, want_denoiser=True)
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    assert torch.equal(trace_hot[1].view(torch.int32), trace_vec[1].view(torch.int32))
    assert torch.equal(D_hot[1].view(torch.int32), D_vec[1].view(torch.int32))
    keep = torch.arange(B) != 1
    assert torch.equal(trace_hot[keep], trace[keep])
    assert torch.equal(D_hot[keep], D[keep])


def test_vector_pipe_shape_33_atoms(pa):
    """33 atoms: no matrix-pipe instantiation of the forward-mode kernel, the vector-pipe kernel takes all 3 x 99 items."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    torch.manual_seed(33)
    net = EGNN_dynamics_AD2_cat(33, 3, hidden_nf=64, n_layers=2, condition_beta=True)
    gen = torch.Generator().manual_seed(34)
    B = 3
    x = O.remove_mean(torch.randn(B, 99, generator=gen), 33, 3)
    h = T([0.05, 0.7, 9.0])
    beta = T([1.0, 1.25, 0.8])
    hc, xc, bc = h.cuda(), x.cuda(), beta.cuda()
    trace, D = net.jacobian_trace(hc, xc, bc, want_denoiser=True)
    acc, den = direction_loop(net, hc, xc, bc, 99)
    assert torch.equal(trace, acc) and torch.equal(D, den)
    wd = {k: v.detach().double() for k, v in net.state_dict().items()}
    tr64, D64 = oracle_trace(wd, h, x, beta, 33, n_layers=2, tanh=True, attention=True)
    want = tr64.numpy()
    scale = float(np.abs(want).mean()) + 1.0
    print(f"[wide trace/33 atoms] max |trace - fp64| = {np.abs(trace.cpu().numpy() - want).max():.3e} "
          f"(mean |trace| {scale - 1.0:.3e}), denoiser rel {rel(D, D64):.3e}")
    np.testing.assert_allclose(trace.cpu().numpy(), want, rtol=5e-5, atol=5e-5 * scale)
    assert rel(D, D64) < 2e-6


def test_debiased_sde_runs_through_the_single_call(pa, cases, monkeypatch):
    """VEReverseSDE(debias_inference=True).f with the ad2cat backbone as score and energy net takes jacobian_trace for the
    divergence of the score; with the method hidden the n*d-launch fallback runs and gives the same bits in every field."""
    import copy

    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
    from pita_amd.energy_net import EnergyNet

    net = cases["h64"]["net"]
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    gen = torch.Generator().manual_seed(12)
    x = O.remove_mean(torch.randn(5, 66, generator=gen), 22, 3).cuda()
    calls = []
    real = EGNN_dynamics_AD2_cat.jacobian_trace

    def spy(self, *a, **kw):
        calls.append(self)
        return real(self, *a, **kw)

    monkeypatch.setattr(EGNN_dynamics_AD2_cat, "jacobian_trace", spy)
    f = lambda: sde.f(torch.tensor(0.15).cuda(), x, 1.25, gam, None, None, resampling_interval=1)
    one = f()
    assert calls == [net]  # the score net's backbone, once
    monkeypatch.delattr(EGNN_dynamics_AD2_cat, "jacobian_trace")
    assert not hasattr(net, "jacobian_trace")
    loop = f()
    assert len(calls) == 1
    for name in ("drift_X", "drift_A", "divergence_score", "cross_term", "dUt_dt"):
        assert torch.equal(getattr(one, name), getattr(loop, name)), name
