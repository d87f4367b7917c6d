"""Forward-mode derivative of the EDM denoiser around the wide EGNN backbone at 33 and 42 atoms (tri-alanine,
ACE-(ALA)3-NME) on the matrix-pipe kernel egnn_wide64_jvp_kernel: two waves per (walker, direction) item, one per
32-column tile, the second tile ragged (1 valid column at 33 atoms, 10 at 42).  Run on an MI355X: pytest -m gpu.

Nets per particle count: hidden 64 x 5 layers with attention + tanh (the reference configuration), 2 layers in each of
the other three attention x tanh combinations and, at 33 atoms, a hidden-48 net (padded feature rows).  Seeded weights
with the coordinate-head rows scaled up (x200 with tanh, x20 without, as test_egnn_ad2cat_other_particle_counts does) so
that the freshly initialised head (gain 1e-3) does not hide errors.

Bounds: the project's standing rule -- the error against the fp64 oracle is at most 4 x the fp32 oracle's own on the same
inputs -- with the fixed bounds of test_wide_trace_gpu.py / test_egnn_aldp_golden kept as floors (at 5 layers and 99 / 126
directions the fp32 oracle's own trace error is 1e-4 .. 1e-3 on traces of 30 .. 60, beyond the 22-atom tests' 5e-5).  The
oracles (vmap(jacrev) of O.denoiser around O.egnn_ad2_cat_forward, fp64 and fp32) are computed once per module on 4
walkers; a batch of B walkers is rows ``arange(B) % 4``."""
import numpy as np
import pytest
import torch

from oracle import pita_oracle as O

pytestmark = pytest.mark.gpu

T = torch.tensor
SIZES = (33, 42)
# tag: hidden, layers, attention, tanh
NET_CFG = {"L5": (64, 5, True, True), "L2_a0t1": (64, 2, False, True), "L2_a1t0": (64, 2, True, False),
           "L2_a0t0": (64, 2, False, False), "h48": (48, 2, True, True)}
NETS = [(n, tag) for n in SIZES for tag in NET_CFG if tag != "h48" or n == 33]
H_VALUES = (0.05, 0.7, 3.0, 40.0)


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


def make_net(n, hidden, L, att, tanh):
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    torch.manual_seed(100 + n)
    net = EGNN_dynamics_AD2_cat(n, 3, hidden_nf=hidden, n_layers=L, tanh=tanh, attention=att, condition_beta=True)
    with torch.no_grad():
        for prm in net.parameters():  # trained-like magnitudes: the fresh coordinate head (gain 1e-3) hides errors
            if prm.dim() == 2 and prm.shape[0] == 1 and prm.shape[1] == hidden:
                prm.mul_(200.0 if tanh else 20.0)
    return net


def direction_loop(net, h, x, beta, D):
    """The launches the single call replaces, as VEReverseSDE._denoiser_jacobian_terms issues them for the trace."""
    acc = torch.zeros(x.shape[0], device="cuda")
    den = None
    for k in range(D):
        out, _ = net.jvp(h, x, beta, direction=k, want_primal=(k == 0), want_tangent=False, diag_acc=acc)
        den = out if k == 0 else den
    return acc, den


def oracle_jacobian(w, h, x, beta, n, dtype, **kw):
    """(J_x D [B, nd, nd], dD/dh [B, nd], D [B, nd]) of the oracle in ``dtype``: vmap(jacrev) of O.denoiser around
    O.egnn_ad2_cat_forward (utils.py:30-51), returned in fp64."""
    from torch.func import jacrev, vmap

    wd = {k: v.to(dtype) for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, n, 3, **kw)
    one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
    hd, xd, bd = h.to(dtype), x.to(dtype), beta.to(dtype)
    Jh, Jx = vmap(jacrev(one, argnums=(0, 1)))(hd, xd, bd)
    return Jx.double(), Jh.double(), O.denoiser(bb, hd, xd, bd).double()


@pytest.fixture(scope="module")
def cases(pa):
    """Per (n, net): the module, 4 walkers (one per noise level) and the fp64 / fp32 oracles on them -- computed once,
    never modified."""
    out = {}
    for n in SIZES:
        gen = torch.Generator().manual_seed(n)
        h = T(H_VALUES)
        x = O.remove_mean(torch.randn(4, n * 3, generator=gen) * 1.5, n, 3) * (1.0 + h.sqrt())[:, None]
        beta = torch.rand(4, generator=gen) + 0.5
        for tag, (hidden, L, att, tanh) in NET_CFG.items():
            if (n, tag) not in NETS:
                continue
            net = make_net(n, hidden, L, att, tanh)
            w = {k: v.detach().clone() for k, v in net.state_dict().items()}
            kw = dict(n_layers=L, tanh=tanh, attention=att)
            Jx64, Jh64, D64 = oracle_jacobian(w, h, x, beta, n, torch.float64, **kw)
            Jx32, Jh32, D32 = oracle_jacobian(w, h, x, beta, n, torch.float32, **kw)
            out[(n, tag)] = dict(net=net, n=n, x=x, h=h, beta=beta, Jx64=Jx64, Jh64=Jh64, D64=D64, Jx32=Jx32, Jh32=Jh32,
                                 D32=D32, trace64=Jx64.diagonal(dim1=1, dim2=2).sum(-1),
                                 trace32=Jx32.diagonal(dim1=1, dim2=2).sum(-1))
    return out


def batch(c, B):
    rows = torch.arange(B) % c["x"].shape[0]
    return rows, c["h"][rows].cuda(), c["x"][rows].cuda(), c["beta"][rows].cuda()


def test_forward_mode_takes_the_matrix_pipe_for_the_peptides(pa, monkeypatch):
    """jvp_uses_matrix_pipe: 22, 33 and 42 atoms have a forward-mode instantiation, 55 atoms (matrix-pipe forward only)
    does not; none under PITA_WIDE_NO_MFMA."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    nets = {n: EGNN_dynamics_AD2_cat(n, 3, hidden_nf=64, n_layers=2, condition_beta=True) for n in (22, 33, 42, 55)}
    for n, net in nets.items():
        assert net.uses_matrix_pipe("cuda:0"), n
        assert net.jvp_uses_matrix_pipe("cuda:0") == (n != 55), n
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        for n, net in nets.items():
            assert not net.jvp_uses_matrix_pipe("cuda:0"), n
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    assert nets[33].jvp_uses_matrix_pipe("cuda:0")
    from pita_amd import egnn_aldp

    assert egnn_aldp.EGNN_dynamics.jvp_uses_matrix_pipe is EGNN_dynamics_AD2_cat.jvp_uses_matrix_pipe


@pytest.fixture(scope="module")
def traces(cases):
    """jacobian_trace(want_denoiser=True) of the 5-layer nets at B = 3 and 11, shared by the tests below."""
    out = {}
    for n in SIZES:
        c = cases[(n, "L5")]
        for B in (3, 11):
            _, h, x, beta = batch(c, B)
            out[(n, B)] = c["net"].jacobian_trace(h, x, beta, want_denoiser=True)
    return out


@pytest.mark.parametrize("B", (1, 3, 11))
@pytest.mark.parametrize("n", SIZES)
def test_single_call_has_the_bits_of_the_direction_loop(cases, traces, n, B):
    """11 walkers are 1 089 / 1 386 items, more than one launch holds resident: the grid-stride loop wraps."""
    c = cases[(n, "L5")]
    net = c["net"]
    _, h, x, beta = batch(c, B)
    assert net.jvp_uses_matrix_pipe("cuda:0")
    trace, D = traces[(n, B)] if (n, B) in traces else net.jacobian_trace(h, x, beta, want_denoiser=True)
    acc, den = direction_loop(net, h, x, beta, 3 * n)
    assert trace.shape == (B,) and D.shape == (B, 3 * n)
    assert torch.isfinite(trace).all() and torch.isfinite(D).all()
    assert torch.equal(trace, acc), (trace - acc).abs().max()
    assert torch.equal(D, den)
    t2, none = net.jacobian_trace(h, x, beta)  # the trace alone: same bits, no denoiser
    assert none is None and torch.equal(t2, trace)


@pytest.mark.parametrize("n", SIZES)
def test_empty_batch_and_batch_position(cases, traces, n):
    c = cases[(n, "L5")]
    _, h, x, beta = batch(c, 0)
    trace, D = c["net"].jacobian_trace(h, x, beta, want_denoiser=True)
    assert trace.shape == (0,) and D.shape == (0, 3 * n)
    assert c["net"].jvp(h, x, beta, direction=3)[1].shape == (0, 3 * n)
    (t11, D11), (t3, D3) = traces[(n, 11)], traces[(n, 3)]
    assert torch.equal(t11[:3], t3) and torch.equal(D11[:3], D3)  # an item's bits do not depend on its place in the grid


@pytest.mark.parametrize("n,tag", NETS)
def test_against_the_fp64_oracle(cases, n, tag):
    c = cases[(n, tag)]
    _, h, x, beta = batch(c, 4)
    assert c["net"].jvp_uses_matrix_pipe("cuda:0")
    trace, D = c["net"].jacobian_trace(h, x, beta, want_denoiser=True)
    want = c["trace64"].numpy()
    mean_abs = float(np.abs(want).mean())
    err = float(np.abs(trace.cpu().numpy().astype(np.float64) - want).max())
    err32 = float(np.abs(c["trace32"].numpy() - want).max())
    rD, rD32 = rel(D, c["D64"]), rel(c["D32"], c["D64"])
    print(f"[wide peptides/n={n}/{tag}] max |trace - fp64| = {err:.3e} (fp32 oracle {err32:.3e}, mean |trace| "
          f"{mean_abs:.3e}), denoiser rel {rD:.3e} (fp32 oracle {rD32:.3e})")
    assert mean_abs > 1.0  # the absolute term below is not vacuous
    assert err <= max(4 * err32, 5e-5 * (mean_abs + 1.0)), (err, err32, mean_abs)
    assert rD < max(4 * rD32, 2e-6), (rD, rD32)


@pytest.mark.parametrize("n", SIZES)
def test_general_direction(cases, n):
    """dD = J_x D . vx + dD/dh . vh for a dense vx and vh = 1 in one launch, and the in-kernel reduction <x, dD>:
    dot_out against <x, dD> of the returned tangent (summed in fp64), 1e-5 relative to that inner product itself; the
    error relative to sum |x_i dD_i| (what a cancelling sum is measured by) is printed beside it."""
    c = cases[(n, "L5")]
    _, h, x, beta = batch(c, 4)
    gen = torch.Generator().manual_seed(9 + n)
    vx, vh = torch.randn(4, 3 * n, generator=gen), torch.ones(4)
    dot = torch.empty(4, device="cuda")
    _, dout = c["net"].jvp(h, x, beta, vx=vx.cuda(), vh=vh.cuda(), want_primal=False, dot_out=dot)
    want = torch.einsum("bqk,bk->bq", c["Jx64"], vx.double()) + c["Jh64"] * vh.double()[:, None]
    ref32 = torch.einsum("bqk,bk->bq", c["Jx32"], vx.double()) + c["Jh32"] * vh.double()[:, None]
    err, err32 = rel(dout, want), rel(ref32, want)
    terms = c["x"].double() * dout.cpu().double()
    dot_abs = (dot.cpu().double() - terms.sum(-1)).abs()
    dot_err, dot_err_mag = dot_abs / terms.sum(-1).abs(), dot_abs / terms.abs().sum(-1)
    print(f"[wide peptides/n={n}] dense direction rel {err:.3e} (fp32 oracle {err32:.3e}), <x, dD> per walker: rel "
          f"{[f'{v:.3e}' for v in dot_err.tolist()]} (rel to sum |terms| {[f'{v:.3e}' for v in dot_err_mag.tolist()]}, "
          f"sum |terms| / |sum| {[f'{v:.1f}' for v in (terms.abs().sum(-1) / terms.sum(-1).abs()).tolist()]})")
    assert err < max(4 * err32, 5e-5), (err, err32)
    assert float(dot_err.max()) <= 1e-5, dot_err


@pytest.mark.parametrize("n", SIZES)
def test_out_of_range_items_are_repaired_by_the_vector_pipe(cases, traces, n, monkeypatch):
    """beta[1] = 1e7 drives walker 1's activations out of the f16 range: its items come from the fp32 vector-pipe kernel
    (bit for bit the trace under PITA_WIDE_NO_MFMA), every other walker keeps the matrix-pipe kernel's bits."""
    c = cases[(n, "L5")]
    net = c["net"]
    B = 3
    _, h, x, beta = batch(c, B)
    assert net.jvp_uses_matrix_pipe("cuda:0")
    trace, D = traces[(n, B)]
    hot = beta.clone()
    hot[1] = 1.0e7
    trace_hot, D_hot = net.jacobian_trace(h, x, hot, want_denoiser=True)
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        assert not net.jvp_uses_matrix_pipe("cuda:0")
        trace_vec, D_vec = net.jacobian_trace(h, x, hot, want_denoiser=True)
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    assert torch.equal(trace_hot[1].view(torch.int32), trace_vec[1].view(torch.int32))
    assert torch.equal(D_hot[1].view(torch.int32), D_vec[1].view(torch.int32))
    keep = torch.arange(B) != 1
    assert torch.equal(trace_hot[keep], trace[keep])
    assert torch.equal(D_hot[keep], D[keep])


def test_debiased_sde_runs_through_the_single_call_33_atoms(pa, cases, monkeypatch):
    """VEReverseSDE(debias_inference=True).f at 33 atoms takes jacobian_trace once for the divergence of the score; with
    the method hidden the n*d-launch fallback runs and gives the same bits in every field."""
    import copy

    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
    from pita_amd.energy_net import EnergyNet

    net = cases[(33, "L2_a1t0")]["net"]
    assert net.jvp_uses_matrix_pipe("cuda:0")
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    gen = torch.Generator().manual_seed(12)
    x = O.remove_mean(torch.randn(4, 99, generator=gen), 33, 3).cuda()
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
        assert torch.isfinite(getattr(one, name)).all(), name
        assert torch.equal(getattr(one, name), getattr(loop, name)), name
