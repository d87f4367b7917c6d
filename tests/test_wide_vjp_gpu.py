"""Reverse-mode sweep of the EDM denoiser around the wide EGNN backbone on the matrix-pipe kernel egnn_wide64_vjp_kernel
(pita_egnn_wide_vjp) at 22, 33 and 42 atoms: one wave per walker at 22 atoms, two (one per 32-column tile, the second
ragged) at 33 and 42.  Run on an MI355X: pytest -m gpu.

Nets: at 22 atoms the two golden nets (egnn_ad2cat_h64_fwd.npz: hidden 64 x 5, attention + tanh; h48: hidden 48 x 2,
plain -- padded feature rows) and the h64 weights with attention=False, on six rows of the golden inputs; at 33 and 42
atoms seeded nets, hidden 64 x 5 with attention + tanh, 2 layers in the other three attention x tanh combinations and, at
33 atoms, hidden 48, with the coordinate-head rows scaled up (x200 with tanh, x20 without) so that the fresh head (gain
1e-3) does not hide errors, on 4 walkers at h = 0.05, 0.7, 3, 40.

Bounds: the error against the fp64 oracle (vmap(jacrev) of O.denoiser around O.egnn_ad2_cat_forward) is at most 4 x the
fp32 oracle's own on the same inputs, with the fixed bounds of test_egnn_ad2cat_reverse_mode_vs_oracle_jacobian as
floors.  The oracles are computed once per module and never modified; a batch of B walkers is rows ``arange(B) % R``."""
import os

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O

pytestmark = pytest.mark.gpu

T = torch.tensor
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the reverse-mode shape table of egnn_wide_mfma_vjp_kernel.hip (profiles/r09_wide_vjp.txt: every one of them beat the
# vector-pipe kernel beyond its spread)
MATRIX_PIPE_ATOMS = (22, 33, 42)
# tag: hidden, layers, attention, tanh
SEEDED_CFG = {"L5": (64, 5, True, True), "L2_a0t1": (64, 2, False, True), "L2_a1t0": (64, 2, True, False),
              "L2_a0t0": (64, 2, False, False), "h48": (48, 2, True, True)}
GOLDEN_CFG = {"L5": ("h64", 5, True, True), "h48": ("h48", 2, False, False), "L5_a0": ("h64", 5, False, True)}
NETS = [(22, tag) for tag in GOLDEN_CFG if 22 in MATRIX_PIPE_ATOMS] + \
       [(n, tag) for n in (33, 42) if n in MATRIX_PIPE_ATOMS for tag in SEEDED_CFG if tag != "h48" or n == 33]
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


def golden_net(tag):
    """(module, x, h, beta) of a 22-atom golden net on six rows of the golden inputs."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    name, L, att, tanh = GOLDEN_CFG[tag]
    g = dict(np.load(os.path.join(GOLDEN, f"egnn_ad2cat_{name}_fwd.npz")))
    w = {k[2:]: T(v) for k, v in g.items() if k.startswith("w.")}
    hidden = w["egnn.embedding.weight"].shape[0]
    if not att:  # the gate's parameters are absent from an attention=False module
        w = {k: v for k, v in w.items() if "att_mlp" not in k}
    net = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=hidden, n_layers=L, tanh=tanh, attention=att, condition_beta=True)
    net.load_state_dict(w)
    sel = np.arange(0, g["x"].shape[0], 2)[:6]
    return net, T(g["x"][sel]), T(g["h"][sel]), T(g["beta"][sel])


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
    """Per (n, net): the module, its oracle walkers and the fp64 / fp32 oracles on them -- computed once, never
    modified."""
    out = {}
    for n, tag in NETS:
        if n == 22:
            net, x, h, beta = golden_net(tag)
            _, L, att, tanh = GOLDEN_CFG[tag]
        else:
            gen = torch.Generator().manual_seed(n)
            h = T(H_VALUES)
            x = O.remove_mean(torch.randn(4, n * 3, generator=gen) * 1.5, n, 3) * (1.0 + h.sqrt())[:, None]
            beta = torch.rand(4, generator=gen) + 0.5
            hidden, L, att, tanh = SEEDED_CFG[tag]
            net = make_net(n, hidden, L, att, tanh)
        w = {k: v.detach().clone() for k, v in net.state_dict().items()}
        kw = dict(n_layers=L, tanh=tanh, attention=att)
        Jx64, Jh64, D64 = oracle_jacobian(w, h, x, beta, n, torch.float64, **kw)
        Jx32, Jh32, D32 = oracle_jacobian(w, h, x, beta, n, torch.float32, **kw)
        out[(n, tag)] = dict(net=net, n=n, x=x, h=h, beta=beta, w=w, kw=kw, Jx64=Jx64, Jh64=Jh64, D64=D64, Jx32=Jx32,
                             Jh32=Jh32, D32=D32)
    return out


def batch(c, B):
    rows = torch.arange(B) % c["x"].shape[0]
    return rows, c["h"][rows].cuda(), c["x"][rows].cuda(), c["beta"][rows].cuda()


@pytest.fixture(scope="module")
def cold(cases):
    """vjp(want_dot_h=True) of the 5-layer nets on their oracle walkers, shared by the tests below."""
    out = {}
    for n in MATRIX_PIPE_ATOMS:
        c = cases[(n, "L5")]
        _, h, x, beta = batch(c, c["x"].shape[0])
        out[n] = c["net"].vjp(h, x, beta, want_dot_h=True)
    return out


def test_reverse_mode_takes_the_matrix_pipe_for_the_peptides(pa, monkeypatch):
    """vjp_uses_matrix_pipe: the atoms of the reverse-mode shape table have an instantiation, 55 atoms (matrix-pipe
    forward only) does not; none under PITA_WIDE_NO_MFMA."""
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    nets = {n: EGNN_dynamics_AD2_cat(n, 3, hidden_nf=64, n_layers=2, condition_beta=True) for n in (22, 33, 42, 55)}
    for n, net in nets.items():
        assert net.uses_matrix_pipe("cuda:0"), n
        assert net.vjp_uses_matrix_pipe("cuda:0") == (n in MATRIX_PIPE_ATOMS), n
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        for n, net in nets.items():
            assert not net.vjp_uses_matrix_pipe("cuda:0"), n
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    assert nets[22].vjp_uses_matrix_pipe("cuda:0")
    from pita_amd import egnn_aldp

    assert egnn_aldp.EGNN_dynamics.vjp_uses_matrix_pipe is EGNN_dynamics_AD2_cat.vjp_uses_matrix_pipe


@pytest.mark.parametrize("n,tag", NETS)
def test_against_the_fp64_oracle(cases, n, tag):
    """cot = x and a dense seeded cotangent: vjp against cot^T J_x, dot_h against <cot, J_h>, D -- each at most 4 x the fp32
    oracle's own error, floors 5e-5 / 2e-4 (|want| + mean |want|) / 2e-6."""
    c = cases[(n, tag)]
    B = c["x"].shape[0]
    _, h, x, beta = batch(c, B)
    assert c["net"].vjp_uses_matrix_pipe("cuda:0")
    gen = torch.Generator().manual_seed(11 + n)
    for name, cot in (("x", None), ("dense", torch.randn(B, 3 * n, generator=gen))):
        c64 = (c["x"] if cot is None else cot).double()
        D, vj, dh = c["net"].vjp(h, x, beta, cot=None if cot is None else cot.cuda(), want_dot_h=True)
        want = torch.einsum("bq,bqk->bk", c64, c["Jx64"])
        e, e32 = rel(vj, want), rel(torch.einsum("bq,bqk->bk", c64, c["Jx32"]), want)
        rD, rD32 = rel(D, c["D64"]), rel(c["D32"], c["D64"])
        want_h = (c64 * c["Jh64"]).sum(-1)
        eh = (dh.cpu().double() - want_h).abs()
        eh32 = ((c64 * c["Jh32"]).sum(-1) - want_h).abs()
        bound_h = torch.maximum(4 * eh32, 2e-4 * (want_h.abs() + want_h.abs().mean()))
        print(f"[wide vjp/n={n}/{tag}/cot={name}] vjp rel {e:.3e} (fp32 oracle {e32:.3e}), denoiser rel {rD:.3e} (fp32 "
              f"oracle {rD32:.3e}), dot_h |err| {[f'{v:.3e}' for v in eh.tolist()]} (fp32 oracle "
              f"{[f'{v:.3e}' for v in eh32.tolist()]}, bound {[f'{v:.3e}' for v in bound_h.tolist()]})")
        assert e < max(4 * e32, 5e-5), (name, e, e32)
        assert rD < max(4 * rD32, 2e-6), (name, rD, rD32)
        assert bool((eh <= bound_h).all()), (name, eh, bound_h)


@pytest.mark.parametrize("n", [n for n in (22, 33) if n in MATRIX_PIPE_ATOMS])
def test_against_the_forward_mode_launches(cases, cold, n):
    """vjp(cot = x) against <x, dD> of the n*d single-direction forward-mode launches it replaces."""
    c = cases[(n, "L5")]
    B = c["x"].shape[0]
    _, h, x, beta = batch(c, B)
    jtx = torch.empty(B, 3 * n, device="cuda")
    for k in range(3 * n):
        c["net"].jvp(h, x, beta, direction=k, want_primal=False, want_tangent=False, dot_out=jtx, dot_col=k)
    e = rel(cold[n][1], jtx)
    print(f"[wide vjp/n={n}] reverse mode against {3 * n} forward-mode launches: rel {e:.3e}")
    assert e < 2e-5, e


@pytest.mark.parametrize("n", MATRIX_PIPE_ATOMS)
def test_variants_keep_the_bits(cases, cold, n):
    c = cases[(n, "L5")]
    B = c["x"].shape[0]
    _, h, x, beta = batch(c, B)
    D, vj, dh = cold[n]
    assert torch.isfinite(D).all() and torch.isfinite(vj).all() and torch.isfinite(dh).all()
    none, vj2 = c["net"].vjp(h, x, beta, want_primal=False)  # no denoiser, no dot_h
    assert none is None and torch.equal(vj2, vj)
    D3, vj3 = c["net"].vjp(h, x, beta)  # no dot_h
    assert torch.equal(vj3, vj) and torch.equal(D3, D)
    _, vj4, dh4 = c["net"].vjp(h, x, beta, want_primal=False, want_dot_h=True)
    assert torch.equal(vj4, vj) and torch.equal(dh4, dh)
    e = c["net"].vjp(h[:0], x[:0], beta[:0], want_dot_h=True)  # the empty batch
    assert e[0].shape == (0, 3 * n) and e[1].shape == (0, 3 * n) and e[2].shape == (0,)


@pytest.mark.parametrize("n", MATRIX_PIPE_ATOMS)
def test_batch_position_and_wrap(cases, cold, n):
    """One launch holds one item per ceil(n / 32) waves of a 4-wave block per CU resident: 4 x 256 = 1 024 walkers at 22
    atoms, 2 x 256 = 512 at 33 and 42 on an MI355X.  The oracle walkers tiled to the first multiple of their count above
    that plus one more copy (1 032 / 520): the block loop wraps, the first and the last copy have the bits of the small
    batch, and so has a rerun."""
    c = cases[(n, "L5")]
    R = c["x"].shape[0]
    resident = torch.cuda.get_device_properties(0).multi_processor_count * (4 // ((n + 31) // 32))
    B = R * (resident // R + 2)
    assert B > resident
    _, h, x, beta = batch(c, B)
    D, vj, dh = c["net"].vjp(h, x, beta, want_dot_h=True)
    for got, small in zip((D, vj, dh), cold[n]):
        assert torch.equal(got[:R], small) and torch.equal(got[-R:], small)
    again = c["net"].vjp(h, x, beta, want_dot_h=True)
    for got, first in zip(again, (D, vj, dh)):
        assert torch.equal(got, first)


@pytest.mark.parametrize("n", MATRIX_PIPE_ATOMS)
def test_out_of_range_walkers_are_repaired_by_the_vector_pipe(cases, cold, n, monkeypatch):
    """beta[1] = 1e7 drives walker 1's activations out of the f16 range: its whole result comes from the fp32 vector-pipe
    kernel (bit for bit the run under PITA_WIDE_NO_MFMA), every other walker keeps the matrix-pipe kernel's bits."""
    c = cases[(n, "L5")]
    net = c["net"]
    B = 6 if n == 22 else 3
    _, h, x, beta = batch(c, B)
    assert net.vjp_uses_matrix_pipe("cuda:0")
    hot = beta.clone()
    hot[1] = 1.0e7
    got = net.vjp(h, x, hot, want_dot_h=True)
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        assert not net.vjp_uses_matrix_pipe("cuda:0")
        vec = net.vjp(h, x, hot, want_dot_h=True)
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    keep = torch.arange(B) != 1
    for g, v, cld in zip(got, vec, cold[n]):
        assert torch.equal(g[1].view(torch.int32), v[1].view(torch.int32))
        assert torch.equal(g[keep], cld[:B][keep])


def test_through_the_plug_in_classes_33_atoms(pa, cases):
    """EnergyNet(net)(h, x, beta) = grad_x E_theta against autograd of the fp64 oracle's E_theta (4 x the fp32 oracle's own
    error, floor 5e-5), and every field of VEReverseSDE(debias_inference=True).f finite."""
    import copy

    from pita_amd.energy_net import EnergyNet

    n = 33 if 33 in MATRIX_PIPE_ATOMS else 22
    c = cases[(n, "L5")]
    net = c["net"]
    assert net.vjp_uses_matrix_pipe("cuda:0")
    _, h, x, beta = batch(c, c["x"].shape[0])

    def grad_ref(dtype):
        wd = {k: v.to(dtype) for k, v in c["w"].items()}
        bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, n, 3, **c["kw"])
        xr = c["x"].to(dtype).requires_grad_(True)
        return torch.autograd.grad(O.energy_theta(bb, c["h"].to(dtype), xr, c["beta"].to(dtype)).sum(), xr)[0].double()

    g64, g32 = grad_ref(torch.float64), grad_ref(torch.float32)
    e, e32 = rel(EnergyNet(net)(h, x, beta), g64), rel(g32, g64)
    print(f"[wide vjp/n={n}] grad_x E_theta rel {e:.3e} (fp32 oracle {e32:.3e})")
    assert e < max(4 * e32, 5e-5), (e, e32)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    xs = O.remove_mean(torch.randn(4, 3 * n, generator=torch.Generator().manual_seed(12)), n, 3).cuda()
    terms = sde.f(torch.tensor(0.15).cuda(), xs, 1.25, gam, None, None, resampling_interval=1)
    for name in terms._FIELDS:
        v = getattr(terms, name)
        assert v is None or torch.isfinite(v).all(), name
    for name in ("drift_X", "drift_A", "divergence_score", "cross_term", "dUt_dt"):
        assert getattr(terms, name) is not None, name
