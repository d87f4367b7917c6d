"""dot_parts of the wide EGNN reverse sweep (pita_egnn_wide_vjp_parts; EGNN_dynamics_AD2_cat.vjp(want_h_parts=True)): the
split (s1 = c_out <cot, F>, s2 = <cot, d(c_out F)/dh>) of <cot, dD/dh> that pita_fk_assemble builds E_theta and
dE_theta/dh from without the 1/h^2 cancellation.  Run on an MI355X: pytest -m gpu.

Nets and walkers: those of tests/test_wide_vjp_gpu.py (imported, with the seeds of its ``cases`` fixture): the golden
22-atom nets L5, h48 and L5_a0, the seeded 33- and 42-atom nets -- one wave per item, two waves per item with a ragged
second tile, padded feature rows, the layers that skip the feature adjoint.  Beside them two nets that no reverse
matrix-pipe row serves (13 atoms, hidden 64 x 2; 7 atoms, hidden 48 x 2).

References: s1 from the fp64 oracle's backbone output, s2 its autograd through h (the construction of
test_hip_parity.py::test_vjp_vs_oracle), dot_h = autograd of <cot, D> through h; the fp32 oracle is the same computation
in float32.  Computed once per module, never modified.  Bound per walker on a piece (and on dot_h, as
test_wide_vjp_gpu.py::test_against_the_fp64_oracle has it): max(4 x the fp32 oracle's own error,
2e-4 (|want| + mean |want|))."""
import copy

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
import test_wide_vjp_gpu as V

pytestmark = pytest.mark.gpu

T = torch.tensor
VECTOR_ONLY = {(13, "v64"): (64, 2, True, True), (7, "v48"): (48, 2, True, True)}  # hidden, layers, attention, tanh


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def pieces_ref(w, kw, n, h, x, beta, cots, dtype):
    """Per cotangent (s1, s2, dot_h) of the oracle in ``dtype``, returned in fp64: one backbone evaluation, s2 by autograd
    of s1 through h, dot_h = d/dh <cot, c_s x + c_out F> as autograd adds it up: s2 plus the c_s path's share."""
    wd = {k: v.to(dtype) for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, n, 3, **kw)
    xd, bd = x.to(dtype), beta.to(dtype)
    hd = h.detach().to(dtype).clone().requires_grad_(True)
    c_s, c_in, c_out, c_noise = O.edm_coeffs(hd)
    F = bb(c_noise, c_in[:, None] * xd, bd)
    out = []
    for cot in cots:
        cc = cot.to(dtype)
        s1 = c_out * (F * cc).sum(1)
        (s2,) = torch.autograd.grad(s1.sum(), hd, retain_graph=True)
        (ds,) = torch.autograd.grad((c_s * (xd * cc).sum(1)).sum(), hd, retain_graph=True)
        out.append((s1.detach().double(), s2.double(), (s2 + ds).double()))
    return out


def seeded_inputs(n):
    gen = torch.Generator().manual_seed(n)  # as the ``cases`` fixture of test_wide_vjp_gpu.py
    h = T(V.H_VALUES)
    x = O.remove_mean(torch.randn(4, n * 3, generator=gen) * 1.5, n, 3) * (1.0 + h.sqrt())[:, None]
    beta = torch.rand(4, generator=gen) + 0.5
    return x, h, beta


@pytest.fixture(scope="module")
def cases(pa):
    out = {}
    for n, tag in list(V.NETS) + list(VECTOR_ONLY):
        kw = {}
        if (n, tag) in VECTOR_ONLY:
            from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

            hidden, L, att, tanh = VECTOR_ONLY[(n, tag)]
            x, h, beta = seeded_inputs(n)
            torch.manual_seed(100 + n)
            h0 = torch.zeros(n, 1)
            net = EGNN_dynamics_AD2_cat(n, 3, hidden_nf=hidden, n_layers=L, tanh=tanh, attention=att, condition_beta=True,
                                        h_initial=h0)
            with torch.no_grad():
                for prm in net.parameters():  # trained-like coordinate head, as make_net of test_wide_vjp_gpu.py
                    if prm.dim() == 2 and prm.shape[0] == 1 and prm.shape[1] == hidden:
                        prm.mul_(200.0)
            kw["h_initial"] = h0
        elif n == 22:
            net, x, h, beta = V.golden_net(tag)
            _, L, att, tanh = V.GOLDEN_CFG[tag]
        else:
            x, h, beta = seeded_inputs(n)
            hidden, L, att, tanh = V.SEEDED_CFG[tag]
            net = V.make_net(n, hidden, L, att, tanh)
        w = {k: v.detach().clone() for k, v in net.state_dict().items()}
        kw.update(n_layers=L, tanh=tanh, attention=att)
        B = x.shape[0]
        dense = torch.randn(B, 3 * n, generator=torch.Generator().manual_seed(11 + n))
        r64 = pieces_ref(w, kw, n, h, x, beta, (x, dense), torch.float64)
        r32 = pieces_ref(w, kw, n, h, x, beta, (x, dense), torch.float32)
        refs = {name: dict(cot=cot, r64=r64[i], r32=r32[i]) for i, (name, cot) in enumerate((("x", x), ("dense", dense)))}
        out[(n, tag)] = dict(net=net, n=n, x=x, h=h, beta=beta, w=w, kw=kw, refs=refs)
    return out


def check_pieces(c, label):
    """test 1 of the module docstring on one net, both cotangents; the net runs on whatever pipe the environment gives."""
    n, net = c["n"], c["net"]
    _, h, x, beta = V.batch(c, c["x"].shape[0])
    for name in ("x", "dense"):
        r = c["refs"][name]
        cot = None if name == "x" else r["cot"].cuda()
        D, vj, dh, parts = net.vjp(h, x, beta, cot=cot, want_dot_h=True, want_h_parts=True)
        assert parts.shape == (x.shape[0], 2) and torch.isfinite(parts).all() and torch.isfinite(dh).all()
        got = (parts[:, 0].cpu().double(), parts[:, 1].cpu().double(), dh.cpu().double())
        for piece, g, w64, w32 in zip(("s1", "s2", "dot_h"), got, r["r64"], r["r32"]):
            err, e32 = (g - w64).abs(), (w32 - w64).abs()
            bound = torch.maximum(4 * e32, 2e-4 * (w64.abs() + w64.abs().mean()))
            print(f"[wide parts/{label}/n={n}/cot={name}] {piece} |err| {[f'{v:.3e}' for v in err.tolist()]} (fp32 oracle "
                  f"{[f'{v:.3e}' for v in e32.tolist()]}, bound {[f'{v:.3e}' for v in bound.tolist()]}, |want| "
                  f"{[f'{v:.3e}' for v in w64.abs().tolist()]})")
            assert bool((err <= bound).all()), (label, name, piece, err, bound)
        # with the closed-form c_s'(h) <cot, x> share the second piece is dot_h again
        whole = got[1] - (c["x"].double() * r["cot"].double()).sum(1) / (1 + c["h"].double()) ** 2
        np.testing.assert_allclose(dh.cpu().numpy(), whole.numpy(), rtol=1e-5, atol=1e-5 * float(whole.abs().mean()),
                                   err_msg=f"{label} {n} {name}")


@pytest.mark.parametrize("n,tag", V.NETS)
def test_pieces_against_the_fp64_oracle(cases, n, tag):
    c = cases[(n, tag)]
    assert c["net"].vjp_uses_matrix_pipe("cuda:0")
    check_pieces(c, f"matrix/{tag}")


@pytest.fixture(scope="module")
def cold(cases):
    """(plain, with parts) of the 5-layer nets on their oracle walkers, shared by the tests below."""
    out = {}
    for n in V.MATRIX_PIPE_ATOMS:
        c = cases[(n, "L5")]
        _, h, x, beta = V.batch(c, c["x"].shape[0])
        out[n] = (c["net"].vjp(h, x, beta, want_dot_h=True), c["net"].vjp(h, x, beta, want_dot_h=True, want_h_parts=True))
    return out


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("n", V.MATRIX_PIPE_ATOMS)
def test_parts_leave_the_other_outputs_their_bits(cases, cold, n):
    c = cases[(n, "L5")]
    _, h, x, beta = V.batch(c, c["x"].shape[0])
    (D0, vj0, dh0), (D, vj, dh, parts) = cold[n]
    assert bits(D, D0) and bits(vj, vj0)
    # dot_h = fl(parts[1] + the kernel's own c_s'(h) <cot, x>): the plain call's up to rounding
    np.testing.assert_allclose(dh.cpu().numpy(), dh0.cpu().numpy(), rtol=1e-5, atol=1e-5 * float(dh0.abs().mean()))
    again = c["net"].vjp(h, x, beta, want_dot_h=True, want_h_parts=True)
    for a, b in zip(again, (D, vj, dh, parts)):
        assert bits(a, b)
    none, vj2, dh2, parts2 = c["net"].vjp(h, x, beta, want_primal=False, want_dot_h=True, want_h_parts=True)
    assert none is None and bits(vj2, vj) and bits(dh2, dh) and bits(parts2, parts)
    e = c["net"].vjp(h[:0], x[:0], beta[:0], want_dot_h=True, want_h_parts=True)  # the empty batch
    assert [tuple(v.shape) for v in e] == [(0, 3 * n), (0, 3 * n), (0,), (0, 2)]
    for B in ((6, 7) if n == 22 else (3,)):  # empty item slots in the last block
        rows, hb, xb, bb = V.batch(c, B)
        got = c["net"].vjp(hb, xb, bb, want_dot_h=True, want_h_parts=True)
        for g, small in zip(got, (D, vj, dh, parts)):
            assert bits(g, small[rows.cuda()]), (n, B)


@pytest.mark.parametrize("n", V.MATRIX_PIPE_ATOMS)
def test_batch_position_and_wrap_with_parts(cases, cold, n):
    """The wrap case of test_wide_vjp_gpu.py::test_batch_position_and_wrap: the oracle walkers tiled to the first multiple
    of their count above the resident item count plus one more copy; first and last copy have the small batch's bits."""
    c = cases[(n, "L5")]
    R = c["x"].shape[0]
    resident = torch.cuda.get_device_properties(0).multi_processor_count * (4 // ((n + 31) // 32))
    B = R * (resident // R + 2)
    assert B > resident
    _, h, x, beta = V.batch(c, B)
    got = c["net"].vjp(h, x, beta, want_dot_h=True, want_h_parts=True)
    for g, small in zip(got, cold[n][1]):
        assert bits(g[:R], small) and bits(g[-R:], small)


def test_vector_pipe_alone_at_22_atoms(cases, monkeypatch):
    c = cases[(22, "L5")]
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        assert not c["net"].vjp_uses_matrix_pipe("cuda:0")
        check_pieces(c, "vector/L5")
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")


@pytest.mark.parametrize("n,tag", list(VECTOR_ONLY))
def test_shapes_without_a_matrix_pipe_row(cases, n, tag):
    c = cases[(n, tag)]
    assert not c["net"].vjp_uses_matrix_pipe("cuda:0")
    check_pieces(c, f"vector/{tag}")
    _, h, x, beta = V.batch(c, 4)
    plain = c["net"].vjp(h, x, beta, want_dot_h=True)
    withp = c["net"].vjp(h, x, beta, want_dot_h=True, want_h_parts=True)
    assert bits(plain[0], withp[0]) and bits(plain[1], withp[1])


@pytest.mark.parametrize("n", [n for n in (22, 33) if n in V.MATRIX_PIPE_ATOMS])
def test_marked_walker_gets_its_parts_from_the_vector_pipe(cases, cold, n, monkeypatch):
    """beta[1] = 1e7 drives walker 1 out of the f16 range: out, vjp, dot_h and parts of it are the vector-pipe kernel's
    (the run under PITA_WIDE_NO_MFMA) bit for bit; every other walker keeps the matrix-pipe bits."""
    c = cases[(n, "L5")]
    net = c["net"]
    B = 6 if n == 22 else 3
    _, h, x, beta = V.batch(c, B)
    assert net.vjp_uses_matrix_pipe("cuda:0")
    hot = beta.clone()
    hot[1] = 1.0e7
    got = net.vjp(h, x, hot, want_dot_h=True, want_h_parts=True)
    monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
    try:
        assert not net.vjp_uses_matrix_pipe("cuda:0")
        vec = net.vjp(h, x, hot, want_dot_h=True, want_h_parts=True)
    finally:
        monkeypatch.delenv("PITA_WIDE_NO_MFMA")
    keep = torch.arange(B) != 1
    for g, v, cld in zip(got, vec, cold[n][1]):
        assert bits(g[1], v[1])
        assert bits(g[keep], cld[:B][keep])


# ---------------------------------------------------------------------------------------------------------------------
# What the split buys: dUt_dt = dE_theta/dh dh/dt of VEReverseSDE(debias_inference=True).f, no pinning
FK_TIMES = (0.1, 0.15, 0.3)
FK_NETS = ((22, 1.0), (33, 1.5))  # atoms, scale of the walkers


def fk_reference(c, n, sched, t, x, beta, dtype):
    """d/dt E_theta(h(t), x) per walker by autograd in ``dtype`` (fp64 returned)."""
    wd = {k: v.to(dtype) for k, v in c["w"].items()}
    bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, n, 3, **c["kw"])
    tt = torch.full((x.shape[0],), t, dtype=dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(O.energy_theta(bb, sched.h(tt), x.to(dtype), beta).sum(), tt)
    return g.double()


@pytest.fixture(scope="module")
def fk_cases(cases):
    """Per (atoms, t): the walkers (generator seed 12, 6 of them, beta = 1.25) and the fp64 and fp32 oracles' dUt_dt."""
    osched = O.Elucidating(0.01, 80.0, 7)
    out = {}
    for n, s in FK_NETS:
        c = cases[(n, "L5")]
        z = O.remove_mean(torch.randn(6, 3 * n, generator=torch.Generator().manual_seed(12)) * s, n, 3)
        for t in FK_TIMES:
            x = z * (1.0 + float(osched.h(T(t, dtype=torch.float64)).sqrt()))
            r64 = fk_reference(c, n, osched, t, x, 1.25, torch.float64)
            r32 = fk_reference(c, n, osched, t, x, 1.25, torch.float32)
            out[(n, t)] = dict(x=x, r64=r64, e32=float((r32 - r64).abs().mean()))
    return out


@pytest.mark.parametrize("n", [n for n, _ in FK_NETS])
def test_what_the_split_buys_in_dUt_dt(pa, cases, fk_cases, n, monkeypatch):
    """Mean |error| of dUt_dt against the fp64 oracle at t = 0.1, 0.15, 0.3, as shipped (assembled from the split) and with
    ``vjp_h_parts`` switched off on the class (the form this backbone had), beside the fp32 oracle's own.
    (a) t = 0.1, 0.15: with the split <= without it.  (b) every t: with the split <= 4 x the fp32 oracle's mean error.
    Measured on an MI355X (profiles/r11_wide_dot_parts.txt): split 0.5 - 1.4 x the fp32 oracle, the old form 7.6 x (22 atoms)
    and 4.7 x (33 atoms) at t = 0.1."""
    from pita_amd.energy_net import EnergyNet

    c = cases[(n, "L5")]
    net = c["net"]
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=True)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    res = {}
    for t in FK_TIMES:
        f = fk_cases[(n, t)]
        xs = f["x"].cuda()
        assert type(net).vjp_h_parts is True
        split = sde.f(torch.tensor(t).cuda(), xs, 1.25, gam, None, None, resampling_interval=1).dUt_dt.cpu().double()
        with monkeypatch.context() as m:
            m.setattr(type(net), "vjp_h_parts", False)
            old = sde.f(torch.tensor(t).cuda(), xs, 1.25, gam, None, None, resampling_interval=1).dUt_dt.cpu().double()
        e_split, e_old = float((split - f["r64"]).abs().mean()), float((old - f["r64"]).abs().mean())
        res[t] = (e_split, e_old)
        print(f"[wide parts/dUt_dt/n={n}/t={t}] mean |dUt_dt| {float(f['r64'].abs().mean()):.3e}: split {e_split:.3e}, old "
              f"form {e_old:.3e}, fp32 oracle {f['e32']:.3e} (split / fp32 oracle {e_split / f['e32']:.2f})")
    for t in (0.1, 0.15):
        assert res[t][0] <= res[t][1], (n, t, res[t])
    for t in FK_TIMES:
        assert res[t][0] <= 4 * fk_cases[(n, t)]["e32"], (n, t, res[t], fk_cases[(n, t)]["e32"])
