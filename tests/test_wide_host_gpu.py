"""Host side of the wide EGNN backbone (pita_egnn_wide_*): which kernels serve a handle, the handle's scratch buffers
across entry points, batches and streams, and the state_dict walk behind pita_egnn_wide_num_weights / _create.  Run on an
MI355X: pytest -m gpu.  Nets: hidden 64 x 2 layers, seeded as make_net of tests/test_wide_vjp_gpu.py, unless noted."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PITA_EINVAL = -1  # include/pita_hip.h


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def make_net(n, hidden=64, L=2, att=True, tanh=True, beta=True):
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    torch.manual_seed(100 + n)
    kw = dict(h_initial=torch.zeros(n, 1)) if n == 10 else {}  # 10 atoms: no topology the module knows
    net = EGNN_dynamics_AD2_cat(n, 3, hidden_nf=hidden, n_layers=L, tanh=tanh, attention=att, condition_beta=beta, **kw)
    with torch.no_grad():
        for prm in net.parameters():  # trained-like magnitudes: the fresh coordinate head (gain 1e-3) hides errors
            if prm.dim() == 2 and prm.shape[0] == 1 and prm.shape[1] == hidden:
                prm.mul_(200.0 if tanh else 20.0)
    return net


# (forward, forward mode, reverse mode) on the matrix pipe per (atoms, layers), PITA_WIDE_NO_MFMA unset
DISPATCH = {
    (10, 1): (0, 0, 0), (10, 5): (0, 0, 0), (10, 16): (0, 0, 0),
    (13, 1): (1, 0, 0), (13, 5): (1, 0, 0), (13, 16): (1, 0, 0),
    (22, 1): (1, 1, 1), (22, 5): (1, 1, 1), (22, 16): (0, 0, 0),
    (33, 1): (1, 1, 1), (33, 5): (1, 1, 1), (33, 16): (0, 0, 0),
    (42, 1): (1, 1, 1), (42, 5): (1, 1, 1), (42, 16): (0, 0, 0),
    (55, 1): (1, 0, 0), (55, 5): (1, 0, 0), (55, 16): (1, 0, 0),
}


@pytest.mark.parametrize("n", (10, 13, 22, 33, 42, 55))
def test_dispatch_answers(pa, monkeypatch, n):
    """pita_egnn_wide_{,jvp_,vjp_}uses_matrix_pipe for 1, 5 and 16 layers against the literal table above, and all zero
    on the same live handles once PITA_WIDE_NO_MFMA is set.  The table was printed by the build of the commit BEFORE the
    host-side restructuring on an MI355X (profiles/r10_wide_host_refactor.txt), not taken from the code under test: it
    pins the particle-system, depth and LDS thresholds of the three shape tables."""
    for L in (1, 5, 16):
        net = make_net(n, L=L)
        monkeypatch.delenv("PITA_WIDE_NO_MFMA", raising=False)
        got = tuple(int(f("cuda:0")) for f in (net.uses_matrix_pipe, net.jvp_uses_matrix_pipe, net.vjp_uses_matrix_pipe))
        print(f"n={n} L={L}: {got}")
        assert got == DISPATCH[(n, L)], (n, L, got)
        monkeypatch.setenv("PITA_WIDE_NO_MFMA", "1")
        off = tuple(int(f("cuda:0")) for f in (net.uses_matrix_pipe, net.jvp_uses_matrix_pipe, net.vjp_uses_matrix_pipe))
        assert off == (0, 0, 0), (n, L, off)


def entry_points(net, n, B, pa):
    """Every entry point that owns or shares a scratch buffer, once, on the current stream: name -> result tensors."""
    gen = torch.Generator().manual_seed(1000 * n + B)
    x = torch.randn(B, n, 3, generator=gen)
    x = (0.3 * (x - x.mean(1, keepdim=True))).reshape(B, 3 * n).cuda()
    h = (torch.rand(B, generator=gen) + 0.05).cuda()
    beta = (torch.rand(B, generator=gen) + 0.5).cuda()
    noise = torch.randn(2, B, 3 * n, generator=gen).cuda()
    sched, gam = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7), pa.ConstantAnnealingFactorSchedule(4 / 3)
    tab = pa.sde_integration.build_step_table(sched, gam, torch.linspace(0.3, 0.0, 3)[:-1], 0.15, 1.0, 1.3).cuda()
    torch.cuda.current_stream().synchronize()  # (the uploads ran on the legacy stream)
    return {"forward": lambda: (net.forward(h, x, beta),),
            "jvp": lambda: net.jvp(h, x, beta, direction=1),
            "jacobian_trace": lambda: net.jacobian_trace(h, x, beta, want_denoiser=True),
            "vjp": lambda: net.vjp(h, x, beta, want_dot_h=True),
            "sampler_run": lambda: (net.sampler_run(x.clone(), tab, 2, noise=noise),)}


@pytest.mark.parametrize("n", (22, 33))
def test_scratch_buffers_grown_reused_and_shared(pa, n):
    """forward, jvp, jacobian_trace, vjp(want_dot_h) and sampler_run (2 steps, explicit noise) on ONE handle at batches
    3, 9, 3 on two streams (22 atoms: one wave per item; 33: two): every result has the bits of the same call on a fresh
    handle -- buffers grown, reused at a smaller size and shared between entry points (the forward-mode marks) hold
    nothing that a later call reads."""
    net = make_net(n)
    assert net.uses_matrix_pipe("cuda:0") and net.jvp_uses_matrix_pipe("cuda:0") and net.vjp_uses_matrix_pipe("cuda:0")
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    ref = {}
    for B in (3, 9):
        for name in entry_points(net, n, B, pa):
            fresh = copy.deepcopy(net)  # (a copy carries no native handle: a new one is created on first use)
            ref[B, name] = [t.clone() for t in entry_points(fresh, n, B, pa)[name]()]
            torch.cuda.synchronize()
    for k, B in enumerate((3, 9, 3)):
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[k % 2]):
            for name, call in entry_points(net, n, B, pa).items():
                got = call()
                streams[k % 2].synchronize()
                assert len(got) == len(ref[B, name])
                for i, (a, b) in enumerate(zip(got, ref[B, name])):
                    assert torch.isfinite(a).all(), (name, B, i)
                    assert torch.equal(a, b), (name, B, k, i, float((a - b).abs().max()))


@pytest.mark.parametrize("hidden", (48, 64))
@pytest.mark.parametrize("att", (False, True))
@pytest.mark.parametrize("beta", (False, True))
def test_weight_count_and_failed_create(pa, hidden, att, beta):
    """pita_egnn_wide_num_weights equals the state dict's element count; a create with one weight too few returns
    PITA_EINVAL and no handle, and a create with the right count then succeeds and evaluates."""
    L = pa._lib.lib()
    net = make_net(22, hidden=hidden, att=att, beta=beta)
    cfg = net._config()
    flat = torch.cat([p.detach().float().reshape(-1) for p in net.state_dict().values()]).contiguous().numpy()
    assert L.pita_egnn_wide_num_weights(ctypes.byref(cfg)) == sum(p.numel() for p in net.state_dict().values()) == flat.size
    h0 = np.ascontiguousarray(net.h_initial.float().numpy())
    with torch.cuda.device(0):
        for n_w, want in ((flat.size - 1, PITA_EINVAL), (flat.size, 0)):
            h = ctypes.c_void_p()
            rc = L.pita_egnn_wide_create(ctypes.byref(h), ctypes.byref(cfg), flat.ctypes.data_as(ctypes.c_void_p), n_w,
                                         h0.ctypes.data_as(ctypes.c_void_p))
            assert rc == want and bool(h.value) == (want == 0), (n_w, rc, h.value)
        x = torch.randn(3, 66, generator=torch.Generator().manual_seed(1)).cuda()
        t, b, out = torch.full((3,), 0.5).cuda(), torch.ones(3).cuda(), torch.empty(3, 66).cuda()
        pa._lib.check(L.pita_egnn_wide_eval(h, 0, t.data_ptr(), x.data_ptr(), b.data_ptr() if beta else 0, out.data_ptr(), 3,
                                            pa._lib.stream_ptr(x.device)), "pita_egnn_wide_eval")
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        assert L.pita_egnn_wide_destroy(h) == 0
