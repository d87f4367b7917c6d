"""The fused sampler's edge loop gathers the partner row j = (i + dd) mod N of every column (padded columns read their own
row) and computes one squared distance per lane half (current geometry in the lower half, input geometry in the upper
half).  A wrong wrap, a wrong padded-lane row or a half reading the wrong table changes a walker's result as soon as the
walker sits at another place in its wave's column tiles -- which is what these tests move:

  * a batch of B walkers against B one-walker launches, bit for bit, at batch sizes that give padded columns, tail groups,
    walkers that straddle a tile boundary and (LJ55) walkers that span two tiles, in the three arithmetic modes;
  * a batch large enough for the regular walkers-per-wave mapping against the same walkers run in small chunks (which
    take the small-group mapping): the two instantiations of the kernel agree bit for bit;
  * forward mode against the fp64 oracle on the same small batches, to the standard of test_egnn_golden;
  * one fused step with attention off and with tanh off (the wave-uniform branches around the edge's geometry and
    aggregation code) against the oracle, with the bounds of test_hip_parity._one_step_vs_oracle.
"""
import os

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O

pytestmark = pytest.mark.gpu
T = torch.tensor

SYSTEMS = {"lj13": (13, 3), "dw4": (4, 2), "aldp22": (22, 3), "lj55": (55, 3)}
BATCHES = [("lj13", 1), ("lj13", 7), ("lj13", 8), ("lj13", 33), ("dw4", 1), ("dw4", 8), ("dw4", 9),
           ("aldp22", 1), ("aldp22", 4), ("aldp22", 5), ("lj55", 1), ("lj55", 2)]
PRECISIONS = ["f32", "bf16x3", "f16x2"]


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    return pita_amd


_NETS = {}


def make_net(pa, golden, n, d, precision=None, tanh=True, attention=True, wfile="egnn_weights_trainedlike.npz"):
    key = (n, d, precision, tanh, attention, wfile)
    if key not in _NETS:
        kw = {} if precision is None else {"precision": precision}
        net = pa.EGNN_dynamics(n, d, hidden_nf=32, n_layers=3, recurrent=True, tanh=tanh, attention=attention,
                               condition_time=True, condition_temperature=True, agg="sum", **kw)
        w = golden(wfile)
        net.load_state_dict({k: T(w[k]) for k in net.state_dict().keys()})
        _NETS[key] = net.cuda()
    return _NETS[key]


def step_table(pa, N):
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    return pa.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, N + 1)[:-1], 1.0 / N, 1.0, 1.0).cuda()


def start_walkers(pa, n, d, B, seed=5):
    return pa.Prior(scale=69.28, n_particles=n, spatial_dim=d, seed=seed).sample(B)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,B", BATCHES)
def test_batch_equals_single_walkers_bitwise(pa, golden, name, B, precision):
    n, d = SYSTEMS[name]
    net = make_net(pa, golden, n, d, precision=precision)
    N = 3
    tab = step_table(pa, N)
    x0 = start_walkers(pa, n, d, B)
    kw = dict(seed=11, remove_mean=True, n_particles=n, n_dim=d)
    full = net.sampler_run(x0.clone(), tab, N, walker_offset=0, **kw)
    assert torch.isfinite(full).all() and not torch.equal(full, x0)
    singles = [net.sampler_run(x0[i:i + 1].clone(), tab, N, walker_offset=i, **kw) for i in range(B)]
    assert torch.equal(torch.cat(singles), full)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,G,extra", [("lj13", 7, 33), ("aldp22", 4, 5)])
def test_regular_mapping_equals_small_chunks_bitwise(pa, golden, name, G, extra, precision):
    """The smallest batch that takes the regular mapping (G walkers per wave: two waves on every SIMD), plus a ragged
    remainder, against the same walkers in chunks that take the small-group mapping."""
    n, d = SYSTEMS[name]
    net = make_net(pa, golden, n, d, precision=precision)
    N = 3
    tab = step_table(pa, N)
    B = torch.cuda.get_device_properties(0).multi_processor_count * 8 * G + extra
    x0 = start_walkers(pa, n, d, B)
    kw = dict(seed=11, remove_mean=True, n_particles=n, n_dim=d)
    full = net.sampler_run(x0.clone(), tab, N, walker_offset=0, **kw)
    assert torch.isfinite(full).all()
    chunk = 1001
    parts = [net.sampler_run(x0[i:i + chunk].clone(), tab, N, walker_offset=i, **kw) for i in range(0, B, chunk)]
    assert torch.equal(torch.cat(parts), full)


_FWD_REF = {}


def _forward_reference(golden, name, B):
    """Inputs of one small batch, the fp64 oracle on them and the fp32 oracle's own error (computed once per batch)."""
    if (name, B) not in _FWD_REF:
        n, d = SYSTEMS[name]
        w = golden("egnn_weights_trainedlike.npz")
        gen = torch.Generator().manual_seed(100 * n + B)
        h = torch.exp(torch.empty(B).uniform_(-3.0, 6.0, generator=gen))  # sigma^2 across the schedule's range
        c_s, c_in, c_out, c_noise = O.edm_coeffs(h)
        x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1.0 + h[:, None]) ** 0.5, n, d)
        xs = c_in[:, None] * x
        beta = torch.empty(B).uniform_(0.5, 2.0, generator=gen)
        nt = min(16, os.cpu_count() or 1)
        old = torch.get_num_threads()
        torch.set_num_threads(nt)
        try:
            F64 = O.egnn_forward({k: T(v).double() for k, v in w.items()}, c_noise.double(), xs.double(), beta.double(), n, d)
            F32 = O.egnn_forward({k: T(v) for k, v in w.items()}, c_noise, xs, beta, n, d)
        finally:
            torch.set_num_threads(old)
        _FWD_REF[(name, B)] = (c_noise, xs, beta, F64, rel(F32, F64))
    return _FWD_REF[(name, B)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,B", BATCHES)
def test_forward_mode_vs_fp64_oracle(pa, golden, name, B, precision):
    n, d = SYSTEMS[name]
    net = make_net(pa, golden, n, d, precision=precision)
    c_noise, xs, beta, F64, err_ref = _forward_reference(golden, name, B)
    F = net(c_noise.cuda(), xs.cuda(), beta.cuda())
    err_hip = rel(F, F64)
    print(f"[{name}/B={B}/{precision}] err_hip_vs_fp64={err_hip:.3e} err_ref_vs_fp64={err_ref:.3e}")
    assert err_hip < max(4 * err_ref, 2e-6), (err_hip, err_ref)


@pytest.mark.parametrize("tanh,attention", [(True, False), (False, True)])
def test_one_step_without_attention_or_tanh_vs_oracle(pa, golden, tanh, attention):
    """One fused step, LJ13, 8 walkers, at the step test_hip_parity._one_step_vs_oracle uses (h ~ 0.6), drift and walkers
    against the fp64 oracle with that test's bounds (1e-4 on the drift, whose 1/h amplifies rounding; 1e-5 on x)."""
    n, d, B = 13, 3, 8
    wfile = "egnn_weights_trainedlike.npz"
    net = make_net(pa, golden, n, d, tanh=tanh, attention=attention, wfile=wfile)
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
    gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
    N, k0 = 50, 37
    times = torch.linspace(1.0, 0.0, N + 1)[:-1]
    tab = pa.sde_integration.build_step_table(sched, gam, times, 1.0 / N, 1.0, 1.0)
    gen = torch.Generator().manual_seed(3)
    h_k = float(tab[k0, pa._lib.ST_H])
    x0 = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1.0 + h_k) ** 0.5, n, d)
    noise = torch.randn(1, B, n * d, generator=gen)
    x = x0.cuda().clone()
    drift = torch.empty_like(x)
    net.sampler_run(x, tab[k0:k0 + 1].cuda().contiguous(), 1, noise=noise.cuda(), drift_out=drift)
    assert torch.isfinite(x).all()
    w = golden(wfile)
    wt = {k: T(v).double() for k, v in w.items()}
    bb = lambda cn, xs, b: O.egnn_forward(wt, cn, xs, b, n, d, tanh=tanh, attention=attention)
    osched, ogam = O.Elucidating(0.05, 80.0, 7), O.GammaConstant(4 / 3)
    t = times[k0].double()
    terms = O.f_not_debiased(bb, osched, ogam, t, x0.double(), 1.0)
    tb = t * torch.ones(B, dtype=torch.float64)
    xo = x0.double() + (terms.drift_X * (1.0 / N) + (osched.g(tb)[:, None] * noise[0].double()) * np.sqrt(1.0 / N))
    xo = O.remove_mean(xo, n, d)
    assert torch.isfinite(xo).all() and float(terms.drift_X.abs().max()) > 0
    print(f"[one step/tanh={tanh}/attention={attention}] drift vs fp64 {rel(drift, terms.drift_X):.2e}, x vs fp64 {rel(x, xo):.2e}")
    assert rel(drift, terms.drift_X) < 1e-4
    assert rel(x, xo) < 1e-5
