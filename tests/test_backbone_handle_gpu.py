"""Lifetime of the native handle that ``_backbone.HipBackbone`` owns, per backbone family at the smallest shapes every
family accepts (B = 3 walkers: DW4-sized hidden-32 EGNN, 13-particle wide EGNN, 2-D MLP): the handle is reused while the
weights are untouched, rebuilt when one changes (and then computes what a fresh module with those weights computes),
never shared with a copy, and -- hidden-32 only -- rebuilt when ``precision`` changes."""
import copy

import pytest
import torch

from oracle import pita_oracle as O

pytestmark = pytest.mark.gpu

B = 3


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()  # fail loudly if the HIP library is missing
    return pita_amd


def _h32():
    from pita_amd import egnn_temp_conditioned

    return egnn_temp_conditioned.EGNN_dynamics(4, 2, hidden_nf=32, n_layers=1, condition_temperature=True, precision="f16x2")


def _wide():
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    return EGNN_dynamics_AD2_cat(13, 3, hidden_nf=16, n_layers=1, condition_beta=True)


def _mlp():
    from pita_amd import mlp

    return mlp.MyMLPTemperature(input_dim=2, out_dim=2, hidden_layers=1)


FAMILIES = {"h32": (_h32, 4, 2), "wide": (_wide, 13, 3), "mlp": (_mlp, 2, 1)}


def _inputs(n, d):
    gen = torch.Generator().manual_seed(5)
    h = torch.tensor([0.3, 2.0, 40.0])
    _, c_in, _, c_noise = O.edm_coeffs(h)
    x = O.remove_mean(torch.randn(B, n * d, generator=gen) * (1 + h.sqrt())[:, None], n, d) * c_in[:, None]
    beta = torch.rand(B, generator=gen) + 0.7
    return c_noise, x, beta


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_handle_is_reused_rebuilt_and_never_shared(pa, family):
    make, n, d = FAMILIES[family]
    torch.manual_seed(11)
    net = make()
    t, x, beta = (v.cuda() for v in _inputs(n, d))
    y0 = net(t, x, beta)
    handle = net._handle
    assert handle is not None and torch.isfinite(y0).all()
    assert torch.equal(net(t, x, beta), y0) and net._handle is handle  # untouched weights: same bits, same handle

    twin = copy.deepcopy(net)
    assert twin._handle is None
    assert torch.equal(twin(t, x, beta), y0)
    assert twin._handle is not handle and twin._handle.value != handle.value and net._handle is handle

    with torch.no_grad():
        next(net.parameters()).mul_(1.5)
    y1 = net(t, x, beta)
    assert net._handle is not handle and not torch.equal(y1, y0)
    fresh = make()
    fresh.load_state_dict(net.state_dict())
    assert torch.equal(fresh(t, x, beta), y1)
    assert torch.equal(twin(t, x, beta), y0)  # the copy owns its weights and its handle


def test_hidden32_precision_is_part_of_the_handle_key(pa):
    """Assigning ``precision`` rebuilds the handle; the f32 and f16x2 results differ and both meet the accuracy
    ``test_hip_parity.test_egnn_golden`` asks of every precision: within max(4 x the fp32 reference's own error against
    fp64, 2e-6) of the fp64 oracle."""
    torch.manual_seed(11)
    net = _h32()
    with torch.no_grad():
        # the coordinate head is created with gain 0.001: the update x_final - x then sits at the rounding of x, every
        # precision rounds it to the same bits and nothing could tell the handles apart; a head of ordinary size (what
        # training gives) makes the dense-layer arithmetic visible in the output
        net.egnn.gcl_0.coord_mlp[2].weight.mul_(1000.0)
    t, x, beta = _inputs(4, 2)
    w = {k: v.detach().clone() for k, v in net.state_dict().items()}
    F64 = O.egnn_forward(w, t.double(), x.double(), beta.double(), 4, 2, n_layers=1, tanh=False, attention=False)
    F32 = O.egnn_forward(w, t, x, beta, 4, 2, n_layers=1, tanh=False, attention=False)
    rel = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())
    tol = max(4 * rel(F32, F64), 2e-6)
    t, x, beta = t.cuda(), x.cuda(), beta.cuda()
    y16 = net(t, x, beta)
    handle, key = net._handle, net._handle_key
    assert key[:2] == (x.device.index, 2)
    net.precision = 0  # "f32"
    y32 = net(t, x, beta)
    assert net._handle is not handle and net._handle_key[:2] == (x.device.index, 0) and net._handle_key[2:] == key[2:]
    print(f"err_f16x2_vs_fp64={rel(y16, F64):.3e} err_f32_vs_fp64={rel(y32, F64):.3e} tol={tol:.3e}")
    assert not torch.equal(y32, y16)
    assert rel(y16, F64) < tol and rel(y32, F64) < tol
    net.precision = 2
    assert torch.equal(net(t, x, beta), y16)
