"""The contract between the HIP backbones and their callers (no GPU needed): which protocol attributes each class has and
lacks (ScoreNet, EnergyNet, VEReverseSDE and WeightedSDEIntegrator dispatch on ``hasattr``), the signatures of the public
entry points, that copies and pickles start without a native handle, and that argument errors are raised before any
device work.  The tables below were written from the classes as they stood before ``_backbone.HipBackbone`` existed."""
import copy
import ctypes
import inspect
import pickle

import pytest
import torch

PROTOCOL = {"edm", "jvp", "vjp", "vjp_h_parts", "jacobian_trace", "jacobian_trace_estimate", "trace_probes",
            "sampler_run", "can_fuse"}
HAS = {"h32": {"edm", "jvp", "vjp", "vjp_h_parts", "jacobian_trace", "trace_probes", "sampler_run"},
       "wide": {"edm", "jvp", "vjp", "vjp_h_parts", "jacobian_trace", "jacobian_trace_estimate", "sampler_run", "can_fuse"},
       "mlp": {"jvp", "vjp", "vjp_h_parts", "jacobian_trace", "sampler_run", "can_fuse"}}

_PROBES = ("(self, h_t, x_t, beta, n_probes, probes=None, seed=0, walker_offset=0, step=0, want_denoiser=False, "
           "want_per_probe=False)")
SIGNATURES = {
    "edm": "(self, what, h_t, x_t, beta)",
    "jvp": ("(self, h_t, x_t, beta, vx=None, direction=-1, vh=None, want_primal=True, want_tangent=True, dot_out=None, "
            "dot_col=0, diag_acc=None)"),
    "vjp": "(self, h_t, x_t, beta, cot=None, want_primal=True, want_dot_h=False, want_h_parts=False)",
    "jacobian_trace": "(self, h_t, x_t, beta, want_denoiser=False)",
    "jacobian_trace_estimate": _PROBES,
    "trace_probes": _PROBES,
    "sampler_run": ("(self, x, step_tab, n_steps, noise=None, seed=0, walker_offset=0, step0=0, remove_mean=True, "
                    "drift_out=None, n_particles=None, n_dim=None, stats_out=None)"),
    "can_fuse": "(self, n_particles, n_dim)",
    "jacobian": ("(self, h_t, x_t, beta, cot=None, want_denoiser=False, want_trace=False, want_vjp=False, "
                 "want_dot_h=False, want_h_parts=False)"),
}
FORWARD = {"h32": "(self, t, xs, beta=None)", "wide": "(self, t, xs, beta=None)", "MyMLP": "(self, t, x, x_self_cond=False)",
           "MyMLPTemperature": "(self, t, x, beta)"}


def _nets(conditioned):
    """(family, instance, D) of every shipped class at a tiny size; ``conditioned``: the beta-conditioned flavours only."""
    from pita_amd import egnn, egnn_aldp, egnn_temp_conditioned, mlp
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    torch.manual_seed(0)
    out = [("h32", egnn_temp_conditioned.EGNN_dynamics(4, 2, hidden_nf=32, n_layers=1, condition_temperature=conditioned), 8),
           ("wide", EGNN_dynamics_AD2_cat(13, 3, hidden_nf=16, n_layers=1, condition_beta=conditioned), 39),
           ("wide", egnn_aldp.EGNN_dynamics(13, 3, hidden_nf=16, n_layers=1, condition_temperature=conditioned), 39)]
    if conditioned:
        out.append(("mlp", mlp.MyMLPTemperature(input_dim=2, out_dim=2, hidden_layers=1), 2))
    else:
        out.append(("h32", egnn.EGNN_dynamics(4, 2, hidden_nf=32, n_layers=1), 8))
        out.append(("mlp", mlp.MyMLP(input_dim=2, out_dim=2, hidden_layers=1), 2))
    return out


def _all_nets():
    return _nets(False) + _nets(True)


def test_each_class_has_exactly_its_protocol_attributes():
    for family, net, _ in _all_nets():
        for obj in (net, type(net)):
            assert {a for a in PROTOCOL if hasattr(obj, a)} == HAS[family], (type(net).__module__, obj)
        assert net.vjp_h_parts is True
        assert hasattr(net, "jacobian") == (family == "mlp")
        assert hasattr(net, "_n_particles") == (family != "mlp")  # keys VEReverseSDE's Rademacher probes


def test_public_signatures_are_the_parents():
    for family, net, _ in _all_nets():
        cls = type(net)
        for name in sorted(HAS[family] - {"vjp_h_parts"}) + (["jacobian"] if family == "mlp" else []):
            assert str(inspect.signature(getattr(cls, name))) == SIGNATURES[name], (cls.__module__, cls.__name__, name)
        want = FORWARD[cls.__name__ if family == "mlp" else family]
        assert str(inspect.signature(cls.forward)) == want, (cls.__module__, cls.__name__)


def test_identities_between_the_flavours():
    from pita_amd import egnn, egnn_aldp, egnn_temp_conditioned
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    for name in HAS["h32"] - {"vjp_h_parts"}:
        assert getattr(egnn.EGNN_dynamics, name) is getattr(egnn_temp_conditioned.EGNN_dynamics, name)
    for name in HAS["wide"] - {"vjp_h_parts"}:
        assert getattr(egnn_aldp.EGNN_dynamics, name) is getattr(EGNN_dynamics_AD2_cat, name)


def test_copies_and_pickles_start_without_a_handle():
    for _, net, _ in _all_nets():
        # what a used module carries, without a device: a (null) handle, its key and the cached tensor list; destroying
        # a null handle is a no-op in the library
        net._handle, net._handle_key = ctypes.c_void_p(), (0,)
        net.__dict__["_tensor_list"] = list(net.parameters()) + list(net.buffers())
        for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
            assert type(twin) is type(net)
            assert twin._handle is None and twin._handle_key is None
            assert "_tensor_list" not in twin.__dict__
            a, b = net.state_dict(), twin.state_dict()
            assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert net._handle is not None and "_tensor_list" in net.__dict__  # the original keeps its own


def test_conditioned_backbone_without_beta_is_a_value_error_before_any_device_work():
    for family, net, D in _nets(True):
        h, x = torch.ones(2), torch.zeros(2, D)  # host tensors: the device path would raise something else first
        calls = [lambda: net(h, x, None), lambda: net.jvp(h, x, None, direction=0), lambda: net.vjp(h, x, None),
                 lambda: net.jacobian_trace(h, x, None)]
        if family != "mlp":
            calls.append(lambda: net.edm(1, h, x, None))
        if family == "h32":
            calls.append(lambda: net.trace_probes(h, x, None, 1))
        if family == "wide":
            calls.append(lambda: net.jacobian_trace_estimate(h, x, None, 1))
        if family == "mlp":
            calls.append(lambda: net.jacobian(h, x, None, want_trace=True))
        for call in calls:
            with pytest.raises(ValueError, match=type(net).__name__):
                call()
            assert net._handle is None


def test_h_parts_without_dot_h_is_refused_before_any_device_work():
    for _, net, D in _all_nets():
        with pytest.raises(ValueError, match="want_h_parts needs want_dot_h"):
            net.vjp(torch.ones(2), torch.zeros(2, D), torch.ones(2), want_h_parts=True, want_dot_h=False)
        assert net._handle is None
