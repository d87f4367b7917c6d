"""E(n)-equivariant GNN backbone executed by the fused HIP kernel.

Mirror of ``EGNN_dynamics`` (pita/src/models/components/egnn_temp_conditioned.py:7-117): same
constructor arguments, same parameter names and creation order (so a seeded construction gives
the reference's weights and its ``state_dict`` / Lightning checkpoints load unchanged), same
``forward(t, xs, beta) -> vel`` contract.  The module only OWNS the parameters; the arithmetic
of EGNN.forward (:172-194) and E_GCL (:197-356) lives in pita_amd/csrc/egnn_kernel.hip.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._backbone import HipBackbone


DEFAULT_PRECISION = "f16x2"  # dense-layer arithmetic of the HIP EGNN when the caller does not choose (see EGNN_dynamics)


class _GCLParams(nn.Module):
    """Parameters of one E_GCL layer, created in the reference's order (:232-260)."""

    def __init__(self, hidden_nf, act_fn, attention, tanh, edges_in_d=1):
        super().__init__()
        h = hidden_nf
        self.edge_mlp = nn.Sequential(nn.Linear(2 * h + 1 + edges_in_d, h), act_fn, nn.Linear(h, h), act_fn)
        self.node_mlp = nn.Sequential(nn.Linear(2 * h, h), act_fn, nn.Linear(h, h))
        head = nn.Linear(h, 1, bias=False)
        torch.nn.init.xavier_uniform_(head.weight, gain=0.001)
        coord = [nn.Linear(h, h), act_fn, head]
        if tanh:
            coord.append(nn.Tanh())
        self.coord_mlp = nn.Sequential(*coord)
        if attention:
            self.att_mlp = nn.Sequential(nn.Linear(h, 1), nn.Sigmoid())


class EGNN(nn.Module):
    """Parameter container matching the reference ``EGNN`` module tree (:120-170)."""

    def __init__(self, in_node_nf, in_edge_nf, hidden_nf, act_fn=nn.SiLU(), n_layers=4, recurrent=True,
                 attention=False, norm_diff=True, out_node_nf=None, tanh=False, coords_range=15, agg="sum",
                 has_virtual=False):
        super().__init__()
        if has_virtual or not recurrent or not norm_diff or agg != "sum" or in_edge_nf != 1:
            raise NotImplementedError("HIP EGNN implements recurrent=True, norm_diff=True, agg='sum', no virtual node")
        if not isinstance(act_fn, nn.SiLU):
            raise NotImplementedError("HIP EGNN implements the SiLU activation used by every reference config")
        out_node_nf = in_node_nf if out_node_nf is None else out_node_nf
        self.hidden_nf, self.n_layers = hidden_nf, n_layers
        self.coords_range = float(coords_range)
        self.attention, self.tanh = attention, tanh
        self.embedding = nn.Linear(in_node_nf, hidden_nf)
        self.embedding_out = nn.Linear(hidden_nf, out_node_nf)  # dead in the reference forward (:80,189)
        for i in range(n_layers):
            self.add_module("gcl_%d" % i, _GCLParams(hidden_nf, act_fn, attention, tanh, in_edge_nf))


class EGNN_dynamics(HipBackbone):
    def __init__(self, n_particles, n_dimension, hidden_nf=64, act_fn=torch.nn.SiLU(), n_layers=4, recurrent=True,
                 attention=False, condition_time=True, tanh=False, agg="sum", energy=False, add_virtual=False,
                 condition_temperature=False, feature_layout="pita", precision=None):
        super().__init__()
        if energy or add_virtual or not condition_time:
            raise NotImplementedError("HIP EGNN_dynamics implements energy=False, add_virtual=False, condition_time=True")
        self.in_node_nf = 2 if condition_temperature else 1
        self.egnn = EGNN(in_node_nf=self.in_node_nf, in_edge_nf=1, hidden_nf=hidden_nf, act_fn=act_fn,
                         n_layers=n_layers, recurrent=recurrent, attention=attention, tanh=tanh, agg=agg)
        self._n_particles, self._n_dimension = n_particles, n_dimension
        self.condition_time, self.condition_temperature = condition_time, condition_temperature
        # "pita" keeps the reference's t/beta interleave quirk (:68-78); "correct" gives (t, beta) per node
        self.feature_layout = {"pita": 0, "correct": 1}[feature_layout]
        # dense-layer arithmetic, all fp32-accurate: "f32" = f32 MFMA (bit-exact fmaf chains), "bf16x3" = bf16 matrix
        # pipe with an exact three-way operand split, "f16x2" = f16 matrix pipe with a two-way round-to-nearest split
        # and power-of-two operand scaling (|activations| < 4094; see csrc/egnn_common.h)
        precision = precision or os.environ.get("PITA_EGNN_PRECISION", DEFAULT_PRECISION)
        self.precision = {"f32": 0, "bf16x3": 1, "f16x2": 2}[precision]
        self.counter = 0

    # ------------------------------------------------------------------ native handle (lifetime: HipBackbone)
    _destroy_symbol = "pita_egnn_destroy"

    def _config(self):
        e = self.egnn
        return _lib.EgnnConfig(self._n_particles, self._n_dimension, e.hidden_nf, e.n_layers, self.in_node_nf,
                               int(e.attention), int(e.tanh), e.coords_range, self.feature_layout, self.precision)

    def _create_handle(self, flat):
        cfg, h = self._config(), ctypes.c_void_p()
        _lib.check(_lib.lib().pita_egnn_create(ctypes.byref(h), ctypes.byref(cfg), flat.ctypes.data_as(ctypes.c_void_p),
                                               flat.size), "pita_egnn_create")
        return h

    def _key_extra(self):
        return (self.precision,)

    def _conditions_on_beta(self):
        return self.condition_temperature

    # ------------------------------------------------------------------ reference interface
    def forward(self, t, xs, beta=None):
        """vel[B, n*d] = backbone(t[B], xs[B, n*d], beta[B]); mean-free (:56-93)."""
        out = self._forward_call("pita_egnn_forward", t, xs, beta)
        self.counter += 1
        return out

    # ------------------------------------------------------------------ fused extensions used by ScoreNet / the sampler
    # (who probes for which of them: the table in _backbone.py)
    def edm(self, what, h_t, x_t, beta):
        """what=1: denoiser D_theta, what=2: score (D_theta - x)/h, EDM preconditioning fused (score_net.py:13-43)."""
        return self._edm_call("pita_egnn_edm", what, h_t, x_t, beta)

    def jvp(self, h_t, x_t, beta, vx=None, direction=-1, vh=None, want_primal=True, want_tangent=True, dot_out=None,
            dot_col=0, diag_acc=None):
        """(D, dD): the denoiser D_theta(h, x) and its forward-mode derivative along ONE tangent direction:
        dD = J_x D . vx + dD/dh . vh.  ``vx``: [B, D] tensor, or None for the unit direction ``direction`` of
        every walker (-1 = zero).  ``vh``: [B] tensor or None.  Optional in-kernel reductions:
        ``dot_out[:, dot_col] = <x, dD>`` and ``diag_acc += dD[:, direction]``.
        (pita_egnn_jvp; fp32-accurate bf16x3 arithmetic.)"""
        return self._jvp_call("pita_egnn_jvp", h_t, x_t, beta, vx, direction, vh, want_primal, want_tangent, dot_out,
                              dot_col, diag_acc)

    def jacobian_trace(self, h_t, x_t, beta, want_denoiser=False):
        """trace(J_x D_theta(h, x)) per walker, exactly, over all dim unit directions (pita_egnn_jacobian_trace: the
        primal network is evaluated once, its per-edge factors cached for the tangent-only launches that follow).
        ``want_denoiser``: also return D_theta(h, x), a by-product of the primal -> (trace, D)."""
        trace, den = self._trace_call("pita_egnn_jacobian_trace", h_t, x_t, beta, want_denoiser, device_guard=True)
        return (trace, den) if want_denoiser else trace

    def trace_probes(self, h_t, x_t, beta, n_probes, probes=None, seed=0, walker_offset=0, step=0, want_denoiser=False,
                     want_per_probe=False):
        """(estimate, D or None, per_probe or None): the Hutchinson estimate of trace(J_x D_theta(h, x)) per walker from
        ``n_probes`` probes, mean_k <v_k, J_x D v_k>, in ONE call (pita_egnn_trace_probes): the probes go through the
        multi-direction kernels of ``jacobian_trace`` in the place of unit vectors, so the probes of a launch share one
        primal evaluation, on the handle's own arithmetic.  ``probes`` [K, B, n*d]: the tangent inputs (parity hook);
        None: Rademacher signs drawn in the kernel, keyed (seed, walker_offset + row, step) -- what
        ``pita_amd.utils.rademacher_probes`` returns for the same key (K <= 256).  ``want_per_probe``: also the [K, B]
        quadratic forms.  Returns None when the particle system has no multi-direction kernel (PITA_EUNSUPPORTED): the
        caller takes ``n_probes`` ``jvp`` launches.  ``VEReverseSDE(divergence="hutchinson", shared_primal=True)``
        takes it."""
        try:
            return self._probes_call("pita_egnn_trace_probes", h_t, x_t, beta, n_probes, probes, seed, walker_offset, step,
                                     want_denoiser, want_per_probe, device_guard=True)
        except _lib.PitaHipError as e:
            if getattr(e, "code", 0) == -2:  # PITA_EUNSUPPORTED, from creating the handle or from the call
                return None
            raise

    vjp_h_parts = True  # vjp(..., want_h_parts=True) is available

    def vjp(self, h_t, x_t, beta, cot=None, want_primal=True, want_dot_h=False, want_h_parts=False):
        """(D, J_x D^T cot): the denoiser and its reverse-mode derivative for a per-walker cotangent (default: x_t
        itself, which is what grad_x E_theta needs).  One launch (pita_egnn_vjp) instead of dim JVP launches.
        ``want_dot_h``: also return <cot, dD/dh> [B] from the same sweep -> (D, vjp, dot_h).
        ``want_h_parts`` (with want_dot_h): also [B, 2] = (c_out <cot, F>, <cot, d(c_out F)/dh>), the split of the same
        derivative that pita_fk_assemble turns into E_theta and dE_theta/dh without cancellation at small h
        -> (D, vjp, dot_h, parts)."""
        return self._vjp_call("pita_egnn_vjp", h_t, x_t, beta, cot, want_primal, want_dot_h, want_h_parts)

    def sampler_run(self, x, step_tab, n_steps, noise=None, seed=0, walker_offset=0, step0=0, remove_mean=True,
                    drift_out=None, n_particles=None, n_dim=None, stats_out=None):
        """In-place fused Euler-Maruyama steps (pita_egnn_sampler_run); x: [B, n*d] device tensor.  ``stats_out``:
        optional contiguous float64 device tensor [n_steps, 4] that accumulates the per-step drift / diffusion moments."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if stats_out is not None:
            assert stats_out.is_cuda and stats_out.dtype == torch.float64 and stats_out.is_contiguous()
            assert stats_out.numel() >= 4 * int(n_steps)
        assert step_tab.is_cuda and step_tab.dtype == torch.float32 and step_tab.is_contiguous()
        _lib.check(_lib.lib().pita_egnn_sampler_run(
            self._native(x.device), x.data_ptr(), x.shape[0], step_tab.data_ptr(), int(n_steps), _lib.ptr(noise),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset), int(step0), int(bool(remove_mean)),
            _lib.ptr(drift_out), _lib.ptr(stats_out), _lib.stream_ptr(x.device)), "pita_egnn_sampler_run")
        return x

    def sampler_work(self, B, device):
        """(16-bit MFMAs, f32 MFMAs) executed per walker-step by the fused sampler at batch B (pita_egnn_sampler_work)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        _lib.check(_lib.lib().pita_egnn_sampler_work(self._native(device), int(B), ctypes.byref(a), ctypes.byref(b)),
                   "pita_egnn_sampler_work")
        return a.value, b.value

    def sampler_mapping(self, B, device):
        """(walkers per wavefront group, wavefronts launched, resident wavefront slots) of the fused sampler at batch B
        (pita_egnn_sampler_mapping)."""
        g, w, s = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.lib().pita_egnn_sampler_mapping(self._native(device), int(B), ctypes.byref(g), ctypes.byref(w),
                                                        ctypes.byref(s)), "pita_egnn_sampler_mapping")
        return g.value, w.value, s.value

