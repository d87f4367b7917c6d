"""What the HIP backbones share: the lifetime of the native handle, the marshalling of ``(h_t, x_t, beta)`` and one
Python body per C signature that more than one family exports.

The protocol between the backbones and their callers.  The callers probe with ``hasattr`` and take the first route they
find; a backbone offers a route by having the attribute, so the shared bodies below are private (``_..._call``) and each
family names only the routes its library entry points serve.  ``h_t`` [B], ``x_t`` [B, D], ``beta`` [B] or a number;
D = n_particles * n_dim.  h32 = ``egnn.EGNN_dynamics`` / ``egnn_temp_conditioned.EGNN_dynamics``, wide =
``EGNN_dynamics_AD2_cat`` / ``egnn_aldp.EGNN_dynamics``, mlp = ``MyMLP`` / ``MyMLPTemperature``.

===========================  =====================  ==========================================================  =============
attribute                    probed by              must return                                                 offered by
===========================  =====================  ==========================================================  =============
``forward(t, x, beta)``      every caller (no       backbone output [B, D]                                      h32 wide mlp
                             probe: required)
``edm(what, h_t, x_t,        ScoreNet               what=1: denoiser D_theta, what=2: score (D_theta - x)/h;    h32 wide
beta)``                                             absent: ScoreNet wraps ``forward`` in two small kernels
``vjp(h_t, x_t, beta, ...)`` EnergyNet,             (D, J_x D^T cot[, <cot, dD/dh>[, h_parts [B, 2]]]);         h32 wide mlp
                             VEReverseSDE           absent: dim (+ 1) ``jvp`` calls
``vjp_h_parts``              VEReverseSDE           True when ``vjp(want_h_parts=True)`` is served              h32 wide mlp
``jvp(h_t, x_t, beta, ...)`` EnergyNet,             (D or None, dD or None) along one direction, with the       h32 wide mlp
                             VEReverseSDE           in-kernel ``dot_out`` / ``diag_acc`` reductions; absent
                                                    together with ``vjp``: no debiased regime
``jacobian_trace(h_t, x_t,   VEReverseSDE           with ``want_denoiser=True`` (how it is called):             h32 wide mlp
beta, want_denoiser)``                              (trace [B], D); absent: dim ``jvp`` calls
``jacobian_trace_estimate(   VEReverseSDE           (estimate [B], D or None, per_probe [K, B] or None);        wide
h_t, x_t, beta, n_probes,    (divergence=           raises where the library refuses
...)``                       "hutchinson")
``trace_probes(...)``        VEReverseSDE           the same triple, or None where the library has no           h32
                             (shared_primal=True)   multi-direction kernel (the caller takes ``jvp`` calls)
``_n_particles``             VEReverseSDE           particle count that keys the Rademacher probes (else 1)     h32 wide
``sampler_run(x, step_tab,   WeightedSDEIntegrator  x, advanced in place by ``n_steps`` fused steps             h32 wide mlp
n_steps, ...)``
``can_fuse(n_particles,      WeightedSDEIntegrator  whether ``sampler_run`` serves that geometry; absent:       wide mlp
n_dim)``                                            it always does
===========================  =====================  ==========================================================  =============
"""
import contextlib

import torch
from torch import nn

from ._lib import check, dev_tensor, lib, ptr, stream_ptr  # bound here: these bodies run once per launch


def as_batch(v, B, device):
    """A number or a tensor as a contiguous fp32 [B] tensor on ``device``."""
    if not isinstance(v, torch.Tensor):
        return torch.full((B,), float(v), device=device, dtype=torch.float32)
    return dev_tensor(v.to(device), "per-walker scalar").reshape(-1).expand(B).contiguous()


class HipBackbone(nn.Module):
    """A parameter-owning module whose arithmetic runs on a native handle built from its ``state_dict``.

    A family supplies ``_destroy_symbol``, ``_create_handle(flat)`` (config struct + its ``pita_*_create``; called with
    the target device current), ``_conditions_on_beta()`` and, where something besides the weights shapes the handle,
    ``_key_extra()``."""

    _destroy_symbol = None

    def __init__(self):
        super().__init__()
        self._handle = None
        self._handle_key = None

    # ------------------------------------------------------------------ native handle
    def _create_handle(self, flat):
        raise NotImplementedError

    def _conditions_on_beta(self):
        raise NotImplementedError

    def _key_extra(self):
        return ()

    def _native(self, device):
        # cheap staleness check on every call: (storage pointer, version counter) of every parameter/buffer
        tensors = self.__dict__.get("_tensor_list")
        if tensors is None:
            tensors = self.__dict__["_tensor_list"] = list(self.parameters()) + list(self.buffers())
        key = (device.index,) + self._key_extra() + tuple((p.data_ptr(), p._version) for p in tensors)
        if self._handle is None or key != self._handle_key:
            self._release()
            params = list(self.state_dict().values())
            flat = torch.cat([p.detach().to("cpu", torch.float32).reshape(-1) for p in params]).contiguous().numpy()
            with torch.cuda.device(device):
                h = self._create_handle(flat)
            self._handle, self._handle_key = h, key
        return self._handle

    def __getstate__(self):
        """The native handle is a per-process device resource: copies / pickles start without one."""
        state = self.__dict__.copy()
        state["_handle"], state["_handle_key"] = None, None
        state.pop("_tensor_list", None)
        return state

    def _release(self):
        if self._handle is not None:
            getattr(lib(), self._destroy_symbol)(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ------------------------------------------------------------------ marshalling
    def _inputs(self, h_t, x_t, beta):
        """(h [B], x [B, D], b [B] or None) as contiguous fp32 device tensors; b is None unless the module conditions
        on beta, and then beta is required."""
        if not self._conditions_on_beta():
            beta = None
        elif beta is None:
            raise ValueError(f"{type(self).__name__} conditions on beta and was called with beta=None")
        x = dev_tensor(x_t, "x_t")
        B = x.shape[0]
        h = dev_tensor(h_t, "h_t").reshape(-1).expand(B).contiguous()
        return h, x, (None if beta is None else as_batch(beta, B, x.device))

    # ------------------------------------------------------------------ one body per C signature
    def _forward_call(self, symbol, t, xs, beta, out_dim=None):
        """pita_egnn_forward / pita_mlp_forward: out[B, out_dim or D] = backbone(t, xs, beta)."""
        t, xs, b = self._inputs(t, xs, beta)
        B, dev = xs.shape[0], xs.device
        out = torch.empty_like(xs) if out_dim is None else torch.empty(B, out_dim, device=dev, dtype=torch.float32)
        check(getattr(lib(), symbol)(self._native(dev), t.data_ptr(), xs.data_ptr(), ptr(b), out.data_ptr(), B,
                                     stream_ptr(dev)), symbol)
        return out

    def _edm_call(self, symbol, what, h_t, x_t, beta):
        """pita_egnn_edm / pita_egnn_wide_eval: what=0 the backbone itself, 1 the denoiser, 2 the score."""
        h, x, b = self._inputs(h_t, x_t, beta)
        dev = x.device
        out = torch.empty_like(x)
        check(getattr(lib(), symbol)(self._native(dev), int(what), h.data_ptr(), x.data_ptr(), ptr(b), out.data_ptr(),
                                     x.shape[0], stream_ptr(dev)), symbol)
        return out

    def _jvp_call(self, symbol, h_t, x_t, beta, vx, direction, vh, want_primal, want_tangent, dot_out, dot_col, diag_acc):
        """pita_egnn_jvp / pita_egnn_wide_jvp / pita_mlp_jvp -> (D or None, dD or None)."""
        h, x, b = self._inputs(h_t, x_t, beta)
        B, dev = x.shape[0], x.device
        if vx is not None:
            vx = dev_tensor(vx, "vx")
        if vh is not None:
            vh = dev_tensor(vh, "vh").reshape(-1).expand(B).contiguous()
        stride = 1
        if dot_out is not None:
            assert dot_out.is_cuda and dot_out.dtype == torch.float32 and dot_out.is_contiguous()
            stride = dot_out.shape[1] if dot_out.dim() == 2 else 1
        out = torch.empty_like(x) if want_primal else None
        dout = torch.empty_like(x) if want_tangent else None
        check(getattr(lib(), symbol)(self._native(dev), h.data_ptr(), x.data_ptr(), ptr(b), ptr(vx), int(direction),
                                     ptr(vh), ptr(out), ptr(dout), ptr(dot_out), stride, int(dot_col), ptr(diag_acc), B,
                                     stream_ptr(dev)), symbol)
        return out, dout

    def _vjp_call(self, symbol, h_t, x_t, beta, cot, want_primal, want_dot_h, want_h_parts):
        """pita_egnn_vjp / pita_egnn_wide_vjp_parts -> (D or None, J_x D^T cot[, dot_h[, parts]])."""
        if want_h_parts and not want_dot_h:
            raise ValueError("want_h_parts needs want_dot_h")
        h, x, b = self._inputs(h_t, x_t, beta)
        B, dev = x.shape[0], x.device
        if cot is not None:
            cot = dev_tensor(cot, "cot")
        out = torch.empty_like(x) if want_primal else None
        vjp = torch.empty_like(x)
        dot_h = torch.empty(B, device=dev) if want_dot_h else None
        parts = torch.empty(B, 2, device=dev) if want_h_parts else None
        check(getattr(lib(), symbol)(self._native(dev), h.data_ptr(), x.data_ptr(), ptr(b), ptr(cot), ptr(out),
                                     vjp.data_ptr(), ptr(dot_h), ptr(parts), B, stream_ptr(dev)), symbol)
        if want_h_parts:
            return out, vjp, dot_h, parts
        return (out, vjp, dot_h) if want_dot_h else (out, vjp)

    def _trace_call(self, symbol, h_t, x_t, beta, want_denoiser, device_guard=False):
        """pita_egnn_jacobian_trace / pita_egnn_wide_jacobian_trace -> (trace [B], D or None).  ``device_guard``: make
        x's device current around the call (the hidden-32 multi-direction entry points are called that way)."""
        h, x, b = self._inputs(h_t, x_t, beta)
        B, dev = x.shape[0], x.device
        net = self._native(dev)
        trace = torch.empty(B, device=dev)
        den = torch.empty_like(x) if want_denoiser else None
        with torch.cuda.device(dev) if device_guard else contextlib.nullcontext():
            check(getattr(lib(), symbol)(net, h.data_ptr(), x.data_ptr(), ptr(b), trace.data_ptr(), ptr(den), B,
                                         stream_ptr(dev)), symbol)
        return trace, den

    def _probes_call(self, symbol, h_t, x_t, beta, n_probes, probes, seed, walker_offset, step, want_denoiser,
                     want_per_probe, device_guard=False):
        """pita_egnn_trace_probes / pita_egnn_wide_trace_probes -> (estimate [B], D or None, per_probe [K, B] or None)."""
        h, x, b = self._inputs(h_t, x_t, beta)
        B, K, dev = x.shape[0], int(n_probes), x.device
        if probes is not None:
            probes = dev_tensor(probes, "probes")
            if tuple(probes.shape) != (K, B, x.shape[1]):
                raise ValueError(f"probes has shape {tuple(probes.shape)}, expected {(K, B, x.shape[1])}")
        est = torch.empty(B, device=dev)
        den = torch.empty_like(x) if want_denoiser else None
        per = torch.empty(max(K, 0), B, device=dev) if want_per_probe else None
        net = self._native(dev)
        with torch.cuda.device(dev) if device_guard else contextlib.nullcontext():
            check(getattr(lib(), symbol)(net, h.data_ptr(), x.data_ptr(), ptr(b), K, ptr(probes),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset), int(step), est.data_ptr(),
                                         ptr(per), ptr(den), B, stream_ptr(dev)), symbol)
        return est, den, per
