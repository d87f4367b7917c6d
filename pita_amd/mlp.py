"""MLP score backbones executed by the HIP MFMA kernel.

Mirror of ``MyMLP`` (pita/src/models/components/mlp.py:199-267) and ``MyMLPTemperature``
(:453-524): sinusoidal embedding of every input coordinate (scale 25), of time (and of beta),
Linear -> GELU, ``hidden_layers`` residual GELU blocks, Linear.  Same constructor arguments,
parameter names (``joint_mlp.N[.ff].{weight,bias}``) and creation order as the reference, so
seeded construction and checkpoints carry over.  The arithmetic is pita_amd/csrc/mlp_kernel.hip; the derivatives of
the EDM denoiser that the debiased regime needs (``jvp``, ``vjp``, ``jacobian_trace``) are csrc/mlp_jac_kernel.hip.
"""
import ctypes

import torch
from torch import nn

from . import _lib
from ._backbone import HipBackbone


class _Block(nn.Module):  # parameter holder for mlp.py:100-118 (x + GELU(ff(x)))
    def __init__(self, size):
        super().__init__()
        self.ff = nn.Linear(size, size)


class _HipMLP(HipBackbone):
    _temperature = False
    _destroy_symbol = "pita_mlp_destroy"

    def __init__(self, hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, time_emb="sinusoidal",
                 input_emb="sinusoidal", add_t_emb=False, concat_t_emb=False, input_dim=2, energy_function=None):
        super().__init__()
        if time_emb != "sinusoidal" or input_emb != "sinusoidal" or add_t_emb or concat_t_emb:
            raise NotImplementedError("HIP MLP implements the sinusoidal-embedding configuration of model/net/mlp.yaml")
        self.hidden_size, self.hidden_layers, self.emb_size = hidden_size, hidden_layers, emb_size
        self.input_dim, self.out_dim = input_dim, out_dim
        concat = emb_size * (input_dim + 1 + (1 if self._temperature else 0))
        layers = [nn.Linear(concat, hidden_size)]
        layers += [_Block(hidden_size) for _ in range(hidden_layers)]
        layers.append(nn.Linear(emb_size, out_dim))  # sized by emb_size like the reference (mlp.py:238-239)
        self.joint_mlp = nn.Sequential(*layers)

    def _freqs(self):
        half = self.emb_size // 2  # the reference's fp32 torch ops (mlp.py:19-21)
        w = torch.log(torch.Tensor([10000.0])) / (half - 1)
        return torch.exp(-w * torch.arange(half)).contiguous()

    def _create_handle(self, flat):
        fr = self._freqs().numpy()
        cfg = _lib.MlpConfig(self.input_dim, self.out_dim, self.hidden_size, self.hidden_layers, self.emb_size,
                             int(self._temperature))
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().pita_mlp_create(ctypes.byref(h), ctypes.byref(cfg), flat.ctypes.data_as(ctypes.c_void_p),
                                              flat.size, fr.ctypes.data_as(ctypes.c_void_p)), "pita_mlp_create")
        return h

    def _conditions_on_beta(self):
        return self._temperature

    # ------------------------------------------------------------------ derivatives of the EDM denoiser (debiased regime)
    # Same contracts as EGNN_dynamics.jvp / vjp / jacobian_trace; one launch each (csrc/mlp_jac_kernel.hip).
    def jvp(self, h_t, x_t, beta, vx=None, direction=-1, vh=None, want_primal=True, want_tangent=True, dot_out=None,
            dot_col=0, diag_acc=None):
        """(D, dD): the denoiser D_theta(h, x) and its forward-mode derivative along ONE tangent direction:
        dD = J_x D . vx + dD/dh . vh.  ``vx``: [B, D] tensor, or None for the unit direction ``direction`` of
        every walker (-1 = zero).  ``vh``: [B] tensor or None.  Optional in-kernel reductions:
        ``dot_out[:, dot_col] = <x, dD>`` and ``diag_acc += dD[:, direction]`` (pita_mlp_jvp)."""
        return self._jvp_call("pita_mlp_jvp", h_t, x_t, beta, vx, direction, vh, want_primal, want_tangent, dot_out,
                              dot_col, diag_acc)

    def jacobian(self, h_t, x_t, beta, cot=None, want_denoiser=False, want_trace=False, want_vjp=False,
                 want_dot_h=False, want_h_parts=False):
        """Every requested derivative of D_theta(h, x) from ONE launch of pita_mlp_jacobian, as a dict with the keys
        ``D`` [B, D], ``trace`` [B], ``vjp`` = J_x D^T cot [B, D], ``dot_h`` = <cot, dD/dh> [B] and ``h_parts`` [B, 2]
        (``cot`` default: x)."""
        h_t, x_t, b = self._inputs(h_t, x_t, beta)
        B = x_t.shape[0]
        if cot is not None:
            cot = _lib.dev_tensor(cot, "cot")
        dev = x_t.device
        res = {"D": torch.empty_like(x_t) if want_denoiser else None,
               "trace": torch.empty(B, device=dev) if want_trace else None,
               "vjp": torch.empty_like(x_t) if want_vjp else None,
               "dot_h": torch.empty(B, device=dev) if want_dot_h else None,
               "h_parts": torch.empty(B, 2, device=dev) if want_h_parts else None}
        _lib.check(_lib.lib().pita_mlp_jacobian(self._native(dev), h_t.data_ptr(), x_t.data_ptr(), _lib.ptr(b),
                                                _lib.ptr(cot), _lib.ptr(res["D"]), _lib.ptr(res["trace"]),
                                                _lib.ptr(res["vjp"]), _lib.ptr(res["dot_h"]), _lib.ptr(res["h_parts"]),
                                                B, _lib.stream_ptr(dev)), "pita_mlp_jacobian")
        return res

    def jacobian_trace(self, h_t, x_t, beta, want_denoiser=False):
        """trace(J_x D_theta(h, x)) per walker, exactly, over all D unit directions (one launch; the tangents share
        the primal's weight stream).  ``want_denoiser``: also return D_theta(h, x) -> (trace, D)."""
        r = self.jacobian(h_t, x_t, beta, want_denoiser=want_denoiser, want_trace=True)
        return (r["trace"], r["D"]) if want_denoiser else r["trace"]

    vjp_h_parts = True  # vjp(..., want_h_parts=True) is available

    def vjp(self, h_t, x_t, beta, cot=None, want_primal=True, want_dot_h=False, want_h_parts=False):
        """(D, J_x D^T cot) for a per-walker cotangent (default: x_t), assembled in-kernel from the D unit tangents:
        (J^T cot)_k = <cot, J e_k>.  ``want_dot_h``: also <cot, dD/dh> [B] -> (D, vjp, dot_h).  ``want_h_parts`` (with
        want_dot_h): also [B, 2] = (c_out <cot, F>, <cot, d(c_out F)/dh>) -> (D, vjp, dot_h, parts); the contract
        of EGNN_dynamics.vjp."""
        if want_h_parts and not want_dot_h:
            raise ValueError("want_h_parts needs want_dot_h")
        r = self.jacobian(h_t, x_t, beta, cot=cot, want_denoiser=want_primal, want_vjp=True, want_dot_h=want_dot_h,
                          want_h_parts=want_h_parts)
        if want_h_parts:
            return r["D"], r["vjp"], r["dot_h"], r["h_parts"]
        return (r["D"], r["vjp"], r["dot_h"]) if want_dot_h else (r["D"], r["vjp"])

    def sampler_run(self, x, step_tab, n_steps, noise=None, seed=0, walker_offset=0, step0=0, remove_mean=True,
                    drift_out=None, n_particles=None, n_dim=None, stats_out=None):
        """In-place fused Euler-Maruyama steps (pita_mlp_sampler_run); x: [B, D] device tensor.  Geometry defaults to
        one "particle" of dimension D (the GMM convention of the integrator)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        assert step_tab.is_cuda and step_tab.dtype == torch.float32 and step_tab.is_contiguous()
        if drift_out is not None:
            raise NotImplementedError("MLP fused sampler: drift_out is not provided (use the per-step path)")
        if stats_out is not None:
            assert stats_out.is_cuda and stats_out.dtype == torch.float64 and stats_out.is_contiguous()
        D = x.shape[1]
        n, d = (1, D) if n_particles is None else (int(n_particles), int(n_dim))
        _lib.check(_lib.lib().pita_mlp_sampler_run(
            self._native(x.device), x.data_ptr(), x.shape[0], step_tab.data_ptr(), int(n_steps), _lib.ptr(noise),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset), int(step0), int(bool(remove_mean)), n, d,
            _lib.ptr(stats_out), _lib.stream_ptr(x.device)), "pita_mlp_sampler_run")
        return x

    def can_fuse(self, n_particles, n_dim):
        D = n_particles * n_dim
        return self.input_dim == D and self.out_dim == D and D <= 64 and n_dim <= 4


class MyMLP(_HipMLP):
    def forward(self, t, x, x_self_cond=False):
        """The third positional argument swallows beta exactly like the reference (mlp.py:244)."""
        return self._forward_call("pita_mlp_forward", t, x, None, out_dim=self.out_dim)


class MyMLPTemperature(_HipMLP):
    _temperature = True

    def forward(self, t, x, beta):
        return self._forward_call("pita_mlp_forward", t, x, beta, out_dim=self.out_dim)

