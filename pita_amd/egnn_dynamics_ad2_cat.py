"""EGNN backbone of the alanine-dipeptide class (hidden 64 x 5 layers, one-hot atom-type node features) on the HIP
kernels of ``pita_egnn_wide_eval``: the matrix-pipe kernel for 22 / 33 / 42 / 13 / 55 particles, the vector-pipe kernel
for every other shape.

Mirror of ``EGNN_dynamics_AD2_cat`` (pita/src/models/components/egnn_dynamics_ad2_cat.py:11-203; the ``_target_`` of
``configs/model/net/egnn_dynamics_ad2_cat.yaml``): same constructor arguments and defaults, same parameter names and
creation order (``egnn.embedding``, ``egnn.embedding_out``, ``egnn.gcl_<l>.{edge_mlp,node_mlp,coord_mlp,att_mlp}``: a
seeded construction gives the reference's weights and its ``state_dict`` loads unchanged), same
``forward(t, xs, beta) -> vel`` contract.  Node features are ``[h_initial (static one-hot rows), t, beta]`` (:157-184);
the arithmetic of ``EGNN.forward`` / ``E_GCL`` (egnn.py:108-346) lives in pita_amd/csrc/egnn_wide_mfma_kernel.hip and
pita_amd/csrc/egnn_wide_kernel.hip (``pita_egnn_wide_eval``).  ``edm`` lets ``ScoreNet`` evaluate the EDM preconditioning in the same launch.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._backbone import HipBackbone
from .egnn_temp_conditioned import EGNN


class EGNN_dynamics_AD2_cat(HipBackbone):
    def __init__(self, n_particles, n_dimensions, hidden_nf=64, act_fn=torch.nn.SiLU(), n_layers=5, recurrent=True,
                 attention=True, tanh=True, atom_encoding_filename="atom_types_ecoding.npy", data_dir="data/alanine",
                 pdb_filename="", agg="sum", M=128, condition_beta=False, h_initial=None):
        super().__init__()
        self._n_particles, self._n_dimensions = n_particles, n_dimensions
        if h_initial is None:
            h_initial = self.get_h_initial()
        self.h_initial = torch.as_tensor(h_initial)
        self.condition_beta = condition_beta
        h_size = self.h_initial.size(1) + 1 + (1 if condition_beta else 0)  # :44-49
        self.egnn = EGNN(in_node_nf=h_size, in_edge_nf=1, hidden_nf=hidden_nf, act_fn=act_fn, n_layers=n_layers,
                         recurrent=recurrent, attention=attention, tanh=tanh, agg=agg)
        self.counter = 0
        self.M = M

    def get_h_initial(self):
        """The static node features of :66-92 for the particle counts that need no topology file."""
        n = self._n_particles
        groups = {22: [([0, 2, 3], 2), ([19, 20, 21], 20), ([11, 12, 13], 12)],
                  33: [([1, 2, 3], 2), ([9, 10, 11], 10), ([19, 20, 21], 18), ([29, 30, 31], 31)],
                  42: [([1, 2, 3], 2), ([11, 12, 13], 12), ([21, 22, 23], 22), ([31, 32, 33], 32), ([39, 40, 41], 40)]}
        if n in groups:
            atom_types = np.arange(n)
            for idx, v in groups[n]:
                atom_types[idx] = v
            return torch.nn.functional.one_hot(torch.tensor(atom_types))
        if n in (13, 55):
            return torch.zeros(n, 1)
        raise NotImplementedError(
            f"EGNN_dynamics_AD2_cat: the node features of {n} particles come from a topology file (mdtraj, :94-155); "
            "pass h_initial=[n_particles, n_features] instead")

    # ------------------------------------------------------------------ native handle (lifetime: HipBackbone)
    _destroy_symbol = "pita_egnn_wide_destroy"

    def _config(self):
        e = self.egnn
        return _lib.EgnnWideConfig(self._n_particles, self._n_dimensions, e.hidden_nf, e.n_layers,
                                   int(self.h_initial.size(1)), int(bool(self.condition_beta)), int(e.attention),
                                   int(e.tanh), e.coords_range)

    def _create_handle(self, flat):
        h0 = np.ascontiguousarray(self.h_initial.detach().to("cpu", torch.float32).numpy())
        cfg, h = self._config(), ctypes.c_void_p()
        _lib.check(_lib.lib().pita_egnn_wide_create(ctypes.byref(h), ctypes.byref(cfg), flat.ctypes.data_as(ctypes.c_void_p),
                                                    flat.size, h0.ctypes.data_as(ctypes.c_void_p)), "pita_egnn_wide_create")
        return h

    def _conditions_on_beta(self):
        return self.condition_beta

    def uses_matrix_pipe(self, device):
        """True when evaluations on ``device`` run on the MFMA kernel (the instantiated particle counts, unless
        PITA_WIDE_NO_MFMA is set)."""
        return bool(_lib.lib().pita_egnn_wide_uses_matrix_pipe(self._native(torch.device(device))))

    def jvp_uses_matrix_pipe(self, device):
        """True when ``jvp`` / ``jacobian_trace`` on ``device`` run on the forward-mode MFMA kernel (22 / 33 / 42
        particles, unless PITA_WIDE_NO_MFMA is set); the vector-pipe kernel alone computes them otherwise."""
        return bool(_lib.lib().pita_egnn_wide_jvp_uses_matrix_pipe(self._native(torch.device(device))))

    def vjp_uses_matrix_pipe(self, device):
        """True when ``vjp`` on ``device`` runs its reverse-mode sweep on the MFMA kernel (22 / 33 / 42 particles, unless
        PITA_WIDE_NO_MFMA is set); the vector-pipe kernel alone computes it otherwise."""
        return bool(_lib.lib().pita_egnn_wide_vjp_uses_matrix_pipe(self._native(torch.device(device))))

    # ------------------------------------------------------------------ reference interface
    def forward(self, t, xs, beta=None):
        """vel[B, n*d] = backbone(t[B], xs[B, n*d], beta[B]); mean-free (:157-203)."""
        self.counter += 1
        return self._edm_call("pita_egnn_wide_eval", 0, t, xs, beta)

    def edm(self, what, h_t, x_t, beta):
        """what=1: denoiser D_theta, what=2: score (D_theta - x)/h, EDM preconditioning fused (score_net.py:13-43)."""
        return self._edm_call("pita_egnn_wide_eval", what, h_t, x_t, beta)

    def can_fuse(self, n_particles, n_dim):
        return int(n_particles) == self._n_particles and int(n_dim) == self._n_dimensions

    def sampler_run(self, x, step_tab, n_steps, noise=None, seed=0, walker_offset=0, step0=0, remove_mean=True,
                    drift_out=None, n_particles=None, n_dim=None, stats_out=None):
        """In-place fused Euler-Maruyama steps of the not-debiased reverse SDE (pita_egnn_wide_sampler_run): the whole
        stretch between two resampling events in ONE launch, like ``EGNN_dynamics.sampler_run``; x: [B, n*d] device
        tensor, ``step_tab`` from ``sde_integration.build_step_table`` (its beta column conditions the net)."""
        if drift_out is not None:
            raise NotImplementedError("EGNN_dynamics_AD2_cat.sampler_run: drift_out")
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if stats_out is not None:
            assert stats_out.is_cuda and stats_out.dtype == torch.float64 and stats_out.is_contiguous()
            assert stats_out.numel() >= 4 * int(n_steps)
        assert step_tab.is_cuda and step_tab.dtype == torch.float32 and step_tab.is_contiguous()
        _lib.check(_lib.lib().pita_egnn_wide_sampler_run(
            self._native(x.device), x.data_ptr(), x.shape[0], step_tab.data_ptr(), int(n_steps), _lib.ptr(noise),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset), int(step0), int(bool(remove_mean)), _lib.ptr(stats_out),
            _lib.stream_ptr(x.device)), "pita_egnn_wide_sampler_run")
        return x

    def jvp(self, h_t, x_t, beta, vx=None, direction=-1, vh=None, want_primal=True, want_tangent=True, dot_out=None,
            dot_col=0, diag_acc=None):
        """(D, dD): the EDM denoiser around this backbone and its forward-mode derivative along ONE direction,
        dD = J_x D . vx + dD/dh . vh -- same contract as ``EGNN_dynamics.jvp`` (pita_egnn_wide_jvp: the matrix-pipe
        kernel where ``jvp_uses_matrix_pipe``, the fp32 vector-pipe kernel otherwise).  With it ``VEReverseSDE(debias_inference=True)`` runs on this backbone: the exact divergence of the
        score (utils.py:30-51), grad_x E_theta (energy_net.py:51-62) and dE_theta/dt (sdes.py:218) are assembled from
        dim + 1 such launches per net (sdes.py's forward-mode path)."""
        return self._jvp_call("pita_egnn_wide_jvp", h_t, x_t, beta, vx, direction, vh, want_primal, want_tangent, dot_out,
                              dot_col, diag_acc)

    def jacobian_trace(self, h_t, x_t, beta, want_denoiser=False):
        """(trace, D or None): trace(J_x D_theta(h, x)) per walker, exactly, over all n*d unit directions, and with
        ``want_denoiser`` D_theta(h, x) -- ONE call (pita_egnn_wide_jacobian_trace: one launch over (walker, direction)
        pairs and a reduction) with the bits of the n*d ``jvp(direction=k, diag_acc=trace)`` launches it replaces.
        ``VEReverseSDE._score_divergence_terms`` takes it for the exact divergence of the score (utils.py:30-51)."""
        return self._trace_call("pita_egnn_wide_jacobian_trace", h_t, x_t, beta, want_denoiser)

    def jacobian_trace_estimate(self, h_t, x_t, beta, n_probes, probes=None, seed=0, walker_offset=0, step=0,
                                want_denoiser=False, want_per_probe=False):
        """(estimate, D or None, per_probe or None): the Hutchinson estimate of trace(J_x D_theta(h, x)) per walker from
        ``n_probes`` probes, mean_k <v_k, J_x D v_k> (the estimator beside ``compute_divergence_exact`` in the
        reference's utils.py) -- ONE call (pita_egnn_wide_trace_probes: one launch over (walker, probe) pairs and a
        reduction), each pair computed as ``jvp(vx=v_k)`` computes it.  ``probes`` [K, B, n*d]: the tangent inputs
        (parity hook); None: Rademacher signs drawn in the kernel, keyed (seed, walker_offset + row, step) like the
        samplers' noise -- what ``pita_amd.utils.rademacher_probes`` returns for the same key (K <= 256).
        ``want_per_probe``: also the [K, B] quadratic forms.  ``VEReverseSDE(divergence="hutchinson")`` takes it."""
        return self._probes_call("pita_egnn_wide_trace_probes", h_t, x_t, beta, n_probes, probes, seed, walker_offset, step,
                                 want_denoiser, want_per_probe)

    vjp_h_parts = True  # vjp(..., want_h_parts=True) is available

    def vjp(self, h_t, x_t, beta, cot=None, want_primal=True, want_dot_h=False, want_h_parts=False):
        """(D, J_x D^T cot[, <cot, dD/dh>]): the EDM denoiser around this backbone and its reverse-mode derivative for a
        per-walker cotangent (default: x_t itself) from ONE launch (pita_egnn_wide_vjp_parts) -- same contract as
        ``EGNN_dynamics.vjp``; ``EnergyNet.forward`` and the debiased drift use it instead of dim + 1 ``jvp`` launches.
        ``want_h_parts`` (with want_dot_h): also [B, 2] = (c_out <cot, F>, <cot, d(c_out F)/dh>), the split of the same
        derivative that pita_fk_assemble turns into E_theta and dE_theta/dh without cancellation at small h
        -> (D, vjp, dot_h, parts)."""
        return self._vjp_call("pita_egnn_wide_vjp_parts", h_t, x_t, beta, cot, want_primal, want_dot_h, want_h_parts)
