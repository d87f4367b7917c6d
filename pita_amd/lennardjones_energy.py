"""Lennard-Jones cluster target evaluated by the HIP pairwise kernel.

Mirror of ``LennardJonesEnergy`` (pita/src/energies/lennardjones_energy.py:158-227): same
constructor arguments, ``__call__(samples, return_force=False)`` returns the detached
log-density (and analytic force instead of autograd).  The arithmetic of
``LennardJonesPotential._energy`` (:121-146) + bgflow's ``distances_from_vectors`` is in
pita_amd/csrc/energy_kernels.hip (pita_lj_logp_force).
"""
import ctypes

import numpy as np
import torch

from ._target import PAIR_MALA_WORKSPACE, HipTarget
from .base_energy_function import BaseMoleculeEnergy


def smooth_core_coefficients(range_min=0.65, range_max=2.0, interpolation=1000, eps=1.0, rm=1.0):
    """The four coefficients (float32, highest power first) of the cubic the reference uses below ``range_min`` when
    ``smooth=True``: first interval of scipy's CubicSpline through the LJ curve sampled on
    ``torch.linspace(range_min, range_max, interpolation)`` in float32 (LennardJonesPotential.__init__,
    lennardjones_energy.py:114-119); ``cubic_spline`` (:39-54) clamps every r < range_min to that interval."""
    from scipy.interpolate import CubicSpline  # the reference's own dependency for this option
    pts = torch.linspace(range_min, range_max, interpolation)
    es = eps * ((rm / pts) ** 12 - 2 * (rm / pts) ** 6)
    c = CubicSpline(pts.numpy(), es.numpy()).c
    return np.ascontiguousarray(torch.tensor(c).float().numpy()[:, 0]), float(pts[0])


class LennardJonesEnergy(HipTarget, BaseMoleculeEnergy):
    def __init__(self, dimensionality, n_particles, spatial_dim, data_path=None, device="cuda",
                 plot_samples_epoch_period=5, plotting_buffer_sample_size=512, energy_factor=1.0, is_molecule=True,
                 smooth=False, temperature=1.0, should_normalize=False, data_normalization_factor=1.0,
                 dist_eps=1e-6, *args, **kwargs):
        if n_particles not in (13, 55):  # lennardjones_energy.py:177-182
            raise NotImplementedError("LennardJonesEnergy: the reference defines LJ13 and LJ55 only")
        self.name = "LJ13_efm" if n_particles == 13 else "LJ55"
        super().__init__(dimensionality=dimensionality, n_particles=n_particles, spatial_dim=spatial_dim,
                         data_path=data_path, data_name="LJ", device=device, is_molecule=is_molecule,
                         temperature=temperature, should_normalize=should_normalize,
                         data_normalization_factor=data_normalization_factor)
        self.energy_factor = float(energy_factor)
        self.dist_eps = float(dist_eps)  # bgflow distances_from_vectors eps
        self.smooth = bool(smooth)
        if self.smooth:  # LennardJonesPotential defaults: range_min=0.65, range_max=2.0, interpolation=1000
            self._smooth_coef, self._smooth_min = smooth_core_coefficients()
        self.plot_samples_epoch_period = plot_samples_epoch_period
        self.plotting_buffer_sample_size = plotting_buffer_sample_size

    def _pair_args(self):
        """n, d, temperature, energy_factor, dist_eps, eps, rm, osc_scale of the pita_lj_* entry points."""
        return (self.n_particles, self.n_spatial_dim, float(self.temperature), self.energy_factor, self.dist_eps, 1.0, 1.0,
                1.0)

    def __call__(self, samples: torch.Tensor, return_force=False):
        x = self._samples(samples, self.should_normalize)
        if self.smooth:
            return self._logp_force_call("pita_lj_smooth_logp_force", x, *self._pair_args(), self._smooth_min,
                                         self._smooth_coef.ctypes.data_as(ctypes.c_void_p), return_force=return_force)
        return self._logp_force_call("pita_lj_logp_force", x, *self._pair_args(), return_force=return_force)

    def fused_descent(self, x, num_steps, dt, noise_scale, sqrt_dt, seed=0, walker_offset=0, step0=0, remove_mean=True,
                      noise=None):
        """The fused descent of the table in _target.py (pita_lj_descent; negative_time_descent, sde_integration.py:353-360)."""
        if self.should_normalize or self.smooth:  # the fused kernels know the plain LJ curve only
            return None
        return self._descent_call("pita_lj_descent", x, noise, self._pair_args(), num_steps, dt, noise_scale, sqrt_dt, seed,
                                  walker_offset, step0, remove_mean)

    def fused_mala(self, x, logp, num_steps, dt_dev, adaptive, total, noise=None, uniforms=None, seed=0, walker_offset=0,
                   walker_ids=None, step0=0, remove_mean=True, rates_out=None):
        """The fused MALA chain of the table in _target.py (pita_lj_mala; metropolis_hastings_mala(_adaptive),
        sde_integration.py:362-470).  LJ13 and LJ55 have fused chains, on plain (not normalised, not smooth) coordinates."""
        if self.should_normalize or self.smooth or self.n_particles not in (13, 55) or self.n_spatial_dim != 3:
            return None
        return self._mala_call("pita_lj_mala", PAIR_MALA_WORKSPACE, x, logp, self._pair_args(), num_steps, dt_dev, adaptive,
                               total, noise, uniforms, seed, walker_offset, walker_ids, step0, remove_mean, rates_out)
