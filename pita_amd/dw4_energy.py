"""DW4-style multi double-well target (BASELINE config C2) on the HIP pairwise kernel.

The reference tree has no DW4 energy (only the dead import
pita/src/energies/base_datamodule.py:13 of ``bgflow.MultiDoubleWellPotential``); this class gives
it the same plug-in shape as LennardJonesEnergy.  E = sum_{i<j} a (d-d0)^4 + b (d-d0)^2 + c,
defaults a=0.9, b=-4, c=0, d0=4 (the DEM/bgflow DW4 parameters).  Parity is pinned only
against the oracle's own restatement.
"""
import torch

from ._target import PAIR_MALA_WORKSPACE, HipTarget
from .base_energy_function import BaseMoleculeEnergy


class MultiDoubleWellEnergy(HipTarget, BaseMoleculeEnergy):
    def __init__(self, dimensionality=8, n_particles=4, spatial_dim=2, data_path=None, device="cuda", a=0.9, b=-4.0,
                 c=0.0, offset=4.0, is_molecule=True, temperature=1.0, should_normalize=False,
                 data_normalization_factor=1.0, *args, **kwargs):
        self.name = f"DW{n_particles}"
        super().__init__(dimensionality=dimensionality, n_particles=n_particles, spatial_dim=spatial_dim,
                         data_path=data_path, data_name="DW", device=device, is_molecule=is_molecule,
                         temperature=temperature, should_normalize=should_normalize,
                         data_normalization_factor=data_normalization_factor)
        self.a, self.b, self.c, self.offset = float(a), float(b), float(c), float(offset)

    def _pair_args(self):
        """n, d, temperature, a, b, c, d0 of the pita_dw_* entry points."""
        return (self.n_particles, self.n_spatial_dim, float(self.temperature), self.a, self.b, self.c, self.offset)

    def __call__(self, samples: torch.Tensor, return_force=False):
        return self._logp_force_call("pita_dw_logp_force", self._samples(samples, self.should_normalize),
                                     *self._pair_args(), return_force=return_force)

    def fused_descent(self, x, num_steps, dt, noise_scale, sqrt_dt, seed=0, walker_offset=0, step0=0, remove_mean=True,
                      noise=None):
        """See LennardJonesEnergy.fused_descent and the table in _target.py."""
        if self.should_normalize:
            return None
        return self._descent_call("pita_dw_descent", x, noise, self._pair_args(), num_steps, dt, noise_scale, sqrt_dt, seed,
                                  walker_offset, step0, remove_mean)

    def fused_mala(self, x, logp, num_steps, dt_dev, adaptive, total, noise=None, uniforms=None, seed=0, walker_offset=0,
                   walker_ids=None, step0=0, remove_mean=True, rates_out=None):
        """See LennardJonesEnergy.fused_mala and the table in _target.py (pita_dw_mala: the DW4 ring kernel)."""
        if self.should_normalize or self.n_particles != 4 or self.n_spatial_dim != 2:
            return None
        return self._mala_call("pita_dw_mala", PAIR_MALA_WORKSPACE, x, logp, self._pair_args(), num_steps, dt_dev, adaptive,
                               total, noise, uniforms, seed, walker_offset, walker_ids, step0, remove_mean, rates_out)
