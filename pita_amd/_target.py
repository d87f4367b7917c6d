"""What the HIP targets share: one Python body per C call shape of the target entry points (log-density + force, fused
descent, fused MALA chain), each allocating its outputs, making the tensor's device current, masking the seed to 64 bits
and checking the return code.

The protocol between a target and ``WeightedSDEIntegrator`` (sde_integration.py).  The integrator probes with ``hasattr`` /
``getattr`` and takes the fused route where it finds one; a target offers a route by having the attribute, so the shared
bodies below are private (``_..._call``) and each class names only the routes its library entry points serve.  ``x``
[B, D] contiguous fp32 on the device, D = n_particles * n_spatial_dim.  lj = ``LennardJonesEnergy``, dw =
``MultiDoubleWellEnergy``, ff = ``ForceFieldEnergy`` / ``ALPEnergy`` (which inherits both fused routes), gmm = ``GMM``.

==========================  ==========================================================================  ============
attribute                   what the integrator expects                                                 offered by
==========================  ==========================================================================  ============
``__call__(samples,         log-density [B] = -E/T, detached; with ``return_force=True`` the pair        lj dw ff gmm
return_force=False)``       (logp [B], force [B, D] = d logp / dx).  Required (no probe); changes
                            nothing in place
``is_molecule``             truthy: MALA centres the walkers (``remove_mean``); absent or false: it      lj dw ff gmm
                            does not
``n_particles``,            the geometry of the per-step kernels and of the Philox keys; absent or       lj dw ff
``n_spatial_dim``           None: one "particle" of dimension D
``fused_descent(x,          all ``num_steps`` of x <- remove_mean(x + F dt + noise_scale sqrt_dt xi)     lj dw ff
num_steps, dt,              in one launch, IN PLACE on ``x``; ``noise`` [num_steps, B, D] or None
noise_scale, sqrt_dt,       (then Philox keyed by seed, walker_offset + row, step0 + step).  Returns
seed=0, walker_offset=0,    ``x`` when it ran; None means "not mine" (normalised coordinates, the
step0=0, remove_mean=True,  smooth LJ core): nothing was changed and the integrator runs the per-step
noise=None)``               path, which gives the same bits.  Absent: the per-step path
``fused_mala(x, logp,       the whole chain of ``num_steps`` MALA steps in fused launches (one for a     lj dw ff
num_steps, dt_dev,          non-adaptive chain, one per step for an adaptive one), IN PLACE on ``x``
adaptive, total,            [B, D], ``logp`` [B] (log-density of x on entry and on return), ``dt_dev``
noise=None, uniforms=None,  (fp64 [1]: step size in, final step size out) and ``rates_out`` (fp32
seed=0, walker_offset=0,    [>= num_steps]: acceptance rate per step).  ``total`` is the walker count
walker_ids=None, step0=0,   the rates are taken over; ``walker_ids`` (int64 [B] or None) are the Philox
remove_mean=True,           keys of compacted batches.  Returns ``x`` when it ran; None means "not
rates_out=None)``           mine" (no fused chain for this geometry or plan, PITA_EUNSUPPORTED from the
                            library included): nothing was changed and the integrator runs the
                            launch-per-kernel chain, which gives the same bits.  Absent: that chain.
                            ``total`` may instead be a ``MalaPopulations`` record: the chain then keeps
                            one step size, count and adaptation per population (the ``_pop`` entry
                            points), ``dt_dev`` is fp64 [P] and ``rates_out`` fp32 [>= num_steps, P]
==========================  ==========================================================================  ============
"""
import collections
import contextlib

import torch

from ._lib import PITA_EUNSUPPORTED, check, dev_tensor, lib, ptr, stream_ptr

_U64 = 0xFFFFFFFFFFFFFFFF
# The workspace of every fused chain is sized by one native function (pair_common.h: mala_workspace_bytes) behind two
# exports; the pair targets (lj, dw) take this one, the force field its own pita_ff_mala_workspace_bytes.
PAIR_MALA_WORKSPACE = "pita_lj_mala_workspace_bytes"
# ... and the per-population chains of every target this one, of (steps, populations)
POP_MALA_WORKSPACE = "pita_mala_pop_workspace_bytes"
_SAME_DEVICE = contextlib.nullcontext()

# ``total`` of a per-population chain: populations of ``size`` consecutive Philox walker keys from key ``base`` on (the
# key of the first row of the call's first population); ``totals``: int64 [P] on the device, the rows of each population
# in the call.  Row w belongs to population (key(w) - base) // size, which the caller keeps in [0, P).
MalaPopulations = collections.namedtuple("MalaPopulations", "size base totals")


def _device_guard(device):
    """``device`` current around a library call (the per-device caches and the launch follow the current device, not the
    tensor's): torch's context manager when another device is current, nothing to enter when it already is -- these
    bodies run once per launch, and the target kernels are launches of a few microseconds."""
    return _SAME_DEVICE if device.index == torch.cuda.current_device() else torch.cuda.device(device)


def _check_populations(pops, steps, dt_dev, rates_out):
    """The shapes a per-population chain writes through: P, or ValueError before anything reaches the library."""
    t = pops.totals
    if t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 1 or not t.is_contiguous():
        raise ValueError("MalaPopulations.totals must be a contiguous int64 [P] tensor, P >= 1")
    P = t.numel()
    if int(pops.size) < 1 or int(pops.base) < 0:
        raise ValueError(f"MalaPopulations: size >= 1 and base >= 0, got size {pops.size}, base {pops.base}")
    if dt_dev.dtype != torch.float64 or dt_dev.numel() != P or not dt_dev.is_contiguous():
        raise ValueError(f"per-population chain: dt_dev must be fp64 [{P}], got {dt_dev.dtype} {tuple(dt_dev.shape)}")
    if rates_out is not None and (rates_out.dtype != torch.float32 or rates_out.dim() != 2 or rates_out.shape[1] != P or
                                  rates_out.shape[0] < steps or not rates_out.is_contiguous()):
        raise ValueError(f"per-population chain: rates_out must be fp32 [>= {steps}, {P}], got {rates_out.dtype} "
                         f"{tuple(rates_out.shape)}")
    return P


class HipTarget:
    """Mix-in of the targets evaluated by libpita_hip.so.  A class with a native handle (the force field) overrides
    ``_native()``; it is called with the tensor's device current and its result leads the C argument list."""

    def _native(self):
        return None

    def _handle_args(self):
        h = self._native()
        return () if h is None else (h,)

    def _samples(self, samples, unnormalize=False):
        """``samples`` as a contiguous fp32 [B, D] device tensor in the units of the kernel."""
        x = dev_tensor(samples, "samples")
        if unnormalize:
            x = self.unnormalize(x)
        return x.reshape(-1, self._dimensionality)

    # ------------------------------------------------------------------ one body per C call shape
    def _logp_force_call(self, symbol, x, *args, return_force=False):
        """pita_{lj,lj_smooth,dw,gmm,ff}_logp_force([handle,] x, logp, force, B, *args, stream) -> logp or (logp, force)."""
        B = x.shape[0]
        logp = torch.empty(B, device=x.device, dtype=torch.float32)
        force = torch.empty_like(x) if return_force else None
        with _device_guard(x.device):
            check(getattr(lib(), symbol)(*self._handle_args(), x.data_ptr(), logp.data_ptr(), ptr(force), B, *args,
                                         stream_ptr(x.device)), symbol)
        return (logp, force) if return_force else logp

    def _descent_call(self, symbol, x, noise, head_args, num_steps, dt, noise_scale, sqrt_dt, seed, walker_offset, step0,
                      remove_mean):
        """pita_{lj,dw,ff}_descent([handle,] x, noise, B, *head_args, steps, dt, ..., stream) -> x, advanced in place."""
        with _device_guard(x.device):
            check(getattr(lib(), symbol)(*self._handle_args(), x.data_ptr(), ptr(noise), x.shape[0], *head_args,
                                         int(num_steps), float(dt), float(noise_scale), float(sqrt_dt), int(seed) & _U64,
                                         int(walker_offset), int(step0), int(bool(remove_mean)), stream_ptr(x.device)),
                  symbol)
        return x

    def _mala_call(self, symbol, workspace_symbol, x, logp, head_args, num_steps, dt_dev, adaptive, total, noise, uniforms,
                   seed, walker_offset, walker_ids, step0, remove_mean, rates_out):
        """pita_{lj,dw,ff}_mala([handle,] x, logp, noise, uniforms, B, *head_args, steps, dt_dev, ..., workspace, stream)
        -> x, or None when the library answers PITA_EUNSUPPORTED.  ``total``: the walker count, or a ``MalaPopulations``
        record -- then the call goes to ``symbol + "_pop"`` with (totals, P, size, base) in the place of the count."""
        L = lib()
        steps = int(num_steps)
        if isinstance(total, MalaPopulations):
            P = _check_populations(total, steps, dt_dev, rates_out)
            symbol, ws_bytes = symbol + "_pop", getattr(L, POP_MALA_WORKSPACE)(steps, P)
            over = (total.totals.data_ptr(), P, int(total.size), int(total.base))
        else:
            ws_bytes, over = getattr(L, workspace_symbol)(steps), (int(total),)
        ws = torch.empty((int(ws_bytes) + 7) // 8, device=x.device, dtype=torch.int64)
        with _device_guard(x.device):
            rc = getattr(L, symbol)(*self._handle_args(), x.data_ptr(), logp.data_ptr(), ptr(noise), ptr(uniforms),
                                    x.shape[0], *head_args, steps, dt_dev.data_ptr(), int(bool(adaptive)),
                                    *over, int(seed) & _U64, int(walker_offset), ptr(walker_ids), int(step0),
                                    int(bool(remove_mean)), ptr(rates_out), ws.data_ptr(), stream_ptr(x.device))
        if rc == PITA_EUNSUPPORTED:
            return None
        check(rc, symbol)
        return x
