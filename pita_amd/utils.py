"""Systematic resampling on the GPU (mirror of ``sample_cat_sys``,
pita/src/models/components/utils.py:111-120)."""
import torch

from . import _lib


def _uniform0(u):
    """An event's uniform as a Python float; None draws one float64 from torch's CPU generator, like the reference."""
    if u is None:
        u = torch.rand(size=(1,), dtype=torch.float64)
    return float(u.reshape(-1)[0]) if isinstance(u, torch.Tensor) else float(u)


def _workspace(nbytes, device):
    """8-byte aligned device scratch of at least ``nbytes`` bytes."""
    return torch.empty((int(nbytes) + 7) // 8, device=device, dtype=torch.float64)


def sample_cat_sys(bs, logits, u=None):
    """ids[bs] (int64 device tensor) for systematic resampling of ``softmax(logits)`` clipped to
    [1e-6, 1] (not renormalised).  ``u`` defaults to one float64 uniform from torch's CPU
    generator, exactly like the reference.  Returns ``(ids, None)`` like the reference."""
    logits = _lib.dev_tensor(logits, "logits").reshape(-1)
    assert logits.shape[0] == bs
    u0 = _uniform0(u)
    ids = torch.empty(bs, device=logits.device, dtype=torch.int64)
    ws = _workspace(_lib.lib().pita_resample_workspace_bytes(bs), logits.device)
    _lib.check(_lib.lib().pita_systematic_resample(logits.data_ptr(), bs, u0, ids.data_ptr(), ws.data_ptr(),
                                                   _lib.stream_ptr(logits.device)), "pita_systematic_resample")
    return ids, None


def sample_cat_sys_adaptive(bs, logits, theta, u=None, out=None):
    """One resampling event decided on the device (pita_adaptive_resample; an extension, the reference resamples
    unconditionally): the event resamples when the effective sample size of the log-weights ``logits`` is at most
    ``theta * bs`` (always at ``theta >= 1``, and whenever an entry is NaN or +inf).  Returns ``(ids, resampled, stats,
    n_unique)``, all device tensors and none of them read by the host here: ``ids`` int64 [bs] are ``sample_cat_sys``'s
    where the event resamples and ``arange(bs)`` where not, ``resampled`` int32 [] is the decision, ``stats`` float64 [6]
    = (max, log mean weight, ESS, ESS / bs, #NaN or +inf, #-inf) and ``n_unique`` int64 [] the number of distinct parents.
    ``u`` defaults to one float64 uniform from torch's CPU generator, exactly like ``sample_cat_sys``.  ``out``: optional
    ``(resampled, stats, n_unique)`` to write into (rows of a caller's per-step buffers)."""
    logits = _lib.dev_tensor(logits, "logits").reshape(-1)
    assert logits.shape[0] == bs
    u0 = _uniform0(u)
    dev = logits.device
    ids = torch.empty(bs, device=dev, dtype=torch.int64)
    if out is None:
        out = (torch.empty((), device=dev, dtype=torch.int32), torch.empty(6, device=dev, dtype=torch.float64),
               torch.empty((), device=dev, dtype=torch.int64))
    resampled, stats, n_unique = out
    L = _lib.lib()
    ws = _workspace(L.pita_adaptive_resample_workspace_bytes(bs), dev)
    _lib.check(L.pita_adaptive_resample(logits.data_ptr(), bs, u0, float(theta), ids.data_ptr(), n_unique.data_ptr(),
                                        stats.data_ptr(), resampled.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)),
               "pita_adaptive_resample")
    return ids, resampled, stats, n_unique


MAX_POPULATION_SIZE = 2048  # walkers one block of pita_population_resample holds in LDS


def sample_cat_sys_populations(logits, n_pop, theta, u=None, out=None):
    """One resampling event for each of ``n_pop`` independent populations in ONE launch (pita_population_resample; an
    extension).  ``logits`` [n_pop * S] holds the populations back to back, S <= 2 048 (a larger S is refused:
    ``sample_cat_sys_population_blocks`` takes any); population p is decided and
    resampled exactly as ``sample_cat_sys_adaptive(S, logits[p * S:(p + 1) * S], theta, u[p])`` would, bit for bit and
    whatever ``n_pop`` and ``p`` are.  Returns ``(ids, resampled, stats, n_unique, logw_next)``, all device tensors and
    none of them read by the host here: ``ids`` int64 [n_pop * S] are GLOBAL rows (p * S + parent), so ``gather_rows``
    takes them as they are; ``resampled`` int32 [n_pop], ``stats`` float64 [n_pop, 6] and ``n_unique`` int64 [n_pop] are
    the per-population outputs of ``sample_cat_sys_adaptive``; ``logw_next`` float32 [n_pop * S] is 0 where a population
    resampled and ``logits`` where it did not.  ``theta >= 1`` is the fixed schedule.
    ``u``: float64 [n_pop] uniforms in [0, 1), on the host or on the device (a device tensor is used as it is and not
    checked); None draws ``torch.rand(n_pop, dtype=float64)`` from torch's CPU generator.  ``out``: optional
    ``(resampled, stats, n_unique)`` to write into (rows of a caller's per-step buffers)."""
    return _population_events("pita_population_resample", logits, n_pop, theta, u, out)


def sample_cat_sys_population_blocks(logits, n_pop, theta, u=None, out=None):
    """``sample_cat_sys_populations`` for populations of ANY size S (pita_population_resample_blocks; an extension): the
    same arguments, the same return tuple and the same contract -- population p is decided and resampled exactly as
    ``sample_cat_sys_adaptive(S, logits[p * S:(p + 1) * S], theta, u[p])`` would, bit for bit and whatever ``n_pop`` and
    ``p`` are.  Always the multi-block route: at most seven launches per call whatever ``n_pop`` is (one statistics block
    per population, the five passes of ``sample_cat_sys`` over a (block, population) grid, the run count), so for
    S <= 2 048 it returns what the one launch of ``sample_cat_sys_populations`` returns, in more launches."""
    return _population_events("pita_population_resample_blocks", logits, n_pop, theta, u, out)


def _population_events(entry, logits, n_pop, theta, u, out):
    """The host side the two population entry points share: ``entry`` and ``entry``_workspace_bytes of the library."""
    logits = _lib.dev_tensor(logits, "logits").reshape(-1)
    n_pop = int(n_pop)
    if n_pop < 1 or logits.shape[0] % n_pop != 0:
        raise ValueError(f"{logits.shape[0]} log-weights do not split into {n_pop} populations")
    S = logits.shape[0] // n_pop
    dev = logits.device
    if u is None:
        u = torch.rand(n_pop, dtype=torch.float64)
    if not isinstance(u, torch.Tensor):
        u = torch.as_tensor(u, dtype=torch.float64)
    if tuple(u.shape) != (n_pop,) or u.dtype != torch.float64:
        raise ValueError(f"u must be a float64 tensor of shape ({n_pop},), got {u.dtype} {tuple(u.shape)}")
    if not u.is_cuda:
        if not bool(((u >= 0.0) & (u < 1.0)).all()):
            raise ValueError("u must lie in [0, 1)")
        u = u.to(dev)
    u = u.contiguous()
    ids = torch.empty(n_pop * S, device=dev, dtype=torch.int64)
    logw_next = torch.empty(n_pop * S, device=dev, dtype=torch.float32)
    if out is None:
        out = (torch.empty(n_pop, device=dev, dtype=torch.int32), torch.empty(n_pop, 6, device=dev, dtype=torch.float64),
               torch.empty(n_pop, device=dev, dtype=torch.int64))
    resampled, stats, n_unique = out
    L = _lib.lib()
    ws = _workspace(getattr(L, entry + "_workspace_bytes")(n_pop, S), dev)
    _lib.check(getattr(L, entry)(logits.data_ptr(), n_pop, S, u.data_ptr(), float(theta), ids.data_ptr(),
                                 n_unique.data_ptr(), stats.data_ptr(), resampled.data_ptr(), logw_next.data_ptr(),
                                 ws.data_ptr(), _lib.stream_ptr(dev)), entry)
    return ids, resampled, stats, n_unique, logw_next


def rademacher_probes(B, n_particles, n_dim, n_probes, seed=0, walker_offset=0, step=0, device="cuda"):
    """[n_probes, B, n_particles * n_dim] Rademacher probes (+1 / -1) of the Hutchinson divergence estimator (the one
    the reference's utils.py ships beside ``compute_divergence_exact``) from the library's Philox stream
    (pita_rademacher_probes): row [k, b] is what the probe kernels of ``jacobian_trace_estimate(probes=None)`` draw for
    probe k of walker ``walker_offset + b`` under the same (seed, step).  1 <= n_probes <= 256."""
    device = torch.device(device)
    out = torch.empty(int(n_probes), int(B), int(n_particles) * int(n_dim), device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pita_rademacher_probes(out.data_ptr(), int(B), int(n_particles), int(n_dim), int(n_probes),
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset), int(step),
                                                     _lib.stream_ptr(device)), "pita_rademacher_probes")
    return out


def gather_rows(x, ids):
    """x[ids] through the HIP row-gather kernel."""
    x = _lib.dev_tensor(x, "x")
    out = torch.empty_like(x)
    _lib.check(_lib.lib().pita_gather_rows(x.data_ptr(), ids.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                           _lib.stream_ptr(x.device)), "pita_gather_rows")
    return out
