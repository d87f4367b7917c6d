"""Systematic resampling on the GPU (mirror of ``sample_cat_sys``,
pita/src/models/components/utils.py:111-120)."""
import torch

from . import _lib


def sample_cat_sys(bs, logits, u=None):
    """ids[bs] (int64 device tensor) for systematic resampling of ``softmax(logits)`` clipped to
    [1e-6, 1] (not renormalised).  ``u`` defaults to one float64 uniform from torch's CPU
    generator, exactly like the reference.  Returns ``(ids, None)`` like the reference."""
    logits = _lib.dev_tensor(logits, "logits").reshape(-1)
    assert logits.shape[0] == bs
    if u is None:
        u = torch.rand(size=(1,), dtype=torch.float64)
    u0 = float(u.reshape(-1)[0]) if isinstance(u, torch.Tensor) else float(u)
    ids = torch.empty(bs, device=logits.device, dtype=torch.int64)
    nbytes = int(_lib.lib().pita_resample_workspace_bytes(bs))
    ws = torch.empty((nbytes + 7) // 8, device=logits.device, dtype=torch.float64)  # 8-byte aligned scratch
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
    if u is None:
        u = torch.rand(size=(1,), dtype=torch.float64)
    u0 = float(u.reshape(-1)[0]) if isinstance(u, torch.Tensor) else float(u)
    dev = logits.device
    ids = torch.empty(bs, device=dev, dtype=torch.int64)
    if out is None:
        out = (torch.empty((), device=dev, dtype=torch.int32), torch.empty(6, device=dev, dtype=torch.float64),
               torch.empty((), device=dev, dtype=torch.int64))
    resampled, stats, n_unique = out
    L = _lib.lib()
    nbytes = int(L.pita_adaptive_resample_workspace_bytes(bs))
    ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)  # 8-byte aligned scratch
    _lib.check(L.pita_adaptive_resample(logits.data_ptr(), bs, u0, float(theta), ids.data_ptr(), n_unique.data_ptr(),
                                        stats.data_ptr(), resampled.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)),
               "pita_adaptive_resample")
    return ids, resampled, stats, n_unique


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
