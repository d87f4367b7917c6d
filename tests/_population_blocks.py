"""Shapes and helpers of the tests of pita_population_resample_blocks (test_population_blocks_cpu.py,
test_population_blocks_gpu.py).  The inputs are those of tests/_populations.py (``weights``, ``batch``, ``uniforms``,
``np_stats``, ``expect_event`` take any S) at population sizes beyond one block's 2 048 walkers:

  2 049  three virtual blocks of 1 024 walkers, the last with one element      3 072  an exact multiple of 1 024
  4 097  five blocks                                                            5 000  a ragged middle size

and P = 1, 3, 40 populations, plus 300 (more populations than compute units) at the smallest size.  The reference of
every population is the single-population path on its slice, compared by bit patterns."""
import torch

SIZES = (2049, 3072, 4097, 5000)
POPS = (1, 3, 40)
SHAPES = tuple((S, P) for S in SIZES for P in POPS) + ((2049, 300),)
SMALL_SIZES = (1, 2, 63, 1025, 2048)  # where the one-launch route exists too


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def same(r0, r1):
    r0, r1 = tuple(r0), tuple(r1)
    return len(r0) == len(r1) and all(torch.equal(bits(a), bits(b)) for a, b in zip(r0, r1))


def by_loop(logits, n_pop, theta, u):
    """The event of every population as a loop of single-population events over the slices:
    (ids as global rows, flags, stats, counts, logw_next)."""
    from pita_amd.utils import sample_cat_sys_adaptive

    logits = logits.reshape(-1)
    S, dev = logits.numel() // n_pop, logits.device
    flags = torch.empty(n_pop, device=dev, dtype=torch.int32)
    stats = torch.empty(n_pop, 6, device=dev, dtype=torch.float64)
    counts = torch.empty(n_pop, device=dev, dtype=torch.int64)
    uh = u.cpu().tolist()
    ids = [sample_cat_sys_adaptive(S, logits[p * S:(p + 1) * S], theta, uh[p], out=(flags[p], stats[p], counts[p]))[0] + p * S
           for p in range(n_pop)]
    nxt = torch.where(flags.repeat_interleave(S) != 0, torch.zeros_like(logits), logits)
    return torch.cat(ids), flags, stats, counts, nxt


def sentinel_buffers(P, S, dev="cuda"):
    """(ids, flags, stats, counts) filled with -7."""
    return (torch.full((P * S,), -7, dtype=torch.int64, device=dev), torch.full((P,), -7, dtype=torch.int32, device=dev),
            torch.full((P, 6), -7.0, dtype=torch.float64, device=dev), torch.full((P,), -7, dtype=torch.int64, device=dev))


def raw_call(pa, a, P, S, u, theta, logw_next, bufs=None, with_counts=True):
    """pita_population_resample_blocks through the raw entry point: (rc, ids, flags, stats, counts)."""
    L = pa._lib.lib()
    dev = a.device
    if bufs is None:
        bufs = (torch.empty(P * S, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                torch.empty(P, 6, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.int64, device=dev))
    ids, flags, stats, counts = bufs
    nbytes = int(L.pita_population_resample_blocks_workspace_bytes(P, max(S, 1)))
    ws = torch.empty(max(1, (nbytes + 7) // 8), dtype=torch.float64, device=dev)
    rc = L.pita_population_resample_blocks(a.data_ptr(), P, S, u.data_ptr(), theta, ids.data_ptr(),
                                           counts.data_ptr() if with_counts else None, stats.data_ptr(), flags.data_ptr(),
                                           pa._lib.ptr(logw_next), ws.data_ptr(), pa._lib.stream_ptr(dev))
    return rc, ids, flags, stats, counts
