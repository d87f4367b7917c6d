"""Timing of the weighted per-population histograms against the unweighted path they extend, in one process:
  pair distances: (a) metrics.histogram(interatomic_dist(x)) -- the [B, n (n - 1) / 2] distance array written by torch ops
                      and read back by pita_histogram
                  (b) pita_pair_distance_histogram from the coordinates, with log-weights
                  at LJ13 x 65 536 and LJ55 x 32 768 walkers
  values:         (a) pita_histogram   (b) pita_weighted_histogram with log-weights   at 65 536 and 2^21 values
each with populations = 1 and 32 for (b), 100 bins, through the C ABI on preallocated buffers.  Everything is warmed up, then
timed in alternating windows of `reps` calls, each window between two device synchronisations; the table gives the median
and the spread of the windows.  Before anything is timed the unit-weight counts of (b) are compared with (a)'s."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
from pita_amd import metrics
from pita_amd.data_utils import interatomic_dist
L, NB = pa._lib.lib(), 100
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7


def windows(cases):
    for fn in cases:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in cases]
    for _ in range(rounds):
        for k, fn in enumerate(cases):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / reps * 1e6)
    return [float(np.median(v)) for v in t], [f"{np.median(v):8.1f} [{min(v):7.1f},{max(v):7.1f}]" for v in t]


def outputs(P):
    return (torch.empty(P, NB, dtype=torch.int64, device="cuda"), torch.empty(P, NB, dtype=torch.int64, device="cuda"),
            torch.empty(P, 4, dtype=torch.float64, device="cuda"))


print(f"{NB} bins, log-weights N(0, 3^2); us per call: median [min, max] of {rounds} windows of {reps} calls")
print(f"{'case':>22} {'(a) unweighted path':>28} {'(b) P = 1':>28} {'(b) P = 32':>28}  (b1)/(a) (b32)/(a)")
for n, B in ((13, 65536), (55, 32768)):
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.normal(0.0, 1.0, (B, n * 3)).astype(np.float32)).cuda()
    lw = torch.from_numpy(rng.normal(0.0, 3.0, B).astype(np.float32)).cuda()
    edges = np.linspace(0.0, 6.0, NB + 1).astype(np.float32)
    e = torch.from_numpy(edges).cuda()
    st = pa._lib.stream_ptr(x.device)
    out = {P: outputs(P) for P in (1, 32)}

    def parent():
        return metrics.histogram(interatomic_dist(x.reshape(B, n, 3)), edges)

    def fused(P, w=lw):
        ws, cs, info = out[P]
        pa._lib.check(L.pita_pair_distance_histogram(x.data_ptr(), pa._lib.ptr(w), P, B // P, n, 3, e.data_ptr(), NB, ws.data_ptr(),
                                                     cs.data_ptr(), info.data_ptr(), st))

    fused(1, None)
    diff = int((out[1][1][0] - parent()).abs().sum())  # torch's norm rounds differently: a value beside an edge may move
    med, cell = windows([parent, lambda: fused(1), lambda: fused(32)])
    print(f"{'pairs LJ%d x %d' % (n, B):>22} {cell[0]:>28} {cell[1]:>28} {cell[2]:>28}  {med[1] / med[0]:8.2f} {med[2] / med[0]:9.2f}"
          f"   (counts moved between bins against (a): {diff} of {B * n * (n - 1) // 2})")
    del x, out
for N in (65536, 2 ** 21):
    rng = np.random.default_rng(N)
    v = torch.from_numpy(rng.normal(2.0, 1.5, N).astype(np.float32)).cuda()
    lw = torch.from_numpy(rng.normal(0.0, 3.0, N).astype(np.float32)).cuda()
    e = torch.from_numpy(np.linspace(-2.0, 6.0, NB + 1).astype(np.float32)).cuda()
    st = pa._lib.stream_ptr(v.device)
    plain = torch.empty(NB, dtype=torch.int64, device="cuda")
    out = {P: outputs(P) for P in (1, 32)}

    def parent():
        pa._lib.check(L.pita_histogram(v.data_ptr(), N, e.data_ptr(), NB, plain.data_ptr(), st))

    def weighted(P, w=lw):
        ws, cs, info = out[P]
        pa._lib.check(L.pita_weighted_histogram(v.data_ptr(), pa._lib.ptr(w), P, N // P, 1, e.data_ptr(), NB, ws.data_ptr(),
                                                cs.data_ptr(), info.data_ptr(), st))

    parent(); weighted(1, None); weighted(32, None); torch.cuda.synchronize()
    assert torch.equal(out[1][1][0], plain) and torch.equal(out[32][1].sum(0), plain), "unit-weight counts must be pita_histogram's"
    med, cell = windows([parent, lambda: weighted(1), lambda: weighted(32)])
    print(f"{'values x %d' % N:>22} {cell[0]:>28} {cell[1]:>28} {cell[2]:>28}  {med[1] / med[0]:8.2f} {med[2] / med[0]:9.2f}")
