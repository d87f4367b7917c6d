"""Timing of the fused Ramachandran histogram against a torch route, in one process:
  (a) torch ops on the device: the two angles of every pair by gathers, cross products and atan2 ([B, n_pair] angle
      arrays in memory), torch.bucketize per axis, torch.bincount of the cell index -- unweighted, one population;
  (b) pita_dihedral_histogram2d from the coordinates, with log-weights, populations = 1 and 32
at 22 atoms x 65 536 walkers (1 pair) and 42 atoms x 32 768 walkers (3 pairs), 64 x 64 bins over [-pi, pi], through the C ABI
on preallocated buffers.  Everything is warmed up, then timed in alternating windows of `reps` calls, each window between
two device synchronisations; the table gives the median and the spread of the windows.  Before anything is timed the
unit-weight counts of (b) are compared with (a)'s, and the angles of pita_dihedral_angles with an fp64 torch evaluation."""
import math, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
from pita_amd import metrics
L, NB = pa._lib.lib(), 64
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


def torch_angles(r, q):
    """[B, n, 3] coordinates, [k, 4] atoms -> [B, k] angles, the library's formula in the dtype of r"""
    b1, b2, b3 = r[:, q[:, 1]] - r[:, q[:, 0]], r[:, q[:, 2]] - r[:, q[:, 1]], r[:, q[:, 3]] - r[:, q[:, 2]]
    n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    return torch.atan2((b1 * n2).sum(-1) * b2.norm(dim=-1), (n1 * n2).sum(-1))


def chain(rng, B, n):
    """random-walk chains with bond length ~0.15: every dihedral of consecutive atoms spread over the circle"""
    steps = rng.normal(0.0, 1.0, (B, n, 3))
    steps *= 0.15 / np.linalg.norm(steps, axis=-1, keepdims=True)
    return torch.from_numpy(np.cumsum(steps, 1).reshape(B, n * 3).astype(np.float32)).cuda()


print(f"{NB} x {NB} bins over [-pi, pi], log-weights N(0, 3^2); us per call: median [min, max] of {rounds} windows of {reps} calls")
print(f"{'case':>26} {'(a) torch route':>28} {'(b) P = 1':>28} {'(b) P = 32':>28}  (b1)/(a) (b32)/(a)")
for n, B, n_pair in ((22, 65536, 1), (42, 32768, 3)):
    rng = np.random.default_rng(n)
    x = chain(rng, B, n)
    lw = torch.from_numpy(rng.normal(0.0, 3.0, B).astype(np.float32)).cuda()
    pairs = np.array([[(4 + 10 * k + j, 5 + 10 * k + j, 6 + 10 * k + j, 7 + 10 * k + j) for j in (0, 1)] for k in range(n_pair)])
    q = torch.from_numpy(pairs.astype(np.int32)).cuda()
    qa, qb = q[:, 0].long(), q[:, 1].long()
    edges = np.linspace(-np.pi, np.pi, NB + 1).astype(np.float32)
    e = torch.from_numpy(edges).cuda()
    st = pa._lib.stream_ptr(x.device)
    out = {P: (torch.empty(P, n_pair, NB, NB, dtype=torch.int64, device="cuda"), torch.empty(P, n_pair, NB, NB, dtype=torch.int64, device="cuda"),
               torch.empty(P, 4, dtype=torch.float64, device="cuda")) for P in (1, 32)}
    offset = (torch.arange(n_pair, device="cuda") * NB * NB)[None]

    def parent():
        r = x.reshape(B, n, 3)
        ia = (torch.bucketize(torch_angles(r, qa), e, right=True) - 1).clamp_(0, NB - 1)  # +pi: the last bin
        ib = (torch.bucketize(torch_angles(r, qb), e, right=True) - 1).clamp_(0, NB - 1)
        return torch.bincount((offset + ia * NB + ib).reshape(-1), minlength=n_pair * NB * NB).reshape(n_pair, NB, NB)

    def fused(P, w=lw):
        ws, cs, info = out[P]
        pa._lib.check(L.pita_dihedral_histogram2d(x.data_ptr(), pa._lib.ptr(w), P, B // P, n, q.data_ptr(), n_pair, e.data_ptr(), NB,
                                                  e.data_ptr(), NB, ws.data_ptr(), cs.data_ptr(), info.data_ptr(), st))

    fused(1, None)
    fused(32, None)
    torch.cuda.synchronize()
    assert torch.equal(out[32][1].sum(0), out[1][1][0]) and int(out[1][1].sum()) == B * n_pair
    diff = int((out[1][1][0] - parent()).abs().sum()) // 2  # torch's arithmetic rounds differently: a value beside an edge may move
    ang = metrics.dihedral_angles(x, pairs.reshape(-1, 4))
    ref = torch_angles(x.double().reshape(B, n, 3), q.reshape(-1, 4).long())
    d = (ang.double() - ref).abs()
    err = float(torch.minimum(d, 2 * math.pi - d).max())
    med, cell = windows([parent, lambda: fused(1), lambda: fused(32)])
    print(f"{'%d atoms x %d, %d pair%s' % (n, B, n_pair, 's' if n_pair > 1 else ''):>26} {cell[0]:>28} {cell[1]:>28} {cell[2]:>28}"
          f"  {med[1] / med[0]:8.2f} {med[2] / med[0]:9.2f}   (walkers in another cell than (a)'s: {diff} of {B * n_pair};"
          f" largest angle error against fp64, unconditioned chains: {err:.2e})")
    del x, out
