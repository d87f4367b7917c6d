"""Timing of the fused mix-RBF Gram kernel against two torch routes, in one process:
  (a) torch, chunked, differences first, fp32: rows of the samples in chunks of CH = 2^28 / (M * D) (the [CH, M, D]
      difference tensor is then 1 GiB), s = (d * d).sum(-1), one exp and one fp64 sum per bandwidth -- unweighted;
  (b) torch.cdist(a_chunk, b) ** 2 in chunks of 2^28 / M rows (a 1 GiB [CH, M] matrix), the same exps and sums -- unweighted;
  (c) pita_rbf_gram_sums, cross mode, with log-weights on the samples, through the C ABI on preallocated buffers
      (launches of the weights passes and of the reduction included), as 1 population and, where listed, as 32
at the five default bandwidths.  Everything is warmed up once, then timed in alternating windows, each between two
device synchronisations; the table gives the median and the spread of the windows.  Before anything is timed the
unit-weight sums of (c) are compared with (a)'s.  Last, the error of (b) and of (c) on a RESAMPLED batch (every row a
copy of one of 1/4 of the rows, as after a resampling event) against an fp64 torch evaluation, self sums, per bandwidth."""
import ctypes, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
L = pa._lib.lib()
SIG = (0.01, 0.1, 1.0, 10.0, 100.0)
GAM = [1.0 / (2.0 * s * s) for s in SIG]
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3


def windows(cases, reps_of):
    for fn in cases:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in cases]
    for _ in range(rounds):
        for k, fn in enumerate(cases):
            t0 = time.perf_counter()
            for _ in range(reps_of[k]):
                fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / reps_of[k] * 1e3)
    return [float(np.median(v)) for v in t], [f"{np.median(v):9.3f} [{min(v):8.3f},{max(v):8.3f}]" for v in t]


def torch_chunked(a, b, dtype=torch.float32, wa=None):
    M, D = b.shape
    ch = max(1, (1 << 28) // (M * D) // (2 if dtype == torch.float64 else 1))
    out = torch.zeros(len(GAM), dtype=torch.float64, device=a.device)
    a, b = a.to(dtype), b.to(dtype)
    for lo in range(0, a.shape[0], ch):
        d = a[lo:lo + ch, None, :] - b[None, :, :]
        s = (d * d).sum(-1)
        for k, g in enumerate(GAM):
            e = torch.exp(-g * s)
            out[k] += (e if wa is None else e * wa[lo:lo + ch, None]).sum(dtype=torch.float64)
    return out


def torch_cdist(a, b):
    M = b.shape[0]
    ch = max(1, (1 << 28) // M)
    out = torch.zeros(len(GAM), dtype=torch.float64, device=a.device)
    for lo in range(0, a.shape[0], ch):
        s = torch.cdist(a[lo:lo + ch], b).square_()
        for k, g in enumerate(GAM):
            out[k] += torch.exp(-g * s).sum(dtype=torch.float64)
    return out


class Fused:
    def __init__(self, a, lw, P, b):
        self.a, self.lw, self.P, self.b = a, lw, P, b
        self.S, self.M = a.shape[0] // P, 0 if b is None else b.shape[0]
        self.ws = torch.empty(L.pita_rbf_gram_workspace_bytes(P, self.S, self.M) // 8, dtype=torch.float64, device="cuda")
        self.sums = torch.empty(P, len(GAM), dtype=torch.float64, device="cuda")
        self.info = torch.empty(P * 5 + 5, dtype=torch.float64, device="cuda")
        self.g = (ctypes.c_double * len(GAM))(*GAM)
        self.st = pa._lib.stream_ptr(a.device)

    def __call__(self, lw="own"):
        lw = self.lw if isinstance(lw, str) else lw
        pa._lib.check(L.pita_rbf_gram_sums(self.a.data_ptr(), pa._lib.ptr(lw), self.P, self.S, pa._lib.ptr(self.b), None, self.M,
                                           self.a.shape[1], self.g, len(GAM), self.sums.data_ptr(), self.info.data_ptr(),
                                           self.info.data_ptr() + 40 * self.P if self.b is not None else None,
                                           self.ws.data_ptr(), self.st))
        return self.sums


print(f"five bandwidths {SIG}, log-weights N(0, 3^2) on the samples in (c); ms per call: median [min, max] of {rounds} windows "
      f"of {reps} calls ((a), (b): 1 call)")
print(f"{'case':>34} {'(a) torch chunked':>30} {'(b) torch.cdist':>30} {'(c) fused':>30}   (c)/(a)   (c)/(b)")
for name, D, B, M, pops in (("GMM-like D=2", 2, 65536, 65536, (1,)), ("LJ13 D=39", 39, 65536, 10000, (1, 32)),
                            ("D=66", 66, 32768, 10000, (1,))):
    rng = np.random.default_rng(D)
    a = torch.from_numpy(rng.normal(0.0, 1.0, (B, D)).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.normal(0.1, 1.0, (M, D)).astype(np.float32)).cuda()
    lw = torch.from_numpy(rng.normal(0.0, 3.0, B).astype(np.float32)).cuda()
    ref = torch_chunked(a, b).cpu().numpy()
    for P in pops:
        f = Fused(a, lw, P, b)
        got = f(None).sum(0).cpu().numpy()
        agree = float(np.abs(got - ref).max() / (float(B) * M))
        med, cell = windows([lambda: torch_chunked(a, b), lambda: torch_cdist(a, b), f], [1, 1, reps])
        print(f"{'%s, %d x %d, P = %d' % (name, B, M, P):>34} {cell[0]:>30} {cell[1]:>30} {cell[2]:>30} {med[2] / med[0]:9.3f} "
              f"{med[2] / med[1]:9.3f}   (unit-weight sums of (c) against (a), normalised: {agree:.2e})")
        del f
    del a, b, lw

print("\nresampled batch, LJ13-like D = 39, 8 192 rows copied from 2 048 distinct ones, unit weights, self sums S_xx / B^2 per "
      "bandwidth:")
rng = np.random.default_rng(7)
base = rng.normal(0.0, 1.0, (2048, 39)).astype(np.float32)
x = torch.from_numpy(base[rng.integers(0, 2048, 8192)]).cuda()
ref = (torch_chunked(x, x, torch.float64) / 8192.0 ** 2).cpu().numpy()
fused = (Fused(x, None, 1, None)()[0] / 8192.0 ** 2).cpu().numpy()
chunked = (torch_chunked(x, x) / 8192.0 ** 2).cpu().numpy()
cd = (torch_cdist(x, x) / 8192.0 ** 2).cpu().numpy()
print(f"{'sigma':>8} {'fp64':>14} {'(a) error':>12} {'(b) cdist error':>16} {'(c) fused error':>16}")
for k, s in enumerate(SIG):
    print(f"{s:8g} {ref[k]:14.6e} {abs(chunked[k] - ref[k]):12.2e} {abs(cd[k] - ref[k]):16.2e} {abs(fused[k] - ref[k]):16.2e}")
