"""Timing of one resampling event of LJ13 walkers (39 coordinates) at 2 048, 16 384 and 65 536 walkers:
  (a) the fixed schedule's sequence: pita_systematic_resample + pita_count_runs + pita_gather_rows
  (b) pita_adaptive_resample with theta = 1 (the event always resamples) + pita_gather_rows
  (c) pita_adaptive_resample with theta = 0 (the event never resamples on these weights) + pita_gather_rows
through the C ABI on preallocated buffers, so that what is timed is the launches.  The three are warmed up, then timed in
alternating windows of `reps` events, each window between two device synchronisations; the table gives the median and the
spread of the windows.  (b) is checked against (a) bit for bit before anything is timed."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
L, D = pa._lib.lib(), 39
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [2048, 16384, 65536]
print(f"one resampling event, D = {D}, log-weights N(0, 1), u0 = 0.3; us per event: median [min, max] of {rounds} windows "
      f"of {reps} events")
print(f"{'B':>7} {'path':>12} {'(a) fixed':>22} {'(b) theta=1':>22} {'(c) theta=0':>22}  (b)/(a)  (c)/(a)")
for B in sizes:
    a = torch.from_numpy(np.float32(np.random.default_rng(1000 + B).standard_normal(B))).cuda()
    x = torch.randn(B, D, device="cuda")
    out = torch.empty_like(x)
    ids, ids_b = torch.empty(B, dtype=torch.int64, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")
    nu, nu_b = torch.zeros((), dtype=torch.int64, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    flag = torch.zeros((), dtype=torch.int32, device="cuda")
    ws = torch.empty((int(L.pita_resample_workspace_bytes(B)) + 7) // 8, dtype=torch.float64, device="cuda")
    ws_b = torch.empty((int(L.pita_adaptive_resample_workspace_bytes(B)) + 7) // 8, dtype=torch.float64, device="cuda")
    st = pa._lib.stream_ptr(a.device)

    def fixed():
        pa._lib.check(L.pita_systematic_resample(a.data_ptr(), B, 0.3, ids.data_ptr(), ws.data_ptr(), st))
        pa._lib.check(L.pita_count_runs(ids.data_ptr(), B, nu.data_ptr(), st))
        pa._lib.check(L.pita_gather_rows(x.data_ptr(), ids.data_ptr(), out.data_ptr(), B, D, st))

    def adaptive(theta):
        pa._lib.check(L.pita_adaptive_resample(a.data_ptr(), B, 0.3, theta, ids_b.data_ptr(), nu_b.data_ptr(), stats.data_ptr(),
                                               flag.data_ptr(), ws_b.data_ptr(), st))
        pa._lib.check(L.pita_gather_rows(x.data_ptr(), ids_b.data_ptr(), out.data_ptr(), B, D, st))

    cases = [fixed, lambda: adaptive(1.0), lambda: adaptive(0.0)]
    fixed(); adaptive(1.0); torch.cuda.synchronize()
    assert torch.equal(ids, ids_b) and int(nu) == int(nu_b) and int(flag) == 1, "theta = 1 must reproduce the fixed event"
    adaptive(0.0); torch.cuda.synchronize()
    assert int(flag) == 0 and int(nu_b) == B
    for fn in cases:  # warm-up of every shape of the timed windows
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    t = [[], [], []]
    for _ in range(rounds):
        for k, fn in enumerate(cases):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / reps * 1e6)
    med = [float(np.median(v)) for v in t]
    cell = [f"{m:7.1f} [{min(v):6.1f},{max(v):6.1f}]" for m, v in zip(med, t)]
    path = "one launch" if L.pita_adaptive_resample_single_launch(B) else "gated"
    print(f"{B:>7} {path:>12} {cell[0]:>22} {cell[1]:>22} {cell[2]:>22}  {med[1] / med[0]:7.2f}  {med[2] / med[0]:7.2f}")
