"""Timing of the reverse-mode sweep on the wide EGNN backbone (EGNN_dynamics_AD2_cat, hidden 64 x 5 layers, attention +
tanh, condition_beta; --particles 22, 33 or 42 atoms): vjp(want_dot_h=True) = pita_egnn_wide_vjp, in one process on one
device, device-event timing.
python tools/time_wide_vjp.py [--particles 22] [--batches 256,2048,4096] [--reps 10] [--warmup 3] [--label TEXT] [--parts]
Prints per batch size the median and min-max in ms.  PITA_WIDE_NO_MFMA=1 in the environment times the vector-pipe kernel
alone.  --parts also asks for the dot_parts split (not in trees before it).  Without it the tool only uses entry points the parent of the matrix-pipe sweep has too, so the same file times a tree of that
commit (A/B: run the two trees alternately in one session on one device, as profiles/r09_wide_vjp.txt records)."""
import argparse, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("PITA_TREE", ROOT))
import pita_amd as pa  # noqa: F401  (fails loudly when the library is missing)
from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=22)
ap.add_argument("--batches", default="256,2048,4096")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--parts", action="store_true", help="vjp(want_dot_h=True, want_h_parts=True): pita_egnn_wide_vjp_parts")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
assert a.reps >= 10, "at least 10 timed repetitions"
N, ND = a.particles, 3 * a.particles
torch.manual_seed(7)
net = EGNN_dynamics_AD2_cat(N, 3, hidden_nf=64, n_layers=5, tanh=True, attention=True, condition_beta=True)
pipe = net.vjp_uses_matrix_pipe("cuda:0") if hasattr(net, "vjp_uses_matrix_pipe") else False
print(f"tools/time_wide_vjp.py {a.label}  tree {os.path.dirname(os.path.abspath(pa.__file__))}  device "
      f"{torch.cuda.get_device_name(0)}  {N} atoms, hidden 64 x 5, attention + tanh; reverse mode on the matrix pipe: "
      f"{pipe}; {a.warmup} warm-up + {a.reps} timed repetitions, device events", flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


what = "want_dot_h, want_h_parts" if a.parts else "want_dot_h"
for B in (int(b) for b in a.batches.split(",")):
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, N, 3, generator=gen)
    x = (x - x.mean(1, keepdim=True)).reshape(B, ND).cuda()
    h = (torch.rand(B, generator=gen) * 2.0 + 0.05).cuda()
    beta = (torch.rand(B, generator=gen) + 0.5).cuda()
    run = (lambda: net.vjp(h, x, beta, want_dot_h=True, want_h_parts=True)) if a.parts else \
          (lambda: net.vjp(h, x, beta, want_dot_h=True))
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(a.reps):
        ms, out = timed(run)
        ts.append(ms)
    fin = all(bool(torch.isfinite(o).all()) for o in out)
    print(f"{a.label} n={N} B={B}: vjp({what}) median {statistics.median(ts):9.3f} ms (min {min(ts):9.3f}, max "
          f"{max(ts):9.3f}) finite {fin} checksum {float(out[1].double().abs().sum()):.9e}", flush=True)
