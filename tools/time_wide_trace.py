"""Timing of trace(J_x D) on the wide EGNN backbone (EGNN_dynamics_AD2_cat, hidden 64 x 5 layers, attention + tanh,
condition_beta; --particles 22, 33 or 42 atoms): the n*d single-direction launches exactly as
VEReverseSDE._denoiser_jacobian_terms issues them against the single call EGNN_dynamics_AD2_cat.jacobian_trace
(pita_egnn_wide_jacobian_trace), alternating, in one process on one device, device-event timing.
python tools/time_wide_trace.py [--particles 22] [--batches 512,2048,4096] [--reps 20] [--warmup 3] [--single-only]
                                [--commit HASH] [--probes K[,K...]]
Prints per batch size the median and min-max of both in ms, whether the two traces agree bit for bit, and the difference
against the loop's own min-max spread.  --single-only: the single call alone (the loop takes n*d times as many launches;
on the vector pipe at 42 atoms that is seconds per repetition).  PITA_WIDE_NO_MFMA=1 in the environment times the
vector-pipe kernels.  --commit: recorded in the header (default: git rev-parse of the tree it runs in).
--probes K[,K...]: instead, time the single exact call against the Hutchinson estimator
EGNN_dynamics_AD2_cat.jacobian_trace_estimate (pita_egnn_wide_trace_probes, probes drawn in the kernel) at each K,
interleaved in one process, and print per K the estimator's measured standard error (from per_probe, root mean square over
the batch) beside the root-mean-square error of the estimate against the exact trace; at 22 atoms also, on the 12 golden
walkers of tests/golden/egnn_ad2cat_h{64,48}_fwd.npz, the measured standard error beside sigma_b / sqrt(K) of the fp64
oracle Jacobian."""
import argparse, os, statistics, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pita_amd as pa
from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=22)
ap.add_argument("--batches", default="512,2048,4096")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--single-only", action="store_true")
ap.add_argument("--commit", default=None)
ap.add_argument("--probes", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
commit = a.commit
if commit is None:
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
    commit = r.stdout.strip() if r.returncode == 0 else "unknown"
print(f"tools/time_wide_trace.py  commit {commit}  device {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
N, ND = a.particles, 3 * a.particles
print(f"EGNN_dynamics_AD2_cat({N}, 3, hidden_nf=64, n_layers=5, attention, tanh, condition_beta), seeded weights; "
      f"{a.warmup} warm-up + {a.reps} timed repetitions per path, alternating, device events")
torch.manual_seed(7)
net = EGNN_dynamics_AD2_cat(N, 3, hidden_nf=64, n_layers=5, tanh=True, attention=True, condition_beta=True)
sde = pa.VEReverseSDE(noise_schedule=None, score_net=None, debias_inference=True)
print(f"forward pass on the matrix pipe: {net.uses_matrix_pipe('cuda:0')}, forward mode on the matrix pipe: "
      f"{net.jvp_uses_matrix_pipe('cuda:0')}")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def probe_timings(B, h, x, beta, Ks):
    """Exact call and the estimator at every K, alternating within each repetition."""
    exact = lambda: net.jacobian_trace(h, x, beta, want_denoiser=True)
    ests = {K: (lambda K=K: net.jacobian_trace_estimate(h, x, beta, K, seed=11, step=5, want_denoiser=True)) for K in Ks}
    for _ in range(a.warmup):
        exact()
        for f in ests.values():
            f()
    torch.cuda.synchronize()
    t = {"exact": []}
    t.update({K: [] for K in Ks})
    for _ in range(a.reps):
        t["exact"].append(timed(exact)[0])
        for K, f in ests.items():
            t[K].append(timed(f)[0])
    s = lambda v: f"median {statistics.median(v):8.3f} (min {min(v):8.3f}, max {max(v):8.3f})"
    me = statistics.median(t["exact"])
    print(f"B={B}: exact single call ({ND} directions) {s(t['exact'])} ms", flush=True)
    trace = exact()[0].double()
    for K in Ks:
        est, _, per = net.jacobian_trace_estimate(h, x, beta, K, seed=11, step=5, want_per_probe=True)
        se = (per.double().var(0, unbiased=True) / K).mean().sqrt().item() if K > 1 else float("nan")
        rms = (est.double() - trace).pow(2).mean().sqrt().item()
        mk = statistics.median(t[K])
        print(f"B={B}: K={K:4d} estimator {s(t[K])} ms = {mk / me:6.3f} of exact (K / n d = {K / ND:6.3f}) | standard error "
              f"from per_probe {se:.4f}, rms (estimate - exact trace) {rms:.4f}, rms |trace| {trace.pow(2).mean().sqrt().item():.3f}",
              flush=True)


def golden_noise(Ks):
    """Measured standard error on the golden walkers beside the oracle's sigma_b / sqrt(K) (22 atoms)."""
    import numpy as np
    from torch.func import jacrev, vmap
    from oracle import pita_oracle as O
    for tag, c in (("h64", dict(n_layers=5, tanh=True, attention=True)), ("h48", dict(n_layers=2, tanh=False, attention=False))):
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", f"egnn_ad2cat_{tag}_fwd.npz")))
        w = {k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("w.")}
        gnet = EGNN_dynamics_AD2_cat(22, 3, hidden_nf=w["egnn.embedding.weight"].shape[0], n_layers=c["n_layers"],
                                     tanh=c["tanh"], attention=c["attention"], condition_beta=True)
        gnet.load_state_dict(w)
        x, h, beta = (torch.tensor(g[k]) for k in ("x", "h", "beta"))
        wd = {k: v.double() for k, v in w.items()}
        bb = lambda cn, xs, b: O.egnn_ad2_cat_forward(wd, cn, xs, b, 22, 3, **c)
        one = lambda hh, xx, b: O.denoiser(bb, hh[None], xx[None], b[None])[0]
        J = vmap(jacrev(one, argnums=1))(h.double(), x.double(), beta.double())
        S = J + J.transpose(1, 2)
        S = S - torch.diag_embed(S.diagonal(dim1=1, dim2=2))
        sigma = (0.5 * S.pow(2).sum((1, 2))).sqrt()
        print(f"golden {tag}: |trace| {J.diagonal(dim1=1, dim2=2).sum(-1).abs().min():.3f} .. "
              f"{J.diagonal(dim1=1, dim2=2).sum(-1).abs().max():.3f}, one-probe sigma_b {sigma.min():.4f} .. {sigma.max():.4f}")
        for K in Ks:
            if K < 2:
                continue
            _, _, per = gnet.jacobian_trace_estimate(h.cuda(), x.cuda(), beta.cuda(), K, seed=11, step=5, want_per_probe=True)
            se = (per.double().var(0, unbiased=True) / K).sqrt().cpu()
            want = sigma / K ** 0.5
            print(f"golden {tag}: K={K:4d} measured standard error {se.min():.4f} .. {se.max():.4f} (mean {se.mean():.4f}) | "
                  f"sigma_b / sqrt(K) {want.min():.4f} .. {want.max():.4f} (mean {want.mean():.4f})", flush=True)


for B in (int(b) for b in a.batches.split(",")):
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, N, 3, generator=gen)
    x = (x - x.mean(1, keepdim=True)).reshape(B, ND).cuda()
    h = (torch.rand(B, generator=gen) * 2.0 + 0.05).cuda()
    beta = (torch.rand(B, generator=gen) + 0.5).cuda()
    loop = lambda: sde._denoiser_jacobian_terms(net, h, x, beta, False)  # (D, trace, jtx, None): n*d launches
    single = lambda: net.jacobian_trace(h, x, beta, want_denoiser=True)  # (trace, D): one call
    s = lambda v: f"median {statistics.median(v):8.3f} (min {min(v):8.3f}, max {max(v):8.3f})"
    if a.probes:
        probe_timings(B, h, x, beta, [int(k) for k in a.probes.split(",")])
        continue
    if a.single_only:
        for _ in range(a.warmup):
            single()
        torch.cuda.synchronize()
        ts = [timed(single)[0] for _ in range(a.reps)]
        print(f"B={B}: single call {s(ts)} ms", flush=True)
        continue
    for _ in range(a.warmup):
        loop(); single()
    torch.cuda.synchronize()
    t = {"loop": [], "single": []}
    for _ in range(a.reps):
        ms, (D_l, tr_l, _, _) = timed(loop)
        t["loop"].append(ms)
        ms, (tr_s, D_s) = timed(single)
        t["single"].append(ms)
    same = torch.equal(tr_l, tr_s) and torch.equal(D_l, D_s)
    gain = statistics.median(t["loop"]) - statistics.median(t["single"])
    spread = max(t["loop"]) - min(t["loop"])
    verdict = "beyond the loop's spread" if gain > spread else ("within the loop's spread" if gain >= -spread
                                                                else "SINGLE CALL SLOWER beyond the loop's spread")
    print(f"B={B}: {ND}-launch loop {s(t['loop'])} ms | single call {s(t['single'])} ms | loop - single {gain:8.3f} ms "
          f"(x{statistics.median(t['loop']) / statistics.median(t['single']):.2f}), loop spread {spread:.3f} ms: {verdict} | "
          f"bits {'identical' if same else 'DIFFER'}", flush=True)
if a.probes and N == 22:
    golden_noise([int(k) for k in a.probes.split(",")])
