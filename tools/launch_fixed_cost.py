"""Per-launch fixed cost of the fused sampler: event-timed launches of c steps, c = 1..100, least-squares fit
t(c) = a + b c, for the f16x2 (backup copy + kernel + repair launch) and bf16x3 (one kernel) paths.

    python tools/launch_fixed_cost.py [B]             # the fit above, B walkers (default 65536)
    python tools/launch_fixed_cost.py 64 wrappers     # host cost per call of the backbones' Python wrappers

``wrappers``: median wall time per call of ``jvp(direction=k, want_primal=False, want_tangent=False)`` (with the
in-kernel reductions the debiased regime asks for), ``vjp`` and ``edm`` on each backbone family.  At B = 64 the kernels
take a few tens of microseconds, so the time between two returns is the wrapper's: argument marshalling, the handle's
staleness check and the ctypes call."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import pita_amd

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
if len(sys.argv) > 2 and sys.argv[2] == "wrappers":
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
    from pita_amd.mlp import MyMLPTemperature

    WARM, CALLS = 50, 300
    torch.manual_seed(12345)
    nets = {"h32": (pita_amd.EGNN_dynamics(13, 3, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                                           condition_time=True, condition_temperature=True, agg="sum"), 39),
            "wide": (EGNN_dynamics_AD2_cat(22, 3, condition_beta=True), 66),
            "mlp": (MyMLPTemperature(input_dim=2, out_dim=2), 2)}
    for fam, (net, D) in nets.items():
        x = torch.randn(B, D, device="cuda")
        h = torch.full((B,), 0.5, device="cuda")
        beta = torch.ones(B, device="cuda")
        jtx, trace = torch.empty(B, D, device="cuda"), torch.zeros(B, device="cuda")
        calls = {"jvp": lambda i: net.jvp(h, x, beta, direction=i % D, want_primal=False, want_tangent=False, dot_out=jtx,
                                          dot_col=i % D, diag_acc=trace),
                 "vjp": lambda i: net.vjp(h, x, beta, want_dot_h=True, want_h_parts=True)}
        if hasattr(net, "edm"):
            calls["edm"] = lambda i: net.edm(2, h, x, beta)
        for name, call in calls.items():
            for i in range(WARM):
                call(i)
            torch.cuda.synchronize()
            ts = np.empty(CALLS)
            for i in range(CALLS):
                t0 = time.perf_counter()
                call(i)
                ts[i] = time.perf_counter() - t0
            torch.cuda.synchronize()
            print(f"wrappers B={B} {fam} {name}: median {np.median(ts) * 1e6:7.2f} us/call  "
                  f"(p10 {np.percentile(ts, 10) * 1e6:.2f}, p90 {np.percentile(ts, 90) * 1e6:.2f}, {CALLS} calls)")
    sys.exit(0)
sched = pita_amd.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
gam = pita_amd.ConstantAnnealingFactorSchedule(4 / 3)
tab = pita_amd.sde_integration.build_step_table(sched, gam, torch.linspace(1.0, 0.0, 1001)[:-1], 1e-3, 1.0, 1.0).cuda()
for prec in ("f16x2", "bf16x3"):
    torch.manual_seed(12345)
    net = pita_amd.EGNN_dynamics(13, 3, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                                 condition_time=True, condition_temperature=True, agg="sum", precision=prec)
    x = pita_amd.Prior(scale=69.28, n_particles=13, spatial_dim=3, seed=1).sample(B)
    cs, ts = [], []
    for c in (1, 2, 5, 10, 20, 50, 100):
        reps = max(3, 100 // c)
        net.sampler_run(x, tab[:c].contiguous(), c)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tabs = [tab[(i * c) % 900:(i * c) % 900 + c].contiguous() for i in range(reps)]
        e0.record()
        for i in range(reps):
            net.sampler_run(x, tabs[i], c, step0=i * c)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        cs.append(c)
        ts.append(ms)
        print(f"{prec} B={B} chunk={c:4d}: {ms:8.3f} ms/launch  {ms / c:7.4f} ms/step  {B * c / ms / 1e3:.3e} walker-steps/s")
    b, a = np.polyfit(cs, ts, 1)
    print(f"{prec}: fit t(c) = {a:.3f} ms + {b:.4f} ms x c")
