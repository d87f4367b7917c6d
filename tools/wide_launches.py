"""The launches behind the entry points of the wide EGNN backbone (EGNN_dynamics_AD2_cat, hidden 64 x 2 layers, attention
+ tanh, condition_beta): forward, score, sampler_run (2 steps), jvp, jacobian_trace and vjp once each on handles of
13 / 22 / 22 / 33 / 42 / 55 / 10 atoms at batches 3 / 3 / 4097 / 3 / 3 / 2 / 3 (22 atoms: the small-batch and the regular
forward mapping; 10 atoms: no matrix-pipe row), then the 22-atom calls again under PITA_WIDE_NO_MFMA=1.
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/wide_launches.py run
    python3 tools/wide_launches.py parse <dir>
`parse` lists, in dispatch order, kernel name, grid, workgroup and LDS size of every wide-EGNN kernel and every runtime
fill / copy kernel (hipMemsetAsync, hipMemcpyAsync) of the trace: two trees issue the same launches when the listings are
equal.  PITA_TREE=<other tree> runs that tree's package (A/B against another commit, as tools/time_wide_vjp.py)."""
import csv, glob, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((13, 3), (22, 3), (22, 4097), (33, 3), (42, 3), (55, 2), (10, 3))


def calls(net, n, B, build_step_table, sched, gam, torch):
    gen = torch.Generator().manual_seed(1000 * n + B)
    x = torch.randn(B, n, 3, generator=gen)
    x = (0.3 * (x - x.mean(1, keepdim=True))).reshape(B, 3 * n).cuda()
    h = (torch.rand(B, generator=gen) + 0.05).cuda()
    beta = (torch.rand(B, generator=gen) + 0.5).cuda()
    tab = build_step_table(sched, gam, torch.linspace(0.3, 0.0, 3)[:-1], 0.15, 1.0, 1.3).cuda()
    net.forward(h, x, beta)
    net.edm(2, h, x, beta)
    net.sampler_run(x.clone(), tab, 2, seed=9)
    net.jvp(h, x, beta, direction=1)
    net.jacobian_trace(h, x, beta, want_denoiser=True)
    net.vjp(h, x, beta, want_dot_h=True)
    torch.cuda.synchronize()


if sys.argv[1] == "run":
    import torch
    sys.path.insert(0, os.environ.get("PITA_TREE", ROOT))
    import pita_amd as pa
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat
    from pita_amd.sde_integration import build_step_table
    sched, gam = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7), pa.ConstantAnnealingFactorSchedule(4 / 3)
    print("tree", os.path.dirname(os.path.abspath(pa.__file__)), flush=True)
    nets = {}
    for n, B in CASES:
        if n not in nets:
            torch.manual_seed(100 + n)
            kw = dict(h_initial=torch.zeros(n, 1)) if n == 10 else {}
            nets[n] = EGNN_dynamics_AD2_cat(n, 3, hidden_nf=64, n_layers=2, tanh=True, attention=True, condition_beta=True, **kw)
        calls(nets[n], n, B, build_step_table, sched, gam, torch)
        print(f"n={n} B={B} done", flush=True)
    os.environ["PITA_WIDE_NO_MFMA"] = "1"  # read by the library at every call
    for B in (3, 4097):
        calls(nets[22], 22, B, build_step_table, sched, gam, torch)
        print(f"n=22 B={B} PITA_WIDE_NO_MFMA=1 done", flush=True)
else:
    rows = []
    for f in glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("pita::", "")
            if "egnn_wide" in name or "rocclr" in name:
                rows.append((int(r["Start_Timestamp"]), name, r.get("Grid_Size_X", r.get("Grid_Size", "?")),
                             r.get("Workgroup_Size_X", r.get("Workgroup_Size", "?")), r.get("LDS_Block_Size", "?")))
    for _, name, grid, wg, lds in sorted(rows):
        print(f"{name}  grid {grid}  workgroup {wg}  lds {lds}")
