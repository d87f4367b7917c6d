"""Two ranks on ONE GPU (gloo): integrate_sde with ``populations`` sharded over the ranks must reproduce the single-rank
run, with no collective per step or per event.
run: python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29542 tools/rehearse_populations.py
2 ranks x 2 populations x 64 walkers against 1 rank x 4 populations, LJ13 with the hidden-32 EGNN.  One line per case:
``populations debias=... <case>: x ..., logw ..., counts ..., resampled ..., log_z ..., collectives {...}``."""
import copy, os, sys
from types import SimpleNamespace
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pita_amd as pa
from pita_amd.energy_net import EnergyNet
from pita_amd.sde_integration import _Comm

torch.distributed.init_process_group("gloo")
rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
torch.cuda.set_device(0)
w = dict(np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "egnn_weights_trainedlike.npz")))
net = pa.EGNN_dynamics(13, 3, hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True,
                       condition_time=True, condition_temperature=True, agg="sum")
net.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
e = pa.LennardJonesEnergy(39, 13, 3)
single = SimpleNamespace(trainer=SimpleNamespace(world_size=1, global_rank=0))

calls = {}
for name in ("all_gather", "shared_uniform", "exchange_rows"):
    def wrap(fn, name=name):
        def counted(self, *a, **k):
            if self.world > 1:
                calls[name] = calls.get(name, 0) + 1
            return fn(self, *a, **k)
        return counted
    setattr(_Comm, name, wrap(getattr(_Comm, name)))

P, S = 2 * world, 64
# 0.08: inside the range of the debiased runs' ESS fractions at their due events (0.054 to 0.109 under the fixed schedule),
# so that some populations resample and others keep their weights
cases = {"fixed": dict(), "adaptive": dict(ess_threshold=0.08),
         "fixed + resample_at_end": dict(resample_at_end=True, end_resampling_step=9),
         "adaptive + MALA": dict(ess_threshold=0.08, post_mcmc_steps=3, dt_negative_time=1e-7)}
ok = True
for debias in (False, True):
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=debias)
    N = 12 if not debias else 6
    x1 = pa.Prior(scale=3.0, n_particles=13, spatial_dim=3, seed=2).sample(P * S)
    for name, extra in cases.items():
        kw = dict(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=N, resampling_interval=3,
                  seed=11, num_negative_time_steps=0, post_mcmc_steps=0, populations=P)
        kw.update(extra)
        kw["end_resampling_step"] = min(kw["end_resampling_step"], N - 1) if "resample_at_end" in extra else N
        n_events = len([s for s in range(kw["end_resampling_step"]) if (s + 1) % 3 == 0]) + int("resample_at_end" in extra)
        u = torch.rand(n_events, P, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        outs = []
        for lm in (None, single):  # None -> torch.distributed world; `single` -> one rank does everything
            calls.clear()
            integ = pa.WeightedSDEIntegrator(lightning_module=lm, **kw)
            x, logw, uniq, _, acc = integ.integrate_sde(x1, e, gam, inverse_temperature=1.0, resample_u=u)
            outs.append((x.cpu(), logw.cpu(), uniq, integ.last_weight_stats, dict(calls)))
        (xa, wa, ca, sa, col), (xb, wb, cb, sb, _) = outs
        word = lambda a, b: "bitwise" if torch.equal(a, b) else "allclose" if torch.allclose(a, b, rtol=1e-4, atol=1e-5) \
            else "DIFFERENT (max %.3g)" % float((a - b).abs().max())
        dz = float(np.abs(sa["log_z"] - sb["log_z"]).max())
        line = (f"populations debias={debias} {name}: x {word(xa, xb)}, logw {word(wa, wb)}, "
                f"counts {'equal' if ca == cb else 'DIFFERENT'}, "
                f"resampled {'equal' if np.array_equal(sa['resampled'], sb['resampled']) else 'DIFFERENT'}, "
                f"n_unique {'equal' if np.array_equal(sa['n_unique'], sb['n_unique']) else 'DIFFERENT'}, "
                f"log_z {'equal' if dz == 0.0 else 'max abs difference %.3g' % dz}, events resampled "
                f"{int(sa['resampled'].sum())} of {int(np.isfinite(sa['ess']).sum())} (ESS fractions "
                f"{np.nanmin(sa['ess_fraction']):.3f} to {np.nanmax(sa['ess_fraction']):.3f}), collectives {col}")
        if rank == 0:
            print(line, flush=True)
        # the end-of-run gathers only: walkers, event log, term moments (two buffers when debiased), log-weights
        gathers = 3 + (2 if debias else int("resample_at_end" in extra))
        ok = ok and "DIFFERENT" not in line and col == {"all_gather": gathers}
torch.distributed.barrier()
torch.distributed.destroy_process_group()
sys.exit(0 if ok else 1)
