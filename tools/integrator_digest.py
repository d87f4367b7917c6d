"""One SHA-256 per ``integrate_sde`` configuration, over everything a run returns: the bytes of x and of the log-weights,
the counts, the acceptance rates and every array of ``last_weight_stats`` in key order (or None).  All inputs are
injected or seeded (``noise=``, ``resample_u=``, ``seed``), so two trees that drive the same libpita_hip.so alike print
the same lines: run it from the parent commit's Python files and from this one's and compare.
usage: python tools/integrator_digest.py ROOT      (ROOT: the directory whose ``pita_amd`` is imported; the golden weights
are this checkout's).  One line per case: ``<case> <sha256>``.
LJ13 (hidden-32 EGNN, 192 walkers, 8 steps, an event every second step, no descent, no MALA): both regimes x populations
None / 1 / 3 x ess_threshold None / 0.6 / 1.0 / 0.0 x resample_at_end off / on (end_resampling_step 7), and the debiased
fixed case with record_terms, the Hutchinson divergence (4 probes) and start_resampling_step 3.
GMM (MyMLP, 4 x 128 walkers, 10 steps, an event every second step, should_mean_free off, 2 descent steps, 3 MALA steps):
both regimes x populations None / 4 x plain / adaptive MALA; resample_at_end on, except in the not-debiased populations=4
cases, where three rows of the target are not finite instead (the set-aside walkers of quirk Q7)."""
import copy
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE)
import pita_amd as pa  # noqa: E402
from pita_amd import mlp  # noqa: E402
from pita_amd.energy_net import EnergyNet  # noqa: E402

GOLDEN = os.path.join(HERE, "tests", "golden")


def digest(out, stats):
    x, logw, counts, _, rates = out
    h = hashlib.sha256()
    for t in (x, logw):
        h.update(str((tuple(t.shape), str(t.dtype))).encode())
        h.update(t.contiguous().cpu().numpy().tobytes())
    assert all(type(c) is int for c in counts), counts
    h.update(np.array(counts, np.int64).tobytes())
    h.update(np.array(rates, np.float64).tobytes())
    if stats is None:
        h.update(b"None")
    else:
        for k, v in stats.items():
            v = np.asarray(v)
            h.update(f"{k} {v.dtype} {v.shape}".encode())
            h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def uniforms(u, populations):
    """Rows of per-population uniforms as the run takes them: [events, P], or one per event without populations."""
    return [r[0] for r in u] if populations is None else [r[:populations] for r in u]


# ------------------------------------------------------------------------------------------------- LJ13
KW = dict(hidden_nf=32, n_layers=3, recurrent=True, tanh=True, attention=True, condition_time=True, agg="sum")
w = {k: torch.tensor(v) for k, v in np.load(os.path.join(GOLDEN, "egnn_weights_trainedlike.npz")).items()}
net = pa.EGNN_dynamics(13, 3, condition_temperature=True, precision="f16x2", **KW)
net.load_state_dict({k: v for k, v in w.items() if k in net.state_dict()})
sched = pa.ElucidatingNoiseSchedule(sigma_min=0.05, sigma_max=80.0, rho=7)
gam = pa.ConstantAnnealingFactorSchedule(4 / 3)
lj = pa.LennardJonesEnergy(39, 13, 3)
N, B = 8, 192
gen = torch.Generator().manual_seed(22)
x1 = torch.randn(B, 39, generator=gen)
x1 = ((x1.reshape(B, 13, 3) - x1.reshape(B, 13, 3).mean(1, keepdim=True)).reshape(B, 39) * 80.0).cuda()
noise = torch.randn(N, B, 39, generator=gen).cuda()
LJ_U = [[0.3, 0.6, 0.9], [0.15, 0.45, 0.75], [0.0, 0.999999, 0.5], [0.21, 0.01, 0.77]]  # 4 events, either way


def lj13(debias, populations, ess_threshold, at_end, sde_kw={}, **kw):
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), energy_net=EnergyNet(copy.deepcopy(net)),
                          debias_inference=debias, **sde_kw)
    args = dict(sde=sde, num_integration_steps=N, start_resampling_step=0, end_resampling_step=7 if at_end else N,
                resampling_interval=2, num_negative_time_steps=0, post_mcmc_steps=0, seed=3, resample_at_end=at_end,
                ess_threshold=ess_threshold, populations=populations)
    args.update(kw)
    integ = pa.WeightedSDEIntegrator(**args)
    out = integ.integrate_sde(x1, lj, gam, inverse_temperature=1.0, noise=noise, resample_u=uniforms(LJ_U, populations))
    return digest(out, integ.last_weight_stats)


for debias in (False, True):
    for populations in (None, 1, 3):
        for ess_threshold in (None, 0.6, 1.0, 0.0):
            for at_end in (False, True):
                print(f"lj13 debias={debias} populations={populations} ess_threshold={ess_threshold} at_end={at_end}",
                      lj13(debias, populations, ess_threshold, at_end), flush=True)
# events from step 3 on: steps 3, 5, 7
print("lj13 debias=True fixed record_terms hutchinson(4) start=3",
      lj13(True, None, None, False, dict(divergence="hutchinson", n_probes=4), record_terms=True, start_resampling_step=3),
      flush=True)

# ------------------------------------------------------------------------------------------------- GMM
s_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
s_net.load_state_dict({k[2:]: torch.tensor(v) for k, v in np.load(os.path.join(GOLDEN, "mlp_gmm_fwd.npz")).items()
                       if k.startswith("w.")})
torch.manual_seed(17)
e_net = mlp.MyMLP(hidden_size=128, hidden_layers=3, emb_size=128, out_dim=2, input_dim=2)
gsched = pa.ElucidatingNoiseSchedule(sigma_min=0.01, sigma_max=80.0, rho=7)
GN, GP, GS = 10, 4, 128
GB = GP * GS
gen = torch.Generator().manual_seed(79)
gx1 = (torch.randn(GB, 2, generator=gen) * 40.0).cuda()
gnoise = torch.randn(GN, GB, 2, generator=gen).cuda()
GU = torch.rand(GN // 2 + 1, GP, generator=gen, dtype=torch.float64).tolist()  # five due events and the one at the end


class HolesInTheTarget:
    """The GMM target with a non-finite log-density on chosen rows of the full batch."""

    def __init__(self, base, rows):
        self.base, self.rows = base, rows

    def __call__(self, x, return_force=False):
        out = self.base(x, return_force=return_force)
        if x.shape[0] == GB:
            logp = out[0] if return_force else out
            logp[self.rows] = torch.tensor([float("nan"), float("-inf"), float("inf")], device=logp.device)
        return out


for debias in (False, True):
    sde = pa.VEReverseSDE(noise_schedule=gsched, score_net=pa.ScoreNet(s_net), energy_net=EnergyNet(e_net),
                          debias_inference=debias)
    for populations in (None, GP):
        for adaptive_mcmc in (False, True):
            holes = populations is not None and not debias
            target = HolesInTheTarget(pa.GMM(), [5, 200, 511]) if holes else pa.GMM()
            integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=GN, start_resampling_step=0,
                                             end_resampling_step=GN, resampling_interval=2, num_negative_time_steps=2,
                                             post_mcmc_steps=3, adaptive_mcmc=adaptive_mcmc, dt_negative_time=1e-3,
                                             should_mean_free=False, seed=5, resample_at_end=not holes,
                                             populations=populations)
            out = integ.integrate_sde(gx1, target, gam, inverse_temperature=1.0, noise=gnoise,
                                      resample_u=uniforms(GU[:GN // 2 + int(not holes)], populations))
            print(f"gmm debias={debias} populations={populations} adaptive_mcmc={adaptive_mcmc} holes={holes}",
                  digest(out, integ.last_weight_stats), flush=True)
