"""The force-field target on amber-sized peptides (tests/_peptides.py): alanine dipeptide with amber's term counts
(22 atoms), zwitterionic tri-alanine (33), ACE-(ALA)3-NME (42) and a 64-atom chain, whose interaction tables need more
than 64 KB of LDS per block.  Against the fp64 oracle (same tolerances as test_hip_parity.test_forcefield_vs_oracle),
fused descent against the per-step path, MALA against the oracle's step, and the whole sampler end to end with the
33- and 42-atom score networks.  Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests._peptides import peptide, peptide_system_xml

pytestmark = pytest.mark.gpu
SCALE = 0.1640
SIZES = {"ala2": 22, "ala3": 33, "ala4": 42, "chain64": 64}


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def _system(name, gb=True):
    tabs, pos = peptide(name)
    if not gb:
        tabs = {k: v for k, v in tabs.items() if not k.startswith("gb_")}
    ff_t = {k: torch.as_tensor(v) for k, v in tabs.items()}
    ff_t = {k: (v.long() if "idx" in k else v.double()) for k, v in ff_t.items()}
    return tabs, ff_t, pos


def _walkers(pos, B, seed, sd=0.004):
    gen = torch.Generator().manual_seed(seed)
    n = pos.shape[0]
    x = torch.tensor(pos.reshape(-1), dtype=torch.float32)[None] + sd * torch.randn(B, 3 * n, generator=gen)
    return O.remove_mean(x / SCALE, n, 3)


@pytest.mark.parametrize("gb", [False, True])
@pytest.mark.parametrize("cutoff", [None, 0.45])
@pytest.mark.parametrize("name", list(SIZES))
def test_peptide_forcefield_vs_oracle(pa, name, cutoff, gb):
    """16 384 walkers; a sample of them against the oracle's autograd forces in fp64; translation invariance."""
    from pita_amd.alp_energy import ForceFieldEnergy

    n = SIZES[name]
    tabs, ff_t, pos = _system(name, gb)
    B = 16384
    x = _walkers(pos, B, 5)
    e = ForceFieldEnergy(tabs, n_particles=n, temperature=300.0, data_normalization_factor=SCALE, cutoff=cutoff)
    lp, f = e(x.cuda(), return_force=True)
    assert torch.equal(lp, e(x.cuda()))
    assert torch.isfinite(lp).all() and torch.isfinite(f).all()
    idx = torch.arange(0, B, 257)
    lpo, fo = O.ff_logp_force(x[idx].double(), ff_t, e.kT, SCALE, cutoff)
    np.testing.assert_allclose(lp[idx.cuda()].cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=2e-3)
    assert rel(f[idx.cuda()], fo) < 5e-5
    assert abs(f.reshape(B, n, 3).sum(1)).max() < 1e-3 * f.abs().max().item()


@pytest.mark.parametrize("name", ["ala4", "chain64"])
def test_peptide_walker_independence(pa, name):
    """A walker's logp and force do not depend on the batch it comes in or on its slot in a block: batches of 1, 7 and
    4 099 (taken from several offsets) give bit-identical results."""
    from pita_amd.alp_energy import ForceFieldEnergy

    n = SIZES[name]
    tabs, _, pos = _system(name)
    x = _walkers(pos, 4099, 8).cuda()
    e = ForceFieldEnergy(tabs, n_particles=n, temperature=300.0, data_normalization_factor=SCALE, cutoff=0.45)
    lp, f = e(x, return_force=True)
    for lo, cnt in ((0, 1), (5, 1), (4098, 1), (0, 7), (3, 7), (2048, 7), (4092, 7)):
        lq, fq = e(x[lo:lo + cnt].contiguous(), return_force=True)
        assert torch.equal(lq, lp[lo:lo + cnt]) and torch.equal(fq, f[lo:lo + cnt]), (lo, cnt)


@pytest.mark.parametrize("name", ["ala2", "ala4"])
def test_peptide_collinear_torsion(pa, name):
    """A walker in which the first three atoms of a torsion lie exactly on one line (the torsion's first normal is
    zero): finite logp and force, and the energy of the oracle (which takes phi = atan2(0, 0) = 0 there as well)."""
    from pita_amd.alp_energy import ForceFieldEnergy

    n = SIZES[name]
    tabs, ff_t, pos = _system(name)
    i, j, k, _ = (int(v) for v in tabs["tors_idx"][0])
    p = pos / SCALE
    # rotate the walker so that j -> k runs along x, then put i on that line behind j: y and z of i, j, k identical
    u = (p[k] - p[j]) / np.linalg.norm(p[k] - p[j])
    a = np.cross(u, [1.0, 0.0, 0.0])
    s, c = np.linalg.norm(a), float(u[0])
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + ax + ax @ ax * ((1 - c) / s**2)
    q = ((p - p[j]) @ R.T).astype(np.float32)
    q[k, 1:] = q[j, 1:]
    q[i] = q[j]
    q[i, 0] = q[j, 0] - np.linalg.norm(p[i] - p[j])
    x = torch.tensor(q.reshape(1, -1))
    e = ForceFieldEnergy(tabs, n_particles=n, temperature=300.0, data_normalization_factor=SCALE, cutoff=None)
    lp, f = e(x.cuda(), return_force=True)
    assert torch.isfinite(lp).all() and torch.isfinite(f).all()
    lpo = -O.ff_energy(x.double(), ff_t, SCALE, None) / e.kT
    np.testing.assert_allclose(lp.cpu().numpy(), lpo.numpy(), rtol=2e-5, atol=2e-3)


@pytest.mark.parametrize("langevin", [False, True])
@pytest.mark.parametrize("name", ["ala2", "ala3", "ala4"])
def test_peptide_fused_descent_equals_per_step(pa, name, langevin):
    """pita_ff_descent takes every handle pita_ff_logp_force takes (one launch plan) and reproduces the per-step path
    bit for bit, with injected and with Philox noise; the fp64 oracle on a sample of the walkers."""
    from pita_amd.alp_energy import ForceFieldEnergy

    n = SIZES[name]
    tabs, ff_t, pos = _system(name)
    x0 = _walkers(pos, 4099, 7).cuda()
    e = ForceFieldEnergy(tabs, n_particles=n, temperature=300.0, data_normalization_factor=SCALE, cutoff=0.45)
    lf = lambda x: O.ff_logp_force(x.double(), ff_t, e.kT, SCALE, 0.45)
    S, dt = 6, 1e-7
    mk = lambda: pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0,
                                          end_resampling_step=1, num_negative_time_steps=S, dt_negative_time=dt,
                                          do_langevin=langevin, seed=3)
    xf = mk().negative_time_descent(x0, e, walker_offset=11)
    xs = mk().negative_time_descent(x0, e, walker_offset=11, fused=False)
    assert torch.equal(xf, xs) and not torch.equal(xf, x0)
    gen = torch.Generator().manual_seed(9)
    nz = torch.randn(S, x0.shape[0], 3 * n, generator=gen)
    xf = mk().negative_time_descent(x0, e, noise=nz.cuda())
    xs = mk().negative_time_descent(x0, e, noise=nz.cuda(), fused=False)
    assert torch.equal(xf, xs)
    sel = torch.arange(0, x0.shape[0], 173)
    xo = O.negative_time_descent(x0.cpu()[sel], lf, S, dt, n, 3, do_langevin=langevin, noise_fn=lambda k, s: nz[k][sel])
    assert rel(xf[sel.cuda()], xo) < 1e-5


def test_peptide_mala_vs_oracle(pa):
    """MALA on the 42-atom ALPEnergy (from its serialized System) with injected normals and uniforms, one step at a
    time, against oracle.mala_step on the same draws: accept decisions agree except where the oracle's log-ratio lies
    within fp32 rounding of log u, positions agree to rel 1e-5 where the decisions agree."""
    from pita_amd.alp_energy import ALPEnergy

    tabs, ff_t, pos = _system("ala4")
    e = ALPEnergy(dimensionality=126, n_particles=42, temperature=300.0, data_normalization_factor=SCALE,
                  system_xml=peptide_system_xml("ala4"))
    lf = lambda x: O.ff_logp_force(x.double(), ff_t, e.kT, SCALE, 2.0)
    B, dt, steps = 2048, 2e-5, 3
    gen = torch.Generator().manual_seed(12)
    x = _walkers(pos, B, 13)
    agree_all, accepted = 0, 0
    for k in range(steps):
        noise = torch.randn(1, B, 126, generator=gen)
        us = torch.rand(1, B, generator=gen)
        integ = pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1,
                                         post_mcmc_steps=1, dt_negative_time=dt, should_mean_free=True)
        out, _ = integ.metropolis_hastings_mala(x.cuda(), e, noise=noise.cuda(), uniforms=us.cuda())
        out = out.cpu()
        xd = x.double()
        lp0, g0 = lf(xd)
        xo, _, acc = O.mala_step(xd, lp0, lf, dt, noise[0].double(), torch.log(us[0].double()))
        xo = O.remove_mean(xo, 42, 3)
        # the oracle's log acceptance ratio (mala_step's formula), to tell a rounding flip from a real disagreement
        xp = xd + 0.5 * dt * g0 + np.sqrt(dt) * noise[0].double()
        lpp, gp = lf(xp)
        ratio = (lpp - lp0) + (-((xd - xp - 0.5 * dt * gp) ** 2).sum(1) + ((xp - xd - 0.5 * dt * g0) ** 2).sum(1)) / (2 * dt)
        hip_acc = (out.double() - xd).norm(dim=1) > 0.5 * (xp - xd).norm(dim=1)
        same = hip_acc == acc
        near = (ratio - torch.log(us[0].double())).abs() < 0.1
        assert bool((same | near).all()), (k, int((~same).sum()), int((~same & ~near).sum()))
        assert rel(out[same], xo[same]) < 1e-5
        agree_all += int(same.sum())
        accepted += int(acc.sum())
        x = out
    print(f"[mala ala4] decisions agree on {agree_all} of {steps * B}; oracle accepted {accepted}")
    assert 0 < accepted < steps * B  # a chain that accepts and rejects


@pytest.mark.parametrize("name", ["ala3", "ala4"])
def test_peptide_sampler_end_to_end(pa, golden, name):
    """ALPEnergy(n_particles=33 / 42, system_xml=...) with EGNN_dynamics_AD2_cat (weights of egnn_ad2cat_sizes.npz)
    through integrate_sde, not debiased, 512 walkers, followed by negative-time descent and MALA: every walker and
    logp finite."""
    from pita_amd.alp_energy import ALPEnergy
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    n = SIZES[name]
    _, _, pos = _system(name)
    e = ALPEnergy(data_path=None, pdb_filename=None, dimensionality=3 * n, n_particles=n, temperature=300.0,
                  data_normalization_factor=SCALE, system_xml=peptide_system_xml(name))
    g = golden("egnn_ad2cat_sizes.npz")
    net = EGNN_dynamics_AD2_cat(n, 3, hidden_nf=32, n_layers=2, condition_beta=True)
    net.load_state_dict({k[len(f"w{n}."):]: torch.tensor(v) for k, v in g.items() if k.startswith(f"w{n}.")})
    sched = pa.ElucidatingNoiseSchedule(sigma_min=0.002, sigma_max=0.05, rho=7)
    sde = pa.VEReverseSDE(noise_schedule=sched, score_net=pa.ScoreNet(net), debias_inference=False)
    integ = pa.WeightedSDEIntegrator(sde=sde, num_integration_steps=20, start_resampling_step=0, end_resampling_step=20,
                                     resampling_interval=-1, num_negative_time_steps=10, post_mcmc_steps=10,
                                     dt_negative_time=1e-7, seed=4)
    x1 = _walkers(pos, 512, 21).cuda()
    x, _, _, _, rates = integ.integrate_sde(x1, e, pa.ConstantAnnealingFactorSchedule(1.0), inverse_temperature=1.0)
    lp = e(x)
    assert x.shape == (512, 3 * n) and torch.isfinite(x).all() and torch.isfinite(lp).all()
    assert len(rates) == 10 and all(0.0 <= r <= 1.0 for r in rates)
