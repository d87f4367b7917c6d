"""The debiased regime on the MLP backbones without a GPU: the yardstick itself (O.f_debiased with an MLP backbone against
central finite differences in fp64) and the register / scratch figures of the derivative kernel (csrc/mlp_jac_kernel.hip)
read from the built object, as DESIGN.md section 4.3 publishes them."""
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import pita_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_oracle_debiased_terms_with_mlp_backbone_vs_finite_differences():
    """O.f_debiased (autograd / vmap(jacrev)) on MLP score and energy backbones against central differences of
    O.energy_theta and O.score in fp64: grad_x E, div s, dE/dt and everything assembled from them."""
    from pita_amd import mlp

    torch.manual_seed(3)
    net = mlp.MyMLPTemperature(hidden_size=32, hidden_layers=2, emb_size=32, out_dim=4, input_dim=4)
    ws = {k: v.double() for k, v in net.state_dict().items()}
    we = {k: 0.8 * v.double() for k, v in net.state_dict().items()}
    kw = dict(emb_size=32, hidden_layers=2, temperature_conditioned=True)
    bs = lambda cn, xs, b: O.mlp_forward(ws, cn, xs, b, **kw)
    be = lambda cn, xs, b: O.mlp_forward(we, cn, xs, b, **kw)
    sched, gam = O.Elucidating(0.01, 80.0, 7), O.GammaConstant(4 / 3)
    beta, B, D, eps = 1.25, 6, 4, 1e-6
    gen = torch.Generator().manual_seed(4)
    for tv in (0.2, 0.7):
        t = torch.tensor(tv, dtype=torch.float64)
        x = torch.randn(B, D, generator=gen, dtype=torch.float64) * 3
        ref = O.f_debiased(bs, be, sched, gam, t, x, beta, clamp_quantile=None)
        tb = t * torch.ones(B, dtype=torch.float64)
        h, g2, gamma = sched.h(tb), sched.g(tb) ** 2, float(gam.gamma(t))
        E = lambda xx, hh=h: O.energy_theta(be, hh, xx, beta)
        s = O.score(bs, h, x, beta)
        gE, div = torch.empty(B, D, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
        for i in range(D):
            e = torch.zeros(D, dtype=torch.float64)
            e[i] = eps
            gE[:, i] = (E(x + e) - E(x - e)) / (2 * eps)
            div += (O.score(bs, h, x + e, beta)[:, i] - O.score(bs, h, x - e, beta)[:, i]) / (2 * eps)
        dEdt = (E(x, sched.h(tb + eps)) - E(x, sched.h(tb - eps))) / (2 * eps)
        bt = s * g2[:, None] / 2
        cross = (-gE * bt).sum(-1)
        div_bt = div * g2 / 2
        drift_A = gamma * gamma * cross + gamma * div_bt + gamma * dEdt + gam.dgamma_dt(tb) * E(x)
        want = dict(drift_X=gamma * -gE * g2[:, None] / 2 + gamma * bt, divergence_score=div_bt, cross_term=cross,
                    dUt_dt=dEdt, drift_A=drift_A)
        for nm, w in want.items():
            got = getattr(ref, nm).detach()
            np.testing.assert_allclose(got.numpy(), w.numpy(), rtol=1e-6, atol=1e-6 * float(w.abs().mean()),
                                       err_msg=f"t={tv} {nm}")


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the ROCm LLVM binutils")
def test_mlp_jacobian_kernel_registers(tmp_path):
    """Every instantiation of mlp_jac_kernel runs one wave per SIMD (512 registers) and carries the primal and its K
    tangent tiles without scratch, the weight loop included (the figures of DESIGN.md section 4.3)."""
    import pita_amd.build as build
    from tests.test_kernel_resources import _kernels

    build.build(verbose=False)
    k = _kernels(os.path.join(ROOT, "pita_amd", "csrc", "mlp_jac_kernel.o"), str(tmp_path))
    jac = {n: r for n, r in k.items() if n.startswith("mlp_jac_kernel")}
    # hidden 32 / 64 / 128 x (jvp: one tangent, jacobian: K = 4 / 2 / 1) x (weight stream, L2 weights)
    assert len(jac) == 10, sorted(jac)
    for name, r in sorted(jac.items()):
        # (.vgpr_count of a gfx950 kernel is the unified figure: architectural VGPRs up to accum_offset plus AGPRs)
        print(f"{name}: {r['vgpr']} registers ({r['agpr']} of them AGPRs), scratch {r['scratch']} B/lane")
        assert r["scratch"] == 0 and r["vgpr"] <= 512, (name, r)
    assert jac["mlp_jac_kernel<4, 1, true>"]["vgpr"] <= 480
