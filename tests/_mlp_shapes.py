"""Shared by tests/test_mlp_shapes_cpu.py and tests/test_mlp_shapes_gpu.py (and the moved helper of
tests/test_mlp_debiased_gpu.py): seeded MLP backbones over the shapes the host code accepts, their fp64 / fp32 oracle
values with derivatives, the fp64 oracle with a perturbed embedding, and the bounds derived from those three.

How a bound is set (never from a kernel's output): for a compared quantity q at one noise level,
    e32   = rel-L2(q from the fp32 oracle, q from the fp64 oracle)             the reference's own fp32 error
    floor = 4 * rel-L2(q from the fp64 oracle with every sinusoidal-embedding entry moved by a seeded uniform value in
            +-1e-6, q from the fp64 oracle)     what the kernels document and the fp32 reference does not have: sin / cos
            of revolutions on the transcendental unit (absolute error ~1e-6) and erf_as (1.5e-7), csrc/mlp_common.h
    bound = max(4 * e32, floor, 1.2e-7)        factor 4 as test_egnn_golden; 1.2e-7 = one fp32 rounding, as _C1_BOUNDS
and no bound may exceed what the older tests allow (CAP_FORWARD, CAP_DERIV)."""
import numpy as np
import torch

from oracle import pita_oracle as O

CAP_FORWARD, CAP_DERIV = 2e-5, 5e-5  # tests/test_hip_parity.py::test_mlp_golden, test_mlp_debiased_gpu.py
ONE_ULP = 1.2e-7
PERTURB = 1e-6
LEVELS = (1e-3, 1e-2, 0.3, 4.0, 70.0, 6400.0)  # 6400 = sigma_max^2: the first step of every run

# (hidden, hidden_layers, D, temperature): D = 39 is LJ13 flattened; 31 / 32 / 33 straddle the output-block edge, 52 / 53 the
# sampler's 64 KB dynamic-LDS arithmetic; D = 1 leaves the hh = 1 lanes of the `var += 2` loops idle; layers 0 and 1
CONFIGS = [(32, 0, 1, False), (32, 1, 31, True), (32, 2, 33, True), (32, 1, 64, False), (64, 1, 32, False),
           (64, 2, 39, True), (64, 2, 64, False), (128, 3, 52, False), (128, 1, 53, True), (128, 3, 64, True),
           (64, 0, 2, True), (128, 0, 3, False)]


def cfg_id(c):
    return f"h{c[0]}_l{c[1]}_d{c[2]}_{'temp' if c[3] else 'plain'}"


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def make_net(hidden, layers, D, temp, out_dim=None, seed=None):
    """(HIP module, fp64 state dict, oracle kwargs) by seeded construction (the reference's parameter order)."""
    from pita_amd import mlp

    torch.manual_seed(1000 + 7 * hidden + 131 * layers + D + (5 if temp else 0) if seed is None else seed)
    cls = mlp.MyMLPTemperature if temp else mlp.MyMLP
    net = cls(hidden_size=hidden, hidden_layers=layers, emb_size=hidden, out_dim=D if out_dim is None else out_dim,
              input_dim=D)
    wd = {k: v.double() for k, v in net.state_dict().items()}
    return net, wd, dict(emb_size=hidden, hidden_layers=layers, temperature_conditioned=temp)


def backbone(wd, kw, dtype=torch.float64):
    w = {k: v.to(dtype) for k, v in wd.items()}
    return lambda cn, xs, b: O.mlp_forward(w, cn, xs, b, **kw)


# ---- the oracle's MLP in two halves, so that the embedding can be replaced or perturbed
def embed(t, x, beta, emb_size, temperature_conditioned, angle32=False):
    """The concatenated sinusoidal embedding of O.mlp_forward.  ``angle32``: the angle (v*scale)*f is formed in fp32
    exactly as O.sinusoidal_embedding forms it on fp32 inputs, then converted; sin / cos in the dtype of ``x``."""
    def one(v, scale):
        if not angle32:
            return O.sinusoidal_embedding(v, emb_size, scale)
        half = emb_size // 2
        w = torch.log(torch.tensor([10000.0])) / (half - 1)
        f = torch.exp(-w * torch.arange(half))
        e = ((v.float() * scale)[:, None] * f[None]).to(v.dtype)
        return torch.cat([torch.sin(e), torch.cos(e)], dim=-1)

    embs = [one(x[:, i], 25.0) for i in range(x.shape[-1])] + [one(t, 1.0)]
    if temperature_conditioned:
        embs.append(one(beta, 1.0))
    return torch.cat(embs, dim=-1)


def mlp_tail(p, z, hidden_layers):
    """O.mlp_forward after the embedding."""
    P = {k: v.to(z.dtype) for k, v in p.items()}
    z = O._gelu(z @ P["joint_mlp.0.weight"].T + P["joint_mlp.0.bias"])
    for l in range(1, hidden_layers + 1):
        z = z + O._gelu(z @ P[f"joint_mlp.{l}.ff.weight"].T + P[f"joint_mlp.{l}.ff.bias"])
    L = hidden_layers + 1
    return z @ P[f"joint_mlp.{L}.weight"].T + P[f"joint_mlp.{L}.bias"]


def forward_restated(wd, kw, t, x, beta, delta=None, angle32=False):
    """O.mlp_forward restated through embed / mlp_tail; ``delta`` [B, C] is added to the embedding."""
    z = embed(t, x, beta, kw["emb_size"], kw["temperature_conditioned"], angle32)
    return mlp_tail(wd, z if delta is None else z + delta, kw["hidden_layers"])


def emb_delta(B, D, kw, seed=12345):
    """The seeded perturbation of every embedding entry: uniform in +-PERTURB, fp64."""
    C = kw["emb_size"] * (D + 1 + (1 if kw["temperature_conditioned"] else 0))
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, C, generator=g, dtype=torch.float64) * 2 - 1) * PERTURB


def perturbed_backbone(wd, kw, delta):
    """The fp64 backbone whose embedding carries ``delta`` [B, C] (rows in batch order)."""
    return lambda cn, xs, b: forward_restated(wd, kw, cn, xs, b, delta=delta)


# ---- derivatives of the denoiser
def _oracle_derivs(bb, h, x, beta):
    """D, F, J_x D [B, D, D], dD/dh [B, D] by vmap(jacrev) through O.denoiser, in the dtype of the inputs."""
    from torch.func import jacrev, vmap

    def one(h1, x1, b1):
        return O.denoiser(bb, h1.reshape(1), x1.reshape(1, -1), b1.reshape(1)).squeeze(0)

    dDdh, J = vmap(jacrev(one, argnums=(0, 1)))(h, x, beta)
    c_s, c_in, c_out, c_noise = O.edm_coeffs(h)
    F = bb(c_noise, c_in[:, None] * x, beta)
    return O.denoiser(bb, h, x, beta), F, J, dDdh


def _perturbed_derivs(wd, kw, h, x, beta, delta):
    """_oracle_derivs of the fp64 oracle whose embedding carries ``delta`` (a constant of each walker)."""
    from torch.func import jacrev, vmap

    def one(h1, x1, b1, d1):
        bb = lambda cn, xs, b: forward_restated(wd, kw, cn, xs, b, delta=d1[None])
        return O.denoiser(bb, h1.reshape(1), x1.reshape(1, -1), b1.reshape(1)).squeeze(0)

    dDdh, J = vmap(jacrev(one, argnums=(0, 1)))(h, x, beta, delta)
    bb = lambda cn, xs, b: forward_restated(wd, kw, cn, xs, b, delta=delta)
    c_s, c_in, c_out, c_noise = O.edm_coeffs(h)
    return O.denoiser(bb, h, x, beta), bb(c_noise, c_in[:, None] * x, beta), J, dDdh


def unit_dirs(D):
    """A unit direction in each output block and at its edges: 0, 31, 32, D-1 where they exist."""
    return sorted({k for k in (0, 31, 32, D - 1) if 0 <= k < D})


def quantities(Dv, F, J, dDdh, h, x, cot, vx, vh):
    """Everything pita_mlp_jacobian / pita_mlp_jvp return, from D, F, J, dD/dh, in their dtype."""
    c_s, c_in, c_out, _ = O.edm_coeffs(h)
    q = {"D": Dv, "trace": torch.diagonal(J, dim1=1, dim2=2).sum(-1)}
    for cname, cv in (("x", x), ("dense", cot)):
        dho = (cv * dDdh).sum(-1)
        q[f"vjp_{cname}"] = torch.einsum("bi,bik->bk", cv, J)
        q[f"dot_h_{cname}"] = dho
        q[f"parts0_{cname}"] = c_out * (cv * F).sum(-1)
        q[f"parts1_{cname}"] = dho + c_s**2 * (cv * x).sum(-1)
    ks = unit_dirs(x.shape[1])
    for k in ks:
        q[f"jvp_unit_{k}"] = J[:, :, k]
    q["jvp_dot_out"] = torch.stack([torch.einsum("bi,bi->b", x, J[:, :, k]) for k in ks], dim=1)
    q["jvp_diag_acc"] = sum(J[:, k, k] for k in ks)
    Jv = torch.einsum("bij,bj->bi", J, vx)
    q["jvp_dense"] = Jv
    q["jvp_vh"] = dDdh * vh[:, None]
    q["jvp_vh_dot"] = (x * dDdh).sum(-1) * vh
    q["jvp_both"] = Jv + dDdh * vh[:, None]
    return q


def sweep_inputs(D, walkers_per_level, seed=0):
    """fp32 inputs of the configuration sweep: the noise levels LEVELS interleaved (walker b has level b % 6)."""
    gen = torch.Generator().manual_seed(900 + D + seed)
    nl = len(LEVELS)
    B = nl * walkers_per_level
    h = torch.tensor(LEVELS)[torch.arange(B) % nl]
    x = (torch.randn(B, D, generator=gen) * (1 + h.sqrt())[:, None]).float()
    beta = (torch.rand(B, generator=gen) + 0.5).float()
    cot = torch.randn(B, D, generator=gen).float()
    vx = torch.randn(B, D, generator=gen).float()
    vh = torch.randn(B, generator=gen).float()
    return dict(h=h, x=x, beta=beta, cot=cot, vx=vx, vh=vh)


def backbone_inputs(inp):
    """(c_noise, c_in x) as fp32 tensors: the SAME values go to the kernel and, converted, to both oracles."""
    _, c_in, _, c_noise = O.edm_coeffs(inp["h"])
    return c_noise.float(), (c_in[:, None] * inp["x"]).float()


def reference_sets(wd, kw, inp, derivs=True):
    """{"F": ...} (+ every derivative quantity) from the fp64 oracle, the fp32 oracle and the perturbed fp64 oracle."""
    B, D = inp["x"].shape
    delta = emb_delta(B, D, kw)
    cn, xs = backbone_inputs(inp)
    out = []
    for mode in ("fp64", "fp32", "perturbed"):
        dt = torch.float32 if mode == "fp32" else torch.float64
        a = {k: v.to(dt) for k, v in inp.items()}
        if mode == "perturbed":
            q = {"F": forward_restated(wd, kw, cn.to(dt), xs.to(dt), a["beta"], delta=delta)}
        else:
            q = {"F": backbone(wd, kw, dt)(cn.to(dt), xs.to(dt), a["beta"])}
        if derivs:
            if mode == "perturbed":
                dv = _perturbed_derivs(wd, kw, a["h"], a["x"], a["beta"], delta)
            else:
                dv = _oracle_derivs(backbone(wd, kw, dt), a["h"], a["x"], a["beta"])
            q.update(quantities(*dv, a["h"], a["x"], a["cot"], a["vx"], a["vh"]))
        out.append({k: v.detach() for k, v in q.items()})
    return tuple(out)


def level_masks(B, n_levels=len(LEVELS)):
    return [(torch.arange(B) % n_levels) == i for i in range(n_levels)]


def derive_bounds(r64, r32, rp, masks):
    """{name: [(bound, e32, floor) per mask]} by the rule in the module docstring."""
    out = {}
    for name in r64:
        rows = []
        for m in masks:
            e32 = rel(r32[name][m], r64[name][m])
            floor = 4 * rel(rp[name][m], r64[name][m])
            rows.append((max(4 * e32, floor, ONE_ULP), e32, floor))
        out[name] = rows
    return out


def cap_of(name):
    return CAP_FORWARD if name == "F" else CAP_DERIV


# ---- the fused sampler's arithmetic as a plain loop
SAMPLER_CASES = [(64, 1, 1, 1), (64, 6, 2, 3), (64, 39, 13, 3), (64, 52, 13, 4), (64, 53, 53, 1), (64, 64, 16, 4),
                 (128, 1, 1, 1), (128, 6, 2, 3), (128, 39, 13, 3), (128, 52, 13, 4), (128, 53, 53, 1), (128, 64, 16, 4),
                 (32, 64, 16, 4)]  # (hidden, D, n_particles, n_dim)


def step_table(n_steps, beta=1.0, sigma_min=0.05, sigma_max=80.0, gamma=4 / 3, diffusion_scale=1.0):
    """The host's fp32 step table for ``n_steps`` Euler-Maruyama steps over t in (0, 1] (no GPU needed)."""
    import pita_amd
    from pita_amd.sde_integration import _build_step_table

    sched = pita_amd.ElucidatingNoiseSchedule(sigma_min=sigma_min, sigma_max=sigma_max, rho=7)
    gam = pita_amd.ConstantAnnealingFactorSchedule(gamma)
    times = torch.linspace(1.0, 0.0, n_steps + 1)[:-1]
    return _build_step_table(sched, gam, times, 1.0 / n_steps, diffusion_scale, beta)


def oracle_sampler_loop(bb, tab, x, noise, n, d, remove_mean, dtype=torch.float64, bb_of_step=None):
    """mlp_sampler_kernel's steps from O.denoiser and the step table, in ``dtype``:
    drift = gamma*((D_theta - x)/h * g2); x += drift*dt + noise_scale*xi*sqrt_dt; then O.remove_mean.
    Returns (x, stats [n_steps, 4]: sums of drift, drift^2, diffusion, diffusion^2 with diffusion = noise_scale*xi).
    ``bb_of_step(s)``: a backbone per step (the perturbed oracle draws a fresh perturbation every step)."""
    from pita_amd import _lib

    x = x.to(dtype).clone()
    tab = tab.to(dtype)
    stats = torch.zeros(tab.shape[0], 4, dtype=dtype)
    for s in range(tab.shape[0]):
        st = tab[s]
        h = st[_lib.ST_H] * torch.ones(x.shape[0], dtype=dtype)
        Dth = O.denoiser(bb if bb_of_step is None else bb_of_step(s), h, x, st[_lib.ST_BETA])
        drift = st[_lib.ST_GAMMA] * ((Dth - x) / st[_lib.ST_H] * st[_lib.ST_G2])
        dif = st[_lib.ST_NOISE_SCALE] * noise[s].to(dtype)
        stats[s] = torch.stack([drift.sum(), (drift * drift).sum(), dif.sum(), (dif * dif).sum()])
        x = x + (drift * st[_lib.ST_DT] + dif * st[_lib.ST_SQRT_DT])
        if remove_mean:
            x = O.remove_mean(x, n, d)
    return x, stats


def sampler_reference_sets(wd, kw, tab, x0, noise, n, d, remove_mean):
    """(fp64, fp32, perturbed fp64) results {"x": final walkers, "stats": [n_steps, 4]} of oracle_sampler_loop."""
    B, D = x0.shape
    out = []
    for mode in ("fp64", "fp32", "perturbed"):
        dt = torch.float32 if mode == "fp32" else torch.float64
        if mode == "perturbed":
            per_step = lambda s: perturbed_backbone(wd, kw, emb_delta(B, D, kw, seed=777 + s))
            xf, st = oracle_sampler_loop(None, tab, x0, noise, n, d, remove_mean, dt, bb_of_step=per_step)
        else:
            xf, st = oracle_sampler_loop(backbone(wd, kw, dt), tab, x0, noise, n, d, remove_mean, dt)
        out.append({"x": xf, "stats": st})
    return tuple(out)


def sampler_inputs(D, n, d, B, n_steps, seed=0, scale=80.0):
    """Walkers drawn at the prior's scale (sigma_max), mean-free for particle systems, and injected noise."""
    gen = torch.Generator().manual_seed(4000 + D + seed)
    x0 = torch.randn(B, D, generator=gen) * scale
    if n > 1:
        x0 = O.remove_mean(x0, n, d)
    return x0.float().contiguous(), torch.randn(n_steps, B, D, generator=gen).float().contiguous()


# ---- the plain forward on unscaled coordinates
LARGE_ANGLE_CONFIGS = [(64, 2, 3, True), (128, 3, 2, True), (32, 2, 6, True), (64, 2, 39, True)]


def large_angle_inputs(D, B, seed=0):
    gen = torch.Generator().manual_seed(50 + D + seed)
    x = (torch.rand(B, D, generator=gen) * 2 - 1) * 400.0  # angles x * 25 * f up to 1e4 rad
    x[0, 0], x[1, -1] = 400.0, -400.0
    t = (torch.rand(B, generator=gen) * 2 - 1) * 50.0
    beta = torch.rand(B, generator=gen) * 50.0
    return x.float(), t.float(), beta.float()


def large_angle_references(wd, kw, x, t, beta):
    """(fp64 restatement of the fp32 angle, fp32 oracle, perturbed restatement) of the plain forward."""
    r64 = forward_restated(wd, kw, t.double(), x.double(), beta.double(), angle32=True)
    r32 = backbone(wd, kw, torch.float32)(t, x, beta)
    rp = forward_restated(wd, kw, t.double(), x.double(), beta.double(), angle32=True,
                            delta=emb_delta(x.shape[0], x.shape[1], kw))
    return r64, r32, rp


# the four sums are held to the forward allowance like the walkers themselves
STATS_CAPS = (CAP_FORWARD,) * 4
STATS_NAMES = ("sum_drift", "sum_drift2", "sum_diffusion", "sum_diffusion2")


def stats_steps(n, remove_mean, n_steps):
    """The steps whose sums are compared.  With ONE particle and mean removal every walker is exactly 0 from the end of
    step 0 on (the mean of one particle is the particle), so the sums of the later steps are B copies of one number,
    gamma g2 c_out F(0) / h, in which the output head cancels ~200-fold (summands of magnitude 1 against |F(0)| ~ 5e-3):
    their relative error measures that one ill-conditioned value, not the sampler.  Step 0, where the walkers still
    differ, is compared; mean removal off covers all steps of the same nets."""
    return [0] if (n == 1 and remove_mean) else list(range(n_steps))


def stats_errors(got, ref, count, steps=None):
    """Errors of the sampler's per-step sums [n_steps, 4] = (sum d, sum d^2, sum n, sum n^2) against ``ref``: the second
    moments relative to themselves; the first moments, sums of signed terms that cancel to ~1e-5 of what was added,
    relative to sqrt(count * second moment) >= sum |term| (Cauchy-Schwarz), the scale their rounding lives on (one
    term of B * D with a wrong sign moves it by ~2 / (B D), four orders above the bounds below).  Worst of ``steps``."""
    got, ref = got.double(), ref.double()
    scale = torch.stack([(count * ref[:, 1]).sqrt(), ref[:, 1], (count * ref[:, 3]).sqrt(), ref[:, 3]], dim=1)
    err = (got - ref).abs() / scale.clamp_min(1e-300)
    return (err if steps is None else err[steps]).max(dim=0).values


def stats_bounds(s64, s32, sp, count, steps=None):
    """[(bound, e32, floor)] of the four sums by the module's rule, before the caps."""
    e32s, fls = stats_errors(s32, s64, count, steps), 4 * stats_errors(sp, s64, count, steps)
    return [(max(4 * float(e), float(f), ONE_ULP), float(e), float(f)) for e, f in zip(e32s, fls)]
