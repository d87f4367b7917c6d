"""The three MLP kernels (mlp_kernel, mlp_sampler_kernel, mlp_jac_kernel) over the shapes, batches and launch
parameters their host code accepts, against the fp64 oracle: input dimensions up to 64 (two output blocks), 0 to 3
residual layers, both weight sources, ragged and tiny batches, the second trip of the grid-stride loop, the fused
sampler against an fp64 loop with its Philox keying and per-step sums, unscaled coordinates (angles up to 1e4 rad) and
the host-side contracts.  Every bound is derived at test time from the oracle alone (tests/_mlp_shapes.py); every walker
of every batch is compared.  Run on an MI355X: pytest -m gpu.  The figures printed there are kept in
profiles/mlp_shapes_measured.txt."""
import numpy as np
import pytest
import torch

from oracle import pita_oracle as O
from tests import _mlp_shapes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


class _Report:
    """Collects error / bound of every compared figure, prints per quantity the one closest to its bound (on a line of
    its own: `grep '^\\[mlp shapes'`), and asserts once at the end, so that a failing run still shows all of them."""

    def __init__(self, tag):
        self.tag, self.worst, self.bad, self.n = tag, {}, [], 0

    def check(self, name, where, err, bound, note=""):
        self.n += 1
        if name not in self.worst or err / bound > self.worst[name][1] / self.worst[name][2]:
            self.worst[name] = (where, float(err), float(bound))
        if not err <= bound:
            self.bad.append((name, where, float(err), float(bound), note))

    def finish(self):
        print(f"\n[mlp shapes {self.tag}] {self.n} figures, error/bound closest to the bound: " +
              ", ".join(f"{k} {e:.1e}/{b:.1e}@{w}" for k, (w, e, b) in self.worst.items()))
        assert not self.bad, (self.tag, self.bad)


def _check_levels(rep, got, r64, bounds, masks, labels):
    for name, g in got.items():
        for m, lab, (b, e32, floor) in zip(masks, labels, bounds[name]):
            rep.check(name, lab, S.rel(g.cpu()[m], r64[name][m]), min(b, S.cap_of(name)), f"e32 {e32:.1e} floor {floor:.1e}")


def _forward(net, cn, xs, beta):
    return net(cn.cuda(), xs.cuda(), beta.cuda() if net._temperature else None)


def _kernel_quantities(net, inp):
    """Every output of pita_mlp_forward / pita_mlp_jacobian / pita_mlp_jvp under the names of S.quantities."""
    c = {k: v.cuda() for k, v in inp.items()}
    h, x, beta = c["h"], c["x"], c["beta"]
    B, D = x.shape
    cn, xs = S.backbone_inputs(inp)
    q = {"F": _forward(net, cn, xs, inp["beta"])}
    tr, Dk = net.jacobian_trace(h, x, beta, want_denoiser=True)
    q["D"], q["trace"] = Dk, tr
    for cname, cv in (("x", None), ("dense", c["cot"])):
        r = net.jacobian(h, x, beta, cot=cv, want_denoiser=True, want_trace=True, want_vjp=True, want_dot_h=True,
                         want_h_parts=True)
        assert torch.equal(r["D"], Dk) and torch.equal(r["trace"], tr), cname  # all five outputs from one launch
        Dv, vj, dh, parts = net.vjp(h, x, beta, cot=cv, want_dot_h=True, want_h_parts=True)
        assert torch.equal(Dv, Dk) and torch.equal(vj, r["vjp"]) and torch.equal(dh, r["dot_h"]), cname
        assert torch.equal(parts, r["h_parts"]), cname
        q[f"vjp_{cname}"], q[f"dot_h_{cname}"] = r["vjp"], r["dot_h"]
        q[f"parts0_{cname}"], q[f"parts1_{cname}"] = r["h_parts"][:, 0], r["h_parts"][:, 1]
    ks = S.unit_dirs(D)
    diag = torch.zeros(B, device="cuda")
    dots = torch.full((B, len(ks)), float("nan"), device="cuda")
    for j, k in enumerate(ks):
        out, dout = net.jvp(h, x, beta, direction=k, dot_out=dots, dot_col=j, diag_acc=diag)
        assert torch.equal(out, Dk), k
        q[f"jvp_unit_{k}"] = dout
    q["jvp_dot_out"], q["jvp_diag_acc"] = dots, diag
    q["jvp_dense"] = net.jvp(h, x, beta, vx=c["vx"])[1]
    dot_h1 = torch.zeros(B, device="cuda")
    q["jvp_vh"] = net.jvp(h, x, beta, vh=c["vh"], dot_out=dot_h1)[1]
    q["jvp_vh_dot"] = dot_h1
    q["jvp_both"] = net.jvp(h, x, beta, vx=c["vx"], vh=c["vh"])[1]
    return q


# ------------------------------------------------------------------ 1. configuration sweep
@pytest.mark.parametrize("cfg", S.CONFIGS, ids=S.cfg_id)
def test_config_sweep_vs_oracle(pa, cfg):
    """Backbone output, denoiser, trace, vjp (cot = x and dense) with dot_h and its split, jvp (unit directions in each
    output block with dot_out / diag_acc, dense vx, vh, both) against the fp64 oracle and vmap(jacrev) of O.denoiser, per
    noise level, B = 642 (a last tile of 2 walkers, two waves of the last workgroup past B)."""
    net, wd, kw = S.make_net(*cfg)
    inp = S.sweep_inputs(cfg[2], 107)
    r64, r32, rp = S.reference_sets(wd, kw, inp)
    masks = S.level_masks(inp["x"].shape[0])
    bounds = S.derive_bounds(r64, r32, rp, masks)
    got = _kernel_quantities(net, inp)
    assert set(got) == set(r64)
    rep = _Report(S.cfg_id(cfg))
    _check_levels(rep, got, r64, bounds, masks, [f"h={h:g}" for h in S.LEVELS])
    rep.finish()


# ------------------------------------------------------------------ 2. batch edges and the grid-stride loop
_EDGE_CASES = [((64, 2, 39, True), 13, 3), ((32, 1, 64, False), 16, 4)]  # streamed weights / hidden 32 (L2 weights)
_JAC_ALL = dict(want_denoiser=True, want_trace=True, want_vjp=True, want_dot_h=True, want_h_parts=True)


def _random_batch(D, B, seed):
    gen = torch.Generator().manual_seed(seed)
    h = 10.0 ** (torch.rand(B, generator=gen) * 6.8 - 3)  # 1e-3 .. 6.3e3
    x = torch.randn(B, D, generator=gen) * (1 + h.sqrt())[:, None]
    beta = torch.rand(B, generator=gen) + 0.5
    return h.float(), x.float(), beta.float()


@pytest.mark.parametrize("case", _EDGE_CASES, ids=lambda c: S.cfg_id(c[0]))
def test_batch_edges_bit_equal_to_a_larger_batch(pa, case):
    """B in {1, 31, 32, 33, 127, 128, 129, 4097} at three offsets of an 8 192-walker batch: forward, all Jacobian
    outputs and three fused sampler steps are bit-equal to the same rows of the whole batch."""
    cfg, n, d = case
    net, _, _ = S.make_net(*cfg)
    D, BIG, N = cfg[2], 8192, 3
    h, x, beta = (v.cuda() for v in _random_batch(D, BIG, 31))
    cn, xs = S.backbone_inputs(dict(h=h.cpu(), x=x.cpu()))
    cn, xs = cn.cuda(), xs.cuda()
    tab = S.step_table(N, beta=1.1).cuda()
    x0, noise = S.sampler_inputs(D, n, d, BIG, N)
    x0, noise = x0.cuda(), noise.cuda()
    fwd = net(cn, xs, beta)
    jac = net.jacobian(h, x, beta, **_JAC_ALL)
    smp = net.sampler_run(x0.clone(), tab, N, noise=noise, n_particles=n, n_dim=d)
    assert torch.isfinite(fwd).all() and torch.isfinite(smp).all() and not torch.equal(smp, x0)
    for m in (1, 31, 32, 33, 127, 128, 129, 4097):
        for off in (0, 1001, BIG - m):
            sl = slice(off, off + m)
            assert torch.equal(net(cn[sl], xs[sl], beta[sl]), fwd[sl]), ("forward", m, off)
            s = net.jacobian(h[sl], x[sl], beta[sl], **_JAC_ALL)
            for k in jac:
                assert torch.equal(s[k], jac[k][sl]), ("jacobian", k, m, off)
            got = net.sampler_run(x0[sl].clone(), tab, N, noise=noise[:, sl].contiguous(), n_particles=n, n_dim=d)
            assert torch.equal(got, smp[sl]), ("sampler", m, off)


_STRIDE_CASES = [((128, 3, 2, False), 1, 2), ((32, 2, 6, True), 2, 3)]  # config C1's shape (streamed) / hidden 32


def _assert_tiled(name, out, block):
    """Every copy of the first `block` rows in `out` is bit-identical to the first one (the ragged tail included)."""
    B = out.shape[0]
    full = B // block
    first = out[:block]
    body = out[:full * block].reshape(full, block, *out.shape[1:])
    same = (body == first[None]).reshape(full, -1).all(dim=1)
    assert bool(same.all()), (name, "copies differing from the first", torch.nonzero(~same).flatten()[:8].tolist())
    tail = out[full * block:]
    assert torch.equal(tail, first[:tail.shape[0]]), (name, "ragged tail")
    assert torch.isfinite(first).all(), name


@pytest.mark.parametrize("case", _STRIDE_CASES, ids=lambda c: S.cfg_id(c[0]))
def test_grid_stride_second_trip(pa, case):
    """B = 524 288 + 128 + 5 walkers (4 097 full workgroup groups and a ragged one: the grid is capped at 4 096, so
    workgroups 0 and 1 make a second trip through the loop, with the weight stream's block counter and LDS double buffer
    wrapped) built by tiling 1 024 distinct walkers: forward, all Jacobian outputs and three fused sampler steps give
    every copy bit-identical to the first, the first 1 024 rows agree with the oracle, and the sampler's sums over all
    walkers with the oracle's."""
    cfg, n, d = case
    net, wd, kw = S.make_net(*cfg)
    D, BLK, N = cfg[2], 1024, 3
    B = 524288 + 128 + 5
    reps = -(-B // BLK)
    tile = lambda v: v.repeat(*([reps] + [1] * (v.dim() - 1)))[:B].contiguous()
    inp = S.sweep_inputs(D, -(-BLK // len(S.LEVELS)), seed=3)
    inp = {k: v[:BLK] for k, v in inp.items()}
    masks = S.level_masks(BLK)
    r64, r32, rp = S.reference_sets(wd, kw, inp)
    bounds = S.derive_bounds(r64, r32, rp, masks)
    big = {k: tile(v).cuda() for k, v in inp.items()}
    cn, xs = S.backbone_inputs(inp)
    rep = _Report(f"grid-stride {S.cfg_id(cfg)}")
    got = {}
    out = net(tile(cn).cuda(), tile(xs).cuda(), big["beta"])
    _assert_tiled("forward", out, BLK)
    got["F"] = out[:BLK]
    for cname, cv in (("x", None), ("dense", big["cot"])):
        r = net.jacobian(big["h"], big["x"], big["beta"], cot=cv, **_JAC_ALL)
        for k, v in r.items():
            _assert_tiled(f"jacobian {k} cot={cname}", v, BLK)
        got["D"], got["trace"] = r["D"][:BLK], r["trace"][:BLK]
        got[f"vjp_{cname}"], got[f"dot_h_{cname}"] = r["vjp"][:BLK], r["dot_h"][:BLK]
        got[f"parts0_{cname}"], got[f"parts1_{cname}"] = r["h_parts"][:BLK, 0], r["h_parts"][:BLK, 1]
        del r
    _check_levels(rep, got, r64, bounds, masks, [f"h={h:g}" for h in S.LEVELS])
    # fused sampler, injected noise tiled like the walkers
    # (mean removal only where there is more than one particle: the mean of ONE particle is the particle, and walkers
    # that are 0 after every step would compare equal whatever the weights of the second trip were)
    rm = n > 1
    tab = S.step_table(N, beta=1.2)
    x0, noise = S.sampler_inputs(D, n, d, BLK, N)
    xb = tile(x0).cuda()
    nb = torch.stack([tile(noise[s]) for s in range(N)]).cuda()
    stats = torch.zeros(N, 4, dtype=torch.float64, device="cuda")
    res = net.sampler_run(xb, tab.cuda(), N, noise=nb, n_particles=n, n_dim=d, remove_mean=rm, stats_out=stats)
    _assert_tiled("sampler", res, BLK)
    assert float(res[:BLK].abs().max()) > 0 and not torch.equal(res[:BLK], x0.cuda())
    s64, s32, sp = S.sampler_reference_sets(wd, kw, tab, x0, noise, n, d, rm)
    e32, floor = S.rel(s32["x"], s64["x"]), 4 * S.rel(sp["x"], s64["x"])
    rep.check("sampler_x", "3 steps", S.rel(res[:BLK], s64["x"]), min(max(4 * e32, floor, S.ONE_ULP), S.CAP_FORWARD),
              f"e32 {e32:.1e} floor {floor:.1e}")
    # the sums over all B walkers: B // 1024 copies of the block's sums plus those of the ragged tail's walkers
    tl = B - (B // BLK) * BLK
    t64, t32, tp = S.sampler_reference_sets(wd, kw, tab, x0[:tl], noise[:, :tl].contiguous(), n, d, rm)
    whole = lambda blk, tail: (B // BLK) * blk["stats"].double() + tail["stats"].double()
    w64 = whole(s64, t64)
    es = S.stats_errors(stats.cpu(), w64, B * D)
    for k, (b, e, f) in enumerate(S.stats_bounds(w64, whole(s32, t32), whole(sp, tp), B * D)):
        rep.check(S.STATS_NAMES[k], "worst step", float(es[k]), min(b, S.STATS_CAPS[k]), f"e32 {e:.1e} floor {f:.1e}")
    rep.finish()


# ------------------------------------------------------------------ 3. fused sampler
def _sampler_id(c):
    return f"h{c[0]}_d{c[1]}_{c[2]}x{c[3]}"


# the order of the cases keeps D = 52 ahead of D = 53 and 64 for either hidden size (the 64 KB dynamic-LDS arithmetic)
@pytest.mark.parametrize("remove_mean", [True, False], ids=["mean_free", "keep_mean"])
@pytest.mark.parametrize("case", S.SAMPLER_CASES, ids=_sampler_id)
def test_fused_sampler_vs_fp64_oracle_loop(pa, case, remove_mean):
    """pita_mlp_sampler_run, 5 steps, injected noise, B = 333 (a last tile of 13 walkers), against the fp64 loop of
    S.oracle_sampler_loop: final walkers and the four per-step sums of stats_out; walkers bit-equal with and without
    stats_out; mean removal on and off (one particle with mean removal: zeros, and the sums of step 0)."""
    hidden, D, n, d = case
    net, wd, kw = S.make_net(hidden, 2, D, True)
    N, B = 5, 333
    assert net.can_fuse(n, d)
    tab = S.step_table(N, beta=1.3)
    x0, noise = S.sampler_inputs(D, n, d, B, N)
    r64, r32, rp = S.sampler_reference_sets(wd, kw, tab, x0, noise, n, d, remove_mean)
    stats = torch.zeros(N, 4, dtype=torch.float64, device="cuda")
    kwargs = dict(noise=noise.cuda(), n_particles=n, n_dim=d, remove_mean=remove_mean)
    got = net.sampler_run(x0.cuda(), tab.cuda(), N, stats_out=stats, **kwargs)
    plain = net.sampler_run(x0.cuda(), tab.cuda(), N, **kwargs)
    assert torch.equal(got, plain), "stats_out changes the walkers"
    assert torch.isfinite(got).all()
    rep = _Report(f"sampler {_sampler_id(case)} remove_mean={remove_mean}")
    if n == 1 and remove_mean:
        # the mean of ONE particle is the particle: zeros by construction, which says nothing about the network (the
        # same nets with mean removal off do); what this case checks is the sums of step 0, see S.stats_steps
        assert float(got.abs().max()) == 0.0 and float(r64["x"].abs().max()) == 0.0
    else:
        e32, floor = S.rel(r32["x"], r64["x"]), 4 * S.rel(rp["x"], r64["x"])
        rep.check("x", "5 steps", S.rel(got, r64["x"]), min(max(4 * e32, floor, S.ONE_ULP), S.CAP_FORWARD),
                  f"e32 {e32:.1e} floor {floor:.1e}")
    if remove_mean and n > 1:
        assert float(got.reshape(B, n, d).mean(1).abs().max()) < 1e-4 * float(got.abs().max())
    steps = S.stats_steps(n, remove_mean, N)
    es = S.stats_errors(stats.cpu(), r64["stats"], B * D, steps)
    for k, (b, e, f) in enumerate(S.stats_bounds(r64["stats"], r32["stats"], rp["stats"], B * D, steps)):
        rep.check(S.STATS_NAMES[k], f"worst of steps {steps[0]}..{steps[-1]}", float(es[k]), min(b, S.STATS_CAPS[k]),
                  f"e32 {e:.1e} floor {f:.1e}")
    rep.finish()


@pytest.mark.parametrize("case", [(64, 39, 13, 3), (128, 64, 16, 4), (32, 64, 16, 4), (64, 1, 1, 1)], ids=_sampler_id)
def test_fused_sampler_philox_sharding_and_step_splitting(pa, case):
    """Philox noise keyed by (seed, walker_offset + walker, step0 + step, particle): two shards with their walker_offset
    equal the whole batch, steps [0, 5) equal [0, 2) then [2, 5) with step0 = 2, reruns are identical, bit for bit; another
    seed or a wrong offset gives other walkers."""
    hidden, D, n, d = case
    net, _, _ = S.make_net(hidden, 2, D, True)
    N, B, cut = 5, 4096 + 133, 2003
    tab = S.step_table(N, beta=0.9).cuda()
    x0 = S.sampler_inputs(D, n, d, B, 1)[0].cuda()
    # (the mean of ONE particle is the particle: mean removal would leave zeros whatever the noise)
    run = lambda x, t=tab, k=N, **kw: net.sampler_run(x.clone(), t, k, n_particles=n, n_dim=d, remove_mean=n > 1, **kw)
    a = run(x0, seed=11, walker_offset=1000)
    assert torch.isfinite(a).all()
    assert torch.equal(run(x0, seed=11, walker_offset=1000), a)
    c0 = run(x0[:cut], seed=11, walker_offset=1000)
    c1 = run(x0[cut:], seed=11, walker_offset=1000 + cut)
    assert torch.equal(torch.cat([c0, c1]), a), "sharding"
    s = run(x0, t=tab[:2].contiguous(), k=2, seed=11, walker_offset=1000, step0=0)
    s = run(s, t=tab[2:].contiguous(), k=N - 2, seed=11, walker_offset=1000, step0=2)
    assert torch.equal(s, a), "step splitting"
    assert not torch.equal(run(x0, seed=12, walker_offset=1000), a)
    assert not torch.equal(run(x0[cut:], seed=11, walker_offset=1000), a[cut:])  # the offset does key the noise
    assert not torch.equal(run(x0, t=tab[2:].contiguous(), k=3, seed=11, walker_offset=1000, step0=0),
                           run(x0, t=tab[2:].contiguous(), k=3, seed=11, walker_offset=1000, step0=2))
    if D > 1:  # every coordinate of a walker draws its own normal
        st = torch.zeros(1, 4, dtype=torch.float64, device="cuda")
        b = net.sampler_run(x0.clone(), tab[:1].contiguous(), 1, seed=11, n_particles=n, n_dim=d, remove_mean=False)
        z = net.sampler_run(x0.clone(), tab[:1].contiguous(), 1, noise=torch.zeros(1, B, D, device="cuda"),
                            n_particles=n, n_dim=d, remove_mean=False, stats_out=st)
        xi = ((b - z).double() / float(tab[0, pa._lib.ST_NOISE_SCALE] * tab[0, pa._lib.ST_SQRT_DT])).cpu()
        assert abs(float(xi.mean())) < 5 / np.sqrt(B * D) and abs(float(xi.std()) - 1) < 5 / np.sqrt(B * D)
        cc = torch.corrcoef(xi.T)
        off = cc - torch.diag(torch.diag(cc))
        assert float(off.abs().max()) < 6 / np.sqrt(B), float(off.abs().max())  # no coordinate repeats another's draw


# ------------------------------------------------------------------ 4. large angles in the plain forward
@pytest.mark.parametrize("cfg", S.LARGE_ANGLE_CONFIGS, ids=S.cfg_id)
def test_plain_forward_on_unscaled_coordinates(pa, cfg):
    """MyMLPTemperature.forward at |x| up to 400 (angles up to 1e4 rad) and t, beta up to 50 against the fp64
    restatement of the reference's fp32 angle (what sincos_rev's fp64 range reduction is for)."""
    net, wd, kw = S.make_net(*cfg)
    x, t, beta = S.large_angle_inputs(cfg[2], 640 + 27)
    r64, r32, rp = S.large_angle_references(wd, kw, x, t, beta)
    e32, floor = S.rel(r32, r64), 4 * S.rel(rp, r64)
    got = net(t.cuda(), x.cuda(), beta.cuda())
    rep = _Report(f"large angles {S.cfg_id(cfg)}")
    rep.check("F", "|x|<=400", S.rel(got, r64), min(max(4 * e32, floor, S.ONE_ULP), S.CAP_FORWARD),
              f"e32 {e32:.1e} floor {floor:.1e}")
    rep.finish()


# ------------------------------------------------------------------ 5. host-side contracts
@pytest.mark.parametrize("hidden,layers,D,out_dim", [(64, 1, 5, 1), (128, 2, 3, 33), (32, 1, 7, 65), (64, 2, 40, 65)])
def test_forward_with_other_head_sizes(pa, hidden, layers, D, out_dim):
    """pita_mlp_forward with out_dim != input_dim: heads of 1, 33 and 65 rows (one, two and three output blocks)."""
    net, wd, kw = S.make_net(hidden, layers, D, True, out_dim=out_dim)
    inp = S.sweep_inputs(D, 53)
    r64, r32, rp = S.reference_sets(wd, kw, inp, derivs=False)
    masks = S.level_masks(inp["x"].shape[0])
    bounds = S.derive_bounds(r64, r32, rp, masks)
    cn, xs = S.backbone_inputs(inp)
    got = {"F": _forward(net, cn, xs, inp["beta"])}
    assert got["F"].shape == (inp["x"].shape[0], out_dim)
    rep = _Report(f"head h{hidden} D={D} out={out_dim}")
    _check_levels(rep, got, r64, bounds, masks, [f"h={h:g}" for h in S.LEVELS])
    rep.finish()


def test_empty_batch_returns_without_a_launch(pa):
    """B = 0: all four entry points return PITA_OK and touch nothing."""
    for cfg in ((64, 1, 3, True), (32, 1, 6, False)):
        net, _, _ = S.make_net(*cfg)
        D = cfg[2]
        z1, zD = torch.empty(0, device="cuda"), torch.empty(0, D, device="cuda")
        assert net(z1, zD, z1).shape == (0, D)
        r = net.jacobian(z1, zD, z1, **_JAC_ALL)
        assert r["D"].shape == (0, D) and r["trace"].shape == (0,) and r["h_parts"].shape == (0, 2)
        diag = torch.empty(0, device="cuda")
        out, dout = net.jvp(z1, zD, z1, direction=0, diag_acc=diag)
        assert out.shape == (0, D) and dout.shape == (0, D)
        stats = torch.zeros(2, 4, dtype=torch.float64, device="cuda")
        x = net.sampler_run(zD.clone(), S.step_table(2).cuda(), 2, seed=1, n_particles=1, n_dim=D, stats_out=stats)
        assert x.shape == (0, D) and float(stats.abs().max()) == 0.0
    torch.cuda.synchronize()


def test_can_fuse_is_what_the_launcher_accepts(pa):
    """_HipMLP.can_fuse(n, d) is True exactly where pita_mlp_sampler_run takes the launch: D = n * d = input_dim = out_dim
    <= 64 with n_dim <= 4; everything else is refused with an error code before any launch."""
    geoms = {1: [(1, 1)], 6: [(2, 3), (3, 2), (6, 1), (1, 6)], 52: [(13, 4)], 53: [(53, 1)], 64: [(16, 4), (64, 1)],
             65: [(13, 5), (65, 1)], 68: [(17, 4)]}
    for hidden in (32, 64):
        for D, gs in geoms.items():
            net, _, _ = S.make_net(hidden, 1, D, False)
            for n, d in gs + [(n + 1, d) for n, d in gs]:  # the second set: n * d != input_dim
                x = torch.randn(40, D, device="cuda")
                try:
                    net.sampler_run(x, S.step_table(1).cuda(), 1, seed=3, n_particles=n, n_dim=d)
                    torch.cuda.synchronize()
                    accepted = True
                except pa._lib.PitaHipError:
                    accepted = False
                assert accepted == bool(net.can_fuse(n, d)), (hidden, D, n, d, accepted)
                if accepted:
                    assert torch.isfinite(x).all()
    odd, _, _ = S.make_net(64, 1, 6, False, out_dim=5)
    assert not odd.can_fuse(2, 3)
    with pytest.raises(pa._lib.PitaHipError):
        odd.sampler_run(torch.randn(8, 6, device="cuda"), S.step_table(1).cuda(), 1, seed=3, n_particles=2, n_dim=3)
