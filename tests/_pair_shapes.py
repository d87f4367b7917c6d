"""Shared by tests/test_pair_shapes_cpu.py and tests/test_pair_shapes_gpu.py: the table of edge shapes of the general
pair-target kernels (pair_energy_n3l_kernel, n <= 64; pair_energy_kernel, 64 < n <= 256; the two fused descents) and of
gmm_kernel, seeded inputs, fp64 references with the matching sums of magnitudes, and thin ctypes callers.  Importing
this module needs no GPU.

How an error is measured.  Per walker, never per batch (one wrong walker of a ragged tail must not hide among 16 000
right ones), and against the sum the kernel actually rounds, not against |logp|: on the lattice inputs the pair energies
cancel (|logp| falls to 0.16 at 21 x 2), so the fp32 oracle itself is 5.5e-5 off relative to |logp|.  Next to the fp64
oracle value the same sum is formed with every term replaced by its magnitude,
    A   = (1/T) (ef * sum |pair energy| + oscillator)                       per walker
    A_f = || (1/T) (w * sum_j |e'(r_ij)/r_ij| |x_i - x_j| + osc |x_i - mean|) ||_2   per walker, over its n*d components
(w = 2 ef for the ordered-pair LJ sum, 1 for DW).  That is the measure ("pair") of every case with n >= 3.  A walker of
n = 2 is ONE pair, and |pair energy| and |e'(r)/r| of one pair vanish inside the inputs' range; lj and dw at 2 x 3 and
2 x 1 alone use the measure "term" (each term of the pair polynomial by magnitude, for the double well also the rounding
of u = r - d0; _pair_terms has the reasoning and the measured figures).  measure_of(kind, n) says which, and both test
modules print it.  The checks are
    |logp - logp64| <= TOL * A,      ||f - f64|| <= TOL * max(||f64||, A_f),      TOL = 2e-5,
2e-5 being what test_lj_vs_oracle_random_and_edges and test_ring_kernels_edge_cases allow for these targets.  The CPU
module shows that the fp32 oracle meets a quarter of that on every case."""
import ctypes
import itertools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import pita_oracle as O

TOL = 2e-5            # tests/test_hip_parity.py: test_lj_vs_oracle_random_and_edges, test_ring_kernels_edge_cases
DESCENT_TOL = 1e-5    # test_fused_descent_equals_per_step, per walker here
ELEM_RTOL, ELEM_ATOL = 1e-5, 1e-6  # test_elementwise_vs_oracle
ONE_ULP = 1.2e-7
DW_COND = 0.02        # see _pair_terms
RANGE_MIN = 0.65      # LennardJonesPotential's smooth core starts here
OFFSET = 0.7          # added to every coordinate: walkers are NOT mean-free
BLOCK_CAP = 4096      # grid cap of launch_pair / launch_descent

SMALL_SHAPES = [(2, 3), (2, 1), (3, 2), (5, 3), (16, 2), (21, 2), (32, 3), (33, 1), (63, 3), (64, 2)]  # n <= 64
LARGE_SHAPES = [(65, 3), (85, 2), (86, 1), (128, 3), (129, 1), (200, 2), (256, 3)]                     # 64 < n <= 256
SHAPES = SMALL_SHAPES + LARGE_SHAPES
LJS_SHAPES = [(2, 3), (16, 2), (33, 1), (64, 2), (65, 3), (129, 1), (256, 3)]
NONUNIT_SHAPES = [(7, 3), (128, 3)]
GRID_STRIDE = [(33, 1, 16390), (129, 1, 4100)]  # 4 * 4096 + 6 walkers at 4 per block; 4100 at one per block

# argument values of pita_amd/lennardjones_energy.py (the plug-in always passes eps = rm = osc_scale = 1)
LJ_PLUGIN = dict(temperature=1.0, energy_factor=1.0, dist_eps=1e-6, eps=1.0, rm=1.0, osc_scale=1.0)
LJ_NONUNIT = dict(temperature=1.5, energy_factor=0.8, dist_eps=1e-6, eps=0.7, rm=1.1, osc_scale=0.5)
DW_DEFAULT = dict(temperature=1.0, a=0.9, b=-4.0, c=0.0, offset=4.0)  # MultiDoubleWellEnergy's defaults
DW_WARM = dict(DW_DEFAULT, temperature=2.0)

Case = namedtuple("Case", "kind n d par_name par batches")


def walkers_per_block(n):
    return 4 * (64 // n) if n <= 64 else 256 // n


def batch_sizes(n):
    wb = walkers_per_block(n)
    return tuple(sorted({b for b in (1, wb - 1, wb, wb + 1, 3 * wb + 1) if b >= 1}))


def case_id(c):
    return f"{c.kind}_{c.n}x{c.d}_{c.par_name}" + (f"_B{c.batches[0]}" if len(c.batches) == 1 and c.batches[0] > 2000 else "")


def _cases():
    out = []
    for n, d in SHAPES:
        out.append(Case("lj", n, d, "plugin", LJ_PLUGIN, batch_sizes(n)))
        out.append(Case("dw", n, d, "default", DW_DEFAULT, batch_sizes(n)))
        out.append(Case("dw", n, d, "T2", DW_WARM, batch_sizes(n)))
        if (n, d) in LJS_SHAPES:
            out.append(Case("ljs", n, d, "plugin", LJ_PLUGIN, batch_sizes(n)))
    for n, d in NONUNIT_SHAPES:
        out.append(Case("lj", n, d, "nonunit", LJ_NONUNIT, batch_sizes(n)))
    for n, d, B in GRID_STRIDE:
        out.append(Case("lj", n, d, "plugin", LJ_PLUGIN, (B,)))
        out.append(Case("dw", n, d, "default", DW_DEFAULT, (B,)))
    return out


CASES = _cases()
# (n, d) of the fused descents, ragged B; and one grid-stride case per kernel family at 2 steps
DESCENT_SHAPES = [(2, 3), (7, 3), (21, 2), (64, 2), (65, 3), (85, 2), (129, 1)]
DESCENT_STEPS, DESCENT_DT = 12, 1e-4
# (kind, n, d, B) past the 4096-block grid of the descent kernels, 2 steps: both kernel families at the shapes of
# GRID_STRIDE on LJ, and both on the double well in 2-D (12 and 3 walkers per block).  The double well at 129 x 1 x 4100
# gave non-finite walkers on the GPU: in ONE dimension its particles pass through each other within a step (they start
# as little as 1e-3 apart and move 2e-2), the fp32 oracle has a pair 2.4e-7 = one ulp apart after the first step, and a
# pair that lands on the same fp32 number has the force direction 0 / 0 -- in the kernels and in the oracle's formula
# alike.  Whether that happens is a matter of the last bit, not of the shape, so the double well's cases are 2-D.
DESCENT_GRID_STRIDE = [("lj", 33, 1, 16390), ("lj", 129, 1, 4100), ("dw", 21, 2, 12 * 4096 + 5), ("dw", 85, 2, 3 * 4096 + 2)]
DESCENT_CONFIGS = [(False, True), (True, True), (False, False), (True, False)]  # (langevin, remove_mean) held to the oracle
ELEM_SHAPES = [(1, 2), (2, 3), (85, 2), (86, 1), (256, 3)]


# ------------------------------------------------------------------ inputs
def _seed(kind, n, d, extra=0):
    return 100003 * {"lj": 1, "ljs": 2, "dw": 3, "gmm": 4}[kind] + 1009 * n + 17 * d + extra


def lattice_sites(n, d):
    """The first n sites of the d-dimensional integer lattice {0..m-1}^d, m the smallest side that holds n."""
    m = 1
    while m**d < n:
        m += 1
    return torch.tensor(list(itertools.islice(itertools.product(range(m), repeat=d), n)), dtype=torch.float64)


def ljs_spacing(n, d):
    """Spacing of the smooth-LJ lattice: 0.7 where that puts at least a tenth of the UNJITTERED lattice's pairs below
    RANGE_MIN, else the largest spacing that does (only the nearest neighbours of a 0.7 lattice lie below 0.65, and
    they are under 5 % of the pairs from 33 x 1 on: the spline branch would hardly run)."""
    s = lattice_sites(n, d)
    dist = (s[:, None] - s[None]).norm(dim=-1)[~torch.eye(n, dtype=torch.bool)]
    need = math.ceil(0.10 * dist.numel())
    kth = float(dist.sort().values[need - 1])  # this many pairs are at lattice distance <= kth
    return min(0.7, 0.999 * RANGE_MIN / kth)


def lattice_walkers(B, n, d, spacing, seed, jitter=0.08):
    """[B, n*d] fp32: lattice sites * spacing + jitter * spacing / 1.1 * N(0,1) clipped at 2.5 sigma + OFFSET.  With
    spacing 1.1 two neighbours stay at least 1.1 - 2 * 2.5 * 0.08 = 0.7 apart along their axis, in every batch size."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(B, n, d, generator=gen, dtype=torch.float64).clamp_(-2.5, 2.5)
    x = lattice_sites(n, d)[None] * spacing + z * (jitter * spacing / 1.1) + OFFSET
    return x.reshape(B, n * d).float().contiguous()


def min_pair_distance(x, n, d, chunk=None):
    """Per walker, in fp64."""
    out = []
    x = x.double().reshape(-1, n, d)
    step = chunk or max(1, (1 << 22) // (n * n * d))
    eye = torch.eye(n, dtype=torch.bool)
    for s in range(0, x.shape[0], step):
        v = x[s:s + step]
        r = (v[:, :, None] - v[:, None]).norm(dim=-1).masked_fill(eye, float("inf"))
        out.append(r.reshape(v.shape[0], -1).min(dim=1).values)
    return torch.cat(out)


def dw_walkers(B, n, d, seed):
    """randn * 2.5 as test_dw4_vs_oracle draws them, + OFFSET; a walker with two particles closer than 1e-3 (in one
    dimension, 129 particles at this scale have such a pair five times in six) is drawn again."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, n * d, generator=gen) * 2.5 + OFFSET
    bad = torch.arange(B)
    for _ in range(1000):
        bad = bad[min_pair_distance(x[bad], n, d) < 1e-3]
        if bad.numel() == 0:
            return x.contiguous()
        x[bad] = torch.randn(bad.numel(), n * d, generator=gen) * 2.5 + OFFSET
    raise AssertionError("dw_walkers: no admissible draw")


def case_inputs(c, B=None):
    B = max(c.batches) if B is None else B
    if c.kind == "dw":
        return dw_walkers(B, c.n, c.d, _seed("dw", c.n, c.d))
    spacing = 1.1 if c.kind == "lj" else ljs_spacing(c.n, c.d)
    return lattice_walkers(B, c.n, c.d, spacing, _seed(c.kind, c.n, c.d))


def fraction_below_core(x, n, d):
    x = x.double().reshape(-1, n, d)
    cnt = tot = 0
    step = max(1, (1 << 22) // (n * n * d))
    off = ~torch.eye(n, dtype=torch.bool)
    for s in range(0, x.shape[0], step):
        v = x[s:s + step]
        r = ((v[:, :, None] - v[:, None]).pow(2).sum(-1) + 1e-6).sqrt()[:, off]
        cnt += int((r < RANGE_MIN).sum())
        tot += r.numel()
    return cnt / tot


# ------------------------------------------------------------------ references
def _spline_c():
    _, c = O.lj_smooth_coeffs()
    return [float(v) for v in c[:, 0]]


def measure_of(kind, n):
    """"pair": the sums of |pair energy| and |e'(r)/r|; "term" (lj and dw at n = 2 only): see _pair_terms."""
    return "term" if n == 2 and kind in ("lj", "dw") else "pair"


def _pair_terms(kind, r, par, measure):
    """(pair energy, e'(r)/r) of every ordered pair at distance r (fp64 or fp32 tensor).  ``measure`` None: the signed
    values.  "pair": their absolute values.  "term", for n = 2: every TERM of the two polynomials by its absolute value,
    s^12 + 2 s^6 for s^12 - 2 s^6, |a| u^4 + |b| u^2 + |c| for the double well.  A walker of n = 2 is one pair; its LJ
    energy crosses zero at r = 2^(-1/6) rm and its force at r = rm, in the middle of the lattice inputs, while the two
    powers that are subtracted stay of order one: in the "pair" measure the fp32 oracle is 1.0e-5 (logp) and 1.6e-5
    (force) off at lj 2 x 3 and 2 x 1, measured, against the 5e-6 it has to meet.  From n = 3 on it meets them (at most
    3.1e-6), so those cases keep "pair"."""
    if measure is None or measure == "pair":
        ab = (lambda t: t.abs()) if measure else (lambda t: t)
        if kind == "dw":
            u = r - par["offset"]
            return ab(par["a"] * u**4 + par["b"] * u**2 + par["c"]), ab((4 * par["a"] * u**3 + 2 * par["b"] * u) / r)
        s6 = (par["rm"] / r) ** 6
        e = par["eps"] * (s6 * s6 - 2 * s6)
        g = par["eps"] * 12.0 * (s6 - s6 * s6) / (r * r)
        if kind == "ljs":
            c0, c1, c2, c3 = _spline_c()
            u = r - float(np.float32(RANGE_MIN))  # the spline's first breakpoint is linspace's fp32 0.65 ...
            core = r < RANGE_MIN                   # ... and the reference's filter compares with the Python float
            e = torch.where(core, c0 * u**3 + c1 * u**2 + c2 * u + c3, e)
            g = torch.where(core, (3 * c0 * u**2 + 2 * c1 * u + c2) / r, g)
        return ab(e), ab(g)
    if kind == "dw":
        u = r - par["offset"]
        e = (par["a"] * u**4).abs() + (par["b"] * u**2).abs() + abs(par["c"])
        g = ((4 * par["a"] * u**3).abs() + (2 * par["b"] * u).abs()) / r
        # u = r - d0 is itself a difference: where r ~ d0 the terms above vanish while u keeps the absolute rounding of
        # r and d0.  That rounding, DW_COND of r + d0 = TOL * DW_COND = 4e-7 relative = 7 fp32 roundings (2^-24 each:
        # two differences, squares, sum, root, subtraction), enters through |de/du| and |d(e'/r)/du|.  Measured without
        # it: the fp32 oracle is 1.7e-5 (logp) and 8.5e-6 (force) off at dw 2 x 3, against the 5e-6 it has to meet.
        w = DW_COND * (r + abs(par["offset"]))
        e = e + w * ((4 * par["a"] * u**3).abs() + (2 * par["b"] * u).abs())
        g = g + w * ((12 * par["a"] * u**2).abs() + abs(2 * par["b"])) / r
        return e, g
    s6 = (par["rm"] / r) ** 6
    e = par["eps"] * (s6 * s6 + 2 * s6)
    g = par["eps"] * 12.0 * (s6 + s6 * s6) / (r * r)
    if kind == "ljs":
        c0, c1, c2, c3 = _spline_c()
        u = r - float(np.float32(RANGE_MIN))
        core = r < RANGE_MIN
        e = torch.where(core, (c0 * u**3).abs() + (c1 * u**2).abs() + (c2 * u).abs() + abs(c3), e)
        g = torch.where(core, ((3 * c0 * u**2).abs() + (2 * c1 * u).abs() + abs(c2)) / r, g)
    return e, g


def pair_sums(kind, x, n, d, par, magnitudes):
    """Closed forms of logp and force of the three targets, summed in the dtype of ``x`` over ordered pairs.  With
    ``magnitudes`` every pair energy, every e'(r)/r, every coordinate difference and every oscillator term enters by its
    absolute value (in the measure measure_of(kind, n)) and the results are (A [B], A_f [B]) of the module docstring; without,
    they are (logp, force) and equal the oracle's (tests/test_pair_shapes_cpu.py)."""
    T = par["temperature"]
    lj = kind != "dw"
    w_e, w_f = (par["energy_factor"], 2.0 * par["energy_factor"]) if lj else (0.5, 1.0)
    eye = torch.eye(n, dtype=torch.bool)
    out_a, out_f = [], []
    x = x.reshape(-1, n, d)
    step = max(1, (1 << 22) // (n * n * d))
    for s in range(0, x.shape[0], step):
        v = x[s:s + step]
        diff = v[:, :, None] - v[:, None]
        r2 = diff.pow(2).sum(-1) + (par["dist_eps"] if lj else 0.0)
        r = r2.masked_fill(eye, 1.0).sqrt()
        e, g = _pair_terms(kind, r, par, measure_of(kind, n) if magnitudes else None)
        e, g = e.masked_fill(eye, 0.0), g.masked_fill(eye, 0.0)
        E = w_e * e.sum(dim=(1, 2))
        G = w_f * (g[..., None] * (diff.abs() if magnitudes else diff)).sum(dim=2)
        if lj:
            c = v - v.mean(dim=1, keepdim=True)
            E = E + 0.5 * par["osc_scale"] * c.pow(2).sum(dim=(1, 2))
            G = G + par["osc_scale"] * (c.abs() if magnitudes else c)
        if magnitudes:
            out_a.append(E / T)
            out_f.append((G / T).reshape(v.shape[0], -1).norm(dim=1))
        else:
            out_a.append(-E / T)
            out_f.append((-G / T).reshape(v.shape[0], -1))
    return torch.cat(out_a), torch.cat(out_f)


def oracle_logp_force(kind, x, n, d, par):
    """The oracle's own functions in the dtype of ``x``, in chunks of walkers (the [B, n, n, d] difference tensor of
    129 x 1 at 4100 walkers is 0.5 GB in one piece)."""
    lps, fs = [], []
    step = max(1, (1 << 22) // (n * n * d))
    for s in range(0, x.shape[0], step):
        v = x[s:s + step]
        if kind == "dw":
            lp, f = O.dw4_logp_force(v, n, d, par["temperature"], par["a"], par["b"], par["c"], par["offset"])
        elif kind == "lj":
            lp, f = O.lj_logp_force(v, n, d, **par)
        else:
            lp, f = O.lj_smooth_logp_force(v, n, d, **par)
        lps.append(lp)
        fs.append(f)
    return torch.cat(lps), torch.cat(fs)


_REF = {}


def reference(c):
    """{x (fp32), logp64, f64, A, A_f, logp32, f32} of the case's largest batch, computed once per process; smaller
    batches are prefixes.  The spline oracle is autograd through bucketize and runs in fp32 only where asked to."""
    key = case_id(c)
    if key not in _REF:
        x = case_inputs(c)
        lp64, f64 = oracle_logp_force(c.kind, x.double(), c.n, c.d, c.par)
        A, Af = pair_sums(c.kind, x.double(), c.n, c.d, c.par, True)
        lp32, f32 = oracle_logp_force(c.kind, x, c.n, c.d, c.par)
        _REF[key] = dict(x=x, logp64=lp64, f64=f64, A=A, Af=Af, logp32=lp32, f32=f32)
    return _REF[key]


def walker_errors(lp, f, ref, B=None):
    """(|logp - logp64| / A, ||f - f64|| / max(||f64||, A_f)) per walker of the first B walkers, as fp64 tensors."""
    B = lp.shape[0] if B is None else B
    lp, f = lp.detach().cpu().double()[:B], f.detach().cpu().double()[:B]
    e_lp = (lp - ref["logp64"][:B]).abs() / ref["A"][:B]
    fn = ref["f64"][:B].norm(dim=1)
    e_f = (f - ref["f64"][:B]).norm(dim=1) / torch.maximum(fn, ref["Af"][:B])
    return e_lp, e_f


def nan_to_inf(t):
    return torch.where(torch.isfinite(t), t, torch.full_like(t, float("inf")))


# ------------------------------------------------------------------ ctypes callers
def _smooth_args(pa):
    coef, r0 = pa.lennardjones_energy.smooth_core_coefficients()
    return coef, r0


def logp_force(pa, kind, x, n, d, par, want_force=True, B=None, fill=float("nan")):
    """(return code, logp, force or None) of pita_lj_logp_force / pita_lj_smooth_logp_force / pita_dw_logp_force on the
    device tensor ``x`` [B, n*d]; outputs are pre-filled with ``fill`` so that an element the kernel skips shows.  ``B``:
    the batch size handed to the entry point (at most the rows of x), the buffers keeping all rows of x."""
    L, lib = pa._lib.lib(), pa._lib
    lp = torch.full((x.shape[0],), fill, device=x.device)
    f = torch.full_like(x, fill) if want_force else None
    B = x.shape[0] if B is None else B
    if kind == "dw":
        rc = L.pita_dw_logp_force(x.data_ptr(), lp.data_ptr(), lib.ptr(f), B, n, d, par["temperature"], par["a"],
                                  par["b"], par["c"], par["offset"], lib.stream_ptr(x.device))
    elif kind == "lj":
        rc = L.pita_lj_logp_force(x.data_ptr(), lp.data_ptr(), lib.ptr(f), B, n, d, par["temperature"],
                                  par["energy_factor"], par["dist_eps"], par["eps"], par["rm"], par["osc_scale"],
                                  lib.stream_ptr(x.device))
    else:
        coef, r0 = _smooth_args(pa)
        rc = L.pita_lj_smooth_logp_force(x.data_ptr(), lp.data_ptr(), lib.ptr(f), B, n, d, par["temperature"],
                                         par["energy_factor"], par["dist_eps"], par["eps"], par["rm"], par["osc_scale"],
                                         r0, coef.ctypes.data_as(ctypes.c_void_p), lib.stream_ptr(x.device))
    return rc, lp, f


def descent(pa, kind, x, noise, n, d, par, nsteps, dt, noise_scale, sqrt_dt, seed, walker_offset, step0, remove_mean):
    """pita_lj_descent / pita_dw_descent in place on the device tensor ``x``; returns the code."""
    L, lib = pa._lib.lib(), pa._lib
    tail = (int(nsteps), float(dt), float(noise_scale), float(sqrt_dt), seed, walker_offset, step0, int(remove_mean),
            lib.stream_ptr(x.device))
    if kind == "dw":
        return L.pita_dw_descent(x.data_ptr(), lib.ptr(noise), x.shape[0], n, d, par["temperature"], par["a"], par["b"],
                                 par["c"], par["offset"], *tail)
    return L.pita_lj_descent(x.data_ptr(), lib.ptr(noise), x.shape[0], n, d, par["temperature"], par["energy_factor"],
                             par["dist_eps"], par["eps"], par["rm"], par["osc_scale"], *tail)


def em_step(pa, x, drift, noise, n, d, dt, noise_scale, sqrt_dt, seed, walker_offset, step, remove_mean, stats=None):
    lib = pa._lib
    return lib.lib().pita_em_step(x.data_ptr(), drift.data_ptr(), lib.ptr(noise), x.shape[0], n, d, float(dt),
                                  float(noise_scale), float(sqrt_dt), seed, walker_offset, step, int(remove_mean),
                                  lib.ptr(stats), lib.stream_ptr(x.device))


def per_step_descent(pa, kind, x, noise, n, d, par, nsteps, dt, noise_scale, sqrt_dt, seed, walker_offset, step0,
                     remove_mean):
    """What the fused descent claims to reproduce bit for bit: nsteps x (the force kernel + pita_em_step)."""
    for k in range(nsteps):
        rc, _, F = logp_force(pa, kind, x, n, d, par)
        assert rc == 0, pa._lib.last_error()
        nz = noise[k].contiguous() if noise is not None else None
        rc = em_step(pa, x, F, nz, n, d, dt, noise_scale, sqrt_dt, seed, walker_offset, step0 + k, remove_mean)
        assert rc == 0, pa._lib.last_error()
    return x


def descent_inputs(kind, n, d, B, nsteps):
    """(x0 [B, n*d], noise [nsteps, B, n*d]) fp32; the walkers by the builders above (not mean-free)."""
    x0 = dw_walkers(B, n, d, _seed("dw", n, d, 5)) if kind == "dw" else lattice_walkers(B, n, d, 1.1, _seed("lj", n, d, 5))
    gen = torch.Generator().manual_seed(_seed(kind, n, d, 9))
    return x0, torch.randn(nsteps, B, n * d, generator=gen).contiguous()


def oracle_descent(kind, x0, noise, n, d, par, nsteps, dt, langevin, mean_free, dtype=torch.float64):
    lf = lambda x: oracle_logp_force(kind, x, n, d, par)
    return O.negative_time_descent(x0.to(dtype), lf, nsteps, dt, n, d, do_langevin=langevin,
                                   noise_fn=lambda k, s: noise[k], mean_free=mean_free)


def descent_walker_errors(x, ref):
    x, ref = x.detach().cpu().double(), ref.double()
    return (x - ref).norm(dim=1) / ref.norm(dim=1)


# ------------------------------------------------------------------ GMM
GMM_DIMS, GMM_KS, GMM_TS, GMM_BS = (1, 2, 3, 4), (1, 2, 40, 257, 2048), (1.0, 2.0), (1, 255, 256, 257)
GMM_LOGP_RTOL, GMM_LOGP_ATOL, GMM_GRAD_RTOL, GMM_GRAD_ATOL = 3e-6, 3e-5, 3e-5, 2e-5  # test_gmm_golden
GMM_FAR_ROWS = 8
GMM_GRID_STRIDE = (1, 3, 256 * 4096 + 300)  # dim, K, B: the second trip of the 4096-block grid


def gmm_inputs(dim, K, B):
    """(x [B, dim], means [K, dim] uniform in +-40, scales [K, dim] log-uniform in 0.3 .. 3, unequal per component AND
    per dimension), fp32.  Rows are drawn at a random component's mean + its scales * N(0,1); GMM_FAR_ROWS rows (where
    B allows) sit at |x| ~ 1e3, where every component but one underflows."""
    gen = torch.Generator().manual_seed(_seed("gmm", K, dim))
    means = (torch.rand(K, dim, generator=gen) * 2 - 1) * 40.0
    scales = 0.3 * 10.0 ** torch.rand(K, dim, generator=gen)
    k = torch.randint(0, K, (B,), generator=gen)
    x = means[k] + scales[k] * torch.randn(B, dim, generator=gen)
    far = list(range(2, B, max(1, B // GMM_FAR_ROWS)))[:GMM_FAR_ROWS] if B >= 16 else []
    if far:
        sign = torch.where(torch.rand(len(far), dim, generator=gen) < 0.5, -1.0, 1.0)
        x[far] = sign * (1000.0 + 100.0 * torch.rand(len(far), dim, generator=gen))
    is_far = torch.zeros(B, dtype=torch.bool)
    is_far[far] = True
    return x.float().contiguous(), means.float().contiguous(), scales.float().contiguous(), is_far


def gmm_tolerances(lp64, g64):
    """Elementwise allowances (logp [B], grad [B, dim]) = atol + rtol |reference| with test_gmm_golden's figures, the
    same on the rows near the modes and on the far rows (the fp32 oracle has its factor 4 on both)."""
    return GMM_LOGP_ATOL + GMM_LOGP_RTOL * lp64.abs(), GMM_GRAD_ATOL + GMM_GRAD_RTOL * g64.abs()


def gmm_call(pa, x, means, scales, T, want_force=True):
    lib = pa._lib
    B, dim = x.shape
    lp = torch.full((B,), float("nan"), device=x.device)
    g = torch.full_like(x, float("nan")) if want_force else None
    rc = lib.lib().pita_gmm_logp_force(x.data_ptr(), lp.data_ptr(), lib.ptr(g), B, dim, means.data_ptr(),
                                       scales.data_ptr(), means.shape[0], float(T), lib.stream_ptr(x.device))
    return rc, lp, g


# ------------------------------------------------------------------ elementwise kernels
def elem_inputs(n, d, B):
    gen = torch.Generator().manual_seed(7000 + 31 * n + d)
    x, dr, nz = (torch.randn(B, n * d, generator=gen).contiguous() for _ in range(3))
    return x + OFFSET, dr * 3.0, nz


def em_reference(x, dr, nz, n, d, dt, noise_scale, sqrt_dt, remove_mean, dtype=torch.float64):
    x, dr, nz = x.to(dtype), dr.to(dtype), nz.to(dtype)
    v = x + (dr * dt + (noise_scale * nz) * sqrt_dt)
    return O.remove_mean(v, n, d) if remove_mean else v


def moment_sums(dr, nz, noise_scale, dtype):
    """(four sums: drift, drift^2, diffusion, diffusion^2 with diffusion = noise_scale * xi; the same four sums of
    magnitudes), accumulated in ``dtype``."""
    dr, dif = dr.to(dtype), (torch.tensor(noise_scale, dtype=dtype) * nz.to(dtype))
    s = torch.stack([dr.sum(), (dr * dr).sum(), dif.sum(), (dif * dif).sum()]).double()
    m = torch.stack([dr.abs().sum(), (dr * dr).sum(), dif.abs().sum(), (dif * dif).sum()]).double()
    return s, m
