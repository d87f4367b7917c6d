"""Shared by tests/test_step_shapes_cpu.py and tests/test_step_shapes_gpu.py: tables, seeded inputs, references, error
measures and thin ctypes callers for the small kernels every debiased step passes through -- pita_fk_assemble,
pita_energy_theta, pita_edm_scale_input, pita_edm_combine, pita_moments, pita_moments4, pita_quantile_clamp,
pita_gather_rows, pita_fill_normal and the three MALA kernels.  Importing this module needs no GPU.

The references are written from the formulas in include/pita_hip.h, not from the kernel sources, with a ``dtype``
argument: in float64 on the float32 arrays the kernel receives they are the oracle, in float32 the yardstick.

How an error is measured (fk_assemble, energy_theta, edm_*).  Per walker, never per batch.  An output's error is divided
by the SAME formula with every operand of every sum or difference replaced by its magnitude, in float64 (``mag=True`` of
the restatements): drift_X, x_scaled, D and score as 2-norms over the walker's D components, the [B] outputs as one
magnitude sum per walker.  The outputs are differences of 1/h- and 1/h^2-sized terms (and 1 - c_s = h/(1+h) is a
difference itself), so |drift_A| or |E| would not be a fair yardstick.  The bound of a case and output is
    max(FACTOR x the worst walker of the float32 restatement on the same inputs, FLOOR),   FACTOR = 8, FLOOR = 2^-22,
the rule of tests/test_mmd_gpu.py and tests/test_dihedrals_gpu.py: the kernels use fmaf and a wave butterfly where the
restatement sums in torch's order.  It is computed from the restatement on the CPU, never from the kernel."""
import math

import numpy as np
import torch

from oracle import pita_oracle as O
from tests._pair_shapes import ELEM_ATOL, ELEM_RTOL, nan_to_inf  # noqa: F401  (re-exported to the two test modules)

FACTOR, FLOOR = 8.0, 2.0 ** -22
U64 = 2.0 ** -53
# h on t in [0, 1] of the shipped schedules as the tests configure them: ElucidatingNoiseSchedule(sigma_min 0.01 or 0.05,
# sigma_max 80) gives h(0) = sigma_min^2 >= 1e-4 and h(1) = 6400, GeometricNoiseSchedule(0.05, 20) h(1) = 400.  The
# geometric h(0) is 0, where every formula here divides by zero; the integrator's time grid linspace(T, 0, N + 1)[:-1]
# never reaches t = 0.
H_MIN, H_MAX = 1e-4, 6400.0
ROWS = (1, 2, 8, 39, 63, 64, 65, 66, 128, 129, 165, 768)
BATCHES = (1, 3, 4, 5, 9)          # four waves (walkers) per block: partial block, full block, one into the second ...
ALL_FLAG_ROWS = (2, 65)
GRID_B, GRID_ROWS = 4 * 8192 + 5, (2, 65)  # past the 8192-block grid; at D = 65 also past 8192 x 256 elements
WAVE_GRID, ELEM_GRID = 8192, 8192 * 256
FLAGS_ON, FLAGS_OFF = (True, True, True, True), (False, False, False, False)
ALL_FLAGS = tuple((a, b, c, d) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True))
FLAG_NAMES = ("beta_e", "beta_s", "logp_target", "dot_parts")
FK_OUT = ("drift_X", "drift_A", "divergence_score", "cross_term", "dUt_dt", "Ut")
f32 = lambda v: float(np.float32(v))
GAMMA, DGAMMA = f32(4 / 3), -0.5                      # GammaConstant(4/3)'s value with GammaLinear(1.5, 1.0)'s slope
PIN_T = 0.4
PIN_W, PIN_DW = f32((1 - PIN_T) ** 3), f32(-3 * (1 - PIN_T) ** 2)
SPECIAL_LOGP = {3: 1e3, 4: -1e3, 5: 5e3, 6: -5e3, 7: float("inf"), 8: float("-inf")}  # row -> logp_target


def flags_id(flags):
    return "".join("1" if f else "0" for f in flags)


def fk_cases():
    out = [(D, fl) for D in ALL_FLAG_ROWS for fl in ALL_FLAGS]
    out += [(D, fl) for D in ROWS if D not in ALL_FLAG_ROWS for fl in (FLAGS_ON, FLAGS_OFF)]
    return out


FK_CASES = fk_cases()
fk_case_id = lambda c: f"D{c[0]}_{flags_id(c[1])}"


# ------------------------------------------------------------------ inputs
def h_values(B, gen):
    """[B] float64: both ends of [H_MIN, H_MAX] first (so every prefix of two or more walkers holds them), then
    log-spaced (B <= 9) or log-uniform points."""
    if B <= 9:
        grid = torch.logspace(math.log10(H_MIN), math.log10(H_MAX), 9, dtype=torch.float64)
        return grid[[0, 8, 4, 2, 6, 1, 3, 5, 7]][:B].clone()
    h = torch.exp(torch.rand(B, generator=gen, dtype=torch.float64) * math.log(H_MAX / H_MIN) + math.log(H_MIN))
    h[0], h[1] = H_MIN, H_MAX
    return h


_FK_IN = {}


def fk_inputs(D, B):
    """The arrays pita_fk_assemble reads, float32 on the CPU, of one seeded batch of B walkers with D components, built
    like a denoiser's outputs: x of size sqrt(1 + h), D = c_s x + c_out F with F of size one, J^T x and <x, dD/dh> of the
    matching sizes, dot_parts consistent with D_E and dot_h before rounding, trace_S around D c_s.  beta_e != beta_s,
    dhdt 3 - 5 % above g2 (g2 is the elucidating schedule's at that h), |logp_target| from 1e2 to 1e4 with both signs and
    the entries of SPECIAL_LOGP at their rows, so that no term of the formulas is invisible."""
    key = (D, B)
    if key in _FK_IN:
        return _FK_IN[key]
    gen = torch.Generator().manual_seed(77000 + 13 * D + (B if B > 9 else 0))
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    h = h_values(B, gen)
    hc = h[:, None]
    c_s, c_in, c_out = 1 / (1 + hc), (1 + hc) ** -0.5, (hc / (1 + hc)) ** 0.5
    x = rn(B, D) * (1 + hc).sqrt()
    F, G, F2 = rn(B, D), rn(B, D), rn(B, D)
    x2 = (x * x).sum(1)
    s1 = (c_out * x * F).sum(1)
    s2 = ((0.5 / (hc.sqrt() * (1 + hc) ** 1.5)) * x * F).sum(1) + (c_out * x * G).sum(1) / (8 * h)
    g2 = 14 * (80 ** (1 / 7) - 0.01 ** (1 / 7)) * h ** (13 / 14)
    logp = torch.where(ru(B) < 0.5, -1.0, 1.0) * 10 ** (2 + 2 * ru(B))
    for row, v in SPECIAL_LOGP.items():
        if row < B:
            logp[row] = v
    a = dict(x=x, h=h, g2=g2, dhdt=g2 * (1.03 + 0.02 * ru(B)), D_E=c_s * x + c_out * F,
             jtx_E=c_s * x + c_out * c_in * rn(B, D) * (1 + hc).sqrt(), dot_h=-(c_s[:, 0] ** 2) * x2 + s2,
             dot_parts=torch.stack([s1, s2], 1), D_S=c_s * x + c_out * F2,
             trace_S=D * c_s[:, 0] + (c_out * c_in)[:, 0] * math.sqrt(D) * rn(B), beta_e=0.5 + ru(B), beta_s=0.5 + ru(B),
             logp_target=logp)
    a = {k: v.float().contiguous() for k, v in a.items()}
    _FK_IN[key] = a
    return a


def prefix(a, B):
    return {k: v[:B].contiguous() for k, v in a.items()}


# ------------------------------------------------------------------ pita_fk_assemble restated from the header
MUTATIONS = ("swap_beta", "no_keep", "pin_dw_sign", "no_clamp", "dhdt_is_g2", "trace_without_D", "no_dgamma_Ut", "parts_h_for_1ph")


def fk_restate(a, flags, dtype, mag=False, mutate=None, gamma=GAMMA, dgamma=DGAMMA, pin_w=PIN_W, pin_dw=PIN_DW):
    """The comment above pita_fk_assemble in include/pita_hip.h, in ``dtype`` on the arrays of ``a``.  ``flags`` =
    (beta_e, beta_s, logp_target, dot_parts given).  ``mag``: the same formulas with every operand of every sum or
    difference by its magnitude (the module docstring's measure).  ``mutate``: one of MUTATIONS, a deliberately wrong
    formula (tests/test_step_shapes_cpu.py shows that inputs and measure see each of them)."""
    use_be, use_bs, use_pin, use_parts = flags
    T = lambda k: a[k].to(dtype)
    m = (lambda t: t.abs()) if mag else (lambda t: t)
    sub = (lambda p, q: p.abs() + q.abs()) if mag else (lambda p, q: p - q)
    neg = (lambda t: t) if mag else (lambda t: -t)
    sc = lambda v: torch.tensor(abs(v) if mag else v, dtype=dtype)
    x, h, g2, dhdt = T("x"), T("h"), T("g2"), T("dhdt")
    B, D = x.shape
    one = torch.ones(B, dtype=dtype)
    be, bs = (T("beta_e") if use_be else one), (T("beta_s") if use_bs else one)
    if mutate == "swap_beta":
        be, bs = bs, be
    w, dw = (sc(pin_w), sc(pin_dw)) if use_pin else (sc(0.0), sc(0.0))
    gam, dgam = sc(gamma), sc(dgamma)
    keep = (1 + w) if mag else (1 - w)
    hc, c_s = h[:, None], 1 / (1 + h)
    # grad E = be ((1+c_s) x - D_E - jtx_E)/h,  grad U = (1-w) grad E,  s = bs (D_S - x)/h,  b = s g2/2
    gradE = be[:, None] * sub(sub((1 + c_s)[:, None] * x, T("D_E")), T("jtx_E")) / hc
    gradU = gradE if mutate == "no_keep" else keep * gradE
    b = bs[:, None] * sub(T("D_S"), x) / hc * g2[:, None] / 2
    out = {"drift_X": m(gam * neg(gradU) * g2[:, None] / 2) + m(gam * b), "cross_term": (m(neg(gradU)) * b).sum(1)}
    x2 = (x * x).sum(1)
    if use_parts:
        # E = be [|x|^2/(2(1+h)) - s1/h],  dE/dh = be [-|x|^2/(2(1+h)^2) + s1/h^2 - s2/h]
        s1, s2 = T("dot_parts")[:, 0], T("dot_parts")[:, 1]
        op = h if mutate == "parts_h_for_1ph" else 1 + h
        E = be * sub(x2 / (2 * op), s1 / h)
        dEdh = be * sub(m(neg(x2 / (2 * op * op))) + m(s1 / (h * h)), s2 / h)
    else:
        # E = be [(1+c_s)|x|^2/(2h) - <D_E,x>/h] and its h-derivative with <x, dD_E/dh> = dot_h; d/dh of (1+c_s)/(2h) is
        # -(1+c_s)/(2h^2) - c_s^2/(2h), both terms of one sign
        DEx = m(T("D_E") * x).sum(1)
        dq = (1 + c_s) / (2 * h * h) + c_s * c_s / (2 * h)
        E = be * sub((1 + c_s) / (2 * h) * x2, DEx / h)
        dEdh = be * sub(m(neg(dq * x2)) + m(DEx / (h * h)), T("dot_h") / h)
    dEdt = dEdh * (g2 if mutate == "dhdt_is_g2" else dhdt)
    U, dUdt = E, dEdt
    if use_pin:
        # U0 = clamp(-logp_target, +-1e3) (torch.clamp: a NaN stays),  U = w U0 + (1-w) E,  dU/dt = dw (U0 - E) + (1-w) dE/dt
        U0 = -T("logp_target")
        if mutate != "no_clamp":
            U0 = torch.clamp(U0, min=-1e3, max=1e3)
        U = m(w * U0) + keep * E
        pin = dw * sub(U0, E)
        dUdt = m(-pin if mutate == "pin_dw_sign" else pin) + keep * dEdt
    tr = T("trace_S") if mutate == "trace_without_D" else sub(T("trace_S"), torch.full((B,), float(D), dtype=dtype))
    div = bs * (tr / h) * g2 / 2
    dA = m(gam * gam * out["cross_term"]) + m(gam * div) + m(gam * dUdt)
    if mutate != "no_dgamma_Ut":
        dA = dA + m(dgam * U)
    out.update(drift_A=dA, divergence_score=div, dUt_dt=dUdt, Ut=U)
    return out


def rel_errors(got, ref, mag):
    """{name: per-walker error / magnitude} in float64; [B, D] outputs as 2-norms over the walker's row.  A walker whose
    value or magnitude is not finite gives a non-finite error (nan_to_inf turns it into a failure)."""
    out = {}
    for k in ref:
        g, r, mg = got[k].detach().cpu().double(), ref[k].double(), mag[k].double()
        out[k] = (g - r).norm(dim=1) / mg.norm(dim=1) if g.dim() == 2 else (g - r).abs() / mg
    return out


_FK_REF = {}


def fk_reference(D, B, flags):
    """{ref (float64), mag, e32 (errors of the float32 restatement), bound {name: float}} of fk_inputs(D, B), once per
    process.  The bound is the module docstring's, over all B walkers (smaller batches are prefixes)."""
    key = (D, B, flags)
    if key not in _FK_REF:
        a = fk_inputs(D, B)
        ref, mag = fk_restate(a, flags, torch.float64), fk_restate(a, flags, torch.float64, mag=True)
        e32 = rel_errors(fk_restate(a, flags, torch.float32), ref, mag)
        _FK_REF[key] = dict(ref=ref, mag=mag, e32=e32, bound={k: bound_of(v) for k, v in e32.items()})
    return _FK_REF[key]


def bound_of(e32):
    return max(FACTOR * float(nan_to_inf(e32).max()), FLOOR)


def fk_call(pa, a, flags, B=None, fill=float("nan"), pin=None, null=()):
    """(return code, {output: device tensor pre-filled with ``fill``}) of pita_fk_assemble on the dict of device
    (or, for the refusals, any) tensors ``a``; optional inputs whose flag is off are passed as NULL, as are the names in
    ``null``.  ``pin``: (pin_w, pin_dw) instead of (PIN_W, PIN_DW) / (0, 0)."""
    lib = pa._lib
    use_be, use_bs, use_pin, use_parts = flags
    x = a["x"]
    rows, D = x.shape
    B = rows if B is None else B
    outs = {k: torch.full((rows, D) if k == "drift_X" else (rows,), fill, device=x.device) for k in FK_OUT}
    p = lambda k, on=True: 0 if (not on or k in null) else a[k].data_ptr()
    o = lambda k: 0 if k in null else outs[k].data_ptr()
    pw, pdw = pin if pin is not None else ((PIN_W, PIN_DW) if use_pin else (0.0, 0.0))
    rc = lib.lib().pita_fk_assemble(p("x"), p("h"), p("g2"), p("dhdt"), p("D_E"), p("jtx_E"), p("dot_h"), p("dot_parts", use_parts),
                                    p("D_S"), p("trace_S"), GAMMA, DGAMMA, p("beta_e", use_be), p("beta_s", use_bs), pw, pdw,
                                    p("logp_target", use_pin), o("drift_X"), o("drift_A"), o("divergence_score"), o("cross_term"),
                                    o("dUt_dt"), o("Ut"), B, D, lib.stream_ptr(x.device) if x.is_cuda else None)
    return rc, outs


# ------------------------------------------------------------------ a closed-form backbone, and the kernels' inputs from it
class TanhBackbone:
    """F(c_noise, x_in, beta) = W2 tanh(W1 x_in + a c_noise + c beta + b1) + b2 in float64 with seeded weights: valid for
    any D, differentiable by torch.func, batched or not."""

    def __init__(self, D, seed, hidden=16):
        gen = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        self.W1, self.a, self.c, self.b1 = rn(hidden, D) / math.sqrt(D), rn(hidden), 0.3 * rn(hidden), 0.1 * rn(hidden)
        self.W2, self.b2 = rn(D, hidden) / math.sqrt(hidden), 0.1 * rn(D)

    def __call__(self, c_noise, x_in, beta):
        z = x_in @ self.W1.T + c_noise[..., None] * self.a + beta[..., None] * self.c + self.b1
        return torch.tanh(z) @ self.W2.T + self.b2


TIE_SCHED, TIE_GAMMA = O.Elucidating(0.01, 80.0, 7), O.GammaLinear(1.5, 1.0)
TIE_BETA = 0.7


def tie_target_logp(x):
    """A target log-density whose values straddle the +-1e3 clamp."""
    return 1500.0 * torch.sin(x.sum(dim=1))


def tie_case(D, B, t, seed):
    """(energy backbone, score backbone, t as a float64 scalar tensor, x [B, D] float64 of size sqrt(1 + h(t)))."""
    gen = torch.Generator().manual_seed(seed)
    tt = torch.tensor(t, dtype=torch.float64)
    x = torch.randn(B, D, generator=gen, dtype=torch.float64) * float((1 + TIE_SCHED.h(tt)).sqrt())
    return TanhBackbone(D, seed + 1), TanhBackbone(D, seed + 2), tt, x


def fk_inputs_from_backbones(eb, sb, t, x, pin, precondition):
    """What the derivative kernels hand pita_fk_assemble -- D_E, J_x D_E^T x, <x, dD_E/dh>, dot_parts, D_S, tr J_x D_S --
    by torch.func in float64 from the two backbones, with h, g2, dh/dt of TIE_SCHED at t and the scalars of TIE_GAMMA
    and of pin_energy.  D_E and D_S are the denoisers WITHOUT beta preconditioning: that enters through beta_e / beta_s."""
    from torch.func import jacfwd, jacrev, vmap

    B, D = x.shape
    tb = t * torch.ones(B, dtype=torch.float64)
    h = TIE_SCHED.h(tb)
    b1 = TIE_BETA * torch.ones(1, dtype=torch.float64)
    den = lambda bb: (lambda h1, x1: O.denoiser(bb, h1[None], x1[None], TIE_BETA, False)[0])

    def cF(h1, x1):  # c_out F(c_noise, c_in x, beta) with x held fixed
        _, c_in, c_out, c_noise = O.edm_coeffs(h1[None])
        return (c_out[:, None] * eb(c_noise, c_in[:, None] * x1[None], b1))[0]

    JE = vmap(jacrev(den(eb), argnums=1))(h, x)
    JS = vmap(jacrev(den(sb), argnums=1))(h, x)
    dDdh = vmap(jacfwd(den(eb), argnums=0))(h, x)
    s1 = (x * vmap(cF)(h, x)).sum(1)
    s2 = (x * vmap(jacfwd(cF, argnums=0))(h, x)).sum(1)
    beta = torch.full((B,), TIE_BETA, dtype=torch.float64)
    a = dict(x=x, h=h, g2=TIE_SCHED.g(tb).pow(2), dhdt=TIE_SCHED.dh_dt(tb), D_E=vmap(den(eb))(h, x),
             jtx_E=torch.einsum("bij,bi->bj", JE, x), dot_h=(x * dDdh).sum(1), dot_parts=torch.stack([s1, s2], 1),
             D_S=vmap(den(sb))(h, x), trace_S=JS.diagonal(dim1=-2, dim2=-1).sum(-1), beta_e=beta, beta_s=beta,
             logp_target=tie_target_logp(x))
    scal = dict(gamma=float(TIE_GAMMA.gamma(t)), dgamma=float(TIE_GAMMA.dgamma_dt(tb)[0]),
                pin_w=float((1 - t) ** 3) if pin else 0.0, pin_dw=float(-3 * (1 - t) ** 2) if pin else 0.0)
    return a, scal


# ------------------------------------------------------------------ pita_energy_theta, pita_edm_scale_input, pita_edm_combine
def edm_inputs(D, B):
    """(h [B], x [B, D] of size sqrt(1 + h), F [B, D] of size one, beta [B] in 0.5 .. 1.5), float32."""
    gen = torch.Generator().manual_seed(88000 + 13 * D + (B if B > 9 else 0))
    h = h_values(B, gen)
    x = torch.randn(B, D, generator=gen, dtype=torch.float64) * (1 + h[:, None]).sqrt()
    F = torch.randn(B, D, generator=gen, dtype=torch.float64)
    beta = 0.5 + torch.rand(B, generator=gen, dtype=torch.float64)
    return tuple(v.float().contiguous() for v in (h, x, F, beta))


def edm_restate(h, x, F, beta, dtype, mag=False):
    """{x_scaled, c_noise, D, score, E} from the comments above pita_edm_scale_input / pita_edm_combine /
    pita_energy_theta in include/pita_hip.h: x_in = c_in x, c_noise = ln(h)/8, D = c_s x + c_out F (times beta + (1-beta) x),
    score = (D_plain - x)/h (times beta), E = (1-c_s)/(2h)|x|^2 - c_out/(c_in h) <F, c_in x> (times beta)."""
    h, x, F = h.to(dtype), x.to(dtype), F.to(dtype)
    m = (lambda t: t.abs()) if mag else (lambda t: t)
    sub = (lambda p, q: p.abs() + q.abs()) if mag else (lambda p, q: p - q)
    hc = h[:, None]
    c_s, c_in = 1 / (1 + hc), 1 / torch.sqrt(1 + hc)
    c_out = torch.sqrt(hc) * c_in
    Dv = m(c_s * x) + m(c_out * F)
    score = sub(Dv, x) / hc
    one = torch.ones_like(h)
    E = sub(sub(one, c_s[:, 0]) / (2 * h) * (x * x).sum(1), (c_out / (c_in * hc))[:, 0] * m(F * (c_in * x)).sum(1))
    if beta is not None:
        bt = beta.to(dtype)[:, None]
        Dv = m(Dv * bt) + m(sub(torch.ones_like(bt), bt) * x)
        score, E = score * bt, E * bt[:, 0]
    return {"x_scaled": m(c_in * x), "c_noise": m(torch.log(h) / 8), "D": Dv, "score": score, "E": E}


_EDM_REF = {}


def edm_reference(D, B, with_beta):
    key = (D, B, with_beta)
    if key not in _EDM_REF:
        h, x, F, beta = edm_inputs(D, B)
        bt = beta if with_beta else None
        ref, mag = edm_restate(h, x, F, bt, torch.float64), edm_restate(h, x, F, bt, torch.float64, mag=True)
        e32 = rel_errors(edm_restate(h, x, F, bt, torch.float32), ref, mag)
        _EDM_REF[key] = dict(inputs=(h, x, F, beta), ref=ref, mag=mag, e32=e32, bound={k: bound_of(v) for k, v in e32.items()})
    return _EDM_REF[key]


def edm_call(pa, h, x, F, beta, B=None, want=("D", "score"), fill=float("nan")):
    """(codes, {x_scaled, c_noise, D, score, E}) of the three entry points on device tensors; D / score not in ``want``
    are passed as NULL and their NaN-filled buffers returned untouched."""
    lib, L = pa._lib, pa._lib.lib()
    rows, D = x.shape
    B = rows if B is None else B
    st = lib.stream_ptr(x.device)
    o = {k: torch.full((rows, D), fill, device=x.device) for k in ("x_scaled", "D", "score")}
    o.update({k: torch.full((rows,), fill, device=x.device) for k in ("c_noise", "E")})
    rcs = (L.pita_edm_scale_input(h.data_ptr(), x.data_ptr(), o["x_scaled"].data_ptr(), o["c_noise"].data_ptr(), B, D, st),
           L.pita_edm_combine(h.data_ptr(), x.data_ptr(), F.data_ptr(), lib.ptr(beta), o["D"].data_ptr() if "D" in want else 0,
                              o["score"].data_ptr() if "score" in want else 0, B, D, st),
           L.pita_energy_theta(h.data_ptr(), x.data_ptr(), F.data_ptr(), lib.ptr(beta), o["E"].data_ptr(), B, D, st))
    return rcs, o


# ------------------------------------------------------------------ pita_moments, pita_moments4
MOMENT_SIZES = (1, 63, 64, 65, 255, 256, 257, 65536 + 3, 262144 + 5)  # the last two pass 256 / 1024 blocks of 256
MOMENTS4_GRID, MOMENTS_GRID = 256, 1024
OUT0 = (3.25, -17.5, 0.625, 9.0, -2.0, 40.5, 1e-3, -7.75)  # what out holds before the call: the += contract


def moment_vectors(n):
    """[4, n] float32: magnitudes log-uniform in 1e-3 .. 1e3, both signs."""
    gen = torch.Generator().manual_seed(99000 + n % 9973)
    mag = 10 ** (torch.rand(4, n, generator=gen, dtype=torch.float64) * 6 - 3)
    return (mag * torch.where(torch.rand(4, n, generator=gen) < 0.5, -1.0, 1.0)).float().contiguous()


def moment_terms(v, out0):
    """((terms of out0_s + sum v, terms of out0_q + sum v^2), their two sums of magnitudes) of one float32 vector, as
    float64 values: the square of a float32 is exact in float64."""
    d = v.double().numpy()
    return (([out0[0], *d], [out0[1], *(d * d)]),
            (abs(out0[0]) + math.fsum(np.abs(d)), abs(out0[1]) + math.fsum(d * d)))


def moment_errors(terms, mags, got):
    """|got - exact sum| / sum of magnitudes for the pair ``got``: math.fsum over the terms and -got is the correctly
    rounded value of the exact difference, so the reference adds no rounding of its own."""
    return [abs(math.fsum(terms[j] + [-float(got[j])])) / mags[j] for j in range(2)]


def moment_bound(n):
    """The kernels accumulate in double and the square of a float32 is exact there, so every rounding is one of an
    addition: per thread, in the wave butterfly, in the atomic adds onto out.  A summation of n + 1 operands in ANY order
    errs by at most (longest chain of additions) x 2^-53 x the sum of magnitudes, and no chain is longer than n."""
    return n * U64


# ------------------------------------------------------------------ pita_quantile_clamp
QUANTILES = (0.0, 0.25, 0.5, 0.9, 1.0)
QUANTILE_SHAPES = ((1, 1), (2, 2), (1024, 1024), (1025, 1025), (2500, 2000), (3000, 1024), (1030, 1))  # (B, chunk)
QUANTILE_KINDS = ("randn", "equal", "negative", "zeros", "denormal", "inf", "lastbyte")
QUANTILE_RTOL = QUANTILE_ATOL = 1e-6  # test_quantile_clamp_kernel
RANK_PATH_MAX = 1024                   # chunks up to this size: rank counting; larger: radix select
LASTBYTE_BASE, LASTBYTE_STEP, LASTBYTE_ULP = 1000.0, 80, 2.0 ** -14  # 1000.0f = 0x447A0000: adding up to 255 ulps changes the key's lowest byte only


def chunks(B, chunk):
    return [(lo, min(lo + chunk, B)) for lo in range(0, B, chunk)]


def _lastbyte_chunk(n):
    """Sorted [n] float32 of four levels LASTBYTE_BASE + (0, 1, 2, 3) x LASTBYTE_STEP ulps whose level changes sit right
    after floor(q (n - 1)) for q = 0.25, 0.5, 0.9: where that rank is fractional the two order statistics of the
    quantile differ, and in the lowest byte of the radix key only."""
    base = np.array([LASTBYTE_BASE], np.float32).view(np.uint32)[0]
    cuts = sorted({int(math.floor(q * (n - 1))) + 1 for q in (0.25, 0.5, 0.9)})
    level = np.zeros(n, np.uint32)
    for c in cuts:
        level[c:] += 1
    return (base + level * np.uint32(LASTBYTE_STEP)).astype(np.uint32).view(np.float32)


def quantile_input(kind, B, chunk):
    gen = torch.Generator().manual_seed(55000 + 7 * B + chunk + 131 * QUANTILE_KINDS.index(kind))
    a = torch.randn(B, generator=gen) * 10
    if kind == "randn":
        a[::7] = a[0]  # ties
    elif kind == "equal":
        a = torch.full((B,), -3.25)
    elif kind == "negative":
        a = -a.abs() - 0.5
    elif kind == "zeros":
        r = torch.rand(B, generator=gen)
        small = torch.where(torch.rand(B, generator=gen) < 0.5, -1.0, 1.0) * 1e-3 * torch.rand(B, generator=gen)
        a = torch.where(r < 0.3, torch.tensor(0.0), torch.where(r < 0.6, torch.tensor(-0.0), small))
    elif kind == "denormal":
        a = a * 1e-41
    elif kind == "inf":
        # under 5 % of EVERY chunk at each end: the first entries of a chunk, at most floor(0.04 n) of each sign
        for lo, hi in chunks(B, chunk):
            k = int(0.04 * (hi - lo))
            a[lo:lo + k] = float("inf")
            a[lo + k:lo + 2 * k] = float("-inf")
            perm = torch.randperm(hi - lo, generator=gen)
            a[lo:hi] = a[lo:hi][perm]
    elif kind == "lastbyte":
        for lo, hi in chunks(B, chunk):
            a[lo:hi] = torch.from_numpy(_lastbyte_chunk(hi - lo))[torch.randperm(hi - lo, generator=gen)]
    return a.float().contiguous()


def chunk_quantiles(a, B, chunk, q):
    return torch.stack([torch.quantile(a[lo:hi], q) for lo, hi in chunks(B, chunk)])


def quantile_reference(a, B, chunk, q):
    """torch.quantile + torch.clamp per chunk on the CPU."""
    want = a.clone()
    for lo, hi in chunks(B, chunk):
        want[lo:hi] = torch.clamp(a[lo:hi], max=torch.quantile(a[lo:hi], q))
    return want


def lastbyte_exact_quantile(n, q):
    """The quantile of _lastbyte_chunk(n) from its own sorted values: rank = q (n - 1) and the weight in float32 as the
    header's torch.quantile semantics have them, the interpolation in float64."""
    s = _lastbyte_chunk(n).astype(np.float64)
    rank = np.float32(q) * np.float32(n - 1)
    klo = int(math.floor(rank))
    khi = min(klo + 1, n - 1) if rank > klo else klo
    return s[klo] + float(rank - np.float32(klo)) * (s[khi] - s[klo]), s[klo] != s[khi]


def quantile_call(pa, a, chunk, q, B=None):
    got = a.cuda().clone()
    rc = pa._lib.lib().pita_quantile_clamp(got.data_ptr(), got.shape[0] if B is None else B, chunk, q, pa._lib.stream_ptr())
    return rc, got


# ------------------------------------------------------------------ pita_gather_rows
GATHER_ROWS, GATHER_BATCHES, GATHER_GRID = (1, 3, 39, 64, 165), (1, 255, 257), (65, GRID_B)
ID_KINDS = ("permutation", "equal", "resampled")


def gather_ids(kind, B, n_src, gen):
    if kind == "permutation":
        return torch.randperm(n_src, generator=gen)[:B].contiguous()
    if kind == "equal":
        return torch.full((B,), n_src - 1, dtype=torch.int64)
    # what a systematic resampling gives: non-decreasing parents, rotated by the event's uniform (one wrap)
    ids = torch.sort(torch.randint(0, n_src, (B,), generator=gen)).values
    return torch.roll(ids, B // 3).contiguous()


# ------------------------------------------------------------------ Philox: host restatement, shapes
PHILOX_SHAPES = ((1, 1), (1, 2), (2, 3), (85, 2), (86, 1), (256, 1), (256, 3))
PHILOX_SEED, PHILOX_OFFSET, PHILOX_STEP = 0x1234567890ABCDEF, (1 << 33) + 5, (3 << 32) + 9
PHILOX_ATOL, PHILOX_RTOL = 2e-5, 1e-5  # test_philox_matches_host_restatement
ELEM_BLOCK_CAP = 4096


def ragged_batch(n):
    return 3 * (256 // n) + 1


def philox_batches(n, d):
    return (ragged_batch(n),) + ((4100,) if (n, d) == (256, 1) else ())


PHILOX_CASES = tuple((n, d, B) for n, d in PHILOX_SHAPES for B in philox_batches(n, d))


def _philox_normals_host(seed, walkers, step, particles):
    """Philox4x32-10 + Box-Muller as documented in include/pita_hip.h, in numpy (uint64 / float64)."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    w, pt = np.meshgrid(np.asarray(walkers, dtype=np.uint64), np.asarray(particles, dtype=np.uint64), indexing="ij")
    mask = np.uint64(0xFFFFFFFF)
    c = [w & mask, w >> np.uint64(32), np.full_like(w, step & 0xFFFFFFFF), pt ^ np.uint64(((step >> 32) << 20) & 0xFFFFFFFF)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    u = [((ci >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0 for ci in c]
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    return np.stack([r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r1 * np.cos(2 * np.pi * u[3])], -1)


def philox_host(B, n, d, seed=PHILOX_SEED, offset=PHILOX_OFFSET, step=PHILOX_STEP):
    """[B, n*d] float64: the first d normals of (walker offset + w, step, particle i)."""
    z = _philox_normals_host(seed, np.uint64(offset) + np.arange(B, dtype=np.uint64), step, np.arange(n))
    return z[:, :, :d].reshape(B, n * d)


def fill_normal(pa, B, n, d, seed=PHILOX_SEED, offset=PHILOX_OFFSET, step=PHILOX_STEP):
    out = torch.full((B, n * d), float("nan"), device="cuda")
    rc = pa._lib.lib().pita_fill_normal(out.data_ptr(), B, n, d, seed, offset, step, pa._lib.stream_ptr())
    return rc, out


# ------------------------------------------------------------------ MALA on a quadratic target
MALA_K = 1.5  # log p = -k |x|^2 / 2, force = -k x: closed form for any (n, d)
MALA_SHAPES = ((1, 1), (1, 2), (2, 3), (85, 2), (86, 1), (128, 3), (256, 1), (256, 3))
# step size per shape: the one of a 1.25-fold ladder at which the float64 reference accepts closest to half of 3 000 walkers
MALA_DT = {(1, 1): 2.7, (1, 2): 1.7, (2, 3): 1.1, (85, 2): 0.45, (86, 1): 0.5, (128, 3): 0.35, (256, 1): 0.37, (256, 3): 0.29}
# (n, d, B) -> seed of a case's inputs where 0 would not do.  A seed has to give an acceptance of 30 - 70 % in the float64
# reference and keep the cap on walkers left out of the decision comparison; tests/test_step_shapes_cpu.py asserts both
# from the reference alone.  Seed 0 does in every case, so the table is empty.
MALA_SEEDS = {}
MALA_EXCLUDE_FRACTION, MALA_EXCLUDE_MAX = 0.02, 5


def mala_cases():
    out = [(n, d, ragged_batch(n)) for n, d in MALA_SHAPES]
    return out + [(256, 1, 4100)]


MALA_CASES = mala_cases()
mala_case_id = lambda c: f"{c[0]}x{c[1]}_B{c[2]}"


def mala_dt(n, d):
    return MALA_DT[(n, d)]


def quad_logp_force(x):
    return -0.5 * MALA_K * (x * x).sum(dim=1), -MALA_K * x


def mala_inputs(n, d, B, seed=None):
    """(x [B, n*d] ~ N(0, 1/k) + 0.2 (not mean-free), noise, uniforms in (0, 1)), float32."""
    seed = MALA_SEEDS.get((n, d, B), 0) if seed is None else seed
    gen = torch.Generator().manual_seed(661000 + 1009 * n + 17 * d + 7919 * seed + B)
    x = torch.randn(B, n * d, generator=gen) / math.sqrt(MALA_K) + 0.2
    nz = torch.randn(B, n * d, generator=gen)
    u = (torch.randint(0, 1 << 24, (B,), generator=gen).float() + 0.5) / 16777216.0
    return x.contiguous(), nz.contiguous(), u.contiguous()


def mala_ratio(x, noise, dt, dtype):
    """(x_prop, ratio = (logp' - logp) + (log q_b - log q_f), logp, logp') of the header's MALA formulas in ``dtype``."""
    x, noise = x.to(dtype), noise.to(dtype)
    lp, F = quad_logp_force(x)
    xp = (x + 0.5 * dt * F) + torch.sqrt(torch.tensor(dt, dtype=dtype)) * noise
    lpp, Fp = quad_logp_force(xp)
    lqf = -((xp - (x + 0.5 * dt * F)) ** 2).sum(1) / (2 * dt)
    lqb = -((x - (xp + 0.5 * dt * Fp)) ** 2).sum(1) / (2 * dt)
    return xp, (lpp - lp) + (lqb - lqf), lp, lpp


_MALA_REF = {}


def mala_reference(n, d, B, seed=None):
    """O.mala_step in float64 on the float32 inputs, with the margin |log u - ratio| of every walker, the worst error
    delta32 of the float32 restatement's ratio, and the walkers left out of the decision comparison (margin < 8 delta32)."""
    key = (n, d, B, seed)
    if key not in _MALA_REF:
        x, nz, u = mala_inputs(n, d, B, seed)
        dt = mala_dt(n, d)
        lp64, _ = quad_logp_force(x.double())
        log_u = torch.log(u.double())
        x_new, lp_new, acc = O.mala_step(x.double(), lp64, quad_logp_force, dt, nz.double(), log_u)
        xp64, r64, _, lpp64 = mala_ratio(x, nz, dt, torch.float64)
        _, r32, _, _ = mala_ratio(x, nz, dt, torch.float32)
        delta32 = float((r32.double() - r64).abs().max())
        margin = (log_u - r64).abs()
        _MALA_REF[key] = dict(x=x, noise=nz, u=u, dt=dt, logp=lp64, x_prop=xp64, logp_prop=lpp64, ratio=r64, x_new=x_new,
                              logp_new=lp_new, acc=acc, acc_restated=log_u < r64, delta32=delta32, margin=margin,
                              left_out=margin < FACTOR * delta32)
    return _MALA_REF[key]


def mala_conditions(r):
    """What a case's seed has to give, from the reference alone: (acceptance within 30 - 70 %, walkers left out within
    the cap, an accepted and a rejected walker among the compared ones)."""
    B = r["acc"].numel()
    rate = float(r["acc"].double().mean())
    n_out = int(r["left_out"].sum())
    kept = r["acc"][~r["left_out"]]
    return (0.3 <= rate <= 0.7, n_out <= min(MALA_EXCLUDE_MAX, math.floor(MALA_EXCLUDE_FRACTION * B)),
            bool(kept.any()) and bool((~kept).any()))


def adapt_reference(dt, acc, total, adaptive):
    """mala_adapt's rule (header): rate = acc / total as the float32 quotient the reference's float mean gives, compared
    in double with 0.55; dt * 1.1 or dt / 1.1 in double."""
    rate = np.float32(acc) / np.float32(total)
    if not adaptive:
        return dt, rate
    return (dt * 1.1 if float(rate) > 0.55 else dt / 1.1), rate


ADAPT_CASES = ((100, 0), (100, 54), (100, 55), (100, 56), (100, 100), (20, 11), (4100, 2254), (4100, 2255), (4100, 2256),
               (7, 3), (7, 4))  # (total, acc_count): 55/100, 11/20 and 2255/4100 round to 0.55f, which is ABOVE the double 0.55
