"""Evaluation quantities the reference reports for generated samples: 1-D Wasserstein
distances between energy samples (``energy_distances``, distribution_distances.py:13-33, POT ``emd2_1d``) and between
interatomic-distance samples (energytemp_module.py:1157-1191).  Energies come from the HIP target kernels; the 1-D
optimal transport between two empirical measures is the sorted-sample coupling (device sort)."""
import math

import torch


def _w_1d(a: torch.Tensor, b: torch.Tensor, p: int):
    a, _ = torch.sort(a.double().flatten())
    b, _ = torch.sort(b.double().flatten())
    if a.numel() != b.numel():  # general sizes: merge the two quantile grids
        qa = torch.arange(1, a.numel() + 1, device=a.device, dtype=torch.float64) / a.numel()
        qb = torch.arange(1, b.numel() + 1, device=b.device, dtype=torch.float64) / b.numel()
        q = torch.unique(torch.cat([qa, qb]))
        w = torch.diff(torch.cat([q.new_zeros(1), q]))
        ia = torch.clamp(torch.searchsorted(qa, q - 1e-15), max=a.numel() - 1)
        ib = torch.clamp(torch.searchsorted(qb, q - 1e-15), max=b.numel() - 1)
        return float((w * (a[ia] - b[ib]).abs() ** p).sum())
    return float(((a - b).abs() ** p).mean())


def _relative_weights(logw: torch.Tensor) -> torch.Tensor:
    """exp(logw - max over the finite entries) in double; NaN and +inf entries get weight 0 (left out), -inf gives 0."""
    lw = logw.double().flatten()
    fin = torch.isfinite(lw)
    m = lw[fin].max() if bool(fin.any()) else lw.new_zeros(())
    return torch.where(fin, torch.exp(lw - m), torch.zeros_like(lw))


def _w_1d_weighted(a: torch.Tensor, wa, b: torch.Tensor, wb, p: int):
    """1-D optimal-transport cost sum |Qa - Qb|^p dq between two WEIGHTED empirical measures (weights ``wa`` / ``wb``
    >= 0 of the shape of ``a`` / ``b``, None = equal weights): the two quantile functions are merged on the union of
    their cumulative-weight grids and compared at the midpoint of every interval.  fp64, torch ops on the inputs' device."""
    def grid(v, w):
        v, order = torch.sort(v.double().flatten())
        w = torch.ones_like(v) if w is None else w.double().flatten()[order]
        c = torch.cumsum(w, 0)
        return v, c / c[-1]

    a, ca = grid(a, wa)
    b, cb = grid(b, wb)
    q, _ = torch.sort(torch.cat([ca, cb]))
    dq = torch.diff(torch.cat([q.new_zeros(1), q]))
    mid = q - 0.5 * dq  # an interval of zero width contributes nothing, wherever its midpoint lands
    ia = torch.clamp(torch.searchsorted(ca, mid), max=a.numel() - 1)
    ib = torch.clamp(torch.searchsorted(cb, mid), max=b.numel() - 1)
    return float((dq * (a[ia] - b[ib]).abs() ** p).sum())


def energy_distances(pred: torch.Tensor, true: torch.Tensor, prefix: str = "", energy_threshold: float = 1000,
                     pred_logweights: torch.Tensor = None):
    """Same dictionary as the reference's ``energy_distances`` (W2 = sqrt of the squared-euclidean 1-D OT cost,
    W1 = euclidean cost, plus the 'cropped' variants that zero out |E| > threshold entries of ``pred``).
    ``pred_logweights`` (an extension, shape of ``pred``): importance log-weights of the generated energies; the
    distances, ``mean_dist`` and the cropped variants then use the self-normalised weights (``_w_1d_weighted``)."""
    mask = (pred < -energy_threshold) | (pred > energy_threshold)
    cp, ct = (~mask) * pred, (~mask) * true if mask.shape == true.shape else true
    if pred_logweights is not None:
        w = _relative_weights(pred_logweights)
        mean = (w * pred.double().flatten()).sum() / w.sum()
        return {f"{prefix}/energy_w2": math.sqrt(_w_1d_weighted(true, None, pred, w, 2)),
                f"{prefix}/energy_w1": _w_1d_weighted(true, None, pred, w, 1),
                f"{prefix}/mean_dist": float((mean - true.double().mean()).abs()),
                f"{prefix}/cropped_energy_w2": math.sqrt(_w_1d_weighted(ct, None, cp, w, 2)),
                f"{prefix}/cropped_energy_w1": _w_1d_weighted(ct, None, cp, w, 1),
                f"{prefix}/num_cropped": int(mask.sum())}
    out = {f"{prefix}/energy_w2": math.sqrt(_w_1d(true, pred, 2)), f"{prefix}/energy_w1": _w_1d(true, pred, 1),
           f"{prefix}/mean_dist": float((pred.double().mean() - true.double().mean()).abs())}
    out[f"{prefix}/cropped_energy_w2"] = math.sqrt(_w_1d(ct, cp, 2))
    out[f"{prefix}/cropped_energy_w1"] = _w_1d(ct, cp, 1)
    out[f"{prefix}/num_cropped"] = int(mask.sum())
    return out


def interatomic_w2(energy_function, pred: torch.Tensor, true: torch.Tensor, pred_logweights: torch.Tensor = None) -> float:
    """W2 between the pooled interatomic-distance samples of two walker sets; with ``pred_logweights`` (one per walker
    of ``pred``) every distance of a generated walker carries that walker's weight."""
    if pred_logweights is not None:
        d_pred = energy_function.interatomic_dist(pred)
        w = _relative_weights(pred_logweights).repeat_interleave(d_pred.shape[-1])
        return math.sqrt(_w_1d_weighted(energy_function.interatomic_dist(true), None, d_pred, w, 2))
    return math.sqrt(_w_1d(energy_function.interatomic_dist(true), energy_function.interatomic_dist(pred), 2))


def histogram(values: torch.Tensor, edges) -> torch.Tensor:
    """Counts of ``values`` (any shape, device tensor) over ``edges`` (ascending, nbins + 1) as ``numpy.histogram`` counts
    them -- half-open bins, the last one closed, out-of-range values and NaNs dropped (pita_histogram: one pass,
    LDS-privatised bins).  Returns int64 [nbins] on the device."""
    from . import _lib

    v = _lib.dev_tensor(values.reshape(-1).float().contiguous(), "values")
    e = torch.as_tensor(edges, dtype=torch.float32).to(v.device).contiguous()
    nb = e.numel() - 1
    counts = torch.empty(nb, dtype=torch.int64, device=v.device)
    _lib.check(_lib.lib().pita_histogram(v.data_ptr(), v.numel(), e.data_ptr(), nb, counts.data_ptr(), _lib.stream_ptr(v.device)),
               "pita_histogram")
    return counts


_LOGWEIGHT_STATS = ("max", "log_mean_weight", "ess", "ess_fraction", "n_bad", "n_neg_inf")


def logweight_stats(logw: torch.Tensor):
    """Diagnostics of importance log-weights (pita_logweight_stats; fp64 sums in a fixed order): for a 1-D device tensor
    a dict of Python floats -- ``max`` over the finite entries, ``log_mean_weight`` = log((1/B) sum exp(logw)), the
    effective sample size ``ess`` = (sum w)^2 / sum w^2 and ``ess_fraction`` = ess / B, ``n_bad`` the number of NaN or
    +inf entries (left out of every sum) and ``n_neg_inf`` the number of -inf entries (weight 0).  For ``[N, B]`` one
    float64 numpy array of length N per key, one row at a time; one host transfer in either case."""
    from . import _lib

    a = _lib.dev_tensor(logw, "logw")
    if a.dim() not in (1, 2) or a.shape[-1] < 1:
        raise ValueError(f"logweight_stats expects [B] or [N, B] log-weights with B >= 1, got {tuple(a.shape)}")
    rows = a.reshape(-1, a.shape[-1])
    out = torch.empty(rows.shape[0], 6, dtype=torch.float64, device=a.device)
    L, st = _lib.lib(), _lib.stream_ptr(a.device)
    for k in range(rows.shape[0]):
        _lib.check(L.pita_logweight_stats(rows[k].data_ptr(), rows.shape[1], out[k].data_ptr(), None, st),
                   "pita_logweight_stats")
    h = out.cpu().numpy()
    if a.dim() == 1:
        return {name: float(h[0, j]) for j, name in enumerate(_LOGWEIGHT_STATS)}
    return {name: h[:, j].copy() for j, name in enumerate(_LOGWEIGHT_STATS)}


def _density(counts: torch.Tensor, edges):
    import numpy as np

    n = counts.cpu().numpy()
    db = np.array(np.diff(np.asarray(edges)), float)  # numpy.histogram(density=True): widths in the edges' own dtype first
    return n / db / n.sum()


class WeightedHistogram:
    """Result of ``weighted_histogram`` / ``pair_distance_histogram`` for P populations:

    * ``raw``     int64 [P, nbins] on the device: the kernel's fixed-point bin sums (below 2^63), bitwise independent of
      the order of the walkers inside a population, of P and of the population's place in the batch;
    * ``counts``  int64 [P, nbins] on the device: plain counts over the walkers that were not left out;
    * ``weights`` float64 [P, nbins] on the device: ``raw * 2^-shift``, sums of the relative weights exp(logw - log_scale);
    * ``log_scale``, ``n_bad``, ``n_neg_inf`` float64 numpy [P]: the maximum finite log-weight of each population (0 where
      there is none), its NaN / +inf entries (left out) and its -inf entries (weight 0);  ``shift`` the fixed-point shift."""

    def __init__(self, raw, counts, info):
        h = info.cpu().numpy()
        self.raw, self.counts = raw, counts
        self.log_scale, self.n_bad, self.n_neg_inf, self.shift = h[:, 0].copy(), h[:, 1].copy(), h[:, 2].copy(), int(h[0, 3])
        self.weights = raw.double() * 2.0 ** -self.shift

    def density(self, edges):
        """Self-normalised density per population, numpy float64 [P, nbins] (``numpy.histogram(density=True, weights=w)``
        row by row); a row is NaN where the population's weight sum is 0."""
        import numpy as np

        w = self.weights.cpu().numpy()
        db = np.array(np.diff(np.asarray(edges)), float)
        tot = w.sum(axis=1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(tot > 0, w / db / tot, np.nan)


def _population_args(n_rows: int, logweights, populations, device):
    P = 1 if populations is None else int(populations)
    if P < 1 or n_rows < 1 or n_rows % P:
        raise ValueError(f"{n_rows} walkers do not split into populations={populations} equal populations")
    lw = None
    if logweights is not None:
        from . import _lib

        lw = _lib.dev_tensor(logweights.reshape(-1), "logweights")
        if lw.numel() != n_rows or lw.device != device:
            raise ValueError(f"logweights: expected {n_rows} entries on {device}, got {lw.numel()} on {lw.device}")
    return P, n_rows // P, lw


def weighted_histogram(values: torch.Tensor, edges, logweights: torch.Tensor = None, populations: int = 1,
                       per_walker: int = 1) -> WeightedHistogram:
    """Importance-weighted histogram per population (pita_weighted_histogram; an extension).  ``values``: device tensor of
    ``B * per_walker`` entries, value k belonging to walker ``k // per_walker``; the B walkers are ``populations`` equal
    slices in the integrator's layout; ``logweights`` [B] (None = unit weights); ``edges`` and the bin rule as in
    ``histogram``.  Order-independent fixed-point sums, see ``WeightedHistogram``."""
    from . import _lib

    v = _lib.dev_tensor(values.reshape(-1).float().contiguous(), "values")
    if per_walker < 1 or v.numel() % per_walker:
        raise ValueError(f"{v.numel()} values are not {per_walker} per walker")
    P, S, lw = _population_args(v.numel() // per_walker, logweights, populations, v.device)
    e = torch.as_tensor(edges, dtype=torch.float32).to(v.device).contiguous()
    nb = e.numel() - 1
    raw, counts = (torch.empty(P, max(nb, 0), dtype=torch.int64, device=v.device) for _ in range(2))
    info = torch.empty(P, 4, dtype=torch.float64, device=v.device)
    _lib.check(_lib.lib().pita_weighted_histogram(v.data_ptr(), _lib.ptr(lw), P, S, per_walker, e.data_ptr(), nb, raw.data_ptr(),
                                                  counts.data_ptr(), info.data_ptr(), _lib.stream_ptr(v.device)),
               "pita_weighted_histogram")
    return WeightedHistogram(raw, counts, info)


def pair_distance_histogram(energy_function, samples: torch.Tensor, edges, logweights: torch.Tensor = None,
                            populations: int = 1) -> WeightedHistogram:
    """The same histogram over the interatomic distances of ``samples`` [B, n * d] (unnormalised as
    ``energy_function.interatomic_dist`` does), computed from the coordinates in one call
    (pita_pair_distance_histogram): the [B, n (n - 1) / 2] distance array is never written."""
    from . import _lib

    n, d = energy_function.n_particles, energy_function.n_spatial_dim
    x = samples.reshape(-1, n * d)
    if energy_function.should_normalize:
        x = energy_function.unnormalize(x)
    x = _lib.dev_tensor(x, "samples")
    P, S, lw = _population_args(x.shape[0], logweights, populations, x.device)
    e = torch.as_tensor(edges, dtype=torch.float32).to(x.device).contiguous()
    nb = e.numel() - 1
    raw, counts = (torch.empty(P, max(nb, 0), dtype=torch.int64, device=x.device) for _ in range(2))
    info = torch.empty(P, 4, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().pita_pair_distance_histogram(x.data_ptr(), _lib.ptr(lw), P, S, n, d, e.data_ptr(), nb, raw.data_ptr(),
                                                       counts.data_ptr(), info.data_ptr(), _lib.stream_ptr(x.device)),
               "pita_pair_distance_histogram")
    return WeightedHistogram(raw, counts, info)


def weighted_mean(values: torch.Tensor, logweights: torch.Tensor = None, populations: int = 1):
    """Self-normalised importance estimate of one value per walker, per population (pita_weighted_moments; fp64 sums in a
    fixed order): a dict of float64 numpy arrays [P] -- ``mean`` = sum w v / sum w, ``var`` = sum w v^2 / sum w - mean^2
    (weighted, biased), ``ess`` and ``ess_fraction`` = ess / pop_size of the population's log-weights (``logweight_stats``
    on its slice; the number of kept walkers without log-weights), ``n_bad`` the walkers left out (log-weight NaN or +inf,
    or a value that is not finite), ``n_neg_inf`` and ``log_scale``.  ``mean`` and ``var`` are NaN where sum w is 0."""
    import numpy as np
    from . import _lib

    v = _lib.dev_tensor(values.reshape(-1), "values")
    P, S, lw = _population_args(v.numel(), logweights, populations, v.device)
    out = torch.empty(P, 6, dtype=torch.float64, device=v.device)
    _lib.check(_lib.lib().pita_weighted_moments(v.data_ptr(), _lib.ptr(lw), P, S, out.data_ptr(), _lib.stream_ptr(v.device)),
               "pita_weighted_moments")
    h = out.cpu().numpy()
    s0, s1, s2 = h[:, 1], h[:, 2], h[:, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(s0 > 0, s1 / s0, np.nan)
        var = np.where(s0 > 0, s2 / s0 - mean * mean, np.nan)
    ess = s0.copy() if lw is None else np.atleast_1d(logweight_stats(lw.reshape(P, S))["ess"])
    return {"mean": mean, "var": var, "ess": ess, "ess_fraction": ess / S, "n_bad": h[:, 4].copy(),
            "n_neg_inf": h[:, 5].copy(), "log_scale": h[:, 0].copy()}


def population_summary(per_pop):
    """Error bar over independent populations: ``per_pop`` is [P] or [P, ...], one estimate per population.  Returns a
    dict with ``mean`` = the plain mean over the populations whose estimate is finite (every entry of the row),
    ``stderr`` = std(ddof=1) / sqrt(n_used) over the same rows (NaN for n_used < 2) and ``n_used``."""
    import numpy as np

    a = np.asarray(per_pop, dtype=np.float64)
    used = a[np.isfinite(a.reshape(a.shape[0], -1)).all(axis=1)]
    n = used.shape[0]
    nan = np.full(a.shape[1:], np.nan)
    return {"mean": used.mean(axis=0) if n >= 1 else nan,
            "stderr": used.std(axis=0, ddof=1) / math.sqrt(n) if n >= 2 else nan, "n_used": n}


def sample_histograms(energy_function, samples: torch.Tensor, test_set: torch.Tensor, energy_samples: torch.Tensor = None,
                      bins: int = 100, logweights: torch.Tensor = None, populations: int = None):
    """The numbers under the reference's sample figure (``get_dataset_fig``, base_molecule_energy_function.py:160-254):
    two pairs of ``bins``-bin density arrays, generated samples against the test set --

    * interatomic distances: bin edges from the TEST set's distances (``hist(dist_test, bins=100, density=True)``), the
      generated distances counted on the same edges (:168-187);
    * energies ``-log p``: ``bins`` equal bins over ``(min(E_test) - 10, max(E_test) + 10)`` (:213-238).

    Bin edges are numpy's own for that range and dtype (``numpy.histogram_bin_edges``), the counting runs on the device.
    Returns a dict of numpy arrays: ``dist_edges, dist_test, dist_samples, energy_edges, energy_test, energy_samples``.

    An extension, off unless asked for: with ``logweights`` ([B] importance log-weights of ``samples``) and / or
    ``populations`` (P equal slices of the walkers, the integrator's layout) the generated side is weighted and taken per
    population -- ``dist_samples_pop`` / ``energy_samples_pop`` [P, bins] are the self-normalised weighted densities of the
    populations (the distances by the fused pair-distance kernel), ``dist_samples`` / ``energy_samples`` their
    ``population_summary`` mean and ``dist_samples_stderr`` / ``energy_samples_stderr`` its standard error.  The test-set
    side is unweighted as before."""
    import numpy as np

    d_test = energy_function.interatomic_dist(test_set).reshape(-1).float()
    mm = torch.stack([d_test.min(), d_test.max()]).cpu().numpy().astype(np.float32)
    d_edges = np.histogram_bin_edges(mm, bins=bins)
    e_test = -energy_function(test_set).float()
    e_gen = -(energy_function(samples) if energy_samples is None else energy_samples).float()
    em = torch.stack([e_test.min(), e_test.max()]).cpu().numpy().astype(np.float32)
    e_edges = np.histogram_bin_edges(em, bins=bins, range=(float(em[0]) - 10, float(em[1]) + 10))
    if logweights is not None or populations is not None:
        P = 1 if populations is None else populations
        d_pop = pair_distance_histogram(energy_function, samples, d_edges, logweights, P).density(d_edges)
        e_pop = weighted_histogram(e_gen, e_edges, logweights, P).density(e_edges)
        d_sum, e_sum = population_summary(d_pop), population_summary(e_pop)
        return {"dist_edges": d_edges, "dist_test": _density(histogram(d_test, d_edges), d_edges),
                "dist_samples": d_sum["mean"], "dist_samples_pop": d_pop, "dist_samples_stderr": d_sum["stderr"],
                "energy_edges": e_edges, "energy_test": _density(histogram(e_test, e_edges), e_edges),
                "energy_samples": e_sum["mean"], "energy_samples_pop": e_pop, "energy_samples_stderr": e_sum["stderr"]}
    d_gen = energy_function.interatomic_dist(samples).reshape(-1).float()
    return {"dist_edges": d_edges, "dist_test": _density(histogram(d_test, d_edges), d_edges),
            "dist_samples": _density(histogram(d_gen, d_edges), d_edges),
            "energy_edges": e_edges, "energy_test": _density(histogram(e_test, e_edges), e_edges),
            "energy_samples": _density(histogram(e_gen, e_edges), e_edges)}


# ------------------------------------------------------------------------------------------------- dihedral observables
# An extension: the reference takes (phi, psi) from mdtraj on the host, unweighted, the batch as one population.
ALDP_PHI_PSI = ((4, 6, 8, 14), (6, 8, 14, 16))  # alanine dipeptide in amber order: phi = (C, N, CA, C), psi = (N, CA, C, N)


def _residues(atom_names, residue_index):
    names, res = list(atom_names), [int(r) for r in residue_index]
    if len(names) != len(res):
        raise ValueError(f"{len(names)} atom names for {len(res)} residue indices")
    atoms = {}
    for i, (nm, r) in enumerate(zip(names, res)):
        atoms.setdefault(r, {}).setdefault(nm, i)
    return atoms


def phi_psi_quads(atom_names, residue_index):
    """Backbone dihedrals from a topology: for every residue r with backbone atoms N, CA, C whose neighbours r - 1 and
    r + 1 exist and carry a C and an N, phi = (C of r - 1, N, CA, C) and psi = (N, CA, C, N of r + 1).  ``atom_names`` /
    ``residue_index``: one name and one residue number per atom, in the order of the coordinates.  Returns
    ``(quads, residues)``: int64 numpy ``[n_res, 2, 4]`` (what ``ramachandran_histogram`` takes) and the residue numbers."""
    import numpy as np

    atoms = _residues(atom_names, residue_index)
    quads, residues = [], []
    for r in sorted(atoms):
        a, prev, nxt = atoms[r], atoms.get(r - 1, {}), atoms.get(r + 1, {})
        if all(k in a for k in ("N", "CA", "C")) and "C" in prev and "N" in nxt:
            quads.append(((prev["C"], a["N"], a["CA"], a["C"]), (a["N"], a["CA"], a["C"], nxt["N"])))
            residues.append(r)
    return np.array(quads, dtype=np.int64).reshape(-1, 2, 4), np.array(residues, dtype=np.int64)


def chirality_quads(atom_names, residue_index):
    """``(CA, N, C, CB)`` for every residue that has these four atoms: int64 numpy ``[n_centres, 4]`` and the residue
    numbers.  With b1 = N - CA, b2 = C - N, b3 = CB - C the numerator of that dihedral is y = (b1 . (b2 x b3)) |b2|, and
    b1 . (b2 x b3) = (N - CA) . ((C - CA) x (CB - CA)): the sign of the angle's sine is the handedness of the centre."""
    import numpy as np

    atoms = _residues(atom_names, residue_index)
    rows = [(r, a) for r, a in sorted(atoms.items()) if all(k in a for k in ("CA", "N", "C", "CB"))]
    return (np.array([(a["CA"], a["N"], a["C"], a["CB"]) for _, a in rows], dtype=np.int64).reshape(-1, 4),
            np.array([r for r, _ in rows], dtype=np.int64))


def _dihedral_args(samples, quads, width, energy_function):
    """Host-side checks first, then the device tensors: ``samples`` [B, n * 3] or [B, n, 3] as float32 [B, n * 3]
    (unnormalised as ``pair_distance_histogram`` does when the target normalises), n, and ``quads`` (trailing shape
    ``width``, or one item of it) as int32 on the samples' device.  The index check is the one the C entry points leave to
    their caller: every index in [0, n) and the four atoms of a quad distinct."""
    import numpy as np
    from . import _lib

    if samples.dim() not in (2, 3) or (samples.dim() == 3 and samples.shape[-1] != 3) or samples.shape[-1] % 3:
        raise ValueError(f"samples: expected [B, n * 3] or [B, n, 3], got {tuple(samples.shape)}")
    n = samples.shape[1] if samples.dim() == 3 else samples.shape[1] // 3
    x = samples.reshape(samples.shape[0], 3 * n)  # (an empty batch keeps its width)
    q = np.asarray(quads)
    if q.ndim == len(width):
        q = q[None]
    if q.ndim != len(width) + 1 or q.shape[1:] != width or q.shape[0] < 1 or q.dtype.kind not in "iu":
        raise ValueError(f"quads: expected integers of shape [k, {', '.join(map(str, width))}], got {q.dtype} {q.shape}")
    if q.min() < 0 or q.max() >= n:
        raise ValueError(f"quads: atom indices must be in [0, {n}), got {int(q.min())} .. {int(q.max())}")
    flat = np.sort(q.reshape(-1, 4), axis=1)
    if (flat[:, 1:] == flat[:, :-1]).any():
        raise ValueError("quads: the four atoms of a dihedral must be distinct")
    if energy_function is not None and energy_function.should_normalize:
        x = energy_function.unnormalize(x)
    x = _lib.dev_tensor(x, "samples")
    return x, n, torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(x.device)


def dihedral_angles(samples: torch.Tensor, quads, energy_function=None) -> torch.Tensor:
    """Dihedral angles in [-pi, pi] of the atom quadruples ``quads`` ([n_dih, 4] or one quad) of every walker
    (pita_dihedral_angles; the force field's torsion, formula and sign, in fp32).  ``samples``: device tensor [B, n * 3] or
    [B, n, 3]; ``energy_function`` (optional): a target whose ``should_normalize`` is set unnormalises the samples first.
    Returns float32 [B, n_dih] on the device; NaN where a coordinate of the quad is not finite."""
    from . import _lib

    x, n, q = _dihedral_args(samples, quads, (4,), energy_function)
    out = torch.empty(x.shape[0], q.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().pita_dihedral_angles(_lib.ptr(x), x.shape[0], n, q.data_ptr(), q.shape[0], _lib.ptr(out),
                                               _lib.stream_ptr(x.device)), "pita_dihedral_angles")
    return out


def chirality_fraction(samples: torch.Tensor, quads, logweights: torch.Tensor = None, populations: int = 1):
    """Weighted fraction of walkers whose ``chirality_quads`` dihedral (CA, N, C, CB) has a positive sine, i.e. whose
    triple product (N - CA) . ((C - CA) x (CB - CA)) is positive, per population and centre: float64 numpy
    ``[P, n_centres]`` (``dihedral_angles`` and ``weighted_mean`` of the indicator; NaN where a population's weight sum is
    0).  Which sign is the L form is not decided here: compare with a structure of known handedness.  A reflection of
    the coordinates turns f into 1 - f."""
    import numpy as np

    theta = dihedral_angles(samples, quads)
    positive = torch.where(torch.isnan(theta), theta, (theta > 0).float())  # a NaN angle leaves the walker out (n_bad)
    return np.stack([weighted_mean(positive[:, k].contiguous(), logweights, populations)["mean"]
                     for k in range(theta.shape[1])], axis=1)


class DihedralHistogram(WeightedHistogram):
    """Result of ``ramachandran_histogram`` for P populations and n_pair angle pairs: ``raw``, ``counts`` (int64) and
    ``weights`` (float64) of shape ``[P, n_pair, nb_a, nb_b]`` on the device, ``log_scale``, ``n_bad``, ``n_neg_inf`` and
    ``shift`` as in ``WeightedHistogram``, and the float32 numpy bin edges ``edges_a`` / ``edges_b`` of the two axes."""

    def __init__(self, raw, counts, info, edges_a, edges_b):
        super().__init__(raw, counts, info)
        self.edges_a, self.edges_b = edges_a, edges_b

    def density(self):
        """Self-normalised 2-D density per population and pair, numpy float64 ``[P, n_pair, nb_a, nb_b]``: weights over
        (cell area * the pair's weight sum), so that it integrates to 1 over the edges; NaN where that sum is 0."""
        import numpy as np

        w = self.weights.cpu().numpy()
        area = np.outer(np.array(np.diff(self.edges_a), float), np.array(np.diff(self.edges_b), float))
        tot = w.sum(axis=(2, 3), keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(tot > 0, w / area / tot, np.nan)

    def marginal(self, axis: int):
        """Exact integer marginals ``(raw, counts)``, int64 ``[P, n_pair, nb]`` on the device: axis 0 keeps the a-axis
        (sums over b), axis 1 the b-axis."""
        if axis not in (0, 1):
            raise ValueError(f"marginal: axis must be 0 (a) or 1 (b), got {axis}")
        return self.raw.sum(dim=3 - axis), self.counts.sum(dim=3 - axis)


def ramachandran_histogram(samples: torch.Tensor, pair_quads, bins: int = 64, logweights: torch.Tensor = None,
                           populations: int = 1, energy_function=None, edges=None) -> DihedralHistogram:
    """Importance-weighted 2-D histograms of dihedral pairs per population, from the coordinates in one call
    (pita_dihedral_histogram2d; the angles are never written).  ``pair_quads``: ``[n_pair, 2, 4]`` as ``phi_psi_quads``
    returns them (or one pair ``[2, 4]``, e.g. ``ALDP_PHI_PSI``), first axis a, second axis b.  ``edges``: None = ``bins``
    equal bins over [-pi, pi] on both axes (``numpy.linspace(-pi, pi, bins + 1).astype(float32)``), one ascending array
    for both axes, or a pair ``(edges_a, edges_b)``; bins as ``histogram`` counts them, so +pi falls into the last bin
    (no wrap-around).  ``samples``, ``energy_function`` as in ``dihedral_angles``; ``logweights``, ``populations`` and the
    order-independent fixed-point sums as in ``weighted_histogram``.  At most 4096 cells (64 x 64) per pair."""
    import numpy as np
    from . import _lib

    # host-side checks first: the split into populations, the edges, then (in _dihedral_args) the shapes and the indices
    _population_args(samples.shape[0], None, populations, None)
    if edges is None:
        ea = eb = np.linspace(-np.pi, np.pi, int(bins) + 1).astype(np.float32)
    elif isinstance(edges, (tuple, list)) and len(edges) == 2 and np.ndim(edges[0]) == 1:
        ea, eb = (np.asarray(e, dtype=np.float32) for e in edges)
    else:
        ea = eb = np.asarray(edges, dtype=np.float32)
    for e in (ea, eb):
        if e.ndim != 1 or e.size < 2 or not (np.diff(e) > 0).all():
            raise ValueError("edges: expected ascending 1-D arrays of at least two entries")
    x, n, q = _dihedral_args(samples, pair_quads, (2, 4), energy_function)
    P, S, lw = _population_args(x.shape[0], logweights, populations, x.device)
    ta, tb = (torch.from_numpy(np.ascontiguousarray(e)).to(x.device) for e in (ea, eb))
    shape = (P, q.shape[0], ea.size - 1, eb.size - 1)
    raw, counts = (torch.empty(shape, dtype=torch.int64, device=x.device) for _ in range(2))
    info = torch.empty(P, 4, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().pita_dihedral_histogram2d(x.data_ptr(), _lib.ptr(lw), P, S, n, q.data_ptr(), q.shape[0], ta.data_ptr(),
                                                    shape[2], tb.data_ptr(), shape[3], raw.data_ptr(), counts.data_ptr(),
                                                    info.data_ptr(), _lib.stream_ptr(x.device)), "pita_dihedral_histogram2d")
    return DihedralHistogram(raw, counts, info, ea, eb)


MMD_SIGMAS = (0.01, 0.1, 1.0, 10.0, 100.0)  # the bandwidths the reference passes to its mix_rbf_mmd2


def _rbf_gram(a, lw_a, P, S, b, lw_b, gammas):
    """One pita_rbf_gram_sums call: (sums [P, n] , info_a [P, 5], info_b [5] or None) as float64 numpy arrays."""
    import ctypes

    from . import _lib

    n, M = len(gammas), 0 if b is None else b.shape[0]
    L = _lib.lib()
    nbytes = L.pita_rbf_gram_workspace_bytes(P, S, M)
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(P * n + 5 * P + 5, dtype=torch.float64, device=a.device)
    sums, info_a, info_b = out[:P * n], out[P * n:P * n + 5 * P], out[P * n + 5 * P:]
    g = (ctypes.c_double * n)(*gammas)
    _lib.check(L.pita_rbf_gram_sums(a.data_ptr(), _lib.ptr(lw_a), P, S, _lib.ptr(b), _lib.ptr(lw_b), M, a.shape[1], g, n,
                                    sums.data_ptr(), info_a.data_ptr(), 0 if b is None else info_b.data_ptr(), ws.data_ptr(),
                                    _lib.stream_ptr(a.device)), "pita_rbf_gram_sums")
    h = out.cpu().numpy()
    return h[:P * n].reshape(P, n).copy(), h[P * n:P * n + 5 * P].reshape(P, 5).copy(), None if b is None else h[-5:].copy()


def rbf_mmd2(samples: torch.Tensor, test_set: torch.Tensor, sigma_list=MMD_SIGMAS, logweights: torch.Tensor = None,
             populations: int = 1, test_logweights: torch.Tensor = None, biased: bool = True, test_self=None):
    """Squared mix-RBF MMD between every population of ``samples`` [B, D] and ``test_set`` [M, D], importance-weighted,
    on the device (pita_rbf_gram_sums: fused fp32 pair kernel with the difference first, double above it; the pair
    matrix is never written).  The reference's mmd.py is not restated in oracle/: the definition in include/pita_hip.h
    is the specification.  k(x, y) = sum_s exp(-|x - y|^2 / (2 sigma_s^2)); rows of population p carry the relative
    weights w of ``logweights`` (None = unit), test rows v of ``test_logweights``.  With S_xx, S_xy, S_yy the weighted
    Gram sums per bandwidth (diagonal included), W = sum w, W2 = sum w^2 and V, V2 likewise:
      biased (the reference's default):  k_xx = S_xx / W^2,  k_yy = S_yy / V^2,  k_xy = S_xy / (W V);
      unbiased:  k_xx = (S_xx - W2) / (W^2 - W2), k_yy likewise (NaN where the denominator is not positive), k_xy as above;
      mmd2[p] = sum_s (k_xx + k_yy - 2 k_xy), neither clamped nor rooted.
    The caller chooses the features (GMM coordinates, peptide coordinates, anything [., D], D <= 768).  Three device
    calls: self on the samples, cross, self on the test set; the last is skipped when ``test_self`` -- the entry of that
    name of an earlier result against the same test set, weights and bandwidths -- is passed back in.
    Returns a dict of float64 numpy arrays: ``mmd2`` [P], ``mmd2_per_sigma``, ``k_xx``, ``k_xy`` [P, n_sigma], ``k_yy``
    [n_sigma], ``sum_w``, ``sum_w2``, ``n_bad``, ``n_neg_inf``, ``log_scale`` [P], and ``test_self`` = {"sums" [n_sigma],
    "info" [5] = {m, V, V2, n_bad, n_neg_inf}, "gammas" [n_sigma], "rows"}.  A population with sum w = 0 gives NaN."""
    import numpy as np
    from . import _lib

    sig = np.asarray(list(sigma_list), dtype=np.float64).reshape(-1)
    if sig.size < 1 or sig.size > 16 or not (np.isfinite(sig).all() and (sig > 0).all()):
        raise ValueError(f"sigma_list: expected 1 to 16 finite positive bandwidths, got {sigma_list}")
    gammas = 1.0 / (2.0 * sig * sig)
    if not np.isfinite(gammas).all():
        raise ValueError(f"sigma_list: 1 / (2 sigma^2) overflows for {sigma_list}")
    if samples.dim() != 2 or test_set.dim() != 2 or samples.shape[1] != test_set.shape[1] or not 1 <= samples.shape[1] <= 768:
        raise ValueError(f"samples [B, D] and test_set [M, D] with 1 <= D <= 768 expected, got {tuple(samples.shape)} and "
                         f"{tuple(test_set.shape)}")
    if samples.device != test_set.device:
        raise ValueError(f"samples are on {samples.device}, test_set on {test_set.device}")
    P, S, _ = _population_args(samples.shape[0], None, populations, None)
    M = test_set.shape[0]
    if M < 1:
        raise ValueError("test_set is empty")
    for name, t, rows in (("logweights", logweights, samples.shape[0]), ("test_logweights", test_logweights, M)):
        if t is not None and (t.numel() != rows or t.device != samples.device):
            raise ValueError(f"{name}: expected {rows} entries on {samples.device}, got {t.numel()} on {t.device}")
    if test_self is not None:
        ok = isinstance(test_self, dict) and {"sums", "info", "gammas", "rows"} <= set(test_self)
        if not (ok and np.array_equal(np.asarray(test_self["gammas"], np.float64), gammas) and int(test_self["rows"]) == M
                and np.shape(test_self["sums"]) == (sig.size,) and np.shape(test_self["info"]) == (5,)):
            raise ValueError("test_self: not the entry of an rbf_mmd2 result with this test set size and these bandwidths")
    x = _lib.dev_tensor(samples, "samples")
    y = _lib.dev_tensor(test_set, "test_set")
    _, _, lw = _population_args(x.shape[0], logweights, populations, x.device)
    _, _, lv = _population_args(M, test_logweights, 1, x.device)
    g = [float(v) for v in gammas]
    s_xx, info_x, _ = _rbf_gram(x, lw, P, S, None, None, g)
    s_xy, _, info_y = _rbf_gram(x, lw, P, S, y, lv, g)
    if test_self is None:
        s_yy, _, _ = _rbf_gram(y, lv, 1, M, None, None, g)
        test_self = {"sums": s_yy[0], "info": info_y, "gammas": gammas.copy(), "rows": M}
    s_yy, info_y = np.asarray(test_self["sums"], np.float64), np.asarray(test_self["info"], np.float64)
    W, W2, V, V2 = info_x[:, 1:2], info_x[:, 2:3], info_y[1], info_y[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        if biased:
            k_xx = np.where(W > 0, s_xx / (W * W), np.nan)
            k_yy = s_yy / (V * V) if V > 0 else np.full_like(s_yy, np.nan)
        else:
            dx, dy = W * W - W2, V * V - V2
            k_xx = np.where(dx > 0, (s_xx - W2) / dx, np.nan)
            k_yy = (s_yy - V2) / dy if dy > 0 else np.full_like(s_yy, np.nan)
        k_xy = np.where(W * V > 0, s_xy / (W * V), np.nan)
    per = k_xx + k_yy[None, :] - 2.0 * k_xy
    return {"mmd2": per.sum(1), "mmd2_per_sigma": per, "k_xx": k_xx, "k_xy": k_xy, "k_yy": k_yy, "sum_w": info_x[:, 1].copy(),
            "sum_w2": info_x[:, 2].copy(), "n_bad": info_x[:, 3].copy(), "n_neg_inf": info_x[:, 4].copy(),
            "log_scale": info_x[:, 0].copy(), "test_self": test_self}


def mix_rbf_mmd2(X: torch.Tensor, Y: torch.Tensor, sigma_list=MMD_SIGMAS, biased: bool = True) -> float:
    """The reference's signature: one unweighted sample set against another, ``rbf_mmd2(...)["mmd2"][0]``."""
    return float(rbf_mmd2(X, Y, sigma_list, biased=biased)["mmd2"][0])
