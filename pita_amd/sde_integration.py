"""Annealed reverse-SDE sampler driving the HIP kernels.

Mirror of ``WeightedSDEIntegrator`` (pita/src/models/components/sde_integration.py:48-470):
same constructor, ``integrate_sde(x1, energy_function, annealing_factor_schedule,
inverse_temperature, annealing_factor_score, resampling_interval)`` and the same 5-tuple result.

How the work is laid out on MI355X (differences from the reference are deliberate):
  * the per-step scalars (h, g^2, gamma, EDM coefficients, dt) are computed once on the HOST in the
    reference's fp32 op order and uploaded as a [N, 16] table;
  * with the HIP EGNN backbone the whole trajectory between two resampling events is ONE kernel
    launch (pita_egnn_sampler_run): walkers stay in registers, no per-step launch, no per-step
    all_gather, no per-step device->host copy of SDETerms (reference :248-258,:289);
  * walkers are sharded over ranks by contiguous slices exactly like :227-233, and gathered ONCE
    at the end (RCCL all_gather); a resampling event is global like the reference's, but only the
    log-weights are gathered -- the walkers move in one all_to_all_single that carries each rank the
    distinct parents it needs (_Comm.exchange_rows);
  * noise is Philox4x32-10 keyed by (seed, GLOBAL walker index, step): the result does not depend
    on the number of GPUs.  ``noise=`` injects recorded normals for parity tests.
  * ``populations=P`` (an extension): the batch is P independent populations of any size, each resampled on its own --
    in one launch per event up to 2 048 walkers (pita_population_resample), in a fixed number of launches beyond
    (pita_population_resample_blocks); events are rank-local, the log-weights and the event log are gathered once after
    the loop.
``sde_terms_all`` has N entries like the reference's (:150,:212).  By default each field is a ``TermStats`` (sum,
sum of squares, count over the global batch, reduced on the device) that answers ``.mean()`` / ``.std()`` -- the only
things the reference's callers ever ask of these tensors (energytemp_module.py:938-945,1132-1143);
``record_terms=True`` materialises the full per-step tensors instead (per-step launch path).

Layout: ``integrate_sde`` puts what is fixed for a run into one ``_Run`` record and runs the regime's loop -- its own for
the default regime (log-weights identically zero, fused launches between events), ``_integrate_debiased`` per step for the
Feynman-Kac weights --, then ``_finish_weights`` (end-of-run reweighting, diagnostics, counts) and ``_post_process``
(descent, MALA, final all-gather).  Who resamples, and with which collectives, is one policy object per run, chosen once
from ``(populations, ess_threshold)``: ``_GlobalEvents`` (fixed schedule, or ESS-triggered with a threshold) or
``_PopulationEvents``; both answer ``skip_zero_weight_events``, ``event``, ``end_event``, ``collect``, ``gather``, ``finish``.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from ._target import MalaPopulations
from .data_utils import remove_mean
from .metrics import logweight_stats
from .sdes import SDETerms, TermStats, VEReverseSDE  # noqa: F401
from .utils import (MAX_POPULATION_SIZE, gather_rows, sample_cat_sys, sample_cat_sys_adaptive,
                    sample_cat_sys_population_blocks, sample_cat_sys_populations)


def _scalar(v):
    return float(v.reshape(-1)[0]) if isinstance(v, torch.Tensor) else float(v)


def _quantile_clamp(a, q, chunk=None):
    """clamp(a, max=quantile(a, q)) on a copy (K11 kernel; sde_integration.py:179): whole vector, or per ``chunk`` entries."""
    a = _lib.dev_tensor(a, "a").clone()
    _lib.check(_lib.lib().pita_quantile_clamp(a.data_ptr(), a.shape[0], a.shape[0] if chunk is None else chunk, float(q),
                                              _lib.stream_ptr(a.device)), "pita_quantile_clamp")
    return a


PROBE_STREAM_ID = 3  # WeightedSDEIntegrator._key: the Hutchinson probes' stream (0: noise, 1 and 2: the MALA chains)
_STEP_TABLES = {}  # key -> table; the last few (schedule, grid) combinations of this process


def _schedule_key(obj):
    """Hashable identity of a schedule by VALUE (class + plain-number attributes); None when it carries anything else."""
    try:
        attrs = vars(obj)
    except TypeError:  # no __dict__ (slots, builtins): not cacheable by value
        return None
    items = []
    for k, v in sorted(attrs.items()):
        if isinstance(v, (bool, int, float, str, type(None))):
            items.append((k, v))
        else:
            return None
    return (type(obj).__module__, type(obj).__qualname__, tuple(items))


def build_step_table(noise_schedule, annealing_factor_schedule, times, dt, diffusion_scale, inverse_temperature):
    """[N, 16] float32 host table of per-step scalars in the reference's fp32 op order
    (score_net.py:26-29; sdes.py:119-122,140,250; sde_integration.py:347).

    The N rows are computed one 0-dim tensor at a time, as the reference computes them (a vectorised evaluation may
    differ in the last bit of a ``pow``): 65 ms for 1 000 steps on the GPU box's host -- 6 % of a whole 1 000-step LJ13
    trajectory and a third of a DW4 one.  The table only depends on the two schedules' parameters and the grid, so the
    last few are kept by value and a repeated ``integrate_sde`` with the same settings gets a copy."""
    ks, ka = _schedule_key(noise_schedule), _schedule_key(annealing_factor_schedule)
    key = None
    if ks is not None and ka is not None:
        tt = torch.as_tensor(times, dtype=torch.float32).detach().cpu().contiguous()
        key = (ks, ka, tt.numpy().tobytes(), float(dt), float(diffusion_scale), float(inverse_temperature))
        hit = _STEP_TABLES.get(key)
        if hit is not None:
            return hit.clone()
    tab = _build_step_table(noise_schedule, annealing_factor_schedule, times, dt, diffusion_scale, inverse_temperature)
    if key is not None:
        if len(_STEP_TABLES) >= 8:
            _STEP_TABLES.pop(next(iter(_STEP_TABLES)))
        _STEP_TABLES[key] = tab.clone()
    return tab


def _build_step_table(noise_schedule, annealing_factor_schedule, times, dt, diffusion_scale, inverse_temperature):
    N = len(times)
    tab = torch.zeros(N, _lib.STEP_STRIDE, dtype=torch.float32)
    sqrt_dt = np.sqrt(dt)
    for k in range(N):
        t = times[k]  # 0-dim fp32 CPU tensor
        ht = noise_schedule.h(t)
        g = noise_schedule.g(t)
        tab[k, _lib.ST_CS] = 1 / (1 + ht)
        c_in = 1 / (1 + ht) ** 0.5
        tab[k, _lib.ST_CIN] = c_in
        tab[k, _lib.ST_COUT] = ht**0.5 * c_in
        tab[k, _lib.ST_CNOISE] = (1 / 8) * torch.log(ht)
        tab[k, _lib.ST_H] = ht
        tab[k, _lib.ST_G2] = g.pow(2)
        tab[k, _lib.ST_GAMMA] = _scalar(annealing_factor_schedule.gamma(t))
        tab[k, _lib.ST_DT] = dt
        tab[k, _lib.ST_NOISE_SCALE] = diffusion_scale * g
        tab[k, _lib.ST_SQRT_DT] = sqrt_dt
        tab[k, _lib.ST_BETA] = float(inverse_temperature)
    return tab


class _Comm:
    """Rank / world / all_gather, from the Lightning module the reference passes
    (sde_integration.py:227-229,248) or from torch.distributed (RCCL) when that is initialised."""

    def __init__(self, lightning_module):
        self.lm = lightning_module
        if lightning_module is not None and getattr(lightning_module, "trainer", None) is not None:
            self.world = int(lightning_module.trainer.world_size)
            self.rank = int(lightning_module.trainer.global_rank)
        elif torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world = torch.distributed.get_world_size()
            self.rank = torch.distributed.get_rank()
        else:
            self.world, self.rank = 1, 0

    def all_gather(self, x):
        if self.world == 1:
            return x
        if self.lm is not None and hasattr(self.lm, "all_gather") and not torch.distributed.is_initialized():
            return self.lm.all_gather(x).reshape(-1, *x.shape[1:])
        out = torch.empty((self.world * x.shape[0],) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
        torch.distributed.all_gather_into_tensor(out, x.contiguous())
        return out

    def all_reduce_sum(self, x):
        if self.world == 1:
            return x
        return self.all_gather(x[None]).reshape(self.world, *x.shape).sum(0)

    def shared_uniform(self, u):
        """The resampling uniform of this event, identical on every rank (the reference draws it from each rank's CPU
        generator, utils.py:111-120, and relies on identically seeded ranks; the exchange below needs agreement)."""
        if u is None:
            u = torch.rand(size=(1,), dtype=torch.float64)
        return self.broadcast_host(torch.as_tensor(u, dtype=torch.float64).reshape(-1)[:1].clone())

    def broadcast_host(self, t):
        """Rank 0's host tensor ``t`` on every rank: an event's uniform, or all those of a run with ``populations`` at once."""
        if self.world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
            if torch.distributed.get_backend() == "nccl":
                td = t.cuda()
                torch.distributed.broadcast(td, 0)
                t = td.cpu()
            else:
                torch.distributed.broadcast(t, 0)
        return t

    def exchange_rows(self, x, ids, Bl):
        """Rows ``ids[rank*Bl:(rank+1)*Bl]`` of the batch whose shards are the ranks' ``x`` [Bl, D]; ``ids`` [world*Bl]
        are the parents of a global systematic resampling: identical on every rank, non-decreasing up to the cyclic
        rotation by the event's uniform (utils.py:111-120: ``(u + i / bs) % 1``).  Instead of
        all-gathering every walker to every rank (the reference, sde_integration.py:248-258), each rank sends a
        destination only the DISTINCT parents it holds that the destination needs (one RCCL all_to_all_single with
        uneven splits); repeated parents are expanded locally."""
        W, r = self.world, self.rank
        if W == 1:
            return gather_rows(x, ids)
        if Bl == 0:  # fewer walkers than ranks: every shard is empty (sde_integration.py:227)
            return x
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            return gather_rows(self.all_gather(x), ids)[r * Bl:(r + 1) * Bl].clone()  # Lightning's all_gather only
        n = W * Bl
        first = torch.ones(n, dtype=torch.bool, device=ids.device)
        first[1:] = ids[1:] != ids[:-1]
        first[::Bl] = True  # a destination's first walker always needs its parent
        src = torch.div(ids, Bl, rounding_mode="floor")
        dest = torch.div(torch.arange(n, device=ids.device), Bl, rounding_mode="floor")
        counts = torch.bincount((dest * W + src)[first], minlength=W * W).reshape(W, W).tolist()  # [dest][src]
        send = x[ids[first & (src == r)] - r * Bl].contiguous()  # grouped by destination, ascending
        recv = torch.empty((sum(counts[r]), x.shape[1]), device=x.device, dtype=x.dtype)
        in_split, out_split = [counts[d][r] for d in range(W)], counts[r]
        if torch.distributed.get_backend() != "nccl" and x.is_cuda:  # gloo rehearsal: through the host
            rc = torch.empty(recv.shape, dtype=x.dtype)
            torch.distributed.all_to_all_single(rc, send.cpu(), output_split_sizes=out_split, input_split_sizes=in_split)
            recv = rc.to(x.device)
        else:
            torch.distributed.all_to_all_single(recv, send, output_split_sizes=out_split, input_split_sizes=in_split)
        self.rows_received = getattr(self, "rows_received", 0) + sum(counts[r]) - counts[r][r]
        # what this rank put on the wire (rows to other ranks; the split it kept for itself never leaves the device)
        self.rows_sent = getattr(self, "rows_sent", 0) + sum(in_split) - in_split[r]
        self.last_splits = {"sent_to": in_split, "received_from": out_split}
        # the received rows are ordered by (source rank, position in my slice); my slice's runs are ordered by position
        fl = first[r * Bl:(r + 1) * Bl]
        jl = torch.nonzero(fl).reshape(-1)
        order = torch.argsort(src[r * Bl:(r + 1) * Bl][jl] * Bl + jl)
        pos = torch.empty_like(order)
        pos[order] = torch.arange(order.numel(), device=order.device)
        return recv[pos[torch.cumsum(fl.to(torch.int64), 0) - 1]]


def _count_distinct(ids):
    """Number of distinct parents of a systematic resampling, as a 0-dim DEVICE tensor (no host synchronisation).  The
    ids are non-decreasing up to the cyclic rotation by the event's uniform (utils.py:111-120), so every distinct parent
    is one cyclic run: distinct = max(1, number of positions whose cyclic predecessor differs).  The reference takes
    ``len(np.unique(choice))`` on the host every step (sde_integration.py:295)."""
    if ids.is_cuda:  # one launch (pita_count_runs) instead of roll + != + cast + sum + clamp
        ids = ids.contiguous()
        out = torch.empty((), device=ids.device, dtype=torch.int64)
        _lib.check(_lib.lib().pita_count_runs(ids.data_ptr(), ids.numel(), out.data_ptr(), _lib.stream_ptr(ids.device)),
                   "pita_count_runs")
        return out
    return (ids != torch.roll(ids, 1)).sum().clamp_min(1)  # host tensors: the gloo / dry-run paths


def _host_counts(counts):
    """The list ``num_unique_idxs`` of the reference (python ints): one transfer for all the events of a run."""
    dev = [(k, c) for k, c in enumerate(counts) if isinstance(c, torch.Tensor)]
    if dev:
        vals = torch.stack([c for _, c in dev]).tolist()
        for (k, _), v in zip(dev, vals):
            counts[k] = int(v)
    return counts


def population_layout(Bg, world, populations, batch_size, max_size=MAX_POPULATION_SIZE):
    """``(S, populations per rank, clamp chunk)`` of a run of ``Bg`` walkers in ``populations`` independent populations
    over ``world`` ranks: S = Bg / populations walkers each, whole populations per rank, and the 0.9-quantile clamp of the
    debiased drift over chunks of ``min(batch_size or S, S)`` walkers, which must tile a population.  ValueError where
    the walkers do not split evenly, a population exceeds ``max_size`` (by default what one block resamples, 2 048; None:
    no limit, the integrator's own call -- larger populations take the multi-block event), populations would straddle
    ranks or the clamp chunks would straddle populations."""
    Bg, world, P = int(Bg), int(world), int(populations)
    if P < 1:
        raise ValueError(f"populations must be at least 1, got {P}")
    if Bg < P or Bg % P != 0:
        raise ValueError(f"{Bg} walkers do not split into {P} populations of equal size")
    S = Bg // P
    if max_size is not None and S > max_size:
        raise ValueError(f"a population of {S} walkers exceeds the limit of {max_size} (one block per population)")
    if P % world != 0:
        raise ValueError(f"{P} populations do not split over {world} ranks: populations never straddle ranks")
    chunk = S if not batch_size else min(int(batch_size), S)
    if S % chunk != 0:
        raise ValueError(f"batch_size {batch_size} does not tile a population of {S} walkers (clamp chunks)")
    return S, P // world, chunk


class _Events:
    """What the two resampling policies of a run share: the log of its events, preallocated on the device with one
    column per population -- the kernel of step s writes row s, the host reads everything once after the loop -- and the
    diagnostics made of it.  ``P`` populations of ``S`` walkers; ``theta``: the ESS threshold, None for the fixed
    schedule; ``zero_a`` (debiased regime): the shard's zero log-weights, never written to."""

    keep_order = False  # after MALA the set-aside walkers go behind the valid ones (quirk Q7)
    synthetic = ()  # due steps settled on the host because the weights are identically zero: ESS = S, mean weight 1

    def _alloc_log(self, rows, cols, device):
        self.stats = torch.full((rows, cols, 6), float("nan"), dtype=torch.float64, device=device)
        self.flags = torch.zeros((rows, cols), dtype=torch.int32, device=device)
        self.counts = torch.full((rows, cols), self.S, dtype=torch.int64, device=device)

    def row(self, step):
        return self.flags[step], self.stats[step], self.counts[step]

    def collect(self, a):  # the row of the run's log-weights that a step's `a` makes
        return a

    def gather(self, rows):  # collected rows -> rows over the global batch
        return rows

    def _weight_stats(self, st, resampled, final_logweights):
        """Per-event arrays [N, P] and ``log_z`` [P] from the log's host copy (``st`` [N, P, 6], ``resampled`` [N, P]) and
        the last row of the run's log-weights (device)."""
        for s in self.synthetic:
            st[s, :, 1], st[s, :, 2], st[s, :, 3] = 0.0, float(self.S), 1.0
            resampled[s] = self.theta >= 1.0
        tail = logweight_stats(final_logweights.reshape(self.P, -1))["log_mean_weight"]
        lmw = st[:, :, 1]
        log_z = np.array([lmw[resampled[:, p], p].sum() for p in range(self.P)], np.float64) + tail
        return {"ess": st[:, :, 2].copy(), "ess_fraction": st[:, :, 3].copy(), "log_mean_weight": lmw.copy(),
                "resampled": resampled, "log_z": log_z}


class _GlobalEvents(_Events):
    """One population over all ranks, like the reference's: an event all-gathers the log-weights, every rank resamples
    them alike with rank 0's uniform, the walkers move in ``_Comm.exchange_rows``.  With a threshold the event is decided
    on the device (no host read) and its uniform is drawn whether or not it resamples (the fixed schedule's stream)."""

    def __init__(self, comm, Bg, Bl, N, theta, resample_u, device, weighted, clamp_chunk):
        self.comm, self.Bg, self.Bl, self.N, self.theta, self.clamp_chunk = comm, Bg, Bl, N, theta, clamp_chunk
        self.P, self.S = 1, comm.world * Bl
        self.u_iter = iter(resample_u) if resample_u is not None else None
        self.n_unique = {}  # step -> distinct parents of its event, 0-dim device tensors (row N: the end-of-run event)
        self.zero_a = torch.zeros(Bl, device=device) if weighted else None
        self.stats = None  # zero weights have no log: their diagnostics are known on the host
        if weighted and theta is not None:
            self._alloc_log(N, 1, device)

    def _uniform(self):
        return self.comm.shared_uniform(next(self.u_iter) if self.u_iter is not None else None)

    def skip_zero_weight_events(self, due):
        """The due events that still run on the device when the log-weights are identically zero: ESS = batch, so below
        a threshold of 1 none resamples -- no kernel, but the uniforms are drawn as the fixed schedule would draw them."""
        if self.theta is not None:
            self.synthetic = due
            if self.theta < 1.0:
                for _ in due:
                    self._uniform()
                return []
        return due

    def event(self, x, a, step):
        """``(x, a)`` after the event of ``step``; ``a`` None: log-weights identically zero (nothing to gather)."""
        ag = torch.zeros(self.S, device=x.device) if a is None else self.comm.all_gather(a)
        u = self._uniform()
        if self.stats is None:
            ids, _ = sample_cat_sys(ag.shape[0], ag, u)
            self.n_unique[step] = _count_distinct(ids)
            return self.comm.exchange_rows(x, ids, self.Bl), self.zero_a
        ids, resampled, _, self.n_unique[step] = sample_cat_sys_adaptive(ag.shape[0], ag, self.theta, u,
                                                                         out=tuple(t[0] for t in self.row(step)))
        x = self.comm.exchange_rows(x, ids, self.Bl)  # identity ids move nothing
        return x, torch.where(resampled != 0, self.zero_a, a)

    def end_event(self, x, a_next):
        """Always resamples, on ``a_next`` clamped at the 0.9 quantile of the gathered vector: ``(x, global a_next)``."""
        a_next = _quantile_clamp(self.comm.all_gather(a_next.contiguous()), 0.9)
        ids, _ = sample_cat_sys(a_next.shape[0], a_next, self._uniform())
        x = self.comm.exchange_rows(x, ids, self.Bl)
        self.n_unique[self.N] = _count_distinct(ids)
        return x, a_next

    def collect(self, a):
        return self.comm.all_gather(a)  # at every step

    def finish(self, final_logweights, n_rows):
        """``(last_weight_stats, counts)``: None under the fixed schedule, per-event arrays [N] otherwise; the counts of
        rows without an event are the batch, the others still device scalars (``_host_counts`` reads them at once)."""
        counts = [self.n_unique.get(s, self.Bg) for s in range(n_rows)]
        if self.theta is None:
            return None, counts
        if self.stats is None:
            st, resampled = np.full((self.N, 1, 6), np.nan), np.zeros((self.N, 1), dtype=bool)
        else:
            st, resampled = self.stats.cpu().numpy(), self.flags.cpu().numpy() != 0
        stats = self._weight_stats(st, resampled, final_logweights)
        return {k: float(v[0]) if k == "log_z" else v[:, 0] for k, v in stats.items()}, counts


class _PopulationEvents(_Events):
    """``populations=P``: the layout, this rank's columns of the run's uniforms [events, P] on the device (drawn or taken
    once, rank 0's on every rank) and the log, with one more row for ``resample_at_end``.  Every event is rank-local: one
    pita_population_resample launch (S <= 2 048) or the fixed launches of pita_population_resample_blocks (larger S) and
    the row gather; log-weights and log are gathered once, after the loop."""

    keep_order = True  # set-aside walkers return to their own rows: row r stays in population r // S

    def __init__(self, comm, Bg, P, batch_size, N, n_events, theta, resample_u, device, weighted):
        self.comm, self.P, self.N, self.theta = comm, P, N, theta
        self.S, self.Pl, self.clamp_chunk = population_layout(Bg, comm.world, P, batch_size, max_size=None)
        self.one_launch = self.S <= MAX_POPULATION_SIZE
        if resample_u is None:
            u = torch.rand((n_events, P), dtype=torch.float64)
        else:
            u = torch.as_tensor(resample_u, dtype=torch.float64).detach().cpu().clone()
            if tuple(u.shape) != (n_events, P):
                raise ValueError(f"resample_u has shape {tuple(u.shape)}, expected (events, populations) = {(n_events, P)}")
            if not bool(((u >= 0.0) & (u < 1.0)).all()):
                raise ValueError("resample_u must lie in [0, 1)")
        u = comm.broadcast_host(u)
        lo = comm.rank * self.Pl
        self.u = u[:, lo:lo + self.Pl].contiguous().to(device)
        self._alloc_log(N + 1, self.Pl, device)
        self.next_event = 0
        self.zero_a = torch.zeros(self.Pl * self.S, device=device) if weighted else None

    def skip_zero_weight_events(self, due):
        """As ``_GlobalEvents``'s; a run's uniforms are drawn up front, so skipping an event only moves the cursor."""
        if self.theta is None or self.theta >= 1.0:
            return due
        self.synthetic = due
        self.next_event += len(due)
        return []

    def _launch(self, x, a, theta, row):
        u = self.u[self.next_event]
        self.next_event += 1
        resample = sample_cat_sys_populations if self.one_launch else sample_cat_sys_population_blocks
        ids, _, _, _, a_next = resample(a, self.Pl, theta, u, out=self.row(row))
        return gather_rows(x, ids), a_next

    def event(self, x, a, step):
        """``(x, a)`` after the event of ``step`` on this rank's populations; ``a`` None: identically zero."""
        if a is None:
            a = torch.zeros(self.Pl * self.S, device=x.device)
        return self._launch(x, a, 1.0 if self.theta is None else self.theta, step)

    def end_event(self, x, a_next):
        """Every population resamples (row N of the log), on ``a_next`` clamped at its 0.9 quantile: ``(x, local a_next)``."""
        a_next = _quantile_clamp(a_next, 0.9, chunk=self.S)
        return self._launch(x, a_next, 1.0, self.N)[0], a_next

    def gather(self, rows):
        """[R, Bl, ...] of every rank -> [R, Bg, ...] in population order (one all-gather)."""
        comm = self.comm
        if comm.world == 1:
            return rows
        g = comm.all_gather(rows.contiguous()).reshape((comm.world,) + tuple(rows.shape))
        return g.transpose(0, 1).reshape((rows.shape[0], comm.world * rows.shape[1]) + tuple(rows.shape[2:]))

    def finish(self, final_logweights, n_rows):
        """``(last_weight_stats with arrays [N, P] and log_z [P], counts as python ints)``: one read of every rank's log."""
        packed = torch.cat([self.stats, self.flags[..., None].double(), self.counts[..., None].double()], dim=-1)
        h = self.gather(packed).cpu().numpy()  # [N + 1, P, 8]
        N = self.N
        stats = self._weight_stats(h[:N, :, :6].copy(), h[:N, :, 6] != 0, final_logweights)
        stats.update(n_unique=h[:N, :, 7].astype(np.int64), log_z=stats.pop("log_z"), populations=self.P)
        return stats, [int(c) for c in h[:n_rows, :, 7].sum(1)]


# What is fixed for one integrate_sde call: the rank's shard (walkers off .. off + Bl of Bg, n particles in d dimensions),
# the noise stream (Philox key, injected normals), the grid and its step table on the host and on the device, the target,
# the annealing schedule, beta, the resampling interval, the fused backbone (or None), the policy, the MALA parity hooks
_Run = collections.namedtuple("_Run", "comm off Bl Bg n d mean_free key noise times tab_h tab target schedule beta interval "
                                      "did_resampling model policy mala_draws")


def _pooled_rates(stats):
    """One acceptance rate per step from per-population ones: sum_p rate_p n_p / sum_p n_p in float64 over the
    populations with valid walkers (``acceptance_rate`` [steps, P], ``n_valid`` [P]); NaN where there is none."""
    nv = stats["n_valid"].astype(np.float64)
    has = nv > 0
    if not has.any():
        return [float("nan")] * stats["acceptance_rate"].shape[0]
    r = stats["acceptance_rate"].astype(np.float64)[:, has]
    return ((r * nv[has]).sum(1) / nv[has].sum()).tolist()


def _terms_from_stats(st4, st8, n_elem, n_walk, computed, debiased):
    """N light SDETerms from the per-step moment buffers (host copies happen once, here).  st4: [N, 4] drift_X /
    diffusion moments; st8: [N, 8] drift_A, divergence_score, cross_term, dUt_dt moments (debiased regime only)."""
    h4 = st4.cpu().tolist()
    h8 = st8.cpu().tolist() if st8 is not None else None
    out = []
    for k, r in enumerate(h4):
        ne, nw = (n_elem, n_walk) if computed[k] else (0, 0)
        t = SDETerms(drift_X=TermStats(r[0], r[1], ne), drift_A=TermStats(0.0, 0.0, nw),
                     diffusion=TermStats(r[2], r[3], ne))
        if debiased:
            q = h8[k]
            t.drift_A = TermStats(q[0], q[1], nw)
            t.divergence_score, t.cross_term, t.dUt_dt = (TermStats(q[2], q[3], nw), TermStats(q[4], q[5], nw),
                                                          TermStats(q[6], q[7], nw))
        out.append(t)
    return out


class WeightedSDEIntegrator:
    def __init__(self, sde, num_integration_steps, start_resampling_step, end_resampling_step, lightning_module=None,
                 partial_annealing_factor_schedule=None, reverse_time=True, diffusion_scale=1.0, time_range=1.0,
                 resampling_interval=-1, num_negative_time_steps=100, post_mcmc_steps=100, adaptive_mcmc=False,
                 batch_size=None, no_grad=True, resample_at_end=False, dt_negative_time=1e-4, do_langevin=False,
                 should_mean_free=True, seed=0, record_terms=False, verbose=False, ess_threshold=None,
                 populations=None, mcmc_per_population=False):
        """``ess_threshold``: None (the reference's fixed schedule: every due event resamples) or a fraction in [0, 1] --
        a due event then resamples only when the effective sample size of the log-weights is at most
        ``ess_threshold * batch``, decided on the device (``sample_cat_sys_adaptive``; an extension the reference does
        not have), and ``last_weight_stats`` holds the per-event diagnostics of the last run.

        ``populations``: None (one population: the whole batch, exactly the launches and bits of before) or P >= 1 -- the
        batch is P independent populations of S = batch / P walkers (any S), rows [p S, (p + 1) S) being population p
        from the first to the last step and in everything returned.  Each population has its own ESS, decision, uniform,
        systematic resampling, distinct-parent count, quantile clamp and ``log_z``; every event is one launch
        (``sample_cat_sys_populations``, S <= 2 048) or seven whatever P is (``sample_cat_sys_population_blocks``, larger
        S) plus the row gather on the rank's own walkers, with no collective, because populations never straddle ranks.  ``resample_u`` is then [events, P] (event-major, ``resample_at_end`` last),
        ``last_weight_stats`` is filled whatever ``ess_threshold`` is, its per-event arrays are [N, P] and ``log_z`` is
        [P].  The one coupling between populations is the post-processing MALA chain of ``adaptive_mcmc=True``: its one
        step size adapts to the acceptance rate over the whole batch -- unless ``mcmc_per_population`` is set.

        ``mcmc_per_population``: False (the chain as above) or True, which needs ``populations`` -- every population
        then has its own MALA step size, acceptance count and adaptation, so what a population returns depends on its own
        walkers alone, bit for bit.  The chain is rank-local (no all-reduce, the fused route whatever the world size).
        ``acceptance_rate_list`` stays one float per step: sum_p rate_p n_p / sum_p n_p in float64 over the populations
        with walkers (n_p: walkers of population p with a finite target log-density), and ``last_mcmc_stats`` holds
        ``acceptance_rate`` (float32 [steps, P], NaN for a population without such walkers), ``step_size`` (float64
        [P], final) and ``n_valid`` (int64 [P]) of the last run; it is None without the mode."""
        if populations is not None:
            if isinstance(populations, bool) or not isinstance(populations, (int, np.integer)) or populations < 1:
                raise ValueError(f"populations must be None or an int >= 1, got {populations!r}")
            populations = int(populations)
        self.populations = populations
        if not isinstance(mcmc_per_population, (bool, np.bool_)):
            raise ValueError(f"mcmc_per_population must be a bool, got {mcmc_per_population!r}")
        if mcmc_per_population and populations is None:
            raise ValueError("mcmc_per_population=True needs populations: without them there is one chain over the batch")
        self.mcmc_per_population = bool(mcmc_per_population)
        self.last_mcmc_stats = None
        if ess_threshold is not None:
            try:
                ok = 0.0 <= float(ess_threshold) <= 1.0  # NaN fails both comparisons
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"ess_threshold must be None or a fraction in [0, 1], got {ess_threshold!r}")
            ess_threshold = float(ess_threshold)
        self.ess_threshold = ess_threshold
        self.last_weight_stats = None
        self.sde = sde
        self.num_integration_steps = num_integration_steps
        self.start_resampling_step, self.end_resampling_step = start_resampling_step, end_resampling_step
        self.reverse_time = reverse_time
        self.diffusion_scale = diffusion_scale
        self.resampling_interval = resampling_interval
        self.time_range = time_range
        self.num_negative_time_steps = num_negative_time_steps
        self.post_mcmc_steps = post_mcmc_steps
        self.adaptive_mcmc = adaptive_mcmc
        self.dt_negative_time = dt_negative_time
        self.batch_size = batch_size
        self.no_grad = no_grad
        self.resample_at_end = resample_at_end
        self.do_langevin = do_langevin
        self.lightning_module = lightning_module
        self.should_mean_free = should_mean_free
        self.start_time = time_range if reverse_time else 0.0
        self.end_time = time_range - self.start_time
        self.seed = seed
        self.record_terms = record_terms
        self.verbose = verbose
        self._runs = 0

    # ------------------------------------------------------------------ helpers
    def maybe_remove_mean(self, x, energy_function):
        if self.should_mean_free:
            return remove_mean(x, energy_function.n_particles, energy_function.n_spatial_dim)
        return x

    def _geometry(self, x, energy_function):
        n = getattr(energy_function, "n_particles", None)
        d = getattr(energy_function, "n_spatial_dim", None)
        if n is None or d is None:  # non-particle target (GMM): one "particle" of dimension D
            n, d = 1, x.shape[1]
        return int(n), int(d)

    def _backbone(self):
        sn = self.sde.score_net
        model = getattr(sn, "model", None)
        fused = model is not None and hasattr(model, "sampler_run") and not getattr(sn, "precondition_beta", False)
        return model if fused else None

    def _key(self, stream_id):
        """Philox seed of one of a run's independent streams: 0 the Euler-Maruyama noise, 1 and 2 the MALA chains,
        PROBE_STREAM_ID the Hutchinson probes of ``VEReverseSDE(divergence="hutchinson")``."""
        return (int(self.seed) * 0x9E3779B97F4A7C15 + (self._runs << 8) + stream_id) & 0xFFFFFFFFFFFFFFFF

    # ------------------------------------------------------------------ A1 integrate_sde
    @torch.no_grad()
    def integrate_sde(self, x1, energy_function, annealing_factor_schedule, inverse_temperature=1.0,
                      annealing_factor_score=1.0, resampling_interval=None, noise=None, resample_u=None,
                      mala_noise=None, mala_uniforms=None):
        """``noise``: optional [N, B, D] device normals (global batch); ``resample_u``: optional
        iterable of float64 uniforms, one per resampling event; ``mala_noise`` [steps, B, D] / ``mala_uniforms``
        [steps, B]: the proposal normals and accept uniforms of the post-processing MALA chain (parity hooks;
        single rank).  With ``populations=P`` the uniforms of a run are drawn once, before the loop, as
        ``torch.rand((events, P), dtype=float64)`` (rank 0's on every rank) and ``resample_u`` of that shape replaces
        them: one row per due event, then one for ``resample_at_end``."""
        if resampling_interval is None:
            resampling_interval = self.resampling_interval
        N = self.num_integration_steps
        x1 = _lib.dev_tensor(x1, "x1")
        dev = x1.device
        comm = _Comm(self.lightning_module)
        if comm.world > 1 and (mala_noise is not None or mala_uniforms is not None):
            # the hooks are shaped for ONE chain over the whole batch; refuse before the trajectory is integrated
            raise ValueError("mala_noise / mala_uniforms are single-rank parity hooks (world size is "
                             f"{comm.world}): every rank draws its own Philox stream instead")
        Bg = x1.shape[0]
        Bl = Bg // comm.world  # sde_integration.py:227
        off = comm.rank * Bl
        x = x1[off:off + Bl].clone()
        n, d = self._geometry(x, energy_function)
        mean_free = bool(self.should_mean_free)
        batch_size = self.batch_size  # as given: population_layout tells None from a number
        if self.batch_size is None:
            self.batch_size = Bg

        times = torch.linspace(self.start_time, self.end_time, N + 1)[:-1]
        dt = self.time_range / N
        tab_h = build_step_table(self.sde.noise_schedule, annealing_factor_schedule, times, dt, self.diffusion_scale,
                                 inverse_temperature)
        tab = tab_h.to(dev)
        if noise is not None:
            if tuple(noise.shape) != (N, Bg, x1.shape[1]):
                raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {(N, Bg, x1.shape[1])}")
            noise = _lib.dev_tensor(noise, "noise")[:, off:off + Bl].contiguous()
        key = self._key(0)
        self._runs += 1

        start = max(0, min(self.start_resampling_step, N))  # before `start` walkers do not move (:278-280)
        if start > 0 and mean_free:
            x = remove_mean(x, n, d)  # :148 is applied every step; idempotent
        did_resampling = resampling_interval != -1 and resampling_interval < N
        events = [] if resampling_interval == -1 else [
            s for s in range(start, min(self.end_resampling_step, N)) if (s + 1) % resampling_interval == 0]
        sde_terms_all = []
        st4 = None if self.record_terms else torch.zeros(N, 4, dtype=torch.float64, device=dev)
        debiased = bool(getattr(self.sde, "debias_inference", False))
        if self.populations is None:
            policy = _GlobalEvents(comm, Bg, Bl, N, self.ess_threshold, resample_u, dev, debiased, self.batch_size or Bl)
        else:
            n_events = len(events) + int(self.resample_at_end and did_resampling)
            policy = _PopulationEvents(comm, Bg, self.populations, batch_size, N, n_events, self.ess_threshold,
                                       resample_u, dev, debiased)
        run = _Run(comm, off, Bl, Bg, n, d, mean_free, key, noise, times, tab_h, tab, energy_function,
                   annealing_factor_schedule, inverse_temperature, resampling_interval, did_resampling, self._backbone(),
                   policy, (mala_noise, mala_uniforms))
        if debiased:
            x, a, logweights, sde_terms_all = self._integrate_debiased(run, x)
        else:
            a = None  # the log-weights are identically zero (drift_A = 0)
            events = policy.skip_zero_weight_events(events)
            s = start
            for stop in events + [N - 1]:  # run steps s..stop inclusive, then (maybe) resample
                if stop < s:
                    continue
                self._run_steps(run, x, s, stop + 1, sde_terms_all, st4)
                s = stop + 1
                if stop in events:
                    x, _ = policy.event(x, None, stop)
                    if mean_free:
                        x = remove_mean(x, n, d)
            # a stride-0 view avoids N*B*4 bytes (reference stacks N copies)
            logweights = torch.zeros(1, Bg, device=dev).expand(N, Bg)
            if st4 is not None:
                # moments come from the world * Bl walkers that are integrated (Bg % world walkers are dropped, :227)
                sde_terms_all = _terms_from_stats(comm.all_reduce_sum(st4), None, comm.world * Bl * x1.shape[1],
                                                  comm.world * Bl, [k >= start for k in range(N)], False)
        x, logweights, counts = self._finish_weights(run, x, a, logweights)
        x, acceptance_rate_list = self._post_process(run, x)
        return x, logweights, _host_counts(counts), sde_terms_all, acceptance_rate_list

    def _finish_weights(self, run, x, a, logweights):
        """After the trajectory: the end-of-run reweighting when asked for, its row appended, the policy's ``finish``.
        ``logweights``: rows as the policy collected them, or (``a`` None) identically zero over the global batch."""
        policy = run.policy
        if self.resample_at_end and run.did_resampling:
            x, a_next = self._resample_at_end(run, x, a)
            logweights = torch.cat([logweights, policy.gather(a_next[None]) if a is None else a_next[None]])
        if a is not None:
            logweights = policy.gather(logweights)
        self.last_weight_stats, counts = policy.finish(logweights[-1], len(logweights))
        return x, logweights, counts

    def _post_process(self, run, x):
        """Negative-time descent, the MALA chain and the all-gather of the final shards: ``(x, acceptance rates)``."""
        if self.num_negative_time_steps > 0:
            x = self.negative_time_descent(x, run.target, walker_offset=run.off)
        keep_order = run.policy.keep_order
        acceptance_rate_list = []
        self.last_mcmc_stats = None
        if self.post_mcmc_steps > 0:
            fn = self.metropolis_hastings_mala_adaptive if self.adaptive_mcmc else self.metropolis_hastings_mala
            kw = dict(dt_init=self.dt_negative_time) if self.adaptive_mcmc else {}
            if self.mcmc_per_population:
                # the rates come from every rank's populations: one gather after the chain, then the pooled rate per step
                x, _ = fn(x, run.target, walker_offset=run.off, noise=run.mala_draws[0], uniforms=run.mala_draws[1],
                          keep_order=keep_order, pop_size=run.policy.S, **kw)
                self.last_mcmc_stats = self._gather_mcmc_stats(run.policy)
                acceptance_rate_list = _pooled_rates(self.last_mcmc_stats)
            else:
                x, acceptance_rate_list = fn(x, run.target, return_acceptance_rate=True, walker_offset=run.off,
                                             comm=run.comm, noise=run.mala_draws[0], uniforms=run.mala_draws[1],
                                             keep_order=keep_order, **kw)
        # X1: the only collective on the resampling-free path
        return self._gather_final(x, run.comm, run.Bl, keep_order), acceptance_rate_list

    # ------------------------------------------------------------------ debiased regime (per step; section 8(f) N1)
    def _integrate_debiased(self, run, x):
        """Feynman-Kac weighted integration (sde_integration.py:131-152,214-297 with sdes.py:151-239): per step the
        drift of x and of the log-weights a per inference chunk, Euler-Maruyama update, window gates, the policy's event
        when due.  Returns ``(x, a, log-weight rows as the policy collects them, sde_terms_all)``."""
        N = self.num_integration_steps
        dev = x.device
        L = _lib.lib()
        comm, policy, Bl, n, d, off, key, noise = run.comm, run.policy, run.Bl, run.n, run.d, run.off, run.key, run.noise
        a = zero_a = policy.zero_a
        logweights, sde_terms_all = [], []
        st4, st8 = (None, None) if self.record_terms else (torch.zeros(N, 4, dtype=torch.float64, device=dev),
                                                            torch.zeros(N, 8, dtype=torch.float64, device=dev))
        st = _lib.stream_ptr(dev)
        # this run's _key(PROBE_STREAM_ID): `key` is its _key(0)
        probe_seed = (key + PROBE_STREAM_ID) & 0xFFFFFFFFFFFFFFFF
        for step in range(N):
            t = run.times[step]  # host scalar: the schedules' scalars (gamma, dgamma/dt) are then read without a device sync
            row = run.tab_h[step]
            if step < self.start_resampling_step:  # walkers frozen, weights zero (:278-280)
                a = zero_a
                logweights.append(policy.collect(a))
                continue
            # one set of launches for the rank's whole shard; the quantile clamp keeps its per-chunk meaning
            kw = {}
            if getattr(self.sde, "divergence", "exact") == "hutchinson":
                # keyed like the noise -- by run, GLOBAL walker index and step --: bitwise repeatable, independent of the
                # number of ranks, and the two copies of a resampled parent draw different probes
                kw["probe_key"] = (probe_seed, off, step)
            terms = self.sde.f(t, x, run.beta, run.schedule, None, run.target, run.interval,
                               clamp_chunk=policy.clamp_chunk, **kw)
            drift = terms.drift_X.contiguous()
            nz = noise[step].contiguous() if noise is not None else None
            _lib.check(L.pita_em_step(x.data_ptr(), drift.data_ptr(), _lib.ptr(nz), Bl, n, d, float(row[_lib.ST_DT]),
                                      float(row[_lib.ST_NOISE_SCALE]), float(row[_lib.ST_SQRT_DT]), key, off, step, 0,
                                      _lib.ptr(st4[step]) if st4 is not None else 0, st), "pita_em_step")
            if st8 is not None:
                vs = [None if v is None else _lib.dev_tensor(v, "SDETerms field").contiguous()
                      for v in (terms.drift_A, terms.divergence_score, terms.cross_term, terms.dUt_dt)]
                for v in vs:  # the kernel reads Bl entries of each field
                    if v is not None and v.numel() != Bl:
                        raise ValueError(f"SDETerms field has {v.numel()} entries, expected one per walker ({Bl})")
                _lib.check(L.pita_moments4(*(_lib.ptr(v) for v in vs), Bl, st8[step].data_ptr(), st), "pita_moments4")
            a = torch.add(a, terms.drift_A, alpha=float(row[_lib.ST_DT]))  # a + drift_A dt in one launch
            if step >= self.end_resampling_step:
                a = zero_a
            if not (run.interval == -1 or (step + 1) % run.interval != 0 or step >= self.end_resampling_step):
                x, a = policy.event(x, a, step)
            if run.mean_free:
                x = remove_mean(x, n, d)
            logweights.append(policy.collect(a))
            if self.record_terms:
                sde_terms_all.append(terms)
        logweights = torch.stack(logweights)
        if st4 is not None:
            sde_terms_all = _terms_from_stats(comm.all_reduce_sum(st4), comm.all_reduce_sum(st8),
                                              comm.world * Bl * x.shape[1], comm.world * Bl,
                                              [k >= self.start_resampling_step for k in range(N)], True)
        return x, a, logweights, sde_terms_all

    def _gather_final(self, x, comm, Bl, keep_order=False):
        """All-gather of the final shards.  After MALA every shard is [its valid walkers, its set-aside walkers]; the
        reference runs the chain on the gathered batch and therefore returns [all valid, all set-aside] (quirk Q7):
        reorder to that when any rank set walkers aside.  ``keep_order`` (a run with ``populations``): the chain put the
        set-aside walkers back in their places, row r stays in population r // S."""
        xg = comm.all_gather(x)
        if comm.world == 1 or self.post_mcmc_steps <= 0 or keep_order:
            return xg
        nv = comm.all_gather(torch.tensor([getattr(self, "_last_mala_valid", Bl)], device=x.device, dtype=torch.int64)).tolist()
        if min(nv) == Bl:
            return xg
        head = [torch.arange(r * Bl, r * Bl + nv[r]) for r in range(comm.world)]
        tail = [torch.arange(r * Bl + nv[r], (r + 1) * Bl) for r in range(comm.world)]
        return xg[torch.cat(head + tail).to(xg.device)]

    def _resample_at_end(self, run, x, a):
        """End-of-trajectory reweighting (sde_integration.py:158-183): a_next = log p_target(x) + gamma E_theta(h(t_end), x)
        (+ the running log-weights a), then the policy's ``end_event``: (this rank's resampled walkers, its row a_next)."""
        t_end = run.times[min(self.end_resampling_step, self.num_integration_steps - 1)]
        # every rank evaluates its own shard (the reference evaluates the gathered batch on every rank); only the
        # log-weights are gathered, the walkers move in the exchange
        tb = torch.full((x.shape[0],), float(t_end), device=x.device)
        model_energy = self.sde.energy_net.forward_energy(self.sde.noise_schedule.h(tb), x, run.beta,
                                                          pin=bool(getattr(self.sde, "pin_energy", False)),
                                                          energy_function=run.target, t=tb)  # :166-173
        a_next = run.target(x) + model_energy * _scalar(run.schedule.gamma(t_end))
        if a is not None:
            a_next = a_next + a
        return run.policy.end_event(x, a_next)

    # ------------------------------------------------------------------ A2-A4 steps [s0, s1)
    def _run_steps(self, run, x, s0, s1, sde_terms_all, st4=None):
        if s1 <= s0:
            return
        model, noise, key, off, n, d, mean_free = run.model, run.noise, run.key, run.off, run.n, run.d, run.mean_free
        if model is not None and not self.record_terms and (not hasattr(model, "can_fuse") or model.can_fuse(n, d)):
            nz = noise[s0:s1].contiguous() if noise is not None else None
            model.sampler_run(x, run.tab[s0:s1].contiguous(), s1 - s0, noise=nz, seed=key, walker_offset=off, step0=s0,
                              remove_mean=mean_free, n_particles=n, n_dim=d,
                              stats_out=st4[s0:s1] if st4 is not None else None)
            return
        # per-step path: any backbone with forward(t, x, beta); drift through ScoreNet, update by pita_em_step
        L = _lib.lib()
        for k in range(s0, s1):
            row = run.tab_h[k]
            ht = torch.full((x.shape[0],), float(row[_lib.ST_H]), device=x.device)
            score = self.sde.score_net(ht, x, run.beta)
            drift = float(row[_lib.ST_GAMMA]) * (score * float(row[_lib.ST_G2]))
            drift = drift.contiguous()
            nz = noise[k].contiguous() if noise is not None else None
            _lib.check(L.pita_em_step(x.data_ptr(), drift.data_ptr(), _lib.ptr(nz), x.shape[0], n, d,
                                      float(row[_lib.ST_DT]), float(row[_lib.ST_NOISE_SCALE]),
                                      float(row[_lib.ST_SQRT_DT]), key, off, k, int(mean_free),
                                      _lib.ptr(st4[k]) if st4 is not None else 0, _lib.stream_ptr(x.device)),
                       "pita_em_step")
            if self.record_terms:
                sde_terms_all.append(SDETerms(drift_X=drift, drift_A=torch.zeros(x.shape[0], device=x.device)))

    # ------------------------------------------------------------------ A16 post-processing
    def negative_time_descent(self, x, energy_function, noise=None, walker_offset=0, fused=True):
        """x += F*dt (+ sqrt(2 dt) xi), remove_mean, repeated (sde_integration.py:353-360).  Pair targets run all
        steps in one launch (pita_lj_descent / pita_dw_descent, bit-identical to the per-step path below)."""
        n, d = self._geometry(x, energy_function)
        dt = float(self.dt_negative_time)
        key = self._key(1)
        L = _lib.lib()
        x = _lib.dev_tensor(x, "x").clone()
        ns, sq = (1.0 if self.do_langevin else 0.0), math.sqrt(2 * dt)
        nsteps = int(self.num_negative_time_steps)
        if noise is not None:
            noise = _lib.dev_tensor(noise, "noise")
            if tuple(noise.shape) != (nsteps,) + tuple(x.shape):
                raise ValueError(f"descent noise has shape {tuple(noise.shape)}, expected {(nsteps,) + tuple(x.shape)}")
        if fused and hasattr(energy_function, "fused_descent") and energy_function.fused_descent(
                x, nsteps, dt, ns, sq, seed=key, walker_offset=walker_offset, step0=0,
                remove_mean=self.should_mean_free, noise=noise) is not None:
            return x
        for k in range(nsteps):
            _, F = energy_function(x, return_force=True)
            nz = noise[k].contiguous() if noise is not None else None
            _lib.check(L.pita_em_step(x.data_ptr(), F.data_ptr(), _lib.ptr(nz), x.shape[0], n, d, dt, ns, sq, key,
                                      walker_offset, k, int(self.should_mean_free), 0, _lib.stream_ptr(x.device)),
                       "pita_em_step")
        return x

    def _gather_mcmc_stats(self, policy):
        """``last_mcmc_stats`` from what the per-population chain left on this rank (``_mala_pop_state``): one gather in
        ``_PopulationEvents.gather``'s layout and one host copy."""
        rates, dt_dev, totals = self._mala_pop_state
        packed = torch.cat([rates.double(), dt_dev[None], totals[None].double()])  # [steps + 2, Pl]; float32 and counts are exact
        h = policy.gather(packed).cpu().numpy()
        return {"acceptance_rate": h[:-2].astype(np.float32), "step_size": h[-2].copy(), "n_valid": h[-1].astype(np.int64)}

    def _mala(self, x, energy_function, adaptive, dt, noise=None, uniforms=None, return_acceptance_rate=False,
              walker_offset=0, comm=None, fused=True, keep_order=False, pop_size=None):
        """MALA with the reference's finite-mask semantics (:362-470): non-finite-logp walkers are set aside and
        re-appended AFTER the valid ones (order not preserved, quirk Q7).  Proposal, accept/reject and the step-size
        adaptation run as HIP kernels with the step size on the device: no host synchronisation inside the chain (the
        acceptance rates are copied to the host afterwards, and only when the caller asks for them).
        With several ranks the acceptance count is all-reduced so the adaptation sees the global rate, as the
        reference (which runs the chain on the gathered batch on every rank) does.  ``keep_order`` (runs with
        ``populations``): the set-aside walkers go back to their own rows instead.
        ``pop_size`` (``mcmc_per_population``): the rows are populations of ``pop_size`` walkers, the first of them at
        Philox key ``walker_offset``, each with its own step size, count and adaptation (the ``_pop`` kernels on either
        route); the chain is rank-local, ``comm`` is not used.  Its per-population rates [steps, Pl], final step sizes
        [Pl] and valid-walker counts [Pl] stay on the device in ``_mala_pop_state``; the rate returned per step is the
        pooled one, sum_p rate_p n_p / sum_p n_p in float64 over the populations with valid walkers."""
        if pop_size is not None:
            return self._mala_populations(x, energy_function, adaptive, dt, int(pop_size), noise, uniforms,
                                          return_acceptance_rate, int(walker_offset), fused, keep_order)
        n, d = self._geometry(x, energy_function)
        L = _lib.lib()
        x, valid, x_valid, logp, ids = self._mala_split(x, energy_function, walker_offset)
        dev, Bv = x.device, x_valid.shape[0]
        total = Bv
        world = comm.world if comm is not None and torch.distributed.is_initialized() else 1
        if world > 1:
            tot = torch.tensor([Bv], device=dev, dtype=torch.int64)
            torch.distributed.all_reduce(tot)
            total = int(tot.item())
        steps = int(self.post_mcmc_steps)
        rates = torch.zeros(max(steps, 1), device=dev)
        done = 0
        if total > 0 and steps > 0:
            dt_dev = torch.tensor([dt], device=dev, dtype=torch.float64)
            count = torch.zeros(1, device=dev, dtype=torch.int32)
            x_prop = torch.empty_like(x_valid)
            key, rm = self._key(2), self._mala_centres(energy_function, adaptive)
            st = _lib.stream_ptr(dev)
            # targets with a fused chain kernel: walkers on chip, one launch for a non-adaptive chain, one per step for
            # an adaptive one (bit-identical to the loop below); the global acceptance rate of several ranks needs the
            # per-step all-reduce below
            if fused and world == 1 and Bv > 0 and hasattr(energy_function, "fused_mala"):
                nz, uu = self._mala_draws(noise, uniforms, steps, x_valid)
                if energy_function.fused_mala(x_valid, logp, steps, dt_dev, adaptive, total, noise=nz, uniforms=uu, seed=key,
                                              walker_offset=walker_offset, walker_ids=ids, step0=0, remove_mean=rm,
                                              rates_out=rates) is not None:
                    out = self._mala_join(x, valid, x_valid, keep_order)
                    return (out, rates[:steps].tolist()) if return_acceptance_rate else (out, None)
            for i in range(steps):
                if Bv > 0:
                    _, grad = energy_function(x_valid, return_force=True)
                    nz = _lib.dev_tensor(noise[i], "noise") if noise is not None else None
                    if nz is not None and tuple(nz.shape) != tuple(x_valid.shape):
                        raise ValueError(f"MALA noise[{i}] has shape {tuple(nz.shape)}, expected {tuple(x_valid.shape)} "
                                         "(one row per walker with a finite target log-density)")
                    _lib.check(L.pita_mala_propose(x_valid.data_ptr(), grad.data_ptr(), x_prop.data_ptr(), _lib.ptr(nz),
                                                   Bv, n, d, dt_dev.data_ptr(), key, walker_offset, _lib.ptr(ids), i, st),
                               "pita_mala_propose")
                    logp_prop, grad_prop = energy_function(x_prop, return_force=True)
                    uu = _lib.dev_tensor(uniforms[i], "uniforms") if uniforms is not None else None
                    if uu is not None and uu.numel() != Bv:
                        raise ValueError(f"MALA uniforms[{i}] has {uu.numel()} entries, expected {Bv}")
                    _lib.check(L.pita_mala_accept(x_valid.data_ptr(), logp.data_ptr(), grad.data_ptr(), x_prop.data_ptr(),
                                                  logp_prop.data_ptr(), grad_prop.data_ptr(), _lib.ptr(uu), Bv, n, d,
                                                  dt_dev.data_ptr(), key, walker_offset, _lib.ptr(ids), i, rm,
                                                  count.data_ptr(), st), "pita_mala_accept")
                if world > 1:
                    torch.distributed.all_reduce(count)
                _lib.check(L.pita_mala_adapt(dt_dev.data_ptr(), count.data_ptr(), total, int(adaptive),
                                             rates[i:].data_ptr(), st), "pita_mala_adapt")
                done += 1
        out = self._mala_join(x, valid, x_valid, keep_order)
        return (out, rates[:done].tolist()) if return_acceptance_rate else (out, None)

    # what the two chains share: the split into valid and set-aside walkers, the centring rule, the injected draws of a
    # fused chain, and the way back to one batch
    def _mala_split(self, x, energy_function, walker_offset):
        """``(x, valid, x_valid, logp, ids)``: the finite mask of the target log-density, the compacted walkers and their
        log-densities, and their Philox keys (None when no walker is set aside)."""
        x = _lib.dev_tensor(x, "x")
        logp_all = energy_function(x)
        valid = torch.isfinite(logp_all)
        x_valid = x[valid].contiguous()
        logp = logp_all[valid].contiguous()
        Bv = x_valid.shape[0]
        # Philox keys follow the walkers' ORIGINAL global indices, not their position in the compacted batch
        ids = (torch.nonzero(valid).reshape(-1) + int(walker_offset)).contiguous() if Bv < x.shape[0] else None
        self._last_mala_valid = Bv
        return x, valid, x_valid, logp, ids

    def _mala_centres(self, energy_function, adaptive):
        # :397-398 centres through maybe_remove_mean, the adaptive variant (:458-461) unconditionally
        return int(bool(getattr(energy_function, "is_molecule", False)) and (adaptive or bool(self.should_mean_free)))

    @staticmethod
    def _mala_draws(noise, uniforms, steps, x_valid):
        """Injected normals [steps, Bv, D] and uniforms [steps, Bv] of a whole chain, stacked and checked (None: Philox)."""
        nz = uu = None
        if noise is not None:
            nz = torch.stack([_lib.dev_tensor(noise[i], "noise") for i in range(steps)]).contiguous()
            if tuple(nz.shape) != (steps,) + tuple(x_valid.shape):
                raise ValueError(f"MALA noise has shape {tuple(nz.shape)}, expected {(steps,) + tuple(x_valid.shape)}")
        if uniforms is not None:
            uu = torch.stack([_lib.dev_tensor(uniforms[i], "uniforms").reshape(-1) for i in range(steps)]).contiguous()
            if tuple(uu.shape) != (steps, x_valid.shape[0]):
                raise ValueError(f"MALA uniforms have shape {tuple(uu.shape)}, expected {(steps, x_valid.shape[0])}")
        return nz, uu

    @staticmethod
    def _mala_join(x, valid, x_valid, keep_order):
        """The batch after the chain: [valid, set-aside] (quirk Q7), or every walker in its own row."""
        if not keep_order:
            return torch.cat([x_valid, x[~valid]], dim=0)
        out = x.clone()
        out[valid] = x_valid
        return out

    def _mala_populations(self, x, energy_function, adaptive, dt, S, noise, uniforms, return_acceptance_rate,
                          walker_offset, fused, keep_order):
        """``_mala`` with ``pop_size=S``: the same chain, step for step, with the per-population kernels."""
        n, d = self._geometry(x, energy_function)
        L = _lib.lib()
        if S < 1 or x.shape[0] % S != 0:
            raise ValueError(f"{x.shape[0]} walkers are no whole populations of {S}")
        Pl = x.shape[0] // S
        x, valid, x_valid, logp, ids = self._mala_split(x, energy_function, walker_offset)
        dev, Bv = x.device, x_valid.shape[0]
        totals = valid.reshape(Pl, S).sum(1)  # int64 [Pl], on the device: the bincount of the valid rows' populations
        steps = int(self.post_mcmc_steps)
        dt_dev = torch.full((Pl,), dt, device=dev, dtype=torch.float64)
        rates = torch.full((max(steps, 0), Pl), float("nan"), device=dev)  # what a population without walkers keeps
        if Bv > 0 and steps > 0:
            pops = MalaPopulations(S, walker_offset, totals)
            key, rm = self._key(2), self._mala_centres(energy_function, adaptive)
            st = _lib.stream_ptr(dev)
            nz, uu = self._mala_draws(noise, uniforms, steps, x_valid)
            if not (fused and hasattr(energy_function, "fused_mala") and energy_function.fused_mala(
                    x_valid, logp, steps, dt_dev, adaptive, pops, noise=nz, uniforms=uu, seed=key,
                    walker_offset=walker_offset, walker_ids=ids, step0=0, remove_mean=rm, rates_out=rates) is not None):
                count = torch.zeros(Pl, device=dev, dtype=torch.int32)
                x_prop = torch.empty_like(x_valid)
                for i in range(steps):
                    _, grad = energy_function(x_valid, return_force=True)
                    _lib.check(L.pita_mala_propose_pop(x_valid.data_ptr(), grad.data_ptr(), x_prop.data_ptr(),
                                                       _lib.ptr(nz[i] if nz is not None else None), Bv, n, d,
                                                       dt_dev.data_ptr(), Pl, S, walker_offset, key, walker_offset,
                                                       _lib.ptr(ids), i, st), "pita_mala_propose_pop")
                    logp_prop, grad_prop = energy_function(x_prop, return_force=True)
                    _lib.check(L.pita_mala_accept_pop(x_valid.data_ptr(), logp.data_ptr(), grad.data_ptr(), x_prop.data_ptr(),
                                                      logp_prop.data_ptr(), grad_prop.data_ptr(),
                                                      _lib.ptr(uu[i] if uu is not None else None), Bv, n, d,
                                                      dt_dev.data_ptr(), Pl, S, walker_offset, key, walker_offset,
                                                      _lib.ptr(ids), i, rm, count.data_ptr(), st), "pita_mala_accept_pop")
                    _lib.check(L.pita_mala_adapt_pop(dt_dev.data_ptr(), count.data_ptr(), totals.data_ptr(), Pl,
                                                     int(adaptive), rates[i].data_ptr(), st), "pita_mala_adapt_pop")
        self._mala_pop_state = (rates, dt_dev, totals)
        out = self._mala_join(x, valid, x_valid, keep_order)
        if not return_acceptance_rate:
            return out, None
        return out, _pooled_rates({"acceptance_rate": rates.cpu().numpy(), "n_valid": totals.cpu().numpy()})

    def metropolis_hastings_mala(self, x, energy_function, return_acceptance_rate=False, noise=None, uniforms=None,
                                 walker_offset=0, comm=None, fused=True, keep_order=False, pop_size=None):
        return self._mala(x, energy_function, False, float(self.dt_negative_time), noise, uniforms,
                          return_acceptance_rate, walker_offset, comm, fused, keep_order, pop_size)

    def metropolis_hastings_mala_adaptive(self, x, energy_function, dt_init, return_acceptance_rate=False, noise=None,
                                          uniforms=None, walker_offset=0, comm=None, fused=True, keep_order=False,
                                          pop_size=None):
        return self._mala(x, energy_function, True, float(dt_init), noise, uniforms, return_acceptance_rate,
                          walker_offset, comm, fused, keep_order, pop_size)
