"""Host side of the per-population MALA chain (no GPU): the constructor flag, the ``MalaPopulations`` record in
``HipTarget._mala_call`` against a stub library, the argument checks of every ``_pop`` entry point, which answer
PITA_EINVAL before any device call, and the new symbols in the header and in the binding's table."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pita_mala_pop_workspace_bytes", "pita_lj_mala_pop", "pita_dw_mala_pop", "pita_ff_mala_pop",
               "pita_mala_propose_pop", "pita_mala_accept_pop", "pita_mala_adapt_pop")


@pytest.fixture(scope="module")
def pa():
    from pita_amd import build as _b

    _b.build(verbose=False)
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def _integrator(pa, **kw):
    return pa.WeightedSDEIntegrator(sde=None, num_integration_steps=1, start_resampling_step=0, end_resampling_step=1, **kw)


def test_constructor_flag(pa):
    assert _integrator(pa).mcmc_per_population is False and _integrator(pa, populations=4).mcmc_per_population is False
    on = _integrator(pa, populations=4, mcmc_per_population=True)
    assert on.mcmc_per_population is True and on.last_mcmc_stats is None
    with pytest.raises(ValueError, match="populations"):
        _integrator(pa, mcmc_per_population=True)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="bool"):
            _integrator(pa, populations=4, mcmc_per_population=bad)


def test_pooled_rate_is_weighted_by_the_valid_walkers(pa):
    from pita_amd.sde_integration import _pooled_rates

    rates = np.array([[0.5, np.nan, 0.25], [1.0, np.nan, 0.0]], np.float32)
    assert _pooled_rates({"acceptance_rate": rates, "n_valid": np.array([10, 0, 30])}) == [(5.0 + 7.5) / 40, 10.0 / 40]
    out = _pooled_rates({"acceptance_rate": rates[:, 1:2], "n_valid": np.array([0])})
    assert len(out) == 2 and all(np.isnan(v) for v in out)


class _StubLib:
    """Records the calls ``_mala_call`` makes; every entry point answers ``rc``."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 8 * (args[0] * (args[1] if len(args) > 1 else 1) + 1) if name.endswith("workspace_bytes") else self.rc

        return call


@pytest.fixture
def stub(pa, monkeypatch):
    from pita_amd import _target

    L = _StubLib()
    monkeypatch.setattr(_target, "lib", lambda: L)
    monkeypatch.setattr(_target, "stream_ptr", lambda device: 77)
    monkeypatch.setattr(_target, "_device_guard", lambda device: contextlib.nullcontext())
    return L


def test_mala_call_takes_the_record_to_the_pop_symbol(pa, stub):
    """One body for both chains: with an int the call is the one of before, argument for argument; with the record the
    symbol gets ``_pop``, the workspace is sized by (steps, P), and (totals, P, size, base) stand where the count stood."""
    from pita_amd._target import POP_MALA_WORKSPACE, HipTarget, MalaPopulations

    t = HipTarget()
    x, logp, ids = torch.zeros(6, 8), torch.zeros(6), torch.arange(6)
    dt1, r1 = torch.zeros(1, dtype=torch.float64), torch.zeros(5)
    head = (4, 2, 1.0)
    assert t._mala_call("pita_dw_mala", "pita_lj_mala_workspace_bytes", x, logp, head, 5, dt1, True, 6, None, None, 2 ** 64 + 3,
                        12, ids, 0, True, r1) is x
    (ws_name, ws_args), (name, args) = stub.calls
    assert (ws_name, ws_args) == ("pita_lj_mala_workspace_bytes", (5,)) and name == "pita_dw_mala"
    assert args[:4] == (x.data_ptr(), logp.data_ptr(), 0, 0) and args[4:8] == (6,) + head
    assert args[8:11] == (5, dt1.data_ptr(), 1) and args[11] == 6
    tail = args[12:]
    assert tail[:6] == (3, 12, ids.data_ptr(), 0, 1, r1.data_ptr()) and tail[7] == 77 and len(tail) == 8
    stub.calls.clear()
    totals = torch.tensor([3, 0, 3], dtype=torch.int64)
    dt3, r3 = torch.zeros(3, dtype=torch.float64), torch.zeros(5, 3)
    pops = MalaPopulations(3, 12, totals)
    assert t._mala_call("pita_dw_mala", "pita_lj_mala_workspace_bytes", x, logp, head, 5, dt3, True, pops, None, None,
                        2 ** 64 + 3, 12, ids, 0, True, r3) is x
    (ws_name, ws_args), (name, args) = stub.calls
    assert (ws_name, ws_args) == (POP_MALA_WORKSPACE, (5, 3)) and name == "pita_dw_mala_pop"
    assert args[:11] == (x.data_ptr(), logp.data_ptr(), 0, 0, 6) + head + (5, dt3.data_ptr(), 1)
    assert args[11:15] == (totals.data_ptr(), 3, 3, 12) and args[15:] == tail[:5] + (r3.data_ptr(),) + args[-2:]
    assert args[-1] == 77 and len(args) == 23
    stub.rc = -2  # PITA_EUNSUPPORTED: "not mine" on either chain
    assert t._mala_call("pita_dw_mala", "pita_lj_mala_workspace_bytes", x, logp, head, 5, dt3, True, pops, None, None, 0, 12,
                        ids, 0, True, r3) is None


def test_mala_call_checks_the_shapes_of_a_population_chain(pa, stub):
    from pita_amd._target import HipTarget, MalaPopulations

    t = HipTarget()
    x, logp = torch.zeros(6, 8), torch.zeros(6)
    totals = torch.tensor([3, 3], dtype=torch.int64)
    good = dict(dt=torch.zeros(2, dtype=torch.float64), rates=torch.zeros(5, 2), pops=MalaPopulations(3, 0, totals))
    for key, bad in (("dt", torch.zeros(1, dtype=torch.float64)), ("dt", torch.zeros(2)), ("rates", torch.zeros(5)),
                     ("rates", torch.zeros(4, 2)), ("rates", torch.zeros(5, 3)), ("pops", MalaPopulations(0, 0, totals)),
                     ("pops", MalaPopulations(3, -1, totals)), ("pops", MalaPopulations(3, 0, totals.int())),
                     ("pops", MalaPopulations(3, 0, totals[:0]))):
        a = dict(good, **{key: bad})
        with pytest.raises(ValueError):
            t._mala_call("pita_lj_mala", "pita_lj_mala_workspace_bytes", x, logp, (), 5, a["dt"], True, a["pops"], None, None, 0,
                         0, None, 0, True, a["rates"])
    assert stub.calls == []  # refused before anything reached the library


def test_pop_workspace_bytes(pa):
    """One 64-bit counter per (step, population) and a spare word; no smaller than the one-step-size chain's at P = 1."""
    L = pa._lib.lib()
    for steps in (0, 1, 7, 100):
        for P in (1, 3, 32, 300):
            assert int(L.pita_mala_pop_workspace_bytes(steps, P)) >= 8 * (steps * P + 1)
        assert int(L.pita_mala_pop_workspace_bytes(steps, 1)) >= int(L.pita_lj_mala_workspace_bytes(steps))
    assert int(L.pita_mala_pop_workspace_bytes(-3, 4)) >= 8 and int(L.pita_mala_pop_workspace_bytes(4, -3)) >= 8


PTR = 4096  # a non-null, 8-byte aligned value that is never dereferenced: every call below fails a check first


def _chain_args(kind, **over):
    a = dict(handle=PTR, x=PTR, logp=PTR, B=4, n=13 if kind == "lj" else 4, d=3 if kind == "lj" else 2, steps=2, dt_dev=PTR,
             totals=PTR, n_pop=2, pop_size=2, workspace=PTR)
    a.update(over)
    head = {"lj": (a["n"], a["d"], 1.0, 1.0, 1e-6, 1.0, 1.0, 1.0), "dw": (a["n"], a["d"], 1.0, 0.9, -4.0, 0.0, 4.0), "ff": ()}[kind]
    lead = (a["handle"],) if kind == "ff" else ()
    return lead + (a["x"], a["logp"], None, None, a["B"]) + head + (a["steps"], a["dt_dev"], 1, a["totals"], a["n_pop"],
                                                                    a["pop_size"], 0, 0, 0, None, 0, 1, None, a["workspace"], None)


@pytest.mark.parametrize("kind", ("lj", "dw", "ff"))
def test_fused_pop_entry_points_check_their_arguments_first(pa, kind):
    L = pa._lib.lib()
    fn = getattr(L, f"pita_{kind}_mala_pop")
    bad = [dict(dt_dev=None), dict(totals=None), dict(workspace=None), dict(n_pop=0), dict(n_pop=-2), dict(pop_size=0),
           dict(workspace=PTR + 4), dict(B=-1), dict(steps=-1)]
    if kind == "ff":
        bad.append(dict(handle=None))
    for over in bad:
        assert fn(*_chain_args(kind, **over)) == -1, over
        assert f"pita_{kind}_mala_pop" in pa._lib.last_error(), over
    if kind != "ff":  # a geometry without a fused chain: "not mine", as the one-step-size entry points answer
        assert fn(*_chain_args(kind, n=7)) == pa._lib.PITA_EUNSUPPORTED


def test_per_kernel_pop_entry_points_check_their_arguments_first(pa):
    L = pa._lib.lib()

    def propose(B=4, dt_dev=PTR, n_pop=2, pop_size=2):
        return L.pita_mala_propose_pop(PTR, PTR, PTR, None, B, 13, 3, dt_dev, n_pop, pop_size, 0, 0, 0, None, 0, None)

    def accept(B=4, dt_dev=PTR, n_pop=2, pop_size=2, count=PTR):
        return L.pita_mala_accept_pop(PTR, PTR, PTR, PTR, PTR, PTR, None, B, 13, 3, dt_dev, n_pop, pop_size, 0, 0, 0, None, 0, 1,
                                      count, None)

    def adapt(dt_dev=PTR, count=PTR, totals=PTR, n_pop=2):
        return L.pita_mala_adapt_pop(dt_dev, count, totals, n_pop, 1, None, None)

    for fn, name, cases in ((propose, "pita_mala_propose_pop", (dict(B=-1), dict(dt_dev=None), dict(n_pop=0), dict(pop_size=0))),
                            (accept, "pita_mala_accept_pop", (dict(B=-1), dict(dt_dev=None), dict(n_pop=0), dict(pop_size=0),
                                                              dict(count=None))),
                            (adapt, "pita_mala_adapt_pop", (dict(dt_dev=None), dict(count=None), dict(totals=None),
                                                            dict(n_pop=0)))):
        for over in cases:
            assert fn(**over) == -1, (name, over)
            assert name in pa._lib.last_error(), (name, over)
    assert propose(B=0) == 0 and accept(B=0) == 0  # an empty batch launches nothing


def test_new_symbols_are_declared_and_bound(pa):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pita_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pita_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(pa._lib.EXPORTS)
    assert pa._lib.ABI_VERSION == 13  # additions only: the existing entry points keep their signatures
    from pita_amd import _target

    for cls in (pa.LennardJonesEnergy, pa.MultiDoubleWellEnergy):
        assert "_pop" not in open(os.path.join(ROOT, "pita_amd", cls.__module__.split(".")[-1] + ".py")).read()
    assert _target.MalaPopulations._fields == ("size", "base", "totals")
