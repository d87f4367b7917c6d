"""Host side of the ESS-triggered resampling events (no GPU): the five new entry points are declared, bound and exported
under the unchanged ABI version, ``WeightedSDEIntegrator(ess_threshold=...)`` validates its argument, and an event that
does not resample -- identity ids -- moves no walker between ranks (gloo, world 2), which is what several ranks rely on
when every one of them reaches the same decision on the gathered log-weights."""
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"pita_logweight_stats_workspace_bytes": 1, "pita_logweight_stats": 5, "pita_adaptive_resample_workspace_bytes": 1,
       "pita_adaptive_resample": 10, "pita_adaptive_resample_single_launch": 1}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pita_hip.h")).read(), flags=re.S)


def test_new_entry_points_declared_bound_and_abi_unchanged():
    from pita_amd import _lib
    from pita_amd import build as _b

    _b.build(verbose=False)
    hdr = _header()
    for name, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not declared in pita_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, (name, m.group(1))
        assert name in _lib.EXPORTS
        assert len(_lib._PROTOS[name][1]) == nargs, name
    assert re.search(r"#define\s+PITA_ABI_VERSION\s+13\b", hdr)
    assert _lib.ABI_VERSION == 13
    L = _lib.lib()  # binds every prototype: AttributeError on a missing symbol
    assert L.pita_abi_version() == 13
    # pure host functions of the new interface
    assert L.pita_adaptive_resample_single_launch(2048) == 1 and L.pita_adaptive_resample_single_launch(2049) == 0
    assert L.pita_adaptive_resample_workspace_bytes(70001) >= L.pita_resample_workspace_bytes(70001)
    assert L.pita_adaptive_resample_workspace_bytes(2048) >= 1


def _integrator(**kw):
    import pita_amd as pa

    return pa.WeightedSDEIntegrator(sde=None, num_integration_steps=4, start_resampling_step=0, end_resampling_step=4,
                                    resampling_interval=1, **kw)


@pytest.mark.parametrize("v", [-0.1, 1.5, float("nan")])
def test_ess_threshold_outside_unit_interval_is_refused(v):
    with pytest.raises(ValueError):
        _integrator(ess_threshold=v)


@pytest.mark.parametrize("v", [None, 0.0, 0.6, 1.0])
def test_ess_threshold_accepted(v):
    integ = _integrator(ess_threshold=v)
    assert integ.ess_threshold == v and integ.last_weight_stats is None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_exchange(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pita_amd.sde_integration import _Comm

        comm = _Comm(None)
        Bl, D = 64, 5
        n = world * Bl
        xg = torch.arange(n * D, dtype=torch.float32).reshape(n, D)
        x = xg[rank * Bl:(rank + 1) * Bl].clone()
        got = comm.exchange_rows(x, torch.arange(n), Bl)  # what an event that does not resample hands over
        assert torch.equal(got, x)
        assert comm.rows_received == 0 and comm.rows_sent == 0
        assert sum(comm.last_splits["sent_to"]) == comm.last_splits["sent_to"][rank]
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_identity_ids_move_no_rows_between_ranks():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_exchange, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(r, "ok") for r in range(world)], res
