"""Populations of any size without a GPU: pita_population_resample_blocks binds and refuses bad arguments before any
device call, ``population_layout(max_size=None)`` lifts the size limit and nothing else, and the shared inputs of the GPU
tests (tests/_populations.py at the sizes of tests/_population_blocks.py) keep their distance from the thresholds."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _population_blocks as PB
from tests import _populations as PP


@pytest.fixture(scope="module")
def built():
    from pita_amd import build as _b

    _b.build(verbose=False)
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pita_population_resample_blocks_workspace_bytes", "pita_population_resample_blocks")


def test_new_prototypes_bind_and_the_abi_version_stays(built):
    L = built._lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pita_hip.h")).read(), flags=re.S)
    for name, ret in zip(NAMES, ("size_t", "int")):
        assert name in built._lib.EXPORTS
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", hdr), f"{name} not declared in include/pita_hip.h"
    assert L.pita_abi_version() == 13 == built._lib.ABI_VERSION
    for P, S in ((1, 1), (3, 2049), (300, 5000)):
        nbytes = L.pita_population_resample_blocks_workspace_bytes(P, S)
        assert nbytes % 8 == 0 and nbytes >= P * L.pita_resample_workspace_bytes(S), (P, S)


def test_bad_arguments_come_back_as_error_codes_without_a_gpu(built):
    """Every check precedes the first HIP call: host buffers stand in for the device pointers and are never touched.
    There is no unsupported size: the only refusals are PITA_EINVAL."""
    L = built._lib.lib()
    P, S = 3, 2049
    buf = {k: ctypes.create_string_buffer(P * S * 8 + 64) for k in
           ("logits", "u", "ids", "nu", "stats", "flag", "next", "ws")}
    before = {k: v.raw for k, v in buf.items()}
    addr = {k: ctypes.addressof(v) for k, v in buf.items()}

    def call(n_pop=P, pop_size=S, theta=0.5, **ptr):
        a = dict(addr, **ptr)
        return L.pita_population_resample_blocks(a["logits"], n_pop, pop_size, a["u"], theta, a["ids"], a["nu"],
                                                 a["stats"], a["flag"], a["next"], a["ws"], None)

    for kw in (dict(logits=None), dict(u=None), dict(ids=None), dict(stats=None), dict(flag=None), dict(ws=None),
               dict(n_pop=0), dict(n_pop=-2), dict(n_pop=2 ** 31), dict(pop_size=0), dict(pop_size=-1), dict(theta=-0.1),
               dict(theta=1.5), dict(theta=float("nan")), dict(ws=addr["ws"] + 4)):
        assert call(**kw) == -1, kw  # PITA_EINVAL
        assert "pita_population_resample_blocks" in built._lib.last_error(), kw
    assert all(buf[k].raw == before[k] for k in buf)


def test_population_layout_without_a_size_limit():
    from pita_amd.sde_integration import population_layout

    assert population_layout(4098, 1, 2, None, max_size=None) == (2049, 2, 2049)
    assert population_layout(65536, 1, 1, None, max_size=None) == (65536, 1, 65536)
    assert population_layout(65536, 2, 4, 4096, max_size=None) == (16384, 2, 4096)
    assert population_layout(65536, 1, 32, None, max_size=None) == (2048, 32, 2048)  # and the answers of before
    assert population_layout(6000, 1, 2, None, max_size=3000) == (3000, 2, 3000)
    for Bg, world, P, bs in ((193, 1, 3, None),  # Bg % P
                             (2, 1, 3, None),  # fewer walkers than populations
                             (8194, 2, 3, None),  # populations would straddle ranks
                             (16384, 1, 4, 3000),  # 4 096 % 3 000
                             (8192, 1, 0, None), (8192, 1, -1, None)):
        with pytest.raises(ValueError):
            population_layout(Bg, world, P, bs, max_size=None)
    for kw in ({}, dict(max_size=2048)):  # the default keeps its limit
        with pytest.raises(ValueError, match="2048"):
            population_layout(4098, 1, 2, None, **kw)
    with pytest.raises(ValueError):
        population_layout(6002, 1, 2, None, max_size=3000)


def test_python_entry_is_exported_beside_its_neighbour(built):
    from pita_amd import sde_integration, utils

    assert callable(utils.sample_cat_sys_population_blocks)
    assert sde_integration.sample_cat_sys_population_blocks is utils.sample_cat_sys_population_blocks
    assert utils.MAX_POPULATION_SIZE == 2048


def test_inputs_keep_their_distance_from_the_thresholds():
    """The margin the GPU tests rely on to assert EVERY decision.  Measured in float64 numpy: the smallest distance of an
    ESS fraction from 0.6 or 0.2 over S in SIZES and p < 40 is 0.10, far above the 1e-3 asserted; the kernel's fp64
    sums have at most 5 000 non-negative terms (relative error <= 5000 * 2^-53 ~ 5.6e-13 in any order)."""
    fr = np.array([[PP.ref_stats(S, p)[3] for p in range(40)] for S in PB.SIZES])
    assert np.minimum(np.abs(fr - 0.6), np.abs(fr - 0.2)).min() >= 1e-3
    for row in fr:  # both sides of both thresholds at every size
        assert (row <= 0.6).sum() == 20 and (row <= 0.2).sum() == 10
