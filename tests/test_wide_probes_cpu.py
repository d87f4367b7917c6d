"""The Hutchinson divergence estimator at the drop-in boundary (no GPU needed): pita_egnn_wide_trace_probes and
pita_rademacher_probes are declared in include/pita_hip.h, bound by the ctypes table and exported by the built library at
ABI version 13; ``VEReverseSDE(divergence=...)`` validates its arguments; the integrator keys the probes with a Philox
stream of their own; the NumPy restatement of the draw (tests/_probes.py) is Philox4x32-10."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pita_egnn_wide_trace_probes": 14, "pita_rademacher_probes": 9}  # name -> number of arguments


def test_probe_exports_are_declared_bound_and_exported():
    from pita_amd import build as _b

    _b.build(verbose=False)  # an up-to-date in-tree build is reused
    import pita_amd

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pita_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+PITA_ABI_VERSION\s+13\b", hdr)
    assert pita_amd._lib.ABI_VERSION == 13
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pita_amd._lib.LIB_PATH], text=True)
    L = pita_amd._lib.lib()  # binds every symbol of the table, checks the version
    assert L.pita_abi_version() == 13
    for name, nargs in NAMES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared in include/pita_hip.h"
        assert name in pita_amd._lib.EXPORTS
        assert len(pita_amd._lib._PROTOS[name][1]) == nargs
        assert re.search(r" T " + name + r"$", nm, flags=re.M), f"{name} not exported by libpita_hip.so"


def test_wide_backbones_expose_the_estimator():
    import pita_amd.utils
    from pita_amd.egnn_aldp import EGNN_dynamics
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    assert callable(getattr(EGNN_dynamics_AD2_cat, "jacobian_trace_estimate"))
    assert EGNN_dynamics.jacobian_trace_estimate is EGNN_dynamics_AD2_cat.jacobian_trace_estimate
    assert callable(pita_amd.utils.rademacher_probes)


def test_sde_validates_the_divergence_arguments():
    from pita_amd.sdes import VEReverseSDE

    sde = VEReverseSDE(noise_schedule=None)
    assert sde.divergence == "exact" and sde.n_probes is None
    with pytest.raises(ValueError):
        VEReverseSDE(noise_schedule=None, divergence="bogus")
    with pytest.raises(ValueError):
        VEReverseSDE(noise_schedule=None, divergence="hutchinson")
    with pytest.raises(ValueError):
        VEReverseSDE(noise_schedule=None, divergence="hutchinson", n_probes=0)
    est = VEReverseSDE(noise_schedule=None, divergence="hutchinson", n_probes=4, cdf=object())  # cdf: accepted, ignored
    assert est.divergence == "hutchinson" and est.n_probes == 4


def test_probe_stream_id_is_the_integrators_own():
    """The stream ids WeightedSDEIntegrator passes to ``_key`` (read from its source) do not include the probes' one, and
    the keys differ for one seed and run."""
    import pita_amd.sde_integration as S

    src = open(S.__file__).read()
    others = {int(m) for m in re.findall(r"self\._key\((\d+)\)", src)}
    assert others == {0, 1, 2}, others
    assert S.PROBE_STREAM_ID not in others and 0 <= S.PROBE_STREAM_ID < 256  # (_runs << 8) + stream_id
    assert "PROBE_STREAM_ID" in src.split("def _integrate_debiased")[1]
    integ = S.WeightedSDEIntegrator.__new__(S.WeightedSDEIntegrator)
    integ.seed, integ._runs = 7, 3
    keys = [integ._key(i) for i in sorted(others | {S.PROBE_STREAM_ID})]
    assert len(set(keys)) == len(keys)


def test_numpy_philox_is_philox4x32_10():
    """Known-answer vectors of Philox4x32-10 (Random123's kat_vectors): the restatement the GPU draw is compared with."""
    from tests._probes import philox4x32_10, rademacher_probes

    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10([np.array([v], dtype=np.uint64) for v in ctr], key[0] | (key[1] << 32))
        assert tuple(int(g[0]) for g in got) == want, (ctr, [hex(int(g[0])) for g in got])
    v = rademacher_probes(4, 22, 3, 5, seed=9, walker_offset=2, step=11)
    assert v.shape == (5, 4, 66) and v.dtype == np.float32 and set(np.unique(v)) == {-1.0, 1.0}
    assert np.array_equal(rademacher_probes(6, 22, 3, 5, seed=9, walker_offset=0, step=11)[:, 2:], v)  # keyed by walker
