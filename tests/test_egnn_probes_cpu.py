"""The shared-primal Hutchinson estimate of the hidden-32 EGNN at the drop-in boundary (no GPU needed):
pita_egnn_trace_probes is declared in include/pita_hip.h, bound by the ctypes table and exported by the built library at
ABI version 13; both hidden-32 classes have ``trace_probes`` and neither has ``jacobian_trace_estimate`` (the attribute
VEReverseSDE dispatches the wide backbone on); ``VEReverseSDE(shared_primal=...)`` validates its argument."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trace_probes_is_declared_bound_and_exported():
    from pita_amd import build as _b

    _b.build(verbose=False)  # an up-to-date in-tree build is reused
    import pita_amd

    name = "pita_egnn_trace_probes"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pita_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+PITA_ABI_VERSION\s+13\b", hdr)
    assert pita_amd._lib.ABI_VERSION == 13
    L = pita_amd._lib.lib()  # binds every symbol of the table, checks the version
    assert L.pita_abi_version() == 13
    assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared in include/pita_hip.h"
    assert name in pita_amd._lib.EXPORTS
    assert len(pita_amd._lib._PROTOS[name][1]) == 14
    assert pita_amd._lib._PROTOS[name] == pita_amd._lib._PROTOS["pita_egnn_wide_trace_probes"]  # the sibling's list
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pita_amd._lib.LIB_PATH], text=True)
    assert re.search(r" T " + name + r"$", nm, flags=re.M), f"{name} not exported by libpita_hip.so"


def test_hidden32_classes_expose_trace_probes_under_its_own_name():
    import inspect

    from pita_amd import egnn, egnn_temp_conditioned

    for cls in (egnn_temp_conditioned.EGNN_dynamics, egnn.EGNN_dynamics):
        assert callable(getattr(cls, "trace_probes"))
        assert not hasattr(cls, "jacobian_trace_estimate")  # VEReverseSDE would take it for the wide backbone's
    assert egnn.EGNN_dynamics.trace_probes is egnn_temp_conditioned.EGNN_dynamics.trace_probes
    names = list(inspect.signature(egnn_temp_conditioned.EGNN_dynamics.trace_probes).parameters)
    assert names == ["self", "h_t", "x_t", "beta", "n_probes", "probes", "seed", "walker_offset", "step", "want_denoiser",
                     "want_per_probe"]


def test_sde_validates_shared_primal():
    from pita_amd.sdes import VEReverseSDE

    assert VEReverseSDE(noise_schedule=None).shared_primal is False
    assert VEReverseSDE(noise_schedule=None, divergence="hutchinson", n_probes=3).shared_primal is False
    assert VEReverseSDE(noise_schedule=None, divergence="hutchinson", n_probes=3, shared_primal=True).shared_primal is True
    with pytest.raises(ValueError):
        VEReverseSDE(noise_schedule=None, shared_primal=True)  # divergence="exact" draws no probes
    with pytest.raises(ValueError):
        VEReverseSDE(noise_schedule=None, divergence="exact", shared_primal=True)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError):
            VEReverseSDE(noise_schedule=None, divergence="hutchinson", n_probes=3, shared_primal=bad)
