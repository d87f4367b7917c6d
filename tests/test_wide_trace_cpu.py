"""pita_egnn_wide_jacobian_trace at the drop-in boundary (no GPU needed): declared in include/pita_hip.h, bound by the
ctypes table, exported by the built library, ABI version 13; EGNN_dynamics_AD2_cat and egnn_aldp.EGNN_dynamics expose the
``jacobian_trace`` that VEReverseSDE._score_divergence_terms looks for."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pita_egnn_wide_jacobian_trace"


def test_wide_jacobian_trace_is_declared_bound_and_exported():
    from pita_amd import build as _b

    _b.build(verbose=False)  # an up-to-date in-tree build is reused
    import pita_amd

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pita_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr), "not declared in include/pita_hip.h"
    assert re.search(r"#define\s+PITA_ABI_VERSION\s+13\b", hdr)
    assert pita_amd._lib.ABI_VERSION == 13
    res, args = pita_amd._lib._PROTOS[NAME]
    assert len(args) == 8  # net, h, x, beta, trace, denoiser_out, B, stream
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pita_amd._lib.LIB_PATH], text=True)
    assert re.search(r" T " + NAME + r"$", nm, flags=re.M), "not exported by libpita_hip.so"
    L = pita_amd._lib.lib()  # binds every symbol of the table, checks the version
    assert L.pita_abi_version() == 13
    assert getattr(L, NAME).argtypes == args


def test_wide_backbones_expose_jacobian_trace():
    from pita_amd.egnn_aldp import EGNN_dynamics
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    assert callable(getattr(EGNN_dynamics_AD2_cat, "jacobian_trace"))
    assert EGNN_dynamics.jacobian_trace is EGNN_dynamics_AD2_cat.jacobian_trace
