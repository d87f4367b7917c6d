"""pita_egnn_wide_vjp_uses_matrix_pipe at the drop-in boundary (no GPU needed): declared in include/pita_hip.h with the
one-pointer signature, bound by the ctypes table with the prototype of its jvp sibling, exported by the built library;
EGNN_dynamics_AD2_cat and egnn_aldp.EGNN_dynamics offer ``vjp_uses_matrix_pipe``."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pita_egnn_wide_vjp_uses_matrix_pipe"


def test_wide_vjp_query_is_declared_bound_and_exported():
    from pita_amd import build as _b

    _b.build(verbose=False)  # an up-to-date in-tree build is reused
    import pita_amd

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pita_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+pita_egnn_wide_t\s*\*\s*\w+\s*\)\s*;", hdr), \
        "not declared in include/pita_hip.h with the one-pointer signature"
    assert NAME in pita_amd._lib.EXPORTS
    assert pita_amd._lib._PROTOS[NAME] == pita_amd._lib._PROTOS["pita_egnn_wide_jvp_uses_matrix_pipe"]
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pita_amd._lib.LIB_PATH], text=True)
    assert re.search(r" T " + NAME + r"$", nm, flags=re.M), "not exported by libpita_hip.so"
    L = pita_amd._lib.lib()  # binds every symbol of the table, checks the version
    assert getattr(L, NAME).argtypes == pita_amd._lib._PROTOS[NAME][1]


def test_wide_backbones_offer_vjp_uses_matrix_pipe():
    from pita_amd.egnn_aldp import EGNN_dynamics
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    assert callable(getattr(EGNN_dynamics_AD2_cat, "vjp_uses_matrix_pipe"))
    assert EGNN_dynamics.vjp_uses_matrix_pipe is EGNN_dynamics_AD2_cat.vjp_uses_matrix_pipe
