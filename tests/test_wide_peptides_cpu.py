"""pita_egnn_wide_jvp_uses_matrix_pipe / EGNN_dynamics_AD2_cat.jvp_uses_matrix_pipe at the drop-in boundary: declared in
the header, bound in _lib.py, offered by both backbone classes.  No GPU needed; tests/test_abi.py compares the header
with the built library's exports, tests/test_wide_peptides_gpu.py runs it."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pita_egnn_wide_jvp_uses_matrix_pipe"


def test_export_is_declared_and_bound():
    import pita_amd

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pita_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+pita_egnn_wide_t\s*\*\s*net\s*\)\s*;", hdr), \
        "not declared in include/pita_hip.h"
    assert NAME in pita_amd._lib.EXPORTS
    res, args = pita_amd._lib._PROTOS[NAME]
    assert res is ctypes.c_int and args == [ctypes.c_void_p]
    assert pita_amd._lib._PROTOS["pita_egnn_wide_uses_matrix_pipe"] == (res, args)  # its forward-pass sibling


def test_both_backbone_classes_offer_the_query():
    from pita_amd import egnn_aldp
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    assert callable(getattr(EGNN_dynamics_AD2_cat, "jvp_uses_matrix_pipe", None))
    assert issubclass(egnn_aldp.EGNN_dynamics, EGNN_dynamics_AD2_cat)
    assert egnn_aldp.EGNN_dynamics.jvp_uses_matrix_pipe is EGNN_dynamics_AD2_cat.jvp_uses_matrix_pipe
