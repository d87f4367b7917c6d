"""pita_egnn_wide_vjp_parts at the drop-in boundary (no GPU needed): declared in include/pita_hip.h with the signature of
pita_egnn_vjp, bound by the ctypes table, exported by the built library, ABI still 13; a null handle is PITA_EINVAL before
any device call; EGNN_dynamics_AD2_cat and egnn_aldp.EGNN_dynamics carry ``vjp_h_parts`` and refuse ``want_h_parts`` without
``want_dot_h`` before any device work."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pita_egnn_wide_vjp_parts"


def test_wide_vjp_parts_is_declared_bound_and_exported():
    from pita_amd import build as _b

    _b.build(verbose=False)  # an up-to-date in-tree build is reused
    import pita_amd

    raw = open(os.path.join(ROOT, "include", "pita_hip.h")).read()
    assert re.search(r"#define\s+PITA_ABI_VERSION\s+13\b", raw) and pita_amd._lib.ABI_VERSION == 13
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    args = r"\s*,\s*".join([r"pita_egnn_wide_t\s*\*\s*net", r"const\s+float\s*\*\s*h", r"const\s+float\s*\*\s*x",
                            r"const\s+float\s*\*\s*beta", r"const\s+float\s*\*\s*cot", r"float\s*\*\s*out",
                            r"float\s*\*\s*vjp", r"float\s*\*\s*dot_h", r"float\s*\*\s*dot_parts", r"int64_t\s+B",
                            r"void\s*\*\s*stream"])
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*" + args + r"\s*\)\s*;", hdr), "not declared in include/pita_hip.h"
    # the comment cites the reference as the hidden-32 entry does
    doc = raw[:raw.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "energy_net.py:33-41" in doc and "sdes.py:218" in doc
    assert NAME in pita_amd._lib.EXPORTS
    assert pita_amd._lib._PROTOS[NAME] == pita_amd._lib._PROTOS["pita_egnn_vjp"]
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pita_amd._lib.LIB_PATH], text=True)
    assert re.search(r" T " + NAME + r"$", nm, flags=re.M), "not exported by libpita_hip.so"
    assert re.search(r" T pita_egnn_wide_vjp$", nm, flags=re.M), "pita_egnn_wide_vjp stays"
    L = pita_amd._lib.lib()  # binds every symbol of the table, checks the version
    assert L.pita_abi_version() == 13
    assert getattr(L, NAME).argtypes == pita_amd._lib._PROTOS[NAME][1]


def test_null_handle_is_einval_without_a_gpu():
    import pita_amd

    L = pita_amd._lib.lib()
    assert L.pita_egnn_wide_vjp_parts(None, None, None, None, None, None, None, None, None, 1, None) == -1  # PITA_EINVAL
    assert pita_amd._lib.last_error()
    assert L.pita_egnn_wide_vjp_parts(None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert L.pita_egnn_wide_vjp(None, None, None, None, None, None, None, None, 1, None) == -1


def test_wide_backbones_offer_the_split():
    from pita_amd.egnn_aldp import EGNN_dynamics
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    assert EGNN_dynamics_AD2_cat.vjp_h_parts is True and EGNN_dynamics.vjp_h_parts is True
    assert EGNN_dynamics.vjp is EGNN_dynamics_AD2_cat.vjp


def test_h_parts_without_dot_h_is_refused_before_any_device_work():
    from pita_amd.egnn_dynamics_ad2_cat import EGNN_dynamics_AD2_cat

    net = EGNN_dynamics_AD2_cat(13, 3, hidden_nf=16, n_layers=1, condition_beta=True)
    # host tensors: anything that reached the device path would raise something else first
    with pytest.raises(ValueError, match="want_h_parts needs want_dot_h"):
        net.vjp(torch.ones(2), torch.zeros(2, 39), torch.ones(2), want_h_parts=True, want_dot_h=False)
    assert net._handle is None  # no native handle was created
