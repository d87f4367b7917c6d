"""Host side of the fused MALA chain on the force-field target (pita_ff_mala; no GPU): the workspace size, argument
validation that answers before any device call, and the Python entry point the integrator dispatches on."""
import inspect

import pytest


@pytest.fixture(scope="module")
def pa():
    from pita_amd import build as _b

    _b.build(verbose=False)
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def test_ff_mala_workspace_bytes(pa):
    """One 64-bit counter per step plus the word launch_mala_finish reads behind them; monotone in the step count."""
    L = pa._lib.lib()
    sizes = [int(L.pita_ff_mala_workspace_bytes(n)) for n in range(0, 200)]
    assert all(b >= 8 * (n + 1) for n, b in enumerate(sizes))
    assert all(b1 >= b0 for b0, b1 in zip(sizes, sizes[1:]))
    assert int(L.pita_ff_mala_workspace_bytes(-3)) >= 8


def test_ff_mala_rejects_null_handle_without_a_device(pa):
    """PITA_EINVAL (-1) with a message, decided from the arguments alone."""
    L = pa._lib.lib()
    rc = L.pita_ff_mala(None, None, None, None, None, 4, 2, None, 0, 4, 0, 0, None, 0, 1, None, None, None)
    assert rc == -1
    msg = pa._lib.last_error()
    assert "pita_ff_mala" in msg and "null" in msg


def test_ff_mala_python_entry_point(pa):
    """ForceFieldEnergy.fused_mala exists (WeightedSDEIntegrator._mala dispatches on it) with the parameter names of
    LennardJonesEnergy.fused_mala; ALPEnergy inherits it."""
    from pita_amd.alp_energy import ALPEnergy, ForceFieldEnergy

    want = list(inspect.signature(pa.LennardJonesEnergy.fused_mala).parameters)
    assert list(inspect.signature(ForceFieldEnergy.fused_mala).parameters) == want
    assert ALPEnergy.fused_mala is ForceFieldEnergy.fused_mala
