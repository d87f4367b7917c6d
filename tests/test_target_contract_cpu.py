"""The contract between the HIP targets and WeightedSDEIntegrator (no GPU needed): the table in pita_amd/_target.py lists
exactly the attributes the integrator probes on a target, each shipped class has exactly the attributes its row says, the
fused routes have one signature across the classes, and every shared body makes the tensor's device current."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FUSED_DESCENT = "(self, x, num_steps, dt, noise_scale, sqrt_dt, seed=0, walker_offset=0, step0=0, remove_mean=True, noise=None)"
FUSED_MALA = ("(self, x, logp, num_steps, dt_dev, adaptive, total, noise=None, uniforms=None, seed=0, walker_offset=0, "
              "walker_ids=None, step0=0, remove_mean=True, rates_out=None)")


def _classes():
    from pita_amd.alp_energy import ALPEnergy, ForceFieldEnergy
    from pita_amd.dw4_energy import MultiDoubleWellEnergy
    from pita_amd.gmm_energy import GMM
    from pita_amd.lennardjones_energy import LennardJonesEnergy

    return {"lj": (LennardJonesEnergy,), "dw": (MultiDoubleWellEnergy,), "ff": (ForceFieldEnergy, ALPEnergy), "gmm": (GMM,)}


def _table():
    """{attribute: (signature text or None, set of family tags)} from the module docstring of pita_amd/_target.py."""
    from pita_amd import _target

    lines = _target.__doc__.splitlines()
    rules = [i for i, ln in enumerate(lines) if ln.startswith("=====")]
    assert len(rules) == 3, "one table: rule, header, rule, rows, rule"
    c1, c2 = (m.start() for m in list(re.finditer(r"=+", lines[rules[0]]))[1:])
    rows, cur = [], None
    for ln in lines[rules[1] + 1:rules[2]]:
        first, last = ln[:c1].strip(), ln[c2:].strip()
        if last:  # a row starts on the line that names its classes
            cur = [first, set(last.split())]
            rows.append(cur)
        else:
            cur[0] += " " + first
    out = {}
    for first, tags in rows:
        names = re.findall(r"``(\w+)", first)
        sig = re.search(r"``\w+(\(.*\))``", first)
        for name in names:
            out[name] = (None if sig is None else sig.group(1), tags)
    return out


def _probed():
    """Attributes sde_integration.py reads from a target (``energy_function``), the call itself included."""
    src = open(os.path.join(ROOT, "pita_amd", "sde_integration.py")).read()
    names = set(re.findall(r"\benergy_function\.(\w+)", src))
    names |= set(re.findall(r"(?:hasattr|getattr)\(energy_function,\s*\"(\w+)\"", src))
    assert re.search(r"\benergy_function\(", src)
    return names | {"__call__"}


def test_table_rows_are_what_the_integrator_probes():
    assert set(_table()) == _probed()
    assert set(_table()) == {"__call__", "is_molecule", "n_particles", "n_spatial_dim", "fused_descent", "fused_mala"}


def test_each_class_defines_exactly_its_rows():
    table, classes = _table(), _classes()
    assert set().union(*(tags for _, tags in table.values())) == set(classes)
    for name in ("__call__", "fused_descent", "fused_mala"):  # class-level attributes; the rest is set per instance
        for tag, group in classes.items():
            for cls in group:
                defined = any(name in vars(k) for k in cls.__mro__ if k.__module__.startswith("pita_amd.") and
                              k.__name__ not in ("BaseEnergyFunction", "BaseMoleculeEnergy"))
                assert defined == (tag in table[name][1]), (cls.__name__, name)
    assert table["is_molecule"][1] == set(classes) and table["n_particles"][1] == table["n_spatial_dim"][1] == {"lj", "dw", "ff"}
    lj = classes["lj"][0](39, 13, 3)
    dw = classes["dw"][0]()
    gmm = classes["gmm"][0](device="cpu")  # host tensors only: nothing here calls the library
    for e in (lj, dw):
        assert e.is_molecule and (e.n_particles, e.n_spatial_dim) in ((13, 3), (4, 2))
    assert not gmm.is_molecule and not hasattr(gmm, "n_particles") and not hasattr(gmm, "n_spatial_dim")
    assert not hasattr(gmm, "fused_descent") and not hasattr(gmm, "fused_mala")


def test_fused_routes_have_one_signature():
    table, classes = _table(), _classes()
    for name, want in (("fused_descent", FUSED_DESCENT), ("fused_mala", FUSED_MALA)):
        assert "(self, " + table[name][0][1:] == want, name  # the table prints the signature without ``self``
        for tag in ("lj", "dw", "ff"):
            assert str(inspect.signature(getattr(classes[tag][0], name))) == want, (tag, name)
    ff, alp = classes["ff"]
    assert alp.fused_descent is ff.fused_descent and alp.fused_mala is ff.fused_mala
    call = "(self, samples: torch.Tensor, return_force=False)"
    for group in classes.values():
        for cls in group:
            assert str(inspect.signature(cls.__call__)) == call, cls.__name__


def test_shared_bodies_guard_the_device_and_mask_the_seed(monkeypatch):
    """Every C call of the mix-in sits under the device guard of the tensor's device (``torch.cuda.device`` whenever
    another device is current); both seeded bodies mask the seed to 64 bits; the classes themselves call the library only
    to create and destroy the force-field handle."""
    import torch

    from pita_amd import _lib, _target

    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    assert _target._device_guard(torch.device("cuda", 0)) is _target._SAME_DEVICE
    other = _target._device_guard(torch.device("cuda", 1))
    assert isinstance(other, torch.cuda.device) and other.idx == 1
    for name in ("_logp_force_call", "_descent_call", "_mala_call"):
        src = inspect.getsource(getattr(_target.HipTarget, name))
        guard, call = src.index("with _device_guard(x.device):"), src.index("(*self._handle_args()")
        assert guard < call, name
        assert ("& _U64" in src) == (name != "_logp_force_call"), name
    assert _target._U64 == 2 ** 64 - 1 and _lib.PITA_EUNSUPPORTED == -2
    for group in _classes().values():
        for cls in group:
            src = inspect.getsource(inspect.getmodule(cls))
            assert set(re.findall(r"\.(pita_\w+)\(", src)) <= {"pita_ff_create", "pita_ff_destroy"}, cls.__name__
            assert "== -2" not in src
