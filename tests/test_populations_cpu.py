"""Walker populations without a GPU: the new entry points bind and refuse bad arguments before any device call, the
layout helper and the constructor accept and refuse what they document, and the shared inputs of the GPU tests keep
their distance from the thresholds."""
import ctypes

import numpy as np
import pytest

from tests import _populations as PP


@pytest.fixture(scope="module")
def built():
    from pita_amd import build as _b

    _b.build(verbose=False)
    import pita_amd

    pita_amd._lib.lib()
    return pita_amd


def test_new_prototypes_bind_and_the_abi_version_stays(built):
    L = built._lib.lib()
    for name in ("pita_population_resample_workspace_bytes", "pita_population_resample"):
        assert name in built._lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.pita_abi_version() == 13 == built._lib.ABI_VERSION
    for P, S in ((1, 1), (300, 2048)):
        nbytes = L.pita_population_resample_workspace_bytes(P, S)
        assert nbytes >= 1 and nbytes % 8 == 0


def test_bad_arguments_come_back_as_error_codes_without_a_gpu(built):
    """Every check precedes the first HIP call: host buffers stand in for the device pointers and are never touched."""
    L = built._lib.lib()
    P, S = 3, 64
    buf = {k: ctypes.create_string_buffer(P * S * 8 + 64) for k in
           ("logits", "u", "ids", "nu", "stats", "flag", "next", "ws")}
    before = {k: v.raw for k, v in buf.items()}
    addr = {k: ctypes.addressof(v) for k, v in buf.items()}

    def call(n_pop=P, pop_size=S, theta=0.5, **ptr):
        a = dict(addr, **ptr)
        return L.pita_population_resample(a["logits"], n_pop, pop_size, a["u"], theta, a["ids"], a["nu"], a["stats"],
                                          a["flag"], a["next"], a["ws"], None)

    for kw in (dict(logits=None), dict(u=None), dict(ids=None), dict(stats=None), dict(flag=None), dict(ws=None),
               dict(n_pop=0), dict(n_pop=-2), dict(pop_size=0), dict(pop_size=-1), dict(theta=-0.1), dict(theta=1.5),
               dict(theta=float("nan")), dict(ws=addr["ws"] + 4)):
        assert call(**kw) == -1, kw  # PITA_EINVAL
        assert built._lib.last_error(), kw
    assert call(pop_size=PP.MAX_S + 1) == -2  # PITA_EUNSUPPORTED, and the message names the limit
    assert str(PP.MAX_S) in built._lib.last_error()
    assert call(pop_size=PP.MAX_S + 1, logits=None) == -2
    assert all(buf[k].raw == before[k] for k in buf)


def test_population_layout():
    from pita_amd.sde_integration import population_layout

    assert population_layout(192, 1, 3, None) == (64, 3, 64)
    assert population_layout(192, 1, 1, None) == (192, 1, 192)
    assert population_layout(65536, 1, 32, None) == (2048, 32, 2048)
    assert population_layout(65536, 8, 32, 65536) == (2048, 4, 2048)  # a chunk never exceeds a population
    assert population_layout(256, 2, 4, 64) == (64, 2, 64)
    assert population_layout(256, 2, 4, 16) == (64, 2, 16)  # clamp chunks tile a population
    assert population_layout(4, 4, 4, 1) == (1, 1, 1)
    for Bg, world, P, bs in ((193, 1, 3, None),  # Bg % P
                             (2, 1, 3, None),  # fewer walkers than populations
                             (4098, 1, 2, None),  # S = 2 049
                             (65536, 1, 1, None),  # S > 2 048
                             (192, 2, 3, None),  # populations would straddle ranks
                             (256, 1, 4, 48),  # 64 % 48
                             (192, 1, 0, None), (192, 1, -1, None)):
        with pytest.raises(ValueError):
            population_layout(Bg, world, P, bs)


def test_constructor_validates_populations(built):
    def make(**kw):
        return built.WeightedSDEIntegrator(sde=None, num_integration_steps=4, start_resampling_step=0,
                                           end_resampling_step=4, **kw)

    assert make().populations is None
    assert make(populations=None).populations is None
    assert make(populations=1).populations == 1
    assert make(populations=np.int64(32)).populations == 32 and type(make(populations=np.int64(32)).populations) is int
    for bad in (0, -1, 2.0, 1.5, "2", True, float("nan")):
        with pytest.raises(ValueError):
            make(populations=bad)


def test_inputs_keep_their_distance_from_the_thresholds():
    """The margin the GPU tests rely on to assert EVERY decision: the kernel's fp64 ESS agrees with numpy's to 1e-9
    relative, the fractions lie at least 1e-5 from 0.6 and 0.2."""
    worst = np.inf
    for S in PP.SIZES:
        f = np.array([PP.ref_stats(S, p)[3] for p in range(max(PP.POPS))])
        worst = min(worst, np.abs(f - 0.6).min(), np.abs(f - 0.2).min())
        if S >= 63:
            for theta in (0.6, 0.2):
                assert 0 < (f <= theta).sum() < f.size, (S, theta)
    assert worst >= 1e-5, worst
    assert np.array_equal(PP.uniforms(8), [0.0, 0.3, 0.999999, 3 / 8, 0.0, 0.3, 0.999999, 7 / 8])
    a = PP.batch(63, 3)
    assert a.dtype == np.float32 and a.shape == (189,) and np.array_equal(a[63:126], PP.weights(63, 1))
