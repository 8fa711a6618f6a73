"""A NaN / inf stays inside its own transform, on the emulated library: every case of tests/nonfinite.py -- the families that pack two independent real
sequences into one complex transform (fastm x-only / y-only, fastg y-only and its Rader rows, the fused inner-layout passes) and one representative of every
other family -- EXECUTED through engine.SpectralPlan, the routed family asserted first; and the land mask of a (t, y, x) cube through the labelled API against
the oracle."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import nonfinite as N  # noqa: E402

L = _lib


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api._plan_cache.clear()
    _lib._load_for_testing(build_emu.build())
    yield
    api._plan_cache.clear()
    _lib._state.update(dll=None, path=None, device="cuda")


def _env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("XRFTHIP_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("rid,batch,B,inpos,bad,detrend,field", [p[1:] for p in N.params()], ids=[p[0] for p in N.params()])
def test_a_bad_sample_stays_in_its_transform(monkeypatch, rid, batch, B, inpos, bad, detrend, field):
    _env(monkeypatch, N.ROWS[rid][2])
    N.run_case(rid, batch, B, inpos, bad, detrend, field, "cpu")


@pytest.mark.parametrize("rid", [r[0] for r in N.PACKED])
def test_the_packed_families_have_one_loader(monkeypatch, rid):
    _env(monkeypatch, N.ROWS[rid][2])
    N.run_declines_other_loaders(rid)


def test_every_position_of_every_packed_form_is_a_case():
    ids = {p[0] for p in N.params()}
    for rid, kw, _env_, _kind, _tag in N.PACKED:
        for pos in N.positions(dict(kw, batch=5)):
            assert f"{rid}-b5-{pos}" in ids
        assert f"{rid}-both-partners" in ids


@pytest.mark.parametrize("size,order,dim", [p[1:] for p in N.api_params()], ids=[p[0] for p in N.api_params()])
def test_land_mask_through_the_api(monkeypatch, size, order, dim):
    _env(monkeypatch, {})
    for dtype in ("float64", "float32"):
        fams = N.run_api_land_mask(size, order, dim, dtype)
        assert fams == N.API_FAMILY[f"{'x'.join(map(str, size))}-{''.join(order)}-{''.join(dim)}"], fams


@pytest.mark.parametrize("op", ["detrend", "fft", "power_spectrum", "cross_spectrum"])
def test_a_line_along_one_axis_refuses_what_scipy_refuses(op):
    """detrend="linear" over ONE axis is scipy.signal.detrend in the reference: input that is not finite is a ValueError there, and here -- also on a length
    no fast plan takes (a prime, 1031 samples), and in the stand-alone detrend."""
    import numpy as np

    import xrft_amd as xa
    from oracle import xrft_oracle as o

    import cases

    v = np.random.default_rng(2).standard_normal((3, 1031))
    v[1, 5] = np.inf
    a, oa = cases.pair(v, ("t", "x"), {"t": np.arange(3.0), "x": np.arange(1031.0)})
    for mod, p in ((o, oa), (xa, a)):
        with pytest.raises(ValueError):
            if op == "detrend":
                mod.detrend(p, ["x"], "linear")
            elif op == "cross_spectrum":
                mod.cross_spectrum(p, p, dim=["x"], detrend="linear")
            else:
                getattr(mod, op)(p, dim=["x"], detrend="linear")
