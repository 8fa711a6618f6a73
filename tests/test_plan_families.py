"""Which kernel family serves a descriptor: one row per family, per demotion and per tie-break, checked through the plan's
introspection (xrfthip_plan_kernel_info and the tag xrfthip_plan_describe prints) on the emulated library.  Plans are created
and inspected, never executed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

from accuracy import ROWS, family, make, radial_map  # noqa: E402,F401  (the routing table lives beside the accuracy bounds: the ladder executes every row)

L = _lib
F32, F64, C64 = torch.float32, torch.float64, torch.complex64


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api._plan_cache.clear()
    _lib._load_for_testing(build_emu.build())
    yield
    api._plan_cache.clear()
    _lib._state.update(dll=None, path=None, device="cuda")


def scattered_map(ny, nx, nb):
    return np.random.default_rng(1).integers(0, nb, size=(ny, nx)).astype(np.int32)


def set_phase(p, axis, ph):
    ph = np.ascontiguousarray(ph, dtype=np.complex128)
    _lib.check(p._dll.xrfthip_plan_set_phase(p._h, axis, ph.ctypes.data_as(C.c_void_p), ph.size))


def set_binmap(p, bm, nb):
    bm = np.ascontiguousarray(bm, dtype=np.int32)
    _lib.check(p._dll.xrfthip_plan_set_binmap(p._h, bm.ctypes.data_as(C.c_void_p), bm.shape[0], bm.shape[1], nb))


RAD256, NB256 = radial_map(256, 256)
RAD64, NB64 = radial_map(64, 64)
RAD1K, NB1K = radial_map(1024, 1024)


@pytest.mark.parametrize("kw,env,kind,tag", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_family(monkeypatch, kw, env, kind, tag):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert family(make(**kw)) == (kind, tag)


def test_fasts_keeps_a_radial_map():
    p = make(ny=256, nx=256, flags=L.ISO, binmap=RAD256, nbins=NB256)
    assert family(p) == (L.K_FASTS, "fasts")


def test_fasts_with_a_scattered_map_falls_to_fasty_where_its_tables_exist():
    p = make(ny=256, nx=256, flags=L.ISO, binmap=scattered_map(256, 256, NB256), nbins=NB256)
    assert family(p) == (L.K_FASTY, "fasty")
    set_binmap(p, RAD256, NB256)  # (sticky)
    assert family(p) == (L.K_FASTY, "fasty")


def test_fasts_with_a_scattered_map_falls_to_generic_elsewhere():
    p = make(ny=64, nx=64, flags=L.ISO, binmap=scattered_map(64, 64, NB64), nbins=NB64)
    assert family(p) == (L.K_GENERIC, "main")


def test_fastg_isotropic_cross_with_a_phase_is_generic_for_good():
    rad, nb = radial_map(50, 50)
    p = make(ny=50, nx=50, dtype=F64, out_mode=L.OUT_CROSS, flags=L.ISO, binmap=rad, nbins=nb)
    assert family(p) == (L.K_FASTG, "fastg")
    set_phase(p, 1, np.exp(0.3j * np.arange(50)))
    assert family(p) == (L.K_GENERIC, "f0")  # (the generic passes of a cross spectrum: field 0 first)
    set_phase(p, 1, np.ones(50))
    assert family(p) == (L.K_GENERIC, "f0")


def test_fastyc_four_step_window_is_generic():
    p = make(ndim=1, nx=1 << 20, dtype=C64, out_mode=L.OUT_COMPLEX, window_x=np.hanning(1 << 20))
    assert family(p) == (L.K_GENERIC, "main")


def test_fastyc_four_step_input_phase():
    n = 1 << 20
    sep = make(ndim=1, nx=n, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.PHASE_IN, phase_x=np.exp(0.001j * np.arange(n)))
    assert family(sep) == (L.K_FASTY, "fasty complex rows, four-step")
    other = make(ndim=1, nx=n, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.PHASE_IN, phase_x=np.exp(1e-6j * np.arange(n) ** 2))
    assert family(other) == (L.K_GENERIC, "main")


def test_fasty_isotropic_tables_that_do_not_fit_are_generic():
    p = make(ny=1024, nx=1024, flags=L.ISO, binmap=RAD1K, nbins=200000)
    assert family(p) == (L.K_GENERIC, "main")
    q = make(ny=1024, nx=1024, flags=L.ISO, binmap=RAD1K, nbins=NB1K)
    assert family(q) == (L.K_FASTY, "fasty")


def test_fasty_isotropic_cross_phase_is_reversible():
    p = make(ny=1024, nx=1024, out_mode=L.OUT_CROSS, flags=L.ISO, binmap=RAD1K, nbins=NB1K)
    assert family(p) == (L.K_FASTY, "fasty")
    ws = p.workspace_bytes
    set_phase(p, 1, np.exp(0.3j * np.arange(1024)))
    assert family(p) == (L.K_GENERIC, "f0")
    assert p.workspace_bytes != ws
    set_phase(p, 1, np.ones(1024))
    assert family(p) == (L.K_FASTY, "fasty")
    assert p.workspace_bytes == ws


def test_bluestein_is_reported_by_the_family_that_runs():
    assert make(ny=1031, nx=64, dtype=F64, flags=L.AXIS_Y).uses_bluestein()
    assert family(make(ny=1031, nx=64, dtype=F64, flags=L.AXIS_Y))[0] == L.K_FASTG_Y
    assert make(ndim=1, nx=1031, dtype=F64).uses_bluestein()
    assert not make(ny=720, nx=1440, dtype=F64).uses_bluestein()
    assert not make(ny=4096, nx=4096, flags=L.ISO, binmap=radial_map(4096, 4096)[0], nbins=2049).uses_bluestein()
