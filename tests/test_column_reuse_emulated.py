"""CPU: reuse of a field's column pass across spectral products, on the product's host code and kernels compiled for the emulator (tests/column_reuse.py has the
scenarios; tests/test_gpu_column_reuse.py runs them on the GPU), and the stand-alone C++ client of xrfthip_exec_ex (tests/c_abi/pass1_example.cpp) built against
the emulated library with AddressSanitizer and UBSan and run as a program of its own."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api, engine  # noqa: E402

import cases  # noqa: E402
import column_reuse as R  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    yield
    api.clear_plan_cache()
    engine.reuse_column_pass(True)
    _lib._state.update(dll=None, path=None, device="cuda")


def _against_oracle(ta, tb, coords, got):
    oa, ob = (o.OArr(t.numpy().astype(np.float64), R.DIMS, coords) for t in (ta, tb))
    cases.check(got[0], o.cross_spectrum(oa, ob, **R.HANN), cases.TOL["float32"])
    cases.check(got[1], o.isotropic_power_spectrum(oa, **R.HANN), cases.TOL["float32"])
    cases.check(got[2], o.isotropic_power_spectrum(ob, **R.HANN), cases.TOL["float32"])


@pytest.mark.parametrize("shape", R.SHAPES, ids=["256x256", "512x256"])
def test_cross_then_isotropic(shape):
    R.cross_then_isotropic(shape, check=_against_oracle if shape[1] > 256 else None)


@pytest.mark.parametrize("shape", R.SHAPES, ids=["256x256", "512x256"])
def test_power_then_isotropic_with_linear_detrend(shape):
    R.power_then_isotropic_detrended(shape)


@pytest.mark.parametrize("shape", R.SHAPES, ids=["256x256", "512x256"])
def test_no_reuse(shape):
    R.no_reuse_cases(shape)


def test_c_abi():
    R.c_abi_errors()


def test_standalone_client_under_sanitizers(tmp_path):
    """produce -> consume through xrfthip_exec_ex from plain C++ (no Python, no torch): the client compiled with -fsanitize=address,undefined, linked against the
    emulated library and run as a program of its own.  (The library's own units under both sanitizers compile for a quarter of an hour: build them the same way,
    with -fsanitize=address,undefined on every unit of build_emu.UNITS, to check the library's side.)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    lib = build_emu.build()
    exe = str(tmp_path / "pass1_example")
    r = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-DXRFT_EMULATE", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        f"-I{build_emu.HERE}", "-I" + os.path.join(os.path.dirname(HERE), "include"), os.path.join(HERE, "c_abi", "pass1_example.cpp"),
                        lib, "-Wl,-rpath," + os.path.dirname(lib), "-lpthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
