"""The layout x parity matrix on the emulated library: a (t = 3, y, x) field in all six axis orders, even and odd lengths on each transform
axis, one and two transform axes, real_dim on each of them, through fft (plain, linear + Hann), power_spectrum, cross_spectrum, cross_phase
and ifft(fft(.)), in float64 and float32.  Every call meets the rounding-level contract of tests/accuracy.py against the oracle, or raises
what the oracle raises."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import accuracy as A  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api._plan_cache.clear()
    _lib._load_for_testing(build_emu.build())
    yield
    api._plan_cache.clear()
    _lib._state.update(dll=None, path=None, device="cuda")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("order,ny,nx,dim,rd", [p[1:] for p in A.matrix_params()], ids=[p[0] for p in A.matrix_params()])
def test_layout_matrix(order, ny, nx, dim, rd, dtype):
    A.run_matrix_cell(order, ny, nx, dim, rd, dtype)


@pytest.mark.parametrize("op", ["fft", "power_spectrum", "cross_spectrum"])
@pytest.mark.parametrize("order", [("y", "x", "t"), ("y", "t", "x")])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_odd_real_axis_first_in_memory_on_the_fused_passes(order, dtype, op):
    A.run_odd_real_axis_first(order, dtype, op)
