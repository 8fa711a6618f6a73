"""The stand-alone C-ABI operations (csrc/ops.cpp, csrc/aux_kernels.h: detrend, detrend3, detrend_inner, spectrum_tail, spectrum_tail_axis, gather_axis, table_mul,
angle, convert) on the emulated library, held to the rounding-level bounds of tests/ops.py against plain high-precision numpy: every dtype, the shapes at which each
launch branch is reached, guard bands around every output, two runs the same bits; the status codes; and the bounds' own sensitivity (numpy only).

The emulator runs a kernel's threads as fibers: the four cases of ops.EMU_SKIP (the second launch of a batch loop: 10^5 workgroups, 30 s a call here) are left to
the GPU suite (tests/test_gpu_ops.py), which runs every case; the host arithmetic of those loops (the chunk counts and offsets per launch) is plain C++ that the
GPU run exercises as it stands."""
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import ops as O  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    api.clear_plan_cache()
    _lib._state.update(dll=None, path=None, device="cuda")


@pytest.mark.parametrize("case,name,kind", O.detrend_params(O.DETREND, emulated=True))
def test_detrend(case, name, kind):
    O.check_detrend(case, name, kind)


@pytest.mark.parametrize("case,name,kind", O.detrend_params(O.DETREND3, emulated=True))
def test_detrend3(case, name, kind):
    O.check_detrend3(case, name, kind)


@pytest.mark.parametrize("case,name,kind", O.detrend_params(O.INNER, emulated=True))
def test_detrend_inner(case, name, kind):
    O.check_detrend_inner(case, name, kind)


@pytest.mark.parametrize("cross", [False, True], ids=["power", "cross"])
@pytest.mark.parametrize("name", O.CNAMES)
@pytest.mark.parametrize("n", O.TAIL_N)
def test_spectrum_tail(n, name, cross):
    O.check_spectrum_tail(n, name, cross)


@pytest.mark.parametrize("cross", [False, True], ids=["power", "cross"])
def test_spectrum_tail_wraps_its_grid(cross):
    O.check_spectrum_tail(O.TAIL_WRAP_N, "complex64", cross)


@pytest.mark.parametrize("cross", [False, True], ids=["power", "cross"])
@pytest.mark.parametrize("name", O.CNAMES)
@pytest.mark.parametrize("last_is_one", [0, 1])
@pytest.mark.parametrize("shape", O.TAIL_AXIS, ids=str)
def test_spectrum_tail_axis(shape, last_is_one, name, cross):
    O.check_spectrum_tail_axis(shape, last_is_one, name, cross)


@pytest.mark.parametrize("esz", [4, 8, 16])
@pytest.mark.parametrize("shape,axis", O.GATHER_SHAPES, ids=[str(s) for s, _a in O.GATHER_SHAPES])
def test_gather_axis(shape, axis, esz):
    O.check_gather_axis(shape, axis, esz)


@pytest.mark.parametrize("name", O.NAMES)
@pytest.mark.parametrize("case", O.TABLE_MUL, ids=str)
def test_table_mul(case, name):
    O.check_table_mul(case, name)


@pytest.mark.parametrize("name", O.CNAMES)
def test_angle(name):
    O.check_angle(name)
    O.check_angle_specials(name)


@pytest.mark.parametrize("src", O.NAMES)
@pytest.mark.parametrize("n", O.CONVERT_N)
def test_convert(n, src):
    O.check_convert(n, src)


def test_status_codes():
    O.check_status_codes()


def test_wrapper_errors():
    O.check_wrapper_errors()


def test_the_bounds_are_sensitive():
    O.check_sensitivity()
