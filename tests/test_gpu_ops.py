"""GPU (-m gpu): the stand-alone C-ABI operations (csrc/ops.cpp, csrc/aux_kernels.h) through the real library on an MI355X, held to the rounding-level bounds of
tests/ops.py against plain high-precision numpy -- the checks of tests/test_ops_emulated.py, with the heavy cases (a second launch of a batch loop, a wrapped grid)
in every dtype and kind.  What only the GPU shows: a missing barrier, the 64-lane shuffle tree of finalize_coef_kernel, the device's atan2 and its conversions."""
import warnings

import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import ops as O  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def real_library():
    from xrft_amd import api

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    api.clear_plan_cache()
    L._state.update(dll=None, path=None, device="cuda")
    L.load()  # raises XrftHipUnavailable if the HIP library is missing: no fallback
    assert L._state["path"].endswith("libxrft_hip.so") and L.device() == "cuda"
    yield
    api.clear_plan_cache()


@pytest.mark.parametrize("case,name,kind", O.detrend_params(O.DETREND))
def test_detrend(case, name, kind):
    O.check_detrend(case, name, kind)


@pytest.mark.parametrize("case,name,kind", O.detrend_params(O.DETREND3))
def test_detrend3(case, name, kind):
    O.check_detrend3(case, name, kind)


@pytest.mark.parametrize("case,name,kind", O.detrend_params(O.INNER))
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
