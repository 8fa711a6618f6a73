"""GPU (-m gpu): reuse of a field's column pass across spectral products on an MI355X -- the scenarios of tests/column_reuse.py on the real libxrft_hip.so:
cross_spectrum(a, b) then isotropic_power_spectrum(a), (b) launch the column pass twice, not four times; every result is bit-identical to the same call with
reuse off; one sequence is held to the oracle."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import cases  # noqa: E402
import column_reuse as R  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def real_library():
    from xrft_amd import api, engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    api.clear_plan_cache()
    L._state.update(dll=None, path=None, device="cuda")
    L.load()  # raises XrftHipUnavailable if the HIP library is missing: no fallback
    assert L._state["path"].endswith("libxrft_hip.so") and L.device() == "cuda"
    yield
    engine.reuse_column_pass(True)
    api.clear_plan_cache()


def _against_oracle(ta, tb, coords, got):
    oa, ob = (o.OArr(t.cpu().numpy().astype(np.float64), R.DIMS, coords) for t in (ta, tb))
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


@pytest.mark.parametrize("shape", R.SHAPES, ids=["256x256", "512x256"])
def test_another_stream(shape):
    R.other_stream(shape)


def test_c_abi():
    R.c_abi_errors()
