"""GPU (-m gpu): the FIR filter's column layout (xrfthip_desc.seg_filter_cols; csrc/fastf.h fastf_kernel<.., true>; xrft_amd.fir_filter along a leading dim)
through the real library on an MI355X.

The plan-level and API-level checks of tests/fir_filter_cols.py (the cases of tests/test_fir_filter_cols_emulated.py); the peak memory, derived: after a warm-up
call, fir_filter of a (2048, 8, 64) float32 cube along time with 65 taps allocates its result (4 MiB) and at most 1 MB more, and with XRFTHIP_FASTW_FILTER_COLS=0 at
least twice the result (the result and the transposed copy); and one case whose input offsets pass 2^31 elements (a sample stride of 2^20), skipped where the card
lacks the 10 GB."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
import extents as E  # noqa: E402
import fir_filter as F  # noqa: E402
import fir_filter_cols as FC  # noqa: E402
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


@pytest.mark.parametrize("case,mode,kind", FC.PLAN_PARAMS, ids=[FC.param_id(p) for p in FC.PLAN_PARAMS])
def test_plan(case, mode, kind):
    FC.check_plan(case, mode, kind)


@pytest.mark.parametrize("mode", FC.MODES)
@pytest.mark.parametrize("case,fewer", FC.PREFIX_CASES, ids=[FC.case_id(c) for c, _ in FC.PREFIX_CASES])
def test_a_shorter_record_has_the_same_bits(case, fewer, mode):
    FC.check_prefix(case, fewer, mode)


@pytest.mark.parametrize("mode", FC.MODES)
@pytest.mark.parametrize("case", FC.GAP_CASES, ids=FC.case_id)
def test_nothing_between_the_columns_or_behind_a_block_is_read(case, mode):
    FC.check_nothing_outside_is_read(case, mode)


@pytest.mark.parametrize("where", [300, 380], ids=["one-segment", "two-segments"])
@pytest.mark.parametrize("mode", ["same", "full"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nonfinite_sample_stays_in_its_column_and_segments(bad, mode, where):
    FC.check_containment(bad, mode, where)


def test_status_codes():
    FC.check_status_codes()


def test_narrow_grids_are_declined_by_default():
    FC.check_narrow_grids_are_declined_by_default()


def test_struct_sizes():
    FC.check_struct_sizes()


def test_no_workspace():
    FC.check_workspace()


@pytest.mark.parametrize("mode", FC.MODES)
@pytest.mark.parametrize("name", sorted(FC.API_CASES))
def test_fir_filter_api(name, mode):
    FC.check_api_case(name, mode)


def test_complex_and_half_precision_data():
    FC.check_api_other_dtypes()


def test_a_refusal_is_remembered_and_the_knobs_arrange():
    FC.check_api_refusal_is_remembered()


def test_peak_memory_is_the_result():
    import scipy.signal

    import xrft_amd as xa

    shape, k = (2048, 8, 64), 65
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)
    da = xa.DataArray(v, ("time", "y", "x"), {"time": np.arange(shape[0]) * 1.0, "y": np.arange(shape[1]), "x": np.arange(shape[2])})
    taps = scipy.signal.firwin(k, 0.2)
    result_bytes = shape[0] * shape[1] * shape[2] * 4

    def peak_of(call):
        res = call()  # warm-up: plans, tables, scratch
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, res

    cols, res = peak_of(lambda: xa.fir_filter(da, "time", taps))
    assert F.filter_plans() and B.newest_plan().seg_filter_cols == 1 and B.newest_plan().seg_stride == 512, B.newest_plan().describe()
    assert res.data.is_contiguous() and res.data.numel() * res.data.element_size() == result_bytes
    with B.env("XRFTHIP_FASTW_FILTER_COLS", 0):
        arranged, res2 = peak_of(lambda: xa.fir_filter(da, "time", taps))
        assert B.newest_plan().seg_filter_cols == 0
    print(f"(2048, 8, 64) float32 along time, K = 65: peak over the resident input {cols} B in columns (result {result_bytes} B), {arranged} B arranged")
    assert cols <= result_bytes + (1 << 20), (cols, result_bytes)
    assert arranged >= 2 * result_bytes  # (the result and the transposed copy)
    assert res.dims == res2.dims and np.array_equal(res.values, res2.values)


def test_input_offsets_beyond_2_to_the_31():
    try:
        FC.run_huge_sample_stride("cuda")
    except E.NeedsMemory as e:
        pytest.skip(str(e))
