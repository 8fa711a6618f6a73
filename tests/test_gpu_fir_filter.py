"""GPU (-m gpu): the FIR filter (xrfthip_desc.seg_filter; csrc/fastf.h; xrft_amd.fir_filter) through the real library on an MI355X.

The plan-level and API-level checks of tests/fir_filter.py (the cases of tests/test_fir_filter_emulated.py), and the peak memory, derived: after a warm-up call,
fir_filter of (64, 65536) float32 series with 65 taps allocates its result (64 x 65536 float32: 16.8 MB) and at most 1 MB more over the resident input; the composed
route allocates at least the unfolded segments besides (more than the result)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
import fir_filter as F  # noqa: E402
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


@pytest.mark.parametrize("case,mode,kind", F.PLAN_PARAMS, ids=[F.param_id(p) for p in F.PLAN_PARAMS])
def test_plan(case, mode, kind):
    F.check_plan(case, mode, kind)


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("case,fewer", F.PREFIX_CASES, ids=[F.case_id(c) for c, _ in F.PREFIX_CASES])
def test_a_shorter_series_has_the_same_bits(case, fewer, mode):
    F.check_prefix(case, fewer, mode)


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("case", F.PITCH_CASES, ids=F.case_id)
def test_pitch_beyond_the_series_with_nan_in_the_gap(case, mode):
    F.check_pitch_and_gap(case, mode)


@pytest.mark.parametrize("where", [300, 380], ids=["one-segment", "two-segments"])
@pytest.mark.parametrize("mode", ["same", "full"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nonfinite_sample_stays_in_its_segments(bad, mode, where):
    F.check_containment(bad, mode, where)


def test_no_table_is_the_all_ones_table():
    F.check_no_table_is_ones()


def test_status_codes():
    F.check_status_codes()


def test_struct_sizes():
    F.check_struct_sizes()


def test_no_workspace():
    F.check_workspace()


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("name", sorted(F.API_CASES))
def test_fir_filter_api(name, mode):
    F.check_api_case(name, mode)


def test_dims_and_coordinates():
    F.check_api_labels()


def test_a_refusal_is_remembered_and_the_knob_composes():
    F.check_api_refusal_is_remembered()


def test_api_errors():
    F.check_api_errors()


def test_the_default_nfft_rule_and_the_longest_taps():
    F.check_default_nfft()


def test_a_sliced_view_is_read_where_it_lies():
    F.check_api_sliced_view()


def test_complex_and_half_precision_data():
    F.check_other_dtypes()


def test_peak_memory_is_the_result():
    import scipy.signal

    import xrft_amd as xa

    ns, n, k = 64, 65536, 65
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((ns, n), generator=g, device="cuda", dtype=torch.float32)
    da = xa.DataArray(v, ("x", "time"), {"x": np.arange(ns), "time": np.arange(n) * 1.0})
    taps = scipy.signal.firwin(k, 0.2)
    result_bytes = ns * n * 4

    def peak_of(call):
        res = call()  # warm-up: plans, tables, scratch
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, res

    fused, res = peak_of(lambda: xa.fir_filter(da, "time", taps))
    assert F.filter_plans() and B.newest_plan().kernel_info()[0] == L.K_FASTW, B.newest_plan().describe()
    assert res.data.numel() * res.data.element_size() == result_bytes
    with B.env("XRFTHIP_FASTW_FILTER", 0):
        composed, res2 = peak_of(lambda: xa.fir_filter(da, "time", taps))
    print(f"(64, 65536) float32, K = 65: peak over the resident input {fused} B fused (result {result_bytes} B), {composed} B composed")
    assert fused <= result_bytes + (1 << 20), (fused, result_bytes)
    assert composed >= 2 * result_bytes  # (the result and the unfolded segments, L / V times its size)
    assert res.dims == res2.dims and res.values.shape == res2.values.shape
