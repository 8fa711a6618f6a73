"""GPU (-m gpu): Welch spectra along a leading axis, read where it lies (xrfthip_desc.seg_stride; the column layout of csrc/fastw.h) through the real library on an
MI355X.

The plan-level and API-level checks of tests/welch_cols.py (the cases of tests/test_welch_cols_emulated.py), and the peak memory, derived: after a warm-up call,
welch_power_spectrum of a (4096, 64, 64) float32 cube over ``time`` with 64-sample segments allocates its result (1 MB) and at most 1 MB more over the resident
set -- no copy of the cube (64 MB)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
import welch as W  # noqa: E402
import welch_cols as WC  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def real_library():
    from xrft_amd import api

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    api.clear_plan_cache()
    L._state.update(dll=None, path=None, device="cuda")
    L.load()  # raises XrftHipUnavailable if the HIP library is missing: no fallback
    assert L._state["path"].endswith("libxrft_hip.so") and L.device() == "cuda"
    with B.every_mean_form():
        yield
    api.clear_plan_cache()


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_id)
def test_column_plan_power(case, form):
    WC.check_plan(case, form)


@pytest.mark.parametrize("case", WC.CONSTANT_CASES, ids=WC.case_id)
def test_column_plan_constant_detrend(case):
    WC.check_plan(case, "constant")


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("case", WC.CROSS_CASES, ids=WC.case_id)
def test_column_plan_cross_with_phase_table(case, form):
    WC.check_plan(case, form, mode=L.OUT_CROSS, lag=W.CROSS_LAG)


@pytest.mark.parametrize("half", [1, 2])
@pytest.mark.parametrize("case", WC.HALF_CASES, ids=WC.case_id)
def test_column_plan_half_output(case, half):
    WC.check_plan(case, "linear-hann-shift", half=half)
    WC.check_plan(case, "plain", mode=L.OUT_CROSS, half=half)


def test_unit_stride_is_the_rows_plan_bit_for_bit():
    WC.check_unit_stride_is_the_rows_plan()


def test_nan_stays_in_its_column():
    WC.check_nan()


def test_gap_and_space_behind_the_span_are_never_read():
    WC.check_gap_is_never_read()


def test_workspace_is_sufficient_and_checked():
    WC.check_workspace()


def test_status_codes():
    WC.check_status_codes()


def test_struct_sizes():
    WC.check_struct_sizes()


@pytest.mark.parametrize("name", sorted(WC.API_CASES))
def test_welch_power_spectrum_in_place(name):
    WC.check_api_case(name)


def test_welch_cross_spectrum_and_coherence_in_place():
    WC.check_api_cross_and_coherence()


def test_float64_long_segments_and_other_views_keep_their_route():
    WC.check_api_not_the_column_plan()


def test_column_blocks_return_the_bits_of_the_whole(monkeypatch):
    WC.check_api_column_blocks(monkeypatch)


def test_peak_memory_is_the_result_not_a_copy_of_the_cube():
    import xrft_amd as xa

    nt, ny, nx, nperseg = 4096, 64, 64, 64
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((nt, ny, nx), generator=g, device="cuda", dtype=torch.float32)
    da = xa.DataArray(v, ("time", "y", "x"), {"time": np.arange(nt) * 1.0, "y": np.arange(ny), "x": np.arange(nx)})
    kw = dict(detrend="linear", window="hann")
    result_bytes = ny * nx * nperseg * 4
    res = xa.welch_power_spectrum(da, "time", nperseg, **kw)  # warm-up: plans, tables, scratch
    del res
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = xa.welch_power_spectrum(da, "time", nperseg, **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    WC.assert_newest_is_column_plan((ny * nx, ny * nx))
    assert res.data.numel() * res.data.element_size() == result_bytes and res.dims == ("y", "x", "freq_time")
    print(f"(4096, 64, 64) float32 over time, nperseg = 64: peak over the resident set {peak} B (result {result_bytes} B, the cube {v.numel() * 4} B)")
    assert peak <= result_bytes + (1 << 20), (peak, result_bytes)
