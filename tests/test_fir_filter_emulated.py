"""The FIR filter (xrfthip_desc.seg_filter; csrc/fastf.h; xrft_amd.fir_filter) on the emulated library, and the CPU-only checks of the bound.

The model (tests/fir_filter.py) is scipy.signal.convolve(..., method="direct") in float64; the bound -- (2 b + 4 u) Hmax A, b the contract of one transform -- is
shown to hold a float32 restatement of the algorithm far inside and to notice a result shifted by one sample and a dropped last tap.
Plan level (engine.SpectralPlan(seg_filter=1), XRFTHIP_K_FASTW and the [fastw overlap-save] line asserted): the cases of tests/fir_filter.py in the three modes with
seeded normal taps and with scipy.signal.firwin(K, 0.2), within the bound; two executions, a series alone and a shorter series the same bits; the imaginary parts of
entries 0 and L / 2 ignored; a pitch with NaN in the gap; a non-finite sample stays in the segments that hold it; no table is the all-ones table; the status codes,
the struct sizes, no workspace.
API level: fir_filter fused, arranged and composed, each within the bound against the model; float64 composes; labels; the remembered refusal; the errors."""
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import fir_filter as F  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    api.clear_plan_cache()
    _lib._state.update(dll=None, path=None, device="cuda")


# ---------------------------------------------------------------------------------- the bound (numpy and scipy only)
def test_the_bound_is_sensitive():
    F.check_the_bound_is_sensitive()


# ---------------------------------------------------------------------------------- plan level
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


# ---------------------------------------------------------------------------------- API level
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
