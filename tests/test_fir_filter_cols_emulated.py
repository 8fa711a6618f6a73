"""The FIR filter's column layout (xrfthip_desc.seg_filter_cols; csrc/fastf.h fastf_kernel<.., true>; xrft_amd.fir_filter along a leading dim) on the emulated
library.

Plan level (engine.SpectralPlan(seg_filter=1, seg_filter_cols=1, seg_stride=S, inner=..), XRFTHIP_K_FASTW, the [fastw overlap-save] and [fastw columns] lines
asserted): the cases of tests/fir_filter_cols.py in the three modes with seeded normal taps and with scipy.signal.firwin(K, 0.2), within the bound of
tests/fir_filter.py against its float64 model, and bit for bit the rows plan on the transposed contiguous copy; a second execution, a column run alone and a shorter
record the same bits; NaN between the columns and behind the blocks never read; a non-finite sample stays in its own column and its segments; the status codes, the
struct sizes, no workspace.
API level: fir_filter along a leading dim through the column plan -- contiguous, within the bound, labels and bits of the call with XRFTHIP_FASTW_FILTER_COLS=0 --
and arranged or composed where the case says so; complex and half precision data; the remembered refusal."""
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import fir_filter_cols as FC  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    api.clear_plan_cache()
    _lib._state.update(dll=None, path=None, device="cuda")


# ---------------------------------------------------------------------------------- plan level
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


# ---------------------------------------------------------------------------------- API level
@pytest.mark.parametrize("mode", FC.MODES)
@pytest.mark.parametrize("name", sorted(FC.API_CASES))
def test_fir_filter_api(name, mode):
    FC.check_api_case(name, mode)


def test_complex_and_half_precision_data():
    FC.check_api_other_dtypes()


def test_a_refusal_is_remembered_and_the_knobs_arrange():
    FC.check_api_refusal_is_remembered()
