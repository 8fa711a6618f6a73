"""Welch spectra along a leading axis, read where it lies (xrfthip_desc.seg_stride; the column layout of csrc/fastw.h), on the emulated library.

Plan level (engine.SpectralPlan(seg_stride=...), XRFTHIP_K_FASTW and the [fastw columns] line asserted): the cases of tests/welch_cols.py -- one full group of 32
columns, a tail group of one, fewer columns than a group, three groups, the 16- and 8-column groups of L = 256 and 512, one column of a wide grid, 9000 columns; boxes
(S > inner), blocks with a pitch, pinned runs -- plain and with linear detrend + Hann + fftshift, a constant detrend, cross spectra with a phase table, the half
output with and without the real-dim factor, against the oracle's spectra of the host's cut within the bound of tests/welch.py; two executions the same bits; S = 1
is the rows plan bit for bit; a NaN stays in its column; the gap between inner and S and the space behind the span are never read; the workspace; the status codes
and the struct sizes.
API level: welch_power_spectrum / welch_cross_spectrum / welch_coherence over the time axis of (time, y, x), (member, time, y, x) and a sliced (time, x), against
the composed expression (labels exactly) and the oracle (values within the bound), the column plan asserted; what still arranges or composes; column blocks."""
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import batch_mean as B  # noqa: E402
import welch as W  # noqa: E402
import welch_cols as WC  # noqa: E402

L = _lib


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings(), B.every_mean_form():
        warnings.simplefilter("ignore")
        yield
    api.clear_plan_cache()
    _lib._state.update(dll=None, path=None, device="cuda")


# ---------------------------------------------------------------------------------- plan level
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


# ---------------------------------------------------------------------------------- API level
@pytest.mark.parametrize("name", sorted(WC.API_CASES))
def test_welch_power_spectrum_in_place(name):
    WC.check_api_case(name)


def test_welch_cross_spectrum_and_coherence_in_place():
    WC.check_api_cross_and_coherence()


def test_float64_long_segments_and_other_views_keep_their_route():
    WC.check_api_not_the_column_plan()


def test_column_blocks_return_the_bits_of_the_whole(monkeypatch):
    WC.check_api_column_blocks(monkeypatch)
