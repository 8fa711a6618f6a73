"""Multitaper spectra (xrfthip_desc.seg_tapers; csrc/fastt.h; xrft_amd.multitaper_*) on the emulated library, and the CPU-only checks of the comparison.

The reference (tests/multitaper.py) is float64 numpy with scipy's DPSS; the bound is the contract of one mean spectrum, batch_mean.bound(1, L, kappa), per series.
Plan level (engine.SpectralPlan(seg_tapers=K, seg_taper_len=N), XRFTHIP_K_FASTW, the [fastw tapers] line and no workspace asserted): the cases of tests/multitaper.py
in the forms plain, constant and linear + shift, within the bound; CROSS with a phase table; the half output with and without the real-dim factor; eigenvalue
weights; two executions, and every series run alone, the same bits; ISHIFT_X changes no bit; a NaN stays in its own series; a pitch and a 4-byte pointer; the status
codes, the struct sizes.
API level: the three functions against the composed route (XRFTHIP_FASTW_TAPERS=0) -- labels exactly, values within the bound -- and against the numpy / scipy
definition; float64 to 1e-12; Parseval; a leading dim; the library's DPSS against scipy's; the errors."""
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import multitaper as M  # noqa: E402

L = _lib


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    api.clear_plan_cache()
    _lib._state.update(dll=None, path=None, device="cuda")


# ---------------------------------------------------------------------------------- the comparison itself (numpy and scipy only)
def test_the_checker_bites():
    M.check_the_checker_bites()


def test_the_library_dpss_is_scipys():
    M.check_dpss_against_scipy()


# ---------------------------------------------------------------------------------- plan level
@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_plan(case, form):
    M.check_plan(case, form)


@pytest.mark.parametrize("case", M.CROSS_CASES, ids=M.case_id)
def test_cross_plan_with_a_phase_table(case):
    M.check_plan(case, "linear-shift", L.OUT_CROSS, lag=M.CROSS_LAG)


@pytest.mark.parametrize("half", [1, 2], ids=["half", "real-dim"])
@pytest.mark.parametrize("case", M.HALF_CASES, ids=M.case_id)
def test_half_output(case, half):
    M.check_plan(case, "constant", half=half)
    M.check_plan(case, "constant", L.OUT_CROSS, lag=M.CROSS_LAG, half=half)


@pytest.mark.parametrize("case", [(64, 50, 3, 3), (2048, 2048, 8, 2)], ids=M.case_id)
def test_eigenvalue_weights(case):
    M.check_plan(case, "linear-shift", weights="eigen")


@pytest.mark.parametrize("case", M.ALONE_CASES, ids=M.case_id)
def test_every_series_equals_the_series_run_alone(case):
    M.check_every_series_alone(case)


def test_ishift_changes_no_bit():
    M.check_ishift_changes_no_bit((64, 50, 3, 3))


def test_a_nan_stays_in_its_own_series():
    M.check_nan((64, 50, 3, 3))


@pytest.mark.parametrize("case", [(64, 50, 3, 3), (1024, 1000, 7, 2)], ids=M.case_id)
def test_pitch_beyond_the_series_and_a_4_byte_pointer(case):
    M.check_pitch_and_pointer(case)


def test_status_codes():
    M.check_status_codes()


def test_struct_sizes():
    M.check_struct_sizes()


# ---------------------------------------------------------------------------------- API level
@pytest.mark.parametrize("name", sorted(M.API_CASES))
def test_multitaper_power_spectrum_api(name):
    M.check_api_case(name)


def test_cross_spectrum_and_coherence():
    M.check_api_cross_and_coherence()


def test_float64_against_the_definition():
    M.check_float64_against_the_definition()


def test_parseval():
    M.check_parseval()


def test_a_leading_dim_equals_the_trailing_call():
    M.check_leading_dim_equals_trailing()


def test_given_tapers_and_half_precision():
    M.check_api_tapers_argument_and_half_precision()


def test_a_refusal_is_remembered_and_composes():
    M.check_api_refusal_is_remembered()


def test_api_errors():
    M.check_api_errors()


def test_the_functions_are_public():
    import xrft_amd as xa

    for name in ("multitaper_power_spectrum", "multitaper_cross_spectrum", "multitaper_coherence"):
        assert callable(getattr(xa, name)) and name in xa.__all__ and name in api.__all__
    assert "xrfthip_plan_set_tapers" in _lib.EXPORTS
