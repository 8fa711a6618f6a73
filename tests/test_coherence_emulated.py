"""The magnitude-squared coherence of two fields (XRFTHIP_OUT_COHERENCE: fasty_rows_mean_kernel<NX, 3> and mean_finish_coherence_kernel, csrc/fasty_mean.h;
xrfthip_coherence; xrft_amd.coherence), on the emulated library.  Fields, reference and bound: tests/coherence.py.

Plan level: the two-pass float32 slabs at 256 x 256 and 256 x 512 with groups of slabs that straddle the outputs and 20 slabs in one group, plain and with linear
detrend + Hann + both shifts; runs pinned so that ONE workgroup walks 18 .. 35 slabs; 1024 x 1024; phase tables and a power-of-two scale change no bit; a field with
itself; the fused plan against the composition of the CROSS and POWER mean plans; the workspace; a NaN stays in its own output; the status codes.
The stand-alone operation against long double.  API level: labels of mean_cross_spectrum, values within the bound, fused and composed routes, name, errors."""
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import batch_mean as B  # noqa: E402
import coherence as K  # noqa: E402

_id = lambda v: B.case_id(v) if isinstance(v, tuple) else str(v)  # noqa: E731


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
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("case", B.FASTY, ids=B.case_id)
def test_coherence_plan(case, form):
    K.check_plan(case, form)


@pytest.mark.parametrize("case,runs,run", B.LONG_FASTY, ids=_id)
def test_long_runs(case, runs, run):
    """ONE workgroup walks 18 .. 35 slabs of an output: full float32 chains of 16, both staging rounds between slabs, partials added to."""
    K.check_plan(case, "linear-hann-shift", runs=runs, run_len=run)


@pytest.mark.parametrize("case", B.LARGE_FASTY, ids=B.case_id)
def test_row_kernels_above_512_points(case):
    K.check_plan(case, "linear-hann-shift")


@pytest.mark.parametrize("form", B.FORMS)
def test_phase_tables_and_power_of_two_scale_change_no_bit(form):
    K.check_invariance(B.FASTY[0], form)


@pytest.mark.parametrize("form", B.FORMS)
def test_a_field_with_itself_is_coherent(form):
    K.check_identical_fields(B.FASTY[0], form)


@pytest.mark.parametrize("case", [B.FASTY[0], B.FASTY[1]], ids=B.case_id)
def test_fused_plan_against_the_three_mean_plans(case):
    K.check_against_existing_forms(case, "linear-hann-shift")


@pytest.mark.parametrize("case", [B.FASTY[0], B.FASTY[2]], ids=B.case_id)
def test_workspace(case):
    K.check_workspace(case, "linear-hann-shift")


def test_nan_stays_in_its_output():
    K.check_nan(B.FASTY[0])


def test_status_codes():
    K.check_status_codes()


def test_exec_needs_two_fields():
    K.check_exec_needs_two_fields()


# ---------------------------------------------------------------------------------- the stand-alone operation
@pytest.mark.parametrize("name", ["complex64", "complex128"])
@pytest.mark.parametrize("n", K.OP_N)
def test_op(n, name):
    K.check_op(n, name)


@pytest.mark.parametrize("name", ["complex64", "complex128"])
def test_op_zero_denominator(name):
    K.check_op_zero_denominator(name)


def test_op_status_and_wrapper():
    K.check_op_status_and_wrapper()


# ---------------------------------------------------------------------------------- API level
@pytest.mark.parametrize("name", sorted(K.API_CASES))
def test_coherence_api(name):
    K.check_api_case(name)


def test_name_and_errors():
    K.check_api_name_and_errors()


def test_refused_plan_is_remembered():
    K.check_refused_plan_is_remembered()
