"""The mean over the batch inside the last pass (xrfthip_desc.mean_batch; csrc/fasty_mean.h, csrc/fasts_mean.h), on the emulated library.

Plan level (engine.SpectralPlan, the kernel kind asserted): the two-pass float32 slabs at 256 x 256 and 256 x 512 with groups of slabs that straddle the outputs and
with a chain longer than 16 terms, the one-pass slabs at 64 x 64, 64 x 128 and 128 x 128 -- each plain and with linear detrend + Hann + both shifts, the two-pass slabs
also as a cross spectrum with a phase table -- against the float64 mean of the oracle's spectra within the bound of tests/batch_mean.py; M = 1 and doubled slabs
bit-identical to the plain plan; two executions the same bits; a NaN stays in its own output; the status codes; the workspace.
API level: mean_power_spectrum / mean_cross_spectrum against power_spectrum(...).mean(...): labels exactly, values within the bound, fused where the issue says so and
composed elsewhere."""
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import batch_mean as B  # noqa: E402


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
@pytest.mark.parametrize("case", B.FASTY + B.FASTS, ids=B.case_id)
def test_mean_plan_power(case, form):
    B.check_power_plan(case, form)


@pytest.mark.parametrize("case", [B.FASTY[0], B.FASTY[2]], ids=B.case_id)
def test_mean_plan_cross_with_phase_table(case):
    B.check_cross_plan(case)


@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("case,runs,run", B.LONG_FASTY + B.LONG_FASTS, ids=lambda v: B.case_id(v) if isinstance(v, tuple) else str(v))
def test_long_runs_power(case, runs, run, form):
    """ONE workgroup walks 18 .. 37 slabs of an output: full float32 chains of 16, flushes between slabs, partials added to."""
    B.check_power_plan(case, form, runs=runs, run_len=run)


@pytest.mark.parametrize("case,runs,run", B.LONG_FASTY, ids=lambda v: B.case_id(v) if isinstance(v, tuple) else str(v))
def test_long_runs_cross(case, runs, run):
    B.check_cross_plan(case, runs=runs, run_len=run)


@pytest.mark.parametrize("case", B.LARGE_FASTY, ids=B.case_id)
def test_row_kernels_above_512_points(case):
    B.check_power_plan(case, "linear-hann-shift")
    B.check_cross_plan(case)


@pytest.mark.parametrize("case", [B.FASTY[1], B.FASTS[0], B.FASTS[5]], ids=B.case_id)  # (256 x 512: the plain plan of a 256 x 256 power spectrum is the one-pass kernel, other roundings)
def test_m1_is_the_plain_plan_and_doubled_slabs_are_exact(case):
    B.check_bit_identities(case)


@pytest.mark.parametrize("case", [B.FASTY[0], B.FASTS[2]], ids=B.case_id)
def test_nan_stays_in_its_output(case):
    B.check_nan(case)


def test_status_codes():
    B.check_status_codes()


def test_default_routing_keeps_the_classes_that_measured_faster():
    B.check_default_routing()


def test_older_descriptors_still_create_their_plans():
    B.check_older_struct_sizes()


# ---------------------------------------------------------------------------------- API level
@pytest.mark.parametrize("name", sorted(B.API_CASES))
def test_mean_power_spectrum_api(name):
    B.check_api_case(name)


def test_mean_cross_spectrum_api():
    B.check_api_cross()


def test_mean_dim_errors():
    B.check_api_errors()
