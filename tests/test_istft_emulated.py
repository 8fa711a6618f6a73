"""The synthesis (xrfthip_desc.seg_synth; csrc/fasto.h; xrft_amd.istft) on the emulated library, and the CPU-only checks of the model and the bound.

The model (tests/istft.py: numpy.fft.irfft of every segment, window, overlap-add, division by the summed squared windows, in float64) is shown to invert the float64
analysis; the bound -- sqrt(R) (b + (R + 2) u) A on the D'-weighted error, b the contract of one transform -- is shown to notice a segment shifted by one sample and
a divisor built from w instead of w^2.
Plan level (engine.SpectralPlan(seg_synth=1), XRFTHIP_K_FASTW and the [fastw overlap-add] line asserted): the cases of tests/istft.py under a boxcar and a Hann
window, within the bound; two executions, a series alone and a shorter run the same bits; the imaginary parts of bins 0 and L / 2 ignored; a pitch with NaN in the
padding; a non-finite bin stays in its own segment's samples; the status codes, the struct sizes, no workspace.
API level: istft(stft(...)) fused, arranged and composed, each within the bound against the model of the library's own stft output; labels; the remembered
refusal; the errors."""
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import istft as I  # noqa: E402
import spectrogram as S  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    api.clear_plan_cache()
    _lib._state.update(dll=None, path=None, device="cuda")


# ---------------------------------------------------------------------------------- the model and the bound (numpy only)
def test_the_model_is_the_inverse():
    I.check_the_model_is_the_inverse()


def test_the_bound_is_sensitive():
    I.check_the_bound_is_sensitive()


# ---------------------------------------------------------------------------------- plan level
@pytest.mark.parametrize("wname", I.WINDOWS, ids=I.win_id)
@pytest.mark.parametrize("case", I.CASES, ids=S.case_id)
def test_plan(case, wname):
    I.check_plan(case, wname)


@pytest.mark.parametrize("wname", I.WINDOWS, ids=I.win_id)
@pytest.mark.parametrize("case,fewer", I.PREFIX_CASES, ids=[S.case_id(c) for c, _ in I.PREFIX_CASES])
def test_a_shorter_run_has_the_same_bits(case, fewer, wname):
    I.check_prefix(case, fewer, wname)


@pytest.mark.parametrize("wname", I.WINDOWS, ids=I.win_id)
@pytest.mark.parametrize("case", [I.CASES[1], I.CASES[4]], ids=S.case_id)
def test_pitch_beyond_the_spectra_with_nan_padding(case, wname):
    I.check_pitch_and_padding(case, wname)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("wname", I.WINDOWS, ids=I.win_id)
def test_a_nonfinite_bin_stays_in_its_segment(wname, bad):
    I.check_containment(wname, bad)


def test_status_codes():
    I.check_status_codes()


def test_struct_sizes():
    I.check_struct_sizes()


def test_no_workspace():
    I.check_workspace()


# ---------------------------------------------------------------------------------- API level
@pytest.mark.parametrize("name", sorted(I.API_CASES))
def test_istft_api(name):
    I.check_api_case(name)


def test_dims_and_coordinates():
    I.check_api_labels()


def test_a_refusal_is_remembered_and_the_knob_composes():
    I.check_api_refusal_is_remembered()


def test_api_errors():
    I.check_api_errors()
