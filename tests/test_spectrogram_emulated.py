"""Spectrograms (xrfthip_desc.seg_keep; csrc/fastk.h), on the emulated library, and the CPU-only pin of the API's scaling to scipy.

Plan level (engine.SpectralPlan, XRFTHIP_K_FASTW and the [fastw segments kept] line asserted): the cases of tests/spectrogram.py in the rows and in the column layout,
plain and with linear detrend + Hann + fftshift, as power and as complex spectra, a constant detrend and the half outputs -- every (series, segment) against the
oracle's spectrum of the host-cut float64 segment within the contract of one transform; two executions the same bits; a pitch beyond the span and a 4-byte aligned
pointer; ISHIFT_X changes no bit of a power result; hop = L against the plain 1-D plan; a non-finite sample stays in the segments that hold it; the status codes, the
struct sizes, no workspace.
API level: spectrogram / stft against the composed expression (labels exactly) and the oracle (values within the bound), fused where a plan takes the call and composed
elsewhere; scipy.signal.spectrogram."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import spectrogram as S  # noqa: E402

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


# ---------------------------------------------------------------------------------- plan level
@pytest.mark.parametrize("mode", S.MODES, ids=S.mode_id)
@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_plan_rows(case, form, mode):
    S.check_plan(case, form, mode)


@pytest.mark.parametrize("mode", S.MODES, ids=S.mode_id)
@pytest.mark.parametrize("case", S.EXTRA_CASES, ids=S.case_id)
def test_plan_rows_constant_detrend_and_half_output(case, mode):
    S.check_plan(case, "constant", mode)
    S.check_plan(case, "linear-hann-shift", mode, half=1)
    if mode == L.OUT_POWER:
        S.check_plan(case, "linear-hann-shift", mode, half=2)


@pytest.mark.parametrize("mode", S.MODES, ids=S.mode_id)
@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("case", S.COL_CASES, ids=S.case_id)
def test_plan_columns(case, form, mode):
    S.check_col_plan(case, form, mode)


def test_plan_columns_half_output():
    S.check_col_plan(S.COL_CASES[1], "linear-hann-shift", L.OUT_POWER, half=2)
    S.check_col_plan(S.COL_CASES[1], "plain", L.OUT_COMPLEX, half=1)


@pytest.mark.parametrize("mode", S.MODES, ids=S.mode_id)
@pytest.mark.parametrize("case", [S.CASES[1], S.CASES[5]], ids=S.case_id)
def test_pitch_beyond_the_span_and_unaligned_pointer(case, mode):
    S.check_pitch_and_padding(case, mode)


def test_ishift_changes_no_bit_of_a_power_result():
    S.check_ishift_changes_no_bit(S.CASES[5])


@pytest.mark.parametrize("mode", S.MODES, ids=S.mode_id)
@pytest.mark.parametrize("form", S.FORMS)
def test_no_overlap_is_the_plain_plan(form, mode):
    S.check_no_overlap_is_the_plain_plan(S.CASES[0], form, mode)
    S.check_no_overlap_is_the_plain_plan((256, 256, 3, 2), form, mode)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("mode", S.MODES, ids=S.mode_id)
@pytest.mark.parametrize("form", S.FORMS)
def test_a_nonfinite_sample_stays_in_its_segments(form, mode, bad):
    S.check_containment(mode, form, bad)
    S.check_containment_cols(mode, form, bad)


def test_status_codes():
    S.check_status_codes()


def test_struct_sizes():
    S.check_struct_sizes()


def test_no_workspace():
    S.check_workspace()


# ---------------------------------------------------------------------------------- API level
@pytest.mark.parametrize("name", sorted(S.API_CASES))
def test_spectrogram_api(name):
    S.check_api_case(name)


def test_a_refusal_is_remembered_and_the_knob_composes():
    S.check_api_refusal_is_remembered()


def test_dims_and_coordinates():
    S.check_api_labels()


def test_api_errors():
    S.check_api_errors()


# ---------------------------------------------------------------------------------- the API's scaling against scipy
def test_spectrogram_is_scipys():
    """spectrogram(window="hann", detrend="linear", window_correction=True, real_dim=dim) of float32 samples is scipy.signal.spectrogram(..., mode="psd") of their
    float64 image, per segment within the bound of one float32 transform (the fused route)."""
    ss = pytest.importorskip("scipy.signal")
    import torch
    import xrft_amd as xa

    import accuracy as A

    api.clear_plan_cache()
    rng = np.random.default_rng(91)
    n, dt, nperseg = 1000, 0.5, 256
    x = (rng.standard_normal((3, n)) + 0.01 * np.arange(n) + 1.0).astype(np.float32)
    da = xa.DataArray(torch.from_numpy(x).to(L.device()), ("x", "time"), {"x": np.arange(3), "time": np.arange(n) * dt})
    got = xa.spectrogram(da, "time", nperseg, window="hann", detrend="linear", window_correction=True, real_dim="time")
    assert S.keep_plans()
    f, tt, want = ss.spectrogram(x.astype(np.float64), fs=1 / dt, window="hann", nperseg=nperseg, noverlap=nperseg // 2, detrend="linear", mode="psd")
    want = np.moveaxis(want, -1, -2)  # (series, segment, frequency)
    assert got.dims == ("x", "time_segment", "freq_time") and got.values.shape == want.shape
    assert np.allclose(got["freq_time"].values, f)
    assert np.allclose(got["time_segment"].values, tt - dt / 2)  # (scipy: the middle of nperseg sample PERIODS; here the middle of the samples)
    for p in range(want.shape[0]):
        for s in range(want.shape[1]):
            seg = x[p, s * 128:s * 128 + nperseg].astype(np.float64)[None]
            A.assert_accurate(got.values[p, s], want[p, s], "float32", nperseg, A.kappa(seg, A.detrended(seg, (1,), L.DETREND_LINEAR)), what=f"scipy ({p}, {s})")
