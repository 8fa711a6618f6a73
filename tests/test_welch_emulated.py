"""Welch spectra (xrfthip_desc.seg_hop; csrc/fastw.h), on the emulated library, and the CPU-only pin of the reference construction to scipy.

Plan level (engine.SpectralPlan, XRFTHIP_K_FASTW asserted): segment lengths 64 .. 4096, hops L, L / 2, 37 and 1, 2 / 3 / 35 (one run) / 36 (two runs) segments, 1 / 3 /
300 series -- plain and with linear detrend + Hann + fftshift, as power and as cross spectra with a phase table, the half output with and without the real-dim
factor -- against the float64 mean of the oracle's spectra of the host's cut, within the bound of tests/welch.py; two executions the same bits; hop = L against
the plain 1-D plan and xrfthip_reduce_axis; ISHIFT_X changes no bit; a NaN stays in its series; a pitch beyond the span and a 4-byte aligned pointer; the status
codes, the struct sizes, the workspace.
API level: welch_power_spectrum / welch_cross_spectrum / welch_coherence against the composed expression (labels exactly, values within the bound), fused where a plan
takes the call and composed elsewhere; float64 against scipy.signal.welch / csd / coherence."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import batch_mean as B  # noqa: E402
import welch as W  # noqa: E402

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
@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_welch_plan_power(case, form):
    W.check_plan(case, form)


@pytest.mark.parametrize("form", W.FORMS)
def test_welch_plan_largest_length(form):
    W.check_plan(W.LARGEST, form)


@pytest.mark.parametrize("case", W.CASES[:2], ids=W.case_id)
def test_welch_plan_constant_detrend(case):
    W.check_plan(case, "constant")


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("case", W.CROSS_CASES, ids=W.case_id)
def test_welch_plan_cross_with_phase_table(case, form):
    W.check_plan(case, form, mode=L.OUT_CROSS, lag=W.CROSS_LAG)


@pytest.mark.parametrize("half", [1, 2])
@pytest.mark.parametrize("case", [W.CASES[1], W.CASES[4]], ids=W.case_id)
def test_welch_plan_half_output(case, half):
    W.check_plan(case, "linear-hann-shift", half=half)
    W.check_plan(case, "plain", mode=L.OUT_CROSS, half=half)


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("case", [W.CASES[0], W.CASES[6]], ids=W.case_id)
def test_no_overlap_is_the_plain_plan_and_reduce_axis(case, form):
    W.check_no_overlap_is_the_plain_plan_and_reduce(case, form)


def test_ishift_changes_no_bit():
    W.check_ishift_changes_no_bit(W.CASES[4])


def test_nan_stays_in_its_series():
    W.check_nan(W.CASES[4])
    W.check_nan(W.CASES[3])


@pytest.mark.parametrize("case", [W.CASES[1], W.CASES[4]], ids=W.case_id)
def test_pitch_beyond_the_span_and_unaligned_pointer(case):
    W.check_pitch_and_padding(case)


def test_status_codes():
    W.check_status_codes()


def test_older_descriptors_still_create_their_plans():
    W.check_older_struct_sizes()


@pytest.mark.parametrize("case", [W.CASES[3], W.CASES[4]], ids=W.case_id)
def test_workspace_is_sufficient_and_checked(case):
    W.check_workspace(case)


# ---------------------------------------------------------------------------------- API level
@pytest.mark.parametrize("name", sorted(W.API_CASES))
def test_welch_power_spectrum_api(name):
    W.check_api_case(name)


def test_welch_cross_spectrum_and_coherence_api():
    W.check_api_cross_and_coherence()


def test_welch_cross_spectrum_of_descending_coordinates_composes():
    W.check_api_cross_descending()


def test_welch_api_errors():
    W.check_api_errors()


# ---------------------------------------------------------------------------------- the reference construction and the API's scaling against scipy (float64, composed route)
def _scipy_series(seed=61):
    rng = np.random.default_rng(seed)
    n = 1000
    x = rng.standard_normal((3, n)) + 0.01 * np.arange(n) + 1.0
    y = np.roll(x, 5, axis=1) + 0.3 * rng.standard_normal((3, n))
    return x, y


@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("detrend", ["constant", "linear"])
def test_float64_welch_is_scipys(detrend, scaling):
    """welch_power_spectrum(window_correction=True, window="hann") on the composed float64 route and the reference construction of tests/welch.py are
    scipy.signal.welch(return_onesided=False) after an fftshift (real_dim: return_onesided=True), to 1e-12 of the peak: two float64 evaluations of 256-point
    transforms differ by about 6e-16, a wrong scaling factor by O(1)."""
    import scipy.signal as ss
    import xrft_amd as xa

    x, _ = _scipy_series()
    dt = 0.5
    crd = {"x": np.arange(3), "time": np.arange(1000) * dt}
    da = xa.DataArray(x, ("x", "time"), crd)
    kw = dict(detrend=detrend, window="hann", window_correction=True, scaling=scaling)
    f, want = ss.welch(x, fs=1 / dt, window="hann", nperseg=256, noverlap=128, detrend=detrend, return_onesided=False, scaling=scaling)
    want = np.fft.fftshift(want, axes=-1)
    got = xa.welch_power_spectrum(da, "time", 256, **kw)
    ref, _ = W.oracle_welch(x, crd, ["x", "time"], "time", 256, 128, **kw)
    assert np.allclose(got["freq_time"].values, np.fft.fftshift(f))
    for name, v in (("api", got.values), ("reference", ref)):
        err = np.abs(v - want).max() / np.abs(want).max()
        print(f"{name} {detrend} {scaling}: {err:.3e} of the peak")
        assert err <= 1e-12
    f1, want1 = ss.welch(x, fs=1 / dt, window="hann", nperseg=256, noverlap=128, detrend=detrend, return_onesided=True, scaling=scaling)
    got1 = xa.welch_power_spectrum(da, "time", 256, real_dim="time", **kw)
    assert np.allclose(got1["freq_time"].values, f1) and np.abs(got1.values - want1).max() / np.abs(want1).max() <= 1e-12
    # trailing samples that do not fill a segment are dropped, and noverlap is honoured
    f2, want2 = ss.welch(x, fs=1 / dt, window="hann", nperseg=200, noverlap=63, detrend=detrend, return_onesided=False, scaling=scaling)
    got2 = xa.welch_power_spectrum(da, "time", 200, 63, **kw)
    assert np.abs(got2.values - np.fft.fftshift(want2, axes=-1)).max() / np.abs(want2).max() <= 1e-12


def test_float64_cross_spectrum_and_coherence_are_scipys():
    """The reference forms F1 conj(F2), scipy.signal.csd(x, y) forms conj(X) Y: welch_cross_spectrum(x, y) = conj(csd(x, y)) = csd(y, x), for coordinates that
    start at 0 (no true-phase factor); the coherence is scipy.signal.coherence."""
    import scipy.signal as ss
    import xrft_amd as xa

    x, y = _scipy_series(62)
    dt = 0.5
    crd = {"x": np.arange(3), "time": np.arange(1000) * dt}
    dx, dy = xa.DataArray(x, ("x", "time"), crd), xa.DataArray(y, ("x", "time"), crd)
    kw = dict(detrend="linear", window="hann", window_correction=True)
    _, want = ss.csd(x, y, fs=1 / dt, window="hann", nperseg=256, noverlap=128, detrend="linear", return_onesided=False)
    want = np.fft.fftshift(want, axes=-1)
    got = xa.welch_cross_spectrum(dx, dy, "time", 256, **kw)
    ref, _ = W.oracle_welch(x, crd, ["x", "time"], "time", 256, 128, y, crd, **kw)
    for name, v in (("api", got.values), ("reference", ref)):
        err = np.abs(v - np.conj(want)).max() / np.abs(want).max()
        print(f"cross {name}: {err:.3e} of the peak")
        assert err <= 1e-12
    _, wyx = ss.csd(y, x, fs=1 / dt, window="hann", nperseg=256, noverlap=128, detrend="linear", return_onesided=False)
    assert np.abs(got.values - np.fft.fftshift(wyx, axes=-1)).max() / np.abs(want).max() <= 1e-12
    _, cwant = ss.coherence(x, y, fs=1 / dt, window="hann", nperseg=256, noverlap=128, detrend="linear")
    coh = xa.welch_coherence(dx, dy, "time", 256, real_dim="time", **kw)
    cerr = np.abs(coh.values - cwant).max()
    print(f"coherence: {cerr:.3e}")
    assert coh.values.dtype == np.float64 and cerr <= 1e-12
