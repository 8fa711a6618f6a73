"""GPU (-m gpu): Welch spectra (xrfthip_desc.seg_hop; csrc/fastw.h) through the real library on an MI355X.

The plan-level and API-level checks of tests/welch.py (the cases of tests/test_welch_emulated.py), and the peak memory, derived: after a warm-up call,
welch_power_spectrum of a (64, 65536) float32 array with 256-sample segments allocates its result (64 KB) and at most 1 MB more over the resident set; the
composed expression allocates at least the 511 spectra of every series."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
import welch as W  # noqa: E402
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
@pytest.mark.parametrize("case", W.CASES + [W.LARGEST], ids=W.case_id)
def test_welch_plan_power(case, form):
    W.check_plan(case, form)


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


@pytest.mark.parametrize("name", sorted(W.API_CASES))
def test_welch_power_spectrum_api(name):
    W.check_api_case(name)


def test_welch_cross_spectrum_and_coherence_api():
    W.check_api_cross_and_coherence()


def test_welch_cross_spectrum_of_descending_coordinates_composes():
    W.check_api_cross_descending()


def test_welch_api_errors():
    W.check_api_errors()


def test_peak_memory_is_the_result():
    import xrft_amd as xa

    ns, n, nperseg = 64, 65536, 256
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((ns, n), generator=g, device="cuda", dtype=torch.float32)
    da = xa.DataArray(v, ("x", "time"), {"x": np.arange(ns), "time": np.arange(n) * 1.0})
    kw = dict(detrend="linear", window="hann")
    result_bytes = ns * nperseg * 4

    def peak_of(call):
        res = call()  # warm-up: plans, tables, scratch
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, res

    fused, res = peak_of(lambda: xa.welch_power_spectrum(da, "time", nperseg, **kw))
    assert B.newest_plan().kernel_info()[0] == L.K_FASTW, B.newest_plan().describe()
    assert res.data.numel() * res.data.element_size() == result_bytes
    composed, res2 = peak_of(lambda: W.composed(da, None, "time", nperseg, nperseg // 2, **kw))
    print(f"(64, 65536) float32, L = 256: peak over the resident set {fused} B fused (result {result_bytes} B), {composed} B composed")
    assert fused <= result_bytes + (1 << 20), (fused, result_bytes)
    assert composed >= ((n - nperseg) // (nperseg // 2) + 1) * result_bytes  # (the assertion above can fail: the composition holds every segment's spectrum)
    assert res.dims == res2.dims and res.values.shape == res2.values.shape
