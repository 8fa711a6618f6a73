"""GPU (-m gpu): spectrograms (xrfthip_desc.seg_keep; csrc/fastk.h) through the real library on an MI355X.

The plan-level and API-level checks of tests/spectrogram.py (the cases of tests/test_spectrogram_emulated.py), and the peak memory, derived: after a warm-up call,
spectrogram of a (64, 65536) float32 array with 256-sample segments allocates its result (511 spectra per series: 33.5 MB) and at most 1 MB more over the resident
set; the composed expression allocates at least the result plus the copy of the segments (as much again)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
import spectrogram as S  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def real_library():
    from xrft_amd import api

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    api.clear_plan_cache()
    L._state.update(dll=None, path=None, device="cuda")
    L.load()  # raises XrftHipUnavailable if the HIP library is missing: no fallback
    assert L._state["path"].endswith("libxrft_hip.so") and L.device() == "cuda"
    yield
    api.clear_plan_cache()


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


@pytest.mark.parametrize("name", sorted(S.API_CASES))
def test_spectrogram_api(name):
    S.check_api_case(name)


def test_a_refusal_is_remembered_and_the_knob_composes():
    S.check_api_refusal_is_remembered()


def test_dims_and_coordinates():
    S.check_api_labels()


def test_api_errors():
    S.check_api_errors()


def test_peak_memory_is_the_result():
    import xrft_amd as xa

    ns, n, nperseg = 64, 65536, 256
    hop = nperseg // 2
    m = (n - nperseg) // hop + 1
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((ns, n), generator=g, device="cuda", dtype=torch.float32)
    da = xa.DataArray(v, ("x", "time"), {"x": np.arange(ns), "time": np.arange(n) * 1.0})
    kw = dict(detrend="linear", window="hann")
    result_bytes = ns * m * nperseg * 4

    def peak_of(call):
        res = call()  # warm-up: plans, tables, scratch
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, res

    fused, res = peak_of(lambda: xa.spectrogram(da, "time", nperseg, **kw))
    assert S.keep_plans() and B.newest_plan().kernel_info()[0] == L.K_FASTW, B.newest_plan().describe()
    assert res.data.numel() * res.data.element_size() == result_bytes
    composed, res2 = peak_of(lambda: S.composed(da, "time", nperseg, hop, False, **kw))
    print(f"(64, 65536) float32, L = 256: peak over the resident set {fused} B fused (result {result_bytes} B), {composed} B composed")
    assert fused <= result_bytes + (1 << 20), (fused, result_bytes)
    assert composed >= 2 * result_bytes  # (the result and the contiguous copy of the segments, the same size)
    assert res.dims == res2.dims and res.values.shape == res2.values.shape
