"""GPU (-m gpu): multitaper spectra (xrfthip_desc.seg_tapers; csrc/fastt.h; xrft_amd.multitaper_*) through the real library on an MI355X.

The plan-level and API-level checks of tests/multitaper.py (the cases of tests/test_multitaper_emulated.py); one case whose second series lies beyond 2^31 elements
(two series at a pitch of 2^31 + 64 in an uninitialised 8.6 GB buffer, L = 64) equals the dense case bit for bit; and the peak memory, derived: after a warm-up call,
multitaper_power_spectrum of a (4096, 1024) float32 array with K = 7 allocates its result (16.8 MB) and at most 1 MB more over the resident input; the composed route
allocates at least K times the input."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
import multitaper as M  # noqa: E402
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


def test_a_series_beyond_2_to_the_31_elements():
    """Two series at a pitch of 2^31 + 64 samples: the second one's offset does not fit 32 bits.  The buffer is never initialised beyond the two series."""
    case = (64, 50, 3, 2)
    pitch = (1 << 31) + 64
    x = M.series(case)
    want = M.run(M.make_plan(case, "linear-shift"), x)
    buf = torch.empty(pitch + 64, dtype=torch.float32, device="cuda")
    view = torch.as_strided(buf, (2, 50), (pitch, 1))
    view.copy_(torch.from_numpy(x).to("cuda"))
    plan = M.make_plan(case, "linear-shift", pitch=pitch)
    assert M.is_taper_plan(plan)
    out, _ = plan.execute(view)
    assert np.array_equal(out.cpu().numpy(), want)
    x1 = M.second_series(x)
    buf1 = torch.empty(pitch + 64, dtype=torch.float32, device="cuda")
    view1 = torch.as_strided(buf1, (2, 50), (pitch, 1))
    view1.copy_(torch.from_numpy(x1).to("cuda"))
    wantc = M.run(M.make_plan(case, "linear-shift", L.OUT_CROSS, lag=M.CROSS_LAG), x, x1)
    outc, _ = M.make_plan(case, "linear-shift", L.OUT_CROSS, lag=M.CROSS_LAG, pitch=pitch).execute(view, view1)
    assert np.array_equal(outc.cpu().numpy(), wantc)


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


def test_peak_memory_is_the_result():
    import xrft_amd as xa

    ns, n, k = 4096, 1024, 7
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((ns, n), generator=g, device="cuda", dtype=torch.float32)
    da = xa.DataArray(v, ("x", "time"), {"x": np.arange(ns), "time": np.arange(n) * 1.0})
    result_bytes = ns * n * 4
    input_bytes = ns * n * 4

    def peak_of(call):
        res = call()  # warm-up: plans, tables, scratch
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, res

    fused, res = peak_of(lambda: xa.multitaper_power_spectrum(da, "time", K=k))
    assert M.taper_plans() and M.is_taper_plan(M.taper_plans()[-1]), B.newest_plan().describe()
    assert res.data.numel() * res.data.element_size() == result_bytes
    with B.env("XRFTHIP_FASTW_TAPERS", 0):
        composed, res2 = peak_of(lambda: xa.multitaper_power_spectrum(da, "time", K=k))
    print(f"(4096, 1024) float32, K = 7: peak over the resident input {fused} B fused (result {result_bytes} B), {composed} B composed")
    assert fused <= result_bytes + (1 << 20), (fused, result_bytes)
    assert composed >= k * input_bytes  # (the K tapered copies, at least)
    assert res.dims == res2.dims and res.values.shape == res2.values.shape
