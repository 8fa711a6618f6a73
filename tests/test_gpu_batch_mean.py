"""GPU (-m gpu): the mean over the batch inside the last pass (xrfthip_desc.mean_batch; csrc/fasty_mean.h, csrc/fasts_mean.h) through the real library on an MI355X.

The plan-level and API-level checks of tests/batch_mean.py (the cases of tests/test_batch_mean_emulated.py), and the peak memory, derived: after a warm-up call,
mean_power_spectrum of a (32, 256, 256) float32 cube allocates its result (256 KB) and at most 1 MB more over the resident set; power_spectrum(...).mean("time") on
the same input allocates at least the 32 spectra."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
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


@pytest.mark.parametrize("name", sorted(B.API_CASES))
def test_mean_power_spectrum_api(name):
    B.check_api_case(name)


def test_mean_cross_spectrum_api():
    B.check_api_cross()


def test_mean_dim_errors():
    B.check_api_errors()


def test_peak_memory_is_the_result():
    import xrft_amd as xa

    nt, ny, nx = 32, 256, 256
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((nt, ny, nx), generator=g, device="cuda", dtype=torch.float32)
    da = xa.DataArray(v, ("time", "y", "x"), {"time": np.arange(nt), "y": np.arange(ny) * 1.0, "x": np.arange(nx) * 1.0})
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    result_bytes = ny * nx * 4

    def peak_of(call):
        res = call()  # warm-up: plans, tables, scratch
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, res

    fused, res = peak_of(lambda: xa.mean_power_spectrum(da, "time", **kw))
    assert B.ran_mean_form(), B.newest_plan().describe()
    assert res.data.numel() * res.data.element_size() == result_bytes
    composed, res2 = peak_of(lambda: xa.power_spectrum(da, **kw).mean("time"))
    print(f"(32, 256, 256) float32: peak over the resident set {fused} B fused (result {result_bytes} B), {composed} B composed")
    assert fused <= result_bytes + (1 << 20), (fused, result_bytes)
    assert composed >= nt * result_bytes, (composed, nt * result_bytes)  # (the assertion above can fail: the composition holds the 32 spectra)
    assert res.dims == res2.dims and res.values.shape == res2.values.shape
