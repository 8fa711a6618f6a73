"""GPU (-m gpu): the magnitude-squared coherence of two fields (XRFTHIP_OUT_COHERENCE, xrfthip_coherence, xrft_amd.coherence) through the real library on an MI355X.

The checks of tests/coherence.py (the cases of tests/test_coherence_emulated.py), and the peak memory, derived: after a warm-up call, coherence of a (32, 256, 256)
float32 pair allocates its result (256 KB) and at most 1 MB more over the resident set; the composed expression allocates at least three results."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
import coherence as K  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402

_id = lambda v: B.case_id(v) if isinstance(v, tuple) else str(v)  # noqa: E731


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


@pytest.mark.parametrize("name", ["complex64", "complex128"])
@pytest.mark.parametrize("n", K.OP_N)
def test_op(n, name):
    K.check_op(n, name)


@pytest.mark.parametrize("name", ["complex64", "complex128"])
def test_op_zero_denominator(name):
    K.check_op_zero_denominator(name)


def test_op_status_and_wrapper():
    K.check_op_status_and_wrapper()


@pytest.mark.parametrize("name", sorted(K.API_CASES))
def test_coherence_api(name):
    K.check_api_case(name)


def test_name_and_errors():
    K.check_api_name_and_errors()


def test_refused_plan_is_remembered():
    K.check_refused_plan_is_remembered()


def test_peak_memory_is_the_result():
    """The construction of test_gpu_batch_mean.py::test_peak_memory_is_the_result."""
    import xrft_amd as xa

    nt, ny, nx = 32, 256, 256
    g = torch.Generator(device="cuda").manual_seed(7)
    crd = {"time": np.arange(nt), "y": np.arange(ny) * 1.0, "x": np.arange(nx) * 1.0}
    da, da2 = (xa.DataArray(torch.randn((nt, ny, nx), generator=g, device="cuda", dtype=torch.float32), ("time", "y", "x"), crd) for _ in range(2))
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

    fused, res = peak_of(lambda: xa.coherence(da, da2, "time", **kw))
    assert B.ran_mean_form() and B.newest_plan().out_mode == L.OUT_COHERENCE, B.newest_plan().describe()
    assert res.data.numel() * res.data.element_size() == result_bytes
    from xrft_amd import engine
    composed, res2 = peak_of(lambda: engine.coherence(xa.mean_cross_spectrum(da, da2, "time", **kw).data, xa.mean_power_spectrum(da, "time", **kw).data,
                                                      xa.mean_power_spectrum(da2, "time", **kw).data))
    print(f"(32, 256, 256) float32 pair: peak over the resident set {fused} B fused (result {result_bytes} B), {composed} B composed")
    assert fused <= result_bytes + (1 << 20), (fused, result_bytes)
    assert composed >= 3 * result_bytes, (composed, 3 * result_bytes)  # (the assertion above can fail: the composition holds a cross spectrum and two powers)
    assert tuple(res2.shape) == res.values.shape
