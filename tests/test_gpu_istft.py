"""GPU (-m gpu): the synthesis (xrfthip_desc.seg_synth; csrc/fasto.h; xrft_amd.istft) through the real library on an MI355X.

The plan-level and API-level checks of tests/istft.py (the cases of tests/test_istft_emulated.py); one case whose offsets pass 2^31 elements on both sides
(L = 64, hop 32, 2047 segments, 33 000 series: 2.16e9 output samples, 2.2e9 input elements filled on the device), its first and last series bit-equal to the same
series run alone; and the peak memory, derived: after a warm-up call, istft of (64, 511, 129) complex64 spectra with 256-sample segments allocates its result
(64 x 65536 float32: 16.8 MB) and at most 1 MB more over the resident set; the composed route allocates at least the inverse-transformed segments besides (twice the
result)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import batch_mean as B  # noqa: E402
import istft as I  # noqa: E402
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


def test_the_bound_is_sensitive():
    I.check_the_bound_is_sensitive()


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


@pytest.mark.parametrize("name", sorted(I.API_CASES))
def test_istft_api(name):
    I.check_api_case(name)


def test_dims_and_coordinates():
    I.check_api_labels()


def test_a_refusal_is_remembered_and_the_knob_composes():
    I.check_api_refusal_is_remembered()


def test_api_errors():
    I.check_api_errors()


def test_offsets_beyond_2_to_31_elements():
    """L = 64, hop 32, M = 2047, P = 33 000: series p's spectra start at element p * 67551 (2.2e9 in all) and its samples at p * 65536 (2.16e9): the last series and
    series 0 have the bits of the same series run alone in a one-series plan."""
    l, h, m, p = 64, 32, 2047, 33000
    nb = l // 2 + 1
    span = (m - 1) * h + l
    assert p * m * nb > 2 ** 31 and p * span > 2 ** 31
    torch.cuda.empty_cache()  # (blocks that earlier tests left in torch's cache count as used)
    free = torch.cuda.mem_get_info()[0]
    if free < 40 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.0f} GB free on the device: the case holds 17.8 GB of spectra and 8.7 GB of samples and asks for 40 GB")
    g = torch.Generator(device="cuda").manual_seed(11)
    base = torch.randn((m, nb, 2), generator=g, device="cuda", dtype=torch.float32)
    amp = 1.0 + (torch.arange(p, device="cuda", dtype=torch.float32) % 7)  # (series differ: one stored under another's index does not pass)
    spec = torch.empty((p, m, nb), dtype=torch.complex64, device="cuda")
    torch.mul(base.reshape(1, m, nb * 2), amp.reshape(p, 1, 1), out=torch.view_as_real(spec).reshape(p, m, nb * 2))
    plan = I.make_plan((l, h, m, p), "hann")
    I.assert_synth_plan(plan)
    out, _ = plan.execute(spec)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (p, span)
    one = I.make_plan((l, h, m, 1), "hann")
    for k in (0, p - 1):
        alone, _ = one.execute(spec[k:k + 1])
        assert torch.equal(out[k], alone[0]), k
        assert bool(torch.isfinite(alone).all()) and float(alone.abs().max()) > 0
    # ... and against the model, the last series
    ref, dp, a = I.model(spec[p - 1:].cpu().numpy(), l, h, I.window("hann", l), 1.0 / l)
    I.assert_within("the last of 33 000 series", out[p - 1:].cpu().numpy(), ref, dp, l, h, a)


def test_peak_memory_is_the_result():
    import xrft_amd as xa

    ns, n, nperseg = 64, 65536, 256
    hop = nperseg // 2
    m = (n - nperseg) // hop + 1
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((ns, n), generator=g, device="cuda", dtype=torch.float32)
    da = xa.DataArray(v, ("x", "time"), {"x": np.arange(ns), "time": np.arange(n) * 1.0})
    kw = dict(window="hann", real_dim="time")
    st = xa.stft(da, "time", nperseg, **kw)
    del da, v
    result_bytes = ns * n * 4
    segment_bytes = ns * m * nperseg * 4

    def peak_of(call):
        res = call()  # warm-up: plans, tables, scratch
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, res

    fused, res = peak_of(lambda: xa.istft(st, "time", **kw))
    assert I.synth_plans() and B.newest_plan().kernel_info()[0] == L.K_FASTW, B.newest_plan().describe()
    assert res.data.numel() * res.data.element_size() == result_bytes
    with B.env("XRFTHIP_FASTW_SYNTH", 0):
        composed, res2 = peak_of(lambda: xa.istft(st, "time", **kw))
    print(f"(64, 511, 129) complex64, L = 256: peak over the resident set {fused} B fused (result {result_bytes} B), {composed} B composed")
    assert fused <= result_bytes + (1 << 20), (fused, result_bytes)
    assert composed >= result_bytes + segment_bytes  # (the result and the inverse-transformed segments, twice its size)
    assert res.dims == res2.dims and res.values.shape == res2.values.shape
