"""GPU (-m gpu): fft over three axes of real data on the fused route (api._fft_3d_fused; csrc/fasth.h, the field form of the last pass) on an MI355X.

* the odd and the row-straddling shapes of tests/three_axis_fft.py, a (64, 128, 128) float32 and a (30, 90, 72) float64 cube, batch 2: against the oracle on
  one batch entry with and without true-phase factors, the routed plan asserted, two calls bit-identical, the twins the plain conjugates bit for bit without phase
  factors, the Nyquist rows of the twins within the contract with them (where the plain conjugate is not);
* peak memory, derived: after a warm-up call, fft of the (2, 64, 128, 128) float32 cube allocates its result, the half spectrum of the two-axis stage and at
  most 1 MB more (the composition holds two full complex arrays)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import accuracy as A  # noqa: E402
import cases  # noqa: E402
import three_axis_fft as T  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402

DIMS = T.DIMS


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


def _cube(shape, dtype, seed):
    import xrft_amd as xa

    nt, ny, nx = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    tdt = torch.float32 if dtype == "float32" else torch.float64
    v = torch.randn((2,) + tuple(shape), generator=g, device="cuda", dtype=tdt)
    v += 0.02 * torch.arange(ny, device="cuda", dtype=tdt).reshape(1, 1, ny, 1) + 0.01 * torch.arange(nt, device="cuda", dtype=tdt).reshape(1, nt, 1, 1)
    coords = T.coords(shape, 2)  # (origins of t and y that are no multiples of the spacing: the Nyquist phase factor is not real)
    return xa.DataArray(v, DIMS, coords), coords


def _oracle_entry(da, coords, k):
    sub = dict(coords, b=coords["b"][k:k + 1])
    return o.OArr(da.data[k:k + 1].cpu().numpy().astype(np.float64), DIMS, sub)


@pytest.mark.parametrize("shape,dtype", [((9, 5, 7), "float32"), ((9, 5, 7), "float64"), ((12, 7, 16), "float32"), ((12, 7, 16), "float64"),
                                         ((64, 128, 128), "float32"), ((30, 90, 72), "float64")], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_three_axis_fft_against_the_oracle(shape, dtype):
    import xrft_amd as xa

    da, coords = _cube(shape, dtype, 41)
    n = int(np.prod(shape))
    oa = _oracle_entry(da, coords, 1)
    kap = A.kappa(oa.values, o.detrend(oa, ["t", "y", "x"], "linear").values)
    for tp in (False, True):
        kw = dict(dim=["t", "y", "x"], detrend="linear", window="hann", true_phase=tp)
        got = xa.fft(da, **kw)
        assert "[fasth]" in T.newest_plan(), T.newest_plan()
        again = xa.fft(da, **kw)
        assert torch.equal(got.data, again.data)  # no atomics, no sums: the same bits
        ref = o.fft(oa, **kw)
        one = got.isel(b=slice(1, 2))
        cases.check(one, ref, cases.TOL[dtype])
        c = A.assert_accurate(one.values, ref.values, dtype, n, kap, what=f"fft {shape} {dtype} true_phase {tp}")
        print(f"fft {shape} {dtype} true_phase {tp}: rms error {c:.2f} u log2 N")
        g = T.unshifted(np.asarray(got.values), True)
        if not tp:
            sm, tw = T.twin_columns(g)
            assert sm.size and np.array_equal(tw, np.conj(sm))  # the twins: plain conjugates, bit for bit
        elif shape[0] % 2 == 0 or shape[1] % 2 == 0:
            r = T.unshifted(ref.values, True)
            rows, rows_ref = T.nyquist_rows_of_twins(g[1:2]), T.nyquist_rows_of_twins(r)
            A.assert_accurate(rows, rows_ref, dtype, n, kap, what=f"Nyquist rows of the twins {shape} {dtype}")
            plain = np.conj(np.roll(r[..., ::-1, ::-1, ::-1], 1, axis=(-3, -2, -1)))
            with pytest.raises(AssertionError):  # (the plain conjugate of the sample, written there, misses the bound)
                A.assert_accurate(T.nyquist_rows_of_twins(plain), rows_ref, dtype, n, kap)


def test_peak_memory_is_the_result_and_the_half_spectrum():
    import xrft_amd as xa

    da, _ = _cube((64, 128, 128), "float32", 43)
    kw = dict(dim=["t", "y", "x"])
    res = xa.fft(da, **kw)  # warm-up: plans, tables, scratch
    assert "[fasth]" in T.newest_plan()
    del res
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = xa.fft(da, **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    out_bytes = res.data.numel() * res.data.element_size()
    half_spectrum_bytes = 2 * 64 * 128 * 65 * 8
    print(f"fft float32 (2, 64, 128, 128) over three axes: peak {peak} B over the resident set, result {out_bytes} B, half spectrum {half_spectrum_bytes} B")
    assert out_bytes == 2 * 64 * 128 * 128 * 8
    assert peak <= out_bytes + half_spectrum_bytes + (1 << 20), (peak, out_bytes, half_spectrum_bytes)
