"""GPU (-m gpu): power_spectrum / cross_spectrum over three axes on the fused route (csrc/fasth.h) on an MI355X.

* the odd and the row-straddling shapes of tests/test_three_axes_emulated.py, a (64, 128, 128) float32 and a (30, 90, 72) float64 cube, batch 2: POWER and CROSS
  against the oracle on one batch entry, the routed plan asserted, the mirrored half bit for bit;
* two repeated calls return identical bits;
* peak memory, derived: after a warm-up call, power_spectrum of the (2, 64, 128, 128) float32 cube allocates its result, the half spectrum of the two-axis
  stage and nothing else (the composition held two full complex arrays: four times the result)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import accuracy as A  # noqa: E402
import cases  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402

DIMS = ("b", "t", "y", "x")


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


def _newest_plan():
    from xrft_amd import api

    return next(reversed(api._plan_cache.values())).describe()


def _cube(shape, dtype, seed):
    import xrft_amd as xa

    nt, ny, nx = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    tdt = torch.float32 if dtype == "float32" else torch.float64
    v = torch.randn((2,) + tuple(shape), generator=g, device="cuda", dtype=tdt)
    v += 0.02 * torch.arange(ny, device="cuda", dtype=tdt).reshape(1, 1, ny, 1) + 0.01 * torch.arange(nt, device="cuda", dtype=tdt).reshape(1, nt, 1, 1)
    coords = {"b": np.arange(2), "t": np.arange(nt) * 1.0, "y": np.arange(ny) * 0.5, "x": np.arange(nx) * 2.0 + 3.0}
    return xa.DataArray(v, DIMS, coords), coords


def _oracle_entry(da, coords, k):
    sub = dict(coords, b=coords["b"][k:k + 1])
    return o.OArr(da.data[k:k + 1].cpu().numpy().astype(np.float64), DIMS, sub)


@pytest.mark.parametrize("shape,dtype", [((9, 5, 7), "float32"), ((9, 5, 7), "float64"), ((12, 7, 16), "float32"), ((12, 7, 16), "float64"),
                                         ((64, 128, 128), "float32"), ((30, 90, 72), "float64")], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_three_axis_spectra_against_the_oracle(shape, dtype):
    import xrft_amd as xa

    da, coords = _cube(shape, dtype, 31)
    db, _ = _cube(shape, dtype, 32)
    kw = dict(dim=["t", "y", "x"], detrend="linear", window="hann")
    n = int(np.prod(shape))
    oa, ob = _oracle_entry(da, coords, 1), _oracle_entry(db, coords, 1)
    kap = A.kappa(oa.values, o.detrend(oa, kw["dim"], "linear").values)
    nx = shape[2]
    for name in ("power_spectrum", "cross_spectrum"):
        args = (da,) if name == "power_spectrum" else (da, db)
        got = getattr(xa, name)(*args, **kw)
        assert "[fasth]" in _newest_plan(), _newest_plan()
        again = getattr(xa, name)(*args, **kw)
        assert torch.equal(got.data, again.data)  # no atomics, no sums: the same bits
        ref = getattr(o, name)(*((oa,) if name == "power_spectrum" else (oa, ob)), **kw)
        one = got.isel(b=slice(1, 2))
        cases.check(one, ref, cases.TOL[dtype])
        c = A.assert_accurate(one.values, ref.values, dtype, n, kap, what=f"{name} {shape} {dtype}")
        print(f"{name} {shape} {dtype}: rms error {c:.2f} u log2 N")
        g = np.fft.ifftshift(np.asarray(got.values), axes=(-3, -2, -1))
        tw = np.roll(g[..., ::-1, ::-1, ::-1], 1, axis=(-3, -2, -1))
        assert np.array_equal(g[..., 1:nx - nx // 2], np.conj(tw[..., 1:nx - nx // 2]))  # the mirrored half: copies (CROSS: conjugates)


def test_peak_memory_is_the_result_and_the_half_spectrum():
    import xrft_amd as xa

    da, _ = _cube((64, 128, 128), "float32", 33)
    kw = dict(dim=["t", "y", "x"])
    res = xa.power_spectrum(da, **kw)  # warm-up: plans, tables, scratch
    assert "[fasth]" in _newest_plan()
    del res
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = xa.power_spectrum(da, **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    out_bytes = res.data.numel() * res.data.element_size()
    half_spectrum_bytes = 2 * 64 * 128 * 65 * 8
    print(f"power_spectrum float32 (2, 64, 128, 128) over three axes: peak {peak} B over the resident set, result {out_bytes} B, half spectrum {half_spectrum_bytes} B")
    assert out_bytes == 2 * 64 * 128 * 128 * 4
    assert peak <= out_bytes + half_spectrum_bytes + (1 << 20), (peak, out_bytes, half_spectrum_bytes)
