"""GPU (-m gpu): isotropic spectra on non-trailing axes where the axes lie -- the per-element radial sums of the fused inner / mid passes
(csrc/fastn.h, fastn_irows_kernel<.., ISO>) on an MI355X against the CPU oracle, with no transposed copy of the input."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import cases  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402

TOL = {"float32": 3e-4, "float64": 1e-10}  # (float32: as test_fastp2_isotropic_vs_oracle)


@pytest.fixture(scope="module", autouse=True)
def real_library():
    from xrft_amd import _lib, api

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    api._plan_cache.clear()
    _lib._state.update(dll=None, path=None, device="cuda")
    _lib.load()  # raises XrftHipUnavailable if the HIP library is missing: no fallback
    assert _lib._state["path"].endswith("libxrft_hip.so") and _lib.device() == "cuda"
    yield
    api._plan_cache.clear()


def _ran_in_place():
    from xrft_amd import api

    d = next(reversed(api._plan_cache.values())).describe()
    return any("[inner layout]" in line and "radial sums" in line for line in d.splitlines())


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_isotropic_spectra_with_the_batch_innermost_without_copies(dtype):
    """isotropic_power_spectrum / isotropic_cross_spectrum over dim = ["y", "x"] of (y, x, t) arrays: after the first call (plan, tables,
    scratch) the only device memory a call allocates is its result -- no transposed copy of the input(s) (11.8 MB each in float32)."""
    import xrft_amd as xa

    shape = (256, 240, 48)
    rng = np.random.default_rng(6)
    v = (rng.standard_normal(shape) + 0.01 * np.arange(shape[0])[:, None, None]).astype(dtype)
    w = (rng.standard_normal(shape) - 0.02 * np.arange(shape[1])[None, :, None]).astype(dtype)
    c = {"y": np.arange(shape[0]) * 0.5, "x": np.arange(shape[1]) * 0.25, "t": np.arange(shape[2]) * 2.0}
    c2 = dict(c, x=c["x"] + 0.375)  # (an offset between the fields: a true-phase factor that is not 1)
    da, db = xa.DataArray(torch.from_numpy(v).cuda(), ("y", "x", "t"), c), xa.DataArray(torch.from_numpy(w).cuda(), ("y", "x", "t"), c2)
    od, ob = o.OArr(v.astype(np.float64), ("y", "x", "t"), c), o.OArr(w.astype(np.float64), ("y", "x", "t"), c2)
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    for fn, ofn, args, oargs in ((xa.isotropic_power_spectrum, o.isotropic_power_spectrum, (da,), (od,)),
                                 (xa.isotropic_cross_spectrum, o.isotropic_cross_spectrum, (da, db), (od, ob))):
        res = fn(*args, **kw)
        assert _ran_in_place()
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = fn(*args, **kw)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        out_bytes = res.data.numel() * res.data.element_size()
        print(f"{fn.__name__} {dtype}: peak {peak} B over the resident set, result {out_bytes} B, one input {v.nbytes} B")
        assert peak <= out_bytes + (1 << 20), (peak, out_bytes)
        assert tuple(res.dims) == ("t", "freq_r")
        cases.check(res, ofn(*oargs, **kw), TOL[dtype])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_isotropic_spectra_with_elements_between_the_axes(dtype):
    """dim = ["t", "x"] of a (t, y, x) = (240, 12, 256) array: the mid layout, every y its own spectrum; repeats bit for bit."""
    import xrft_amd as xa

    shape = (240, 12, 256)
    rng = np.random.default_rng(16)
    v = (rng.standard_normal(shape) + 0.01 * np.arange(shape[0])[:, None, None]).astype(dtype)
    w = rng.standard_normal(shape).astype(dtype)
    c = {"t": np.arange(shape[0]) * 6.0, "y": np.arange(shape[1]) * 1.0, "x": np.arange(shape[2]) * 2.5}
    da, db = xa.DataArray(torch.from_numpy(v).cuda(), ("t", "y", "x"), c), xa.DataArray(torch.from_numpy(w).cuda(), ("t", "y", "x"), c)
    od, ob = o.OArr(v.astype(np.float64), ("t", "y", "x"), c), o.OArr(w.astype(np.float64), ("t", "y", "x"), c)
    for kw in (dict(dim=["t", "x"], detrend="linear", window="hann"), dict(dim=["x", "t"], truncate=True, nfactor=2)):
        got = xa.isotropic_power_spectrum(da, **kw)
        assert _ran_in_place() and tuple(got.dims) == ("y", "freq_r")
        cases.check(got, o.isotropic_power_spectrum(od, **kw), TOL[dtype])
        assert np.array_equal(np.asarray(xa.isotropic_power_spectrum(da, **kw).values), np.asarray(got.values))
        gc = xa.isotropic_cross_spectrum(da, db, **kw)
        assert _ran_in_place()
        cases.check(gc, o.isotropic_cross_spectrum(od, ob, **kw), TOL[dtype])
        assert np.array_equal(np.asarray(xa.isotropic_cross_spectrum(da, db, **kw).values), np.asarray(gc.values))


def test_isotropic_power_spectrum_full_size_1024x1024x64():
    """(1024, 1024, 64) float32 (y, x, t): the oracle on 4 elements, sum conservation against power_spectrum on all, bit-identical repeats."""
    import xrft_amd as xa

    g = torch.Generator(device="cuda").manual_seed(207)
    x = torch.randn((1024, 1024, 64), dtype=torch.float32, device="cuda", generator=g)
    c = {"y": np.arange(1024) * 0.5, "x": np.arange(1024) * 0.25, "t": np.arange(64.0)}
    da = xa.DataArray(x, ("y", "x", "t"), c)
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    got = xa.isotropic_power_spectrum(da, **kw)
    assert _ran_in_place() and tuple(got.dims) == ("t", "freq_r")
    sel = [0, 21, 42, 63]
    ref = o.isotropic_power_spectrum(o.OArr(x[:, :, sel].cpu().numpy().astype(np.float64), ("y", "x", "t"), dict(c, t=c["t"][sel])), **kw)
    gv = got.data.cpu().numpy() if isinstance(got.data, torch.Tensor) else np.asarray(got.values)
    assert np.array_equal(np.asarray(got["freq_r"].values), np.asarray(ref.coord("freq_r")))
    err = np.abs(gv[sel] - ref.values).max() / np.abs(ref.values).max()
    binrel, l1 = cases.fine_errors(gv[sel], ref.values)
    print(f"full size: max rel err {err:.3e}, L1 {l1:.3e}, worst per-bin {binrel:.3e}")
    assert err < 3e-4 and l1 < 3e-4 and binrel < cases.BIN_REL
    ps = xa.power_spectrum(da, **kw)  # (test_xrft.py:963: the radial sums conserve the total, every element)
    np.testing.assert_allclose(gv.sum(axis=-1), ps.data.double().sum(dim=(0, 1)).cpu().numpy(), rtol=1e-5)
    del ps
    for _ in range(2):
        again = xa.isotropic_power_spectrum(da, **kw)
        assert np.array_equal(again.data.cpu().numpy() if isinstance(again.data, torch.Tensor) else np.asarray(again.values), gv)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_nan_stays_in_its_element(dtype):
    """The guarded column pass: a NaN in element 5 of a (y, x, t) array leaves its pair partner (and every other element) finite and the oracle's."""
    import xrft_amd as xa

    shape = (96, 80, 9)
    rng = np.random.default_rng(26)
    v = rng.standard_normal(shape).astype(dtype)
    v[11, 13, 5] = np.nan
    c = {"y": np.arange(shape[0]) * 0.5, "x": np.arange(shape[1]) * 0.25, "t": np.arange(shape[2]) * 2.0}
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    got = xa.isotropic_power_spectrum(xa.DataArray(torch.from_numpy(v).cuda(), ("y", "x", "t"), c), **kw)
    assert _ran_in_place()
    g = got.data.cpu().numpy() if isinstance(got.data, torch.Tensor) else np.asarray(got.values)
    ref = o.isotropic_power_spectrum(o.OArr(v.astype(np.float64), ("y", "x", "t"), c), **kw).values
    keep = np.arange(shape[2]) != 5
    assert np.all(np.isfinite(g[keep])) and np.abs(g[keep] - ref[keep]).max() < TOL[dtype] * np.abs(ref[keep]).max()
    assert np.all(np.isnan(g[5][np.isnan(ref[5])])) and np.isnan(ref[5]).any()
