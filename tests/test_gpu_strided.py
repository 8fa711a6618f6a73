"""GPU (-m gpu): input strides in the plan descriptor on an MI355X -- a box cut out of a larger field is transformed where it lies.

* no copy: after a warm-up call, power_spectrum of a box of a larger device array allocates its result and nothing else (the contiguous copy of the
  box was 256 MB at the float32 shape), meets the oracle on one slab, and equals the result for ``box.contiguous()`` bit for bit;
* every family taught to read strided input, at GPU-sized rows of the table of tests/accuracy.py: the strided plan on a box in a buffer of NaN against
  the dense plan on the contiguous copy, bit for bit (tests/strided.py) -- a 4096^2 FastY slab at pitch 8192 and 65 536-sample FastR rows with a batch
  stride among them."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import accuracy as A  # noqa: E402
import cases  # noqa: E402
import strided as S  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402
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


def _newest_plan():
    from xrft_amd import api

    return next(reversed(api._plan_cache.values())).describe()


@pytest.mark.parametrize("dtype,parent,ys,xs,tag", [
    ("float32", (16, 4096, 4096), slice(1024, 3072), slice(1024, 3072), "[fasty]"),
    ("float64", (32, 1440, 720), slice(360, 1080), slice(180, 540), "[fastm]"),
], ids=["f32-2048x2048-of-4096x4096", "f64-720x360-of-1440x720"])
def test_power_spectrum_of_a_box_without_a_copy(dtype, parent, ys, xs, tag):
    import xrft_amd as xa

    tdt = torch.float32 if dtype == "float32" else torch.float64
    g = torch.Generator(device="cuda").manual_seed(12)
    nt, ny, nx = parent
    big = torch.randn(parent, generator=g, device="cuda", dtype=tdt)
    big += 0.01 * torch.arange(ny, device="cuda", dtype=tdt).reshape(1, ny, 1)
    coords = {"t": np.arange(nt) * 1.0, "y": np.arange(ny) * 0.5, "x": np.arange(nx) * 0.25}
    box = xa.DataArray(big, ("t", "y", "x"), coords).isel(y=ys, x=xs)
    assert not box.data.is_contiguous() and box.data.data_ptr() % 16 == 0
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    res = xa.power_spectrum(box, **kw)  # warm-up: plan, tables, scratch
    d = _newest_plan()
    assert tag in d and f"in pitch {nx} / slab {ny * nx}" in d, d
    del res
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = xa.power_spectrum(box, **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    out_bytes = res.data.numel() * res.data.element_size()
    box_bytes = box.data.numel() * box.data.element_size()
    print(f"power_spectrum {dtype} {tuple(box.data.shape)} of {parent}: peak {peak} B over the resident set, result {out_bytes} B, the box {box_bytes} B")
    assert peak <= out_bytes + (1 << 20), (peak, out_bytes)
    # one slab against the oracle
    k = nt // 2
    sub = {"t": coords["t"][k:k + 1], "y": coords["y"][ys], "x": coords["x"][xs]}
    ref = o.power_spectrum(o.OArr(box.data[k:k + 1].cpu().numpy().astype(np.float64), ("t", "y", "x"), sub), **kw)
    got = res.isel(t=slice(k, k + 1))
    cases.check(got, ref, cases.TOL[dtype])
    # ... and the dense plan on the contiguous copy: the same bits
    out = res.data
    del res, got
    dense = xa.power_spectrum(xa.DataArray(box.data.contiguous(), box.dims, box.coords), **kw)
    assert "in pitch" not in _newest_plan()
    assert torch.equal(out, dense.data)


# (family, row of the table of tests/accuracy.py, the box's extra pitch in elements, batch)
GPU_ROWS = [
    ("FastY", "fasty", 4096, 2),          # a 4096^2 slab at pitch 8192
    ("FastY", "fasty-cross", 8, 3),
    ("FastS", "fasts-over-fasty", 8, 5),
    ("FastS", "fasts", 8, 5),
    ("FastM", "fastm", 8, 3),
    ("FastM", "fastm-f32", 8, 3),
    ("FastN", "fastn", 8, 2),
    ("FastN", "fastn-complex-f32", 8, 3),
    ("FastG", "fastg", 8, 7),
    ("FastG", "fastg-f32", 8, 7),
    ("FastG-rows", "fastg-rows", 8, 300),
    ("FastR", "fastr", 64, 5),            # 65 536-sample rows with a batch stride
    # rows beyond the table (tests/strided.py EXTRA): the strided code paths the table's rows do not reach
    ("FastR", "fastr-32768", 64, 5), ("FastR", "fastr-16384", 64, 9), ("FastR", "fastr-8192", 64, 9), ("FastR", "fastr-4096", 64, 9),  # fastr2_kernel
    ("FastM", "fastm-wide", 8, 3),        # pass 1 with four sequences per workgroup (float32, 2000 rows)
    ("FastN", "fastn-odd", 8, 3), ("FastN", "fastn-odd-f32", 8, 3),  # columns that are not packed in pairs
    ("FastN", "fastn-chirp-f32", 8, 3), ("FastN", "fastn-chirp", 8, 3), ("FastN", "fastn-rader-f32", 8, 3), ("FastN", "fastn-rader", 8, 3),  # the forms of its column kernel
    ("FastN", "fastn-r20-f32", 8, 3),
    ("FastG", "fastg-odd", 8, 7), ("FastG", "fastg-odd-f32", 8, 7),
    ("FastG-rows", "fastg-rows-f32", 8, 300), ("FastG-rows", "fastg-rows-odd", 8, 300),
] + [("FastS", f"fasts-{ny}x{nx}", 8, 5) for ny in (64, 128, 256) for nx in (64, 128, 256)]


def _gpu_params():
    out = []
    for fam, rid, pad, batch in GPU_ROWS:
        for mode in S.SERVES[fam]:
            if rid == "fasty" and mode not in ("power-linear-windows", "iso-sums-only"):
                continue  # (the 4096^2 slab: the headline modes; the 1024^2 row runs all four)
            out.append(pytest.param(rid, mode, pad, batch, id=f"{fam}-{rid}-{mode}"))
    return out


@pytest.mark.parametrize("rid,mode,pad,batch", _gpu_params())
def test_strided_plan_is_bit_identical_to_the_dense_plan(rid, mode, pad, batch):
    kw, kind, tag = S.table_row(rid)
    p = S.run_plan_case(kw, kind, tag, mode, dev="cuda", batch=batch, pad_x=pad, form=S.FASTN_FORM.get(rid))
    if rid == "fasty":
        assert "in pitch 8192" in p.describe()


def test_overlapping_windows_on_the_headline_family():
    """in_stride_batch = ny * pitch / 2 over one buffer (FastY, 1024 x 1024 windows half a slab apart)."""
    ny = nx = 1024
    pitch = nx + 64
    sb = ny * pitch // 2
    g = torch.Generator(device="cuda").manual_seed(3)
    buf = torch.randn(sb * 5 + ny * pitch, generator=g, device="cuda", dtype=torch.float32)
    x = torch.as_strided(buf, (6, ny, nx), (sb, pitch, 1))
    kw = dict(ny=ny, nx=nx, batch=6, detrend=L.DETREND_LINEAR)
    strided, dense = A.make(**kw, in_stride_y=pitch, in_stride_batch=sb), A.make(**kw)
    assert A.family(strided) == A.family(dense) == (L.K_FASTY, "fasty")
    out_s, _ = strided.execute(x)
    out_d, _ = dense.execute(x.contiguous())
    assert torch.equal(out_s, out_d) and S.finite(out_s)
