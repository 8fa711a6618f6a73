"""Input strides in the plan descriptor (xrfthip_desc.in_stride_y / in_stride_batch), on the emulated library: a box cut out of a larger field is
transformed where it lies, with no contiguous copy.

The property held at the plan level: a strided plan runs the family, the grouping and the arithmetic of the dense plan of the same shape, so its result on
the view is BIT-IDENTICAL to the dense plan's on ``view.contiguous()`` -- for every family taught to read strided input (FastY, FastM, FastN, FastS, FastG
slabs, FastG row groups, FastR) and every mode it serves.  The box sits in a buffer of NaN (a kernel that reads outside the view's rows poisons its
result), for one case per family with its last sample on the last element of the buffer (scripts/run_emu_asan.sh then catches a read past the end).
One case per family is also held to the rounding-level bound of tests/accuracy.py against the float64 reference, so that the dense plan is not the only
yardstick.  At the API level, power_spectrum / fft / cross_spectrum / isotropic_power_spectrum of ``da.isel(y=slice(..), x=slice(..))`` run the strided
plan (its describe() shows the pitch) and meet the oracle; views the descriptor cannot express take the copying path, with the same values."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

import xrft_amd as xa  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402
from xrft_amd import _lib, api, engine  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402

import accuracy as A  # noqa: E402
import cases  # noqa: E402
import strided as S  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    api.clear_plan_cache()
    _lib._state.update(dll=None, path=None, device="cuda")


def newest_plan():
    return next(reversed(api._plan_cache.values())).describe()


# ---------------------------------------------------------------------------------- 1. the plan, per taught family
@pytest.mark.parametrize("rid,mode", S.plan_params())
def test_strided_plan_is_bit_identical_to_the_dense_plan(rid, mode):
    kw, kind, tag = S.table_row(rid)
    S.run_plan_case(kw, kind, tag, mode, form=S.FASTN_FORM.get(rid))


@pytest.mark.parametrize("fam,rid", [(f, r) for f, rows in S.FAMILIES.items() for r in rows], ids=lambda v: str(v))
def test_strided_plan_meets_the_rounding_bound(fam, rid):
    """The same view against the float64 reference of its samples, at the bound of tests/accuracy.py (C_RMS u log2 N + the detrend term)."""
    kw, kind, tag = S.table_row(rid)
    kw.update(out_mode=L.OUT_POWER, detrend=L.DETREND_LINEAR, flags=0, batch=2)
    kw.pop("iso", None)
    dtype = kw.get("dtype", A.F32)
    x, sy, sb = S.box_in_nan(kw, np.random.default_rng(9), "middle", dtype)
    p = A.make(**kw, in_stride_y=sy, in_stride_batch=sb)
    assert A.family(p) == (kind, tag)
    out, _ = p.execute(x)
    shape, axes, _ = A._axes(kw)
    x64 = x.contiguous().to(torch.float64).numpy().reshape(shape)
    ref, _ = A.reference(kw, x64)
    kap = A.kappa(x64, A.detrended(x64, axes, L.DETREND_LINEAR))
    A.assert_accurate(out.numpy().reshape(ref.shape), ref, dtype, A.points(kw), kap, what=f"{fam} strided power spectrum")


# ---------------------------------------------------------------------------------- 2. overlapping windows of one buffer
@pytest.mark.parametrize("rid", ["fastg", "fasty-small", "fasts", "fastm-small"])
def test_overlapping_windows(rid):
    """in_stride_batch = ny * pitch / 2: every slab starts half a slab after the one before it (the input is never written)."""
    kw, kind, tag = S.table_row(rid)
    kw.update(out_mode=L.OUT_POWER, detrend=L.DETREND_LINEAR, batch=4)
    dtype = kw.get("dtype", A.F32)
    ny, nx = kw["ny"], kw["nx"]
    pitch = nx + 8
    sb = ny * pitch // 2
    buf = torch.from_numpy(np.random.default_rng(3).standard_normal(sb * 3 + ny * pitch)).to(dtype)
    x = torch.as_strided(buf, (4, ny, nx), (sb, pitch, 1))
    strided = A.make(**kw, in_stride_y=pitch, in_stride_batch=sb)
    dense = A.make(**kw)
    assert A.family(strided) == A.family(dense) == (kind, tag)
    out_s, _ = strided.execute(x)
    out_d, _ = dense.execute(x.contiguous())  # the materialised windows
    assert torch.equal(out_s, out_d) and S.finite(out_s)


# ---------------------------------------------------------------------------------- 3. refusals
def status_of(**kw):
    with pytest.raises(_lib.XrftHipError) as e:
        A.make(**kw)
    return e.value.status


def test_bad_strides_are_bad_arguments():
    assert status_of(ny=50, nx=50, dtype=A.F64, in_stride_y=-64) == L.BAD_ARG
    assert status_of(ny=50, nx=50, dtype=A.F64, in_stride_batch=-4096) == L.BAD_ARG
    assert status_of(ny=50, nx=50, dtype=A.F64, in_stride_y=48) == L.BAD_ARG  # 0 < in_stride_y < nx
    assert status_of(ny=128, nx=256, inner=4, in_stride_y=260) == L.BAD_ARG
    assert status_of(ny=64, nx=96, mid=3, out_mode=L.OUT_COMPLEX, in_stride_batch=64 * 96 * 3 + 16) == L.BAD_ARG
    assert status_of(ny=100, nx=200, dtype=A.F64, flags=L.AXIS_Y, in_stride_y=208) == L.BAD_ARG
    # a C2R_X plan's rows are the stored nx / 2 + 1 complex values
    assert status_of(ny=50, nx=50, dtype=A.C128, out_mode=L.OUT_COMPLEX, flags=L.INVERSE | L.C2R_X, in_stride_y=25) == L.BAD_ARG


def test_misaligned_pointer_is_refused_at_exec():
    kw = dict(ny=50, nx=50, dtype=A.F64, batch=2)
    p = A.make(**kw, in_stride_y=52, in_stride_batch=50 * 52 + 4)
    buf = torch.zeros(2 * (50 * 52 + 4) + 8, dtype=A.F64)
    out = torch.empty((2, 50, 50), dtype=A.F64)
    ws = torch.empty(max(p.workspace_bytes, 256), dtype=torch.uint8)
    call = lambda off: p._dll.xrfthip_exec(p._h, C.c_void_p(buf.data_ptr() + off), None, C.c_void_p(out.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws.numel(), None)
    assert buf.data_ptr() % 16 == 0
    assert call(8) == L.BAD_ARG
    assert call(0) == 0 and call(16) == 0
    with pytest.raises(ValueError):  # ... and by the wrapper, before the call
        p.execute(torch.as_strided(buf, (2, 50, 50), (50 * 52 + 4, 52, 1), 1))
    cross = A.make(**kw, out_mode=L.OUT_CROSS, in_stride_y=52, in_stride_batch=50 * 52 + 4)
    oc = torch.empty((2, 50, 50), dtype=A.C128)
    assert cross._dll.xrfthip_exec(cross._h, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 8), C.c_void_p(oc.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws.numel(), None) == L.BAD_ARG


def test_the_caller_copies():
    """XRFTHIP_UNSUPPORTED_LENGTH: strides the kernels' vector loads cannot take, a slab beyond 32-bit offsets, a family that is not taught."""
    assert status_of(ny=256, nx=512, in_stride_y=514) == L.UNSUPPORTED_LENGTH           # 2056 bytes: not a multiple of 16
    assert status_of(ny=256, nx=512, in_stride_y=516, in_stride_batch=256 * 516 + 2) == L.UNSUPPORTED_LENGTH
    assert status_of(ny=50, nx=50, dtype=A.F64, in_stride_y=51) == L.UNSUPPORTED_LENGTH
    assert status_of(ny=4096, nx=4096, in_stride_y=1 << 20) == L.UNSUPPORTED_LENGTH     # ny * in_stride_y = 2^32 > 2^31 - 1
    assert status_of(ny=1024, nx=1024, in_stride_y=(1 << 21) - 4) == L.UNSUPPORTED_LENGTH
    # families that do not read strided input: the complex two-pass pipeline, the x-only table kernel, the generic passes, complex input of fastg
    assert status_of(ny=1024, nx=1024, dtype=A.C64, out_mode=L.OUT_COMPLEX, in_stride_y=1032) == L.UNSUPPORTED_LENGTH
    assert status_of(ndim=1, nx=1000, dtype=A.F64, in_stride_batch=1008) == L.UNSUPPORTED_LENGTH
    assert status_of(ndim=1, nx=1031, dtype=A.F64, in_stride_batch=1040) == L.UNSUPPORTED_LENGTH
    assert status_of(ny=96, nx=128, dtype=A.C64, out_mode=L.OUT_COMPLEX, in_stride_y=136) == L.UNSUPPORTED_LENGTH
    # the dense descriptor of each of these shapes builds
    for kw in (dict(ny=1024, nx=1024, dtype=A.C64, out_mode=L.OUT_COMPLEX), dict(ndim=1, nx=1000, dtype=A.F64), dict(ndim=1, nx=1031, dtype=A.F64)):
        A.make(**kw)


def test_strides_that_say_dense_are_the_dense_plan():
    p = A.make(ndim=1, nx=1000, dtype=A.F64, in_stride_batch=1000)  # (a family that is not taught serves it: nothing is strided)
    assert A.family(p) == (L.K_FASTM_X, "fastm x-only") and "in pitch" not in p.describe()
    q = A.make(ny=50, nx=50, dtype=A.F64, in_stride_y=50, in_stride_batch=2500)
    assert "in pitch" not in q.describe()


@pytest.mark.parametrize("field", ["inner", "mid", "in_stride_y"])
def test_earlier_descriptor_sizes_still_build_a_dense_plan(field):
    dll = _lib.load()
    size = getattr(_lib.Desc, field).offset  # the struct_size of the version that ended before this field
    d = _lib.Desc(size, 2, 2, 50, 50, L.F64, L.OUT_POWER, 0, 0, 1.0, 0, 0, 1, 1, 0, 0)
    tail = ["inner", "mid", "in_stride_y", "in_stride_batch"]
    for name in tail[tail.index(field):]:  # what lies beyond struct_size is not read
        setattr(d, name, -5)
    h = C.c_void_p(0)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
    buf = C.create_string_buffer(8192)
    dll.xrfthip_plan_describe(h, buf, len(buf))
    text = buf.value.decode()
    dll.xrfthip_plan_destroy(h)
    assert "[fastg]" in text and "in pitch" not in text and "inner layout" not in text
    bad = _lib.Desc(size + 4, 2, 2, 50, 50, L.F64, L.OUT_POWER, 0, 0, 1.0, 0, 0, 1, 1, 0, 0)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(bad)) == L.BAD_ARG


# ---------------------------------------------------------------------------------- 4. the API
def boxes(dtype, shape=(3, 96, 160), ys=slice(24, 88), xs=slice(16, 144), seed=21):
    """(the product's box -- a view of a larger torch tensor --, the oracle's box from the same samples)"""
    rng = np.random.default_rng(seed)
    nt, ny, nx = shape
    v = (rng.standard_normal(shape) + 0.02 * np.arange(ny).reshape(1, ny, 1) - 0.01 * np.arange(nx).reshape(1, 1, nx) + 1.0).astype(dtype)
    coords = {"t": np.arange(nt) * 1.0, "y": np.arange(ny) * 0.5, "x": np.arange(nx) * 2.0 + 3.0}
    da = xa.DataArray(torch.from_numpy(v), ("t", "y", "x"), coords)
    box = da.isel(y=ys, x=xs)
    sub = {"t": coords["t"], "y": coords["y"][ys], "x": coords["x"][xs]}
    ref = v[:, ys, xs]
    od = o.OArr(ref.astype(np.float64) if dtype == "float32" else ref, ("t", "y", "x"), sub)
    return box, od


API_OPS = {
    "power_spectrum": lambda m, a, b: m.power_spectrum(a, dim=["y", "x"], detrend="linear", window="hann"),
    "fft-real_dim": lambda m, a, b: m.fft(a, dim=["y", "x"], real_dim="x", detrend="constant"),
    "cross_spectrum": lambda m, a, b: m.cross_spectrum(a, b, dim=["y", "x"], detrend="constant", window="hann"),
    "isotropic_power_spectrum": lambda m, a, b: m.isotropic_power_spectrum(a, dim=["y", "x"], detrend="linear", window="hann"),
}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("op", list(API_OPS))
def test_api_transforms_the_box_where_it_lies(op, dtype):
    box, od = boxes(dtype)
    box2, od2 = boxes(dtype, seed=22)
    assert not box.data.is_contiguous()
    api.clear_plan_cache()
    got = API_OPS[op](xa, box, box2)
    ref = API_OPS[op](o, od, od2)
    cases.check(got, ref, cases.TOL[dtype])
    assert "in pitch 160 / slab 15360" in newest_plan(), newest_plan()
    # ... and the contiguous copy of the box gives the same values through the dense plan
    dense = xa.DataArray(box.data.contiguous(), box.dims, box.coords)
    dense2 = xa.DataArray(box2.data.contiguous(), box2.dims, box2.coords)
    again = API_OPS[op](xa, dense, dense2)
    assert "in pitch" not in newest_plan()
    assert np.array_equal(np.asarray(got.values), np.asarray(again.values))


@pytest.mark.parametrize("why", ["odd-x-origin", "step-2", "leading-dims-do-not-collapse"])
def test_api_copies_a_view_the_descriptor_cannot_express(why):
    rng = np.random.default_rng(31)
    if why == "leading-dims-do-not-collapse":
        v = rng.standard_normal((2, 3, 64, 128)).astype("float32")
        dims = ("a", "t", "y", "x")
        coords = {"a": np.arange(2.0), "t": np.arange(3.0), "y": np.arange(64) * 0.5, "x": np.arange(128) * 2.0}
        sel = dict(t=slice(0, 2))
    else:
        v = rng.standard_normal((3, 64, 300)).astype("float32")
        dims = ("t", "y", "x")
        coords = {"t": np.arange(3.0), "y": np.arange(64) * 0.5, "x": np.arange(300) * 2.0}
        sel = dict(x=slice(3, 131)) if why == "odd-x-origin" else dict(x=slice(0, 256, 2))
    da = xa.DataArray(torch.from_numpy(v), dims, coords)
    box = da.isel(**sel)
    assert not box.data.is_contiguous()
    idx = tuple(sel.get(d, slice(None)) for d in dims)
    od = o.OArr(v[idx].astype(np.float64), dims, {d: (coords[d][sel[d]] if d in sel else coords[d]) for d in dims})
    api.clear_plan_cache()
    got = xa.power_spectrum(box, dim=["y", "x"], detrend="linear", window="hann")
    cases.check(got, o.power_spectrum(od, dim=["y", "x"], detrend="linear", window="hann"), cases.TOL["float32"])
    assert "in pitch" not in newest_plan()
    dense = xa.power_spectrum(xa.DataArray(box.data.contiguous(), dims, box.coords), dim=["y", "x"], detrend="linear", window="hann")
    assert np.array_equal(np.asarray(got.values), np.asarray(dense.values))


def test_api_copies_a_second_field_with_other_strides():
    box, od = boxes("float64")
    box2, od2 = boxes("float64", shape=(3, 96, 176), seed=23)  # the same box of a wider parent: another pitch
    assert box2.data.stride() != box.data.stride() and box2.data.shape == box.data.shape
    api.clear_plan_cache()
    got = xa.cross_spectrum(box, box2, dim=["y", "x"], detrend="constant", window="hann")
    od2 = o.OArr(od2.values, od.dims, {d: od.coord(d) for d in od.dims})
    cases.check(got, o.cross_spectrum(od, od2, dim=["y", "x"], detrend="constant", window="hann"), cases.TOL["float64"])
    assert "in pitch" not in newest_plan()


def test_api_falls_back_where_the_family_is_not_taught():
    """A complex box: the dense plan of its shape runs a family that does not read strided input -- the library says so, the box is copied."""
    rng = np.random.default_rng(41)
    v = (rng.standard_normal((2, 96, 160)) + 1j * rng.standard_normal((2, 96, 160))).astype("complex128")
    coords = {"t": np.arange(2.0), "y": np.arange(96) * 0.5, "x": np.arange(160) * 2.0}
    box = xa.DataArray(torch.from_numpy(v), ("t", "y", "x"), coords).isel(y=slice(24, 88), x=slice(16, 144))
    od = o.OArr(v[:, 24:88, 16:144], ("t", "y", "x"), {"t": coords["t"], "y": coords["y"][24:88], "x": coords["x"][16:144]})
    api.clear_plan_cache()
    for _ in range(2):  # (the second call does not ask the library again)
        got = xa.fft(box, dim=["y", "x"])
        cases.check(got, o.fft(od, dim=["y", "x"]), cases.TOL["complex128"])
        assert "in pitch" not in newest_plan()
    assert len(api._STRIDED_REFUSED) == 1
