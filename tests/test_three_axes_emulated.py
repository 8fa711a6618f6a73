"""power_spectrum / cross_spectrum over THREE axes on the fused route (round 9), on the emulated library: detrend, the two-axis plan with the half spectrum as
its output, then ONE plan (xrfthip_desc.herm_ny / herm_nx, csrc/fasth.h) that transforms along the first of the three axes and writes the full shifted power /
cross result, the redundant half from the Hermitian twin.

Held here: the oracle's N-D result (cases.check at cases.TOL) and the rounding-level contract of tests/accuracy.py on every shape x precision x batch x shift x
detrend x window x order of ``dim``; the routing (describe() of the newest plan carries [fasth]); every mirrored element equals its sample bit for bit (CROSS: its
conjugate); every element of the output is written (a NaN-filled buffer) and two calls agree bit for bit; the fused route against the composition it replaces
(api._FUSE_THREE_AXES = False) within the contract; calls outside the route compose as before, with the composition's bits; the descriptor's refusals."""
import ctypes as C
import itertools
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
from xrft_amd import _lib, api  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402

import accuracy as A  # noqa: E402
from accuracy import herm_full, herm_kw  # noqa: E402
import cases  # noqa: E402

# (nt, ny, nx): a small even cube; all odd (no Nyquist column, twins for kx = 1 .. (nx - 1) / 2); all even; column blocks that straddle rows ky; nt = 2 x 3 x 5
SHAPES = [(8, 6, 10), (9, 5, 7), (16, 16, 16), (12, 7, 16), (30, 4, 6)]
ORDERS = [["t", "y", "x"], ["x", "t", "y"]]
DIMS = ("b", "t", "y", "x")


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api.clear_plan_cache()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    api._FUSE_THREE_AXES = True
    api.clear_plan_cache()
    _lib._state.update(dll=None, path=None, device="cuda")


def newest_plan():
    return next(reversed(api._plan_cache.values())).describe()


def fields(shape, batch, dtype, seed=5, x0=3.0):
    """Two (b, t, y, x) fields with a hyperplane under the noise, as the product's arrays and the oracle's (the same samples as float64)."""
    nt, ny, nx = shape
    rng = np.random.default_rng(seed)
    full = (batch,) + tuple(shape)
    ramp = 0.05 * np.arange(nt).reshape(1, nt, 1, 1) + 0.03 * np.arange(ny).reshape(1, 1, ny, 1) - 0.02 * np.arange(nx).reshape(1, 1, 1, nx) + 1.0
    v0 = (rng.standard_normal(full) + ramp).astype(dtype)
    v1 = rng.standard_normal(full).astype(dtype)
    coords = {"b": np.arange(batch), "t": np.arange(nt) * 1.0, "y": np.arange(ny) * 0.5 + 1.0, "x": np.arange(nx) * 2.0 + x0}
    return cases.pair(v0, DIMS, coords), cases.pair(v1, DIMS, coords)


def unshifted(v, shift):
    return np.fft.ifftshift(v, axes=(-3, -2, -1)) if shift else v


def mirrored(v):
    """(the samples, their twins v[..., -kt, -ky, -kx]) of the columns 1 <= kx <= nx - (nx / 2 + 1) of an unshifted result: the columns whose twin is not a column of
    the half spectrum, so that the twin is a copy (the columns kx = 0 and nx / 2 hold both partners as transforms of their own)."""
    nx = v.shape[-1]
    tw = np.roll(v[..., ::-1, ::-1, ::-1], 1, axis=(-3, -2, -1))
    return v[..., 1:nx - nx // 2], tw[..., 1:nx - nx // 2]


# ---------------------------------------------------------------------------------- 1. the API: oracle, contract, routing, mirror bits
@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_three_axis_spectra(shape, dtype, batch, shift):
    (da, oa), (db, ob) = fields(shape, batch, dtype)
    n = int(np.prod(shape))
    for det, win, dim in itertools.product([None, "linear"], [None, "hann"], ORDERS):
        kw = dict(dim=dim, shift=shift, detrend=det, window=win)
        what = f"{shape} {dtype} batch {batch} {kw}"
        kap = A.kappa(oa.values, o.detrend(oa, dim, "linear").values) if det else 0.0
        got = xa.power_spectrum(da, **kw)
        assert "[fasth]" in newest_plan(), what
        ref = o.power_spectrum(oa, **kw)
        cases.check(got, ref, cases.TOL[dtype])
        A.assert_accurate(got.values, ref.values, dtype, n, kap, what="power_spectrum " + what)
        g = unshifted(np.asarray(got.values), shift)
        sm, tw = mirrored(g)
        assert g.dtype == np.dtype(dtype) and sm.size and np.array_equal(sm, tw), what  # every mirrored element is its sample, bit for bit
        got = xa.cross_spectrum(da, db, **kw)
        assert "[fasth]" in newest_plan(), what
        ref = o.cross_spectrum(oa, ob, **kw)
        cases.check(got, ref, cases.TOL[dtype])
        A.assert_accurate(got.values, ref.values, dtype, n, kap, what="cross_spectrum " + what)
        g = unshifted(np.asarray(got.values), shift)
        sm, tw = mirrored(g)
        assert np.array_equal(sm, np.conj(tw)), what


def test_labels_are_the_compositions():
    """Dims, coordinate names in their order, values and attributes (spacing, direct_lag) are what the composed stages give."""
    (da, _), (db, _) = fields((8, 6, 10), 2, "float64")
    for dim in ORDERS:
        for call in (lambda: xa.power_spectrum(da, dim=dim, window="hann", detrend="constant"), lambda: xa.cross_spectrum(da, db, dim=dim)):
            fused = call()
            assert "[fasth]" in newest_plan()
            api._FUSE_THREE_AXES = False
            try:
                comp = call()
            finally:
                api._FUSE_THREE_AXES = True
            assert fused.dims == comp.dims and list(fused.coords) == list(comp.coords)
            for k in comp.coords:
                assert np.array_equal(fused[k].values, comp[k].values) and fused[k].attrs == comp[k].attrs, k


# ---------------------------------------------------------------------------------- 2. fused against composed
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_against_composed(shape, dtype):
    (da, oa), (db, _) = fields(shape, 2, dtype, seed=8)
    n = int(np.prod(shape))
    for det, win, shift in itertools.product([None, "linear"], [None, "hann"], [True, False]):
        kw = dict(dim=["t", "y", "x"], shift=shift, detrend=det, window=win)
        kap = A.kappa(oa.values, o.detrend(oa, kw["dim"], "linear").values) if det else 0.0
        for call in (lambda: xa.power_spectrum(da, **kw), lambda: xa.cross_spectrum(da, db, **kw)):
            fused = call()
            assert "[fasth]" in newest_plan()
            api._FUSE_THREE_AXES = False
            try:
                api._plan_cache.clear()
                comp = call()
                assert all("[fasth]" not in p.describe() for p in api._plan_cache.values())
            finally:
                api._FUSE_THREE_AXES = True
            assert fused.dims == comp.dims
            A.assert_accurate(fused.values, comp.values, dtype, n, kap, what=f"fused vs composed {shape} {dtype} {kw}")


# ---------------------------------------------------------------------------------- 3. calls outside the route compose as before
def _declined(call):
    """The call's result with the switch on equals the composition's bits, and no plan of it is the new one."""
    api._plan_cache.clear()
    on = call()
    assert api._plan_cache and all("[fasth]" not in p.describe() for p in api._plan_cache.values())
    api._FUSE_THREE_AXES = False
    try:
        off = call()
    finally:
        api._FUSE_THREE_AXES = True
    assert on.dims == off.dims and np.array_equal(np.asarray(on.values), np.asarray(off.values), equal_nan=True)
    assert list(on.coords) == list(off.coords)


def test_a_descending_coordinate_composes():
    (da, _), (db, _) = fields((8, 6, 10), 2, "float64")
    c = {k: v.values for k, v in da.coords.items()}
    c["y"] = c["y"][::-1].copy()
    da, db = xa.DataArray(da.data, DIMS, c), xa.DataArray(db.data, DIMS, c)
    _declined(lambda: xa.cross_spectrum(da, db, dim=["t", "y", "x"]))  # (true_phase: the flipped axis, xrft.py:436-441)


def test_complex_data_composes():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((2, 8, 6, 10)) + 1j * rng.standard_normal((2, 8, 6, 10))
    (da, _), _ = fields((8, 6, 10), 2, "float64")
    dc = xa.DataArray(torch.from_numpy(v), DIMS, {k: c.values for k, c in da.coords.items()})
    _declined(lambda: xa.power_spectrum(dc, dim=["t", "y", "x"]))


def test_real_dim_composes():
    (da, _), (db, _) = fields((8, 6, 10), 2, "float32")
    _declined(lambda: xa.power_spectrum(da, dim=["t", "y", "x"], real_dim="x", window="hann"))
    _declined(lambda: xa.cross_spectrum(da, db, dim=["t", "y", "x"], real_dim="x"))


def test_two_fields_with_different_lags_compose():
    (da, _), _ = fields((8, 6, 10), 2, "float64")
    _, (db, _) = fields((8, 6, 10), 2, "float64", x0=7.0)  # (another origin along x: another lag, a true-phase factor that does not cancel)
    _declined(lambda: xa.cross_spectrum(da, db, dim=["t", "y", "x"]))


def test_a_length_without_a_butterfly_composes():
    (da, oa), _ = fields((34, 4, 6), 1, "float64")  # 34 = 2 x 17: the Rader form of the one-axis kernel is not carried over
    _declined(lambda: xa.power_spectrum(da, dim=["t", "y", "x"]))
    cases.check(xa.power_spectrum(da, dim=["t", "y", "x"]), o.power_spectrum(oa, dim=["t", "y", "x"]), cases.TOL["float64"])


def test_other_than_the_trailing_three_axes_composes():
    rng = np.random.default_rng(3)
    c = {"t": np.arange(8.0), "y": np.arange(6) * 0.5, "x": np.arange(10) * 2.0, "b": np.arange(2)}
    da = xa.DataArray(torch.from_numpy(rng.standard_normal((8, 6, 10, 2))), ("t", "y", "x", "b"), c)
    _declined(lambda: xa.power_spectrum(da, dim=["t", "y", "x"]))


# ---------------------------------------------------------------------------------- 4. the plan: every element written, repeats, refusals
def half_spectra(shape, batch, cdtype, seed=4):
    nt, ny, nx = shape
    rng = np.random.default_rng(seed)
    h = [np.fft.rfftn(rng.standard_normal((batch, nt, ny, nx)), axes=(-2, -1)) for _ in range(2)]
    return [torch.from_numpy(np.ascontiguousarray(v)).to(cdtype).reshape(batch, nt, ny * (nx // 2 + 1)) for v in h]


@pytest.mark.parametrize("flags", [0, L.SHIFT_Y | L.SHIFT_X, L.SHIFT_X | L.ISHIFT_Y], ids=["plain", "shifted", "yx-shifted-ishift"])
@pytest.mark.parametrize("mode", [L.OUT_POWER, L.OUT_CROSS], ids=["power", "cross"])
@pytest.mark.parametrize("cdtype", [A.C64, A.C128], ids=["c64", "c128"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_stale_output_and_identical_repeats(shape, cdtype, mode, flags):
    nt, ny, nx = shape
    p = A.make(**herm_kw(shape, cdtype, mode, flags), window_y=np.hanning(nt + 1)[:-1] + 0.5)
    assert A.family(p) == (L.K_FASTH, "fasth")
    h0, h1 = half_spectra(shape, 2, cdtype)
    outs = []
    for _ in range(2):
        buf = torch.full((2, nt, ny, nx), float("nan"), dtype=p.out_dtype())
        out, _ = p.execute(h0, h1 if mode == L.OUT_CROSS else None, out=buf)
        assert out.data_ptr() == buf.data_ptr() and not torch.isnan(torch.view_as_real(out) if out.is_complex() else out).any()  # every element written
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    # ... and what was written is the window, the transform along t, the product, the twins and the rotations
    kw = herm_kw(shape, cdtype, mode)
    w = (np.hanning(nt + 1)[:-1] + 0.5).reshape(1, nt, 1)
    x0, x1 = (h.to(torch.complex128).numpy() * w for h in (h0, h1))
    if flags & L.ISHIFT_Y:
        x0, x1 = (np.fft.ifftshift(x, axes=1) for x in (x0, x1))
    plain = {k: v for k, v in kw.items() if not k.startswith("herm_")}
    ref, _ = A.reference(plain, x0, x1)  # (the one-axis transform and the product on the stored half; the twins and the rotations are applied here, apart from A.reference's own herm form)
    ref = herm_full(ref, ny, nx, mode == L.OUT_CROSS)
    if flags & L.SHIFT_Y:
        ref = np.fft.fftshift(ref, axes=1)
    if flags & L.SHIFT_X:
        ref = np.fft.fftshift(ref, axes=(2, 3))
    A.assert_accurate(outs[0].numpy(), ref, cdtype, nt, what=f"herm plan {shape} flags {flags:#x}")


def status_of(**kw):
    with pytest.raises(_lib.XrftHipError) as e:
        A.make(**kw)
    return e.value.status


def test_invalid_descriptors_are_bad_arguments():
    good = herm_kw((8, 6, 10), A.C64, L.OUT_POWER)
    A.make(**good)
    assert status_of(**dict(good, flags=0)) == L.BAD_ARG                      # not an AXIS_Y plan
    assert status_of(**dict(good, ndim=1, ny=1)) == L.BAD_ARG
    assert status_of(**dict(good, nx=6 * 6 + 1)) == L.BAD_ARG                 # nx is not herm_ny (herm_nx / 2 + 1)
    assert status_of(**dict(good, nx=6 * 10)) == L.BAD_ARG
    assert status_of(**dict(good, herm_nx=0)) == L.BAD_ARG                    # one field without the other
    assert status_of(**dict(good, herm_ny=0)) == L.BAD_ARG
    assert status_of(**dict(good, herm_ny=-6)) == L.BAD_ARG
    for dt in (A.F32, A.F64):
        assert status_of(**dict(good, dtype=dt)) == L.BAD_ARG                 # real input
    for mode in (L.OUT_COMPLEX, L.OUT_PHASE):
        assert status_of(**dict(good, out_mode=mode)) == L.BAD_ARG
    for f in (L.HALF_X, L.ISHIFT_X, L.FLIP_Y, L.FLIP_X, L.FLIP0_Y, L.REALDIM_X2, L.ISO, L.INVERSE, L.PHASE_IN, L.C2R_X, L.HALF_Y):
        assert status_of(**dict(good, flags=L.AXIS_Y | f)) == L.BAD_ARG, hex(f)
    assert status_of(**dict(good, detrend=L.DETREND_LINEAR)) == L.BAD_ARG
    assert status_of(**dict(good, inner=4)) == L.BAD_ARG
    assert status_of(**dict(good, mid=3)) == L.BAD_ARG
    assert status_of(**dict(good, in_stride_y=64)) == L.BAD_ARG
    assert status_of(**dict(good, in_stride_batch=8 * 36 + 16)) == L.BAD_ARG
    assert status_of(**dict(good, phase_y=np.exp(0.1j * np.arange(8)))) == L.BAD_ARG   # a phase table
    assert status_of(**dict(good, window_x=np.ones(36))) == L.BAD_ARG                  # a window on the Hermitian axes
    # the flags it takes
    for f in (L.SHIFT_Y, L.ISHIFT_Y, L.SHIFT_X, L.SHIFT_Y | L.SHIFT_X | L.ISHIFT_Y):
        A.make(**dict(good, flags=L.AXIS_Y | f))
    # SHIFT_X stays a bad argument of an AXIS_Y plan without the fields
    assert status_of(ny=8, nx=36, dtype=A.C64, flags=L.AXIS_Y | L.SHIFT_X) == L.BAD_ARG


def test_lengths_the_last_pass_declines_are_unsupported():
    assert status_of(**herm_kw((34, 4, 6), A.C128, L.OUT_POWER)) == L.UNSUPPORTED_LENGTH    # 2 x 17: no Rader form
    assert status_of(**herm_kw((103, 4, 6), A.C64, L.OUT_POWER)) == L.UNSUPPORTED_LENGTH    # a prime: no Bluestein form
    assert status_of(**herm_kw((1024, 4, 6), A.C64, L.OUT_CROSS)) == L.UNSUPPORTED_LENGTH   # the tile of 128 output bytes per row does not fit the LDS
    for nt in (2, 7, 11, 13, 14, 77, 360, 512):
        assert A.family(A.make(**herm_kw((nt, 4, 6), A.C128, L.OUT_CROSS))) == (L.K_FASTH, "fasth")


@pytest.mark.parametrize("field", ["inner", "mid", "in_stride_y", "herm_ny"])
def test_earlier_descriptor_sizes_still_build(field):
    dll = _lib.load()
    size = getattr(_lib.Desc, field).offset  # the struct_size of the version that ended before this field
    d = _lib.Desc(size, 2, 2, 50, 50, L.F64, L.OUT_POWER, 0, 0, 1.0, 0, 0, 1, 1, 0, 0, 0, 0)
    tail = ["inner", "mid", "in_stride_y", "in_stride_batch", "herm_ny", "herm_nx"]
    for name in tail[tail.index(field):]:  # what lies beyond struct_size is not read
        setattr(d, name, -5)
    h = C.c_void_p(0)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
    buf = C.create_string_buffer(8192)
    dll.xrfthip_plan_describe(h, buf, len(buf))
    text = buf.value.decode()
    dll.xrfthip_plan_destroy(h)
    assert "[fastg]" in text and "[fasth]" not in text and "in pitch" not in text and "inner layout" not in text
    bad = _lib.Desc(size + 4, 2, 2, 50, 50, L.F64, L.OUT_POWER, 0, 0, 1.0, 0, 0, 1, 1, 0, 0, 0, 0)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(bad)) == L.BAD_ARG
