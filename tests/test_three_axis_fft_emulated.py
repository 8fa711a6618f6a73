"""fft / dft over THREE axes of real data on the fused route (api._fft_3d_fused), on the emulated library: detrend, the two-axis plan with the half spectrum as its
output, then ONE plan (xrfthip_desc.herm_ny / herm_nx with XRFTHIP_HERM_FIELD, csrc/fasth.h) that transforms along the first of the three axes and writes the full
shifted complex result, the redundant half as the conjugate of the Hermitian twin times the true-phase factors of its own indices.

Held here: the oracle's N-D result (cases.check at cases.TOL) and the rounding-level contract of tests/accuracy.py on every shape x precision x batch x shift x
true_phase x true_amplitude x detrend x window x order of ``dim``; the routing (describe() of the newest plan carries [fasth]); the twin rule -- without phase
factors a twin is its sample's conjugate bit for bit, with them the Nyquist rows of the twins meet the oracle where the plain conjugate would not; every element
of the output is written and two calls agree bit for bit; the plan against numpy with and without phase tables; the descriptor's refusals; the fused route
against the composition it replaces (api._FUSE_THREE_AXES = False); calls outside the route compose as before, with the composition's bits; a NaN stays in its
own batch entry."""
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
import cases  # noqa: E402
import three_axis_fft as T  # noqa: E402
from three_axis_fft import DIMS, ORDERS, SHAPES  # noqa: E402

IDS = dict(ids=lambda s: "x".join(map(str, s)))


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


def composed(call):
    api._FUSE_THREE_AXES = False
    try:
        return call()
    finally:
        api._FUSE_THREE_AXES = True


# ---------------------------------------------------------------------------------- 1. the API: oracle, contract, routing, twin bits
@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_three_axis_fft(shape, dtype, batch, shift):
    da, oa = T.field(shape, batch, dtype)
    n = int(np.prod(shape))
    cdt = np.dtype("complex64" if dtype == "float32" else "complex128")
    kappa = {dim[0]: A.kappa(oa.values, o.detrend(oa, dim, "linear").values) for dim in ORDERS}
    for tp, ta, det, win, dim in itertools.product([True, False], [True, False], [None, "linear"], [None, "hann"], ORDERS):
        kw = dict(dim=dim, shift=shift, true_phase=tp, true_amplitude=ta, detrend=det, window=win)
        what = f"{shape} {dtype} batch {batch} {kw}"
        kap = kappa[dim[0]] if det else 0.0
        ref = o.fft(oa, **kw)
        for name in ("fft", "dft"):
            got = getattr(xa, name)(da, **kw)
            assert "[fasth]" in T.newest_plan(), what  # (fails on the composition: no plan of it is the last pass)
            assert np.asarray(got.values).dtype == cdt, what
            cases.check(got, ref, cases.TOL[dtype])
            A.assert_accurate(got.values, ref.values, dtype, n, kap, what=f"{name} {what}")
        if not tp:
            sm, tw = T.twin_columns(T.unshifted(np.asarray(got.values), shift))
            assert sm.size and np.array_equal(tw, np.conj(sm)), what  # without phase factors every twin is its sample's conjugate, bit for bit


# ---------------------------------------------------------------------------------- 2. the twin rule under true_phase
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] % 2 == 0 or s[1] % 2 == 0], **IDS)
def test_twins_at_nyquist_rows_carry_their_own_phase(shape, dtype):
    """fftfreq gives the index n / 2 of an even n the frequency -1 / (2 dx) for itself and for its own twin: on the rows kt = nt / 2 and ky = ny / 2 a twin's factor
    is NOT the conjugate of its sample's.  The origins of t and y are no multiples of the spacing (three_axis_fft.coords), so the factor there is not real."""
    da, oa = T.field(shape, 2, dtype)
    n = int(np.prod(shape))
    for shift in (True, False):
        kw = dict(dim=["t", "y", "x"], shift=shift, true_phase=True)
        got = T.unshifted(np.asarray(xa.fft(da, **kw).values), shift)
        assert "[fasth]" in T.newest_plan()
        ref = T.unshifted(o.fft(oa, **kw).values, shift)
        rows, rows_ref = T.nyquist_rows_of_twins(got), T.nyquist_rows_of_twins(ref)
        assert rows.size
        A.assert_accurate(rows, rows_ref, dtype, n, what=f"Nyquist rows of the twins {shape} {dtype} shift {shift}")
        # the check is sensitive: the plain conjugate of the sample, written there, misses the bound
        plain = np.conj(np.roll(ref[..., ::-1, ::-1, ::-1], 1, axis=(-3, -2, -1)))
        with pytest.raises(AssertionError):
            A.assert_accurate(T.nyquist_rows_of_twins(plain), rows_ref, dtype, n)


# ---------------------------------------------------------------------------------- 3. the plan: every element written, repeats, numpy, refusals
@pytest.mark.parametrize("phases", [False, True], ids=["nophase", "phase"])
@pytest.mark.parametrize("flags", [0, L.SHIFT_Y | L.SHIFT_X, L.SHIFT_X | L.ISHIFT_Y], ids=["plain", "shifted", "yx-shifted-ishift"])
@pytest.mark.parametrize("cdtype", [A.C64, A.C128], ids=["c64", "c128"])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_field_plan_against_numpy(shape, cdtype, flags, phases):
    nt, ny, nx = shape
    win = np.hanning(nt + 1)[:-1] + 0.5
    ph = T.phase_tables(shape) if phases else None
    extra = dict(phase_y=ph[0], phase_x=ph[1], phase_hx=ph[2]) if phases else {}
    p = A.make(**T.herm_field_kw(shape, cdtype, flags), window_y=win, **extra)
    assert A.family(p) == (L.K_FASTH, "fasth") and "field" in p.describe()
    h, h128 = T.half_spectrum(shape, 2, cdtype)
    outs = []
    for _ in range(2):
        buf = torch.full((2, nt, ny, nx), float("nan"), dtype=p.out_dtype())
        out, _ = p.execute(h, out=buf)
        assert out.data_ptr() == buf.data_ptr() and out.is_complex() and not torch.isnan(torch.view_as_real(out)).any()  # every element written
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    ref = T.field_plan_reference(h128, shape, flags, win, ph)
    # the contract of the ONE transform the plan does (N = nt); the three factors are three more roundings of the size of u, inside C_RMS log2 nt >= 6
    A.assert_accurate(outs[0].numpy(), ref, cdtype, nt, what=f"field plan {shape} flags {flags:#x} phases {phases}")
    if not phases:
        g = outs[0].numpy()
        g = np.fft.ifftshift(g, axes=1) if flags & L.SHIFT_Y else g
        g = np.fft.ifftshift(g, axes=(2, 3)) if flags & L.SHIFT_X else g
        sm, tw = T.twin_columns(g)
        assert sm.size and np.array_equal(tw, np.conj(sm))  # without tables the twin is the plain conjugate, bit for bit


def status_of(**kw):
    with pytest.raises(_lib.XrftHipError) as e:
        A.make(**kw)
    return e.value.status


def test_field_plan_refusals():
    good = T.herm_field_kw((8, 6, 10), A.C64)
    A.make(**good)
    assert status_of(ny=8, nx=36, dtype=A.C64, out_mode=L.OUT_COMPLEX, flags=L.AXIS_Y | L.HERM_FIELD) == L.BAD_ARG  # the flag without herm_ny / herm_nx
    assert status_of(ny=8, nx=36, dtype=A.F32, out_mode=L.OUT_COMPLEX, flags=L.HERM_FIELD) == L.BAD_ARG
    for mode in (L.OUT_POWER, L.OUT_CROSS, L.OUT_PHASE):
        assert status_of(**dict(good, out_mode=mode)) == L.BAD_ARG
    assert status_of(**dict(good, flags=L.AXIS_Y)) == L.BAD_ARG                       # COMPLEX without the flag: as ever
    assert status_of(**dict(good, window_x=np.ones(36))) == L.BAD_ARG                 # a window on the Hermitian axes
    assert status_of(**dict(good, phase_y=np.ones(9, dtype=complex))) == L.BAD_ARG    # tables of the wrong length: t ...
    assert status_of(**dict(good, phase_x=np.ones(36, dtype=complex))) == L.BAD_ARG   # ... y (herm_ny entries, not the plan's nx) ...
    assert status_of(**dict(good, phase_hx=np.ones(6, dtype=complex))) == L.BAD_ARG   # ... x (the FULL axis, not the stored half)
    A.make(**dict(good, phase_y=np.ones(8, dtype=complex), phase_x=np.ones(6, dtype=complex), phase_hx=np.ones(10, dtype=complex)))
    # a third table on any other plan
    assert status_of(ny=8, nx=36, dtype=A.C64, out_mode=L.OUT_COMPLEX, flags=L.AXIS_Y, phase_hx=np.ones(36, dtype=complex)) == L.BAD_ARG
    assert status_of(**dict(A.herm_kw((8, 6, 10), A.C64, L.OUT_POWER), phase_hx=np.ones(10, dtype=complex))) == L.BAD_ARG
    for f in (L.HALF_X, L.ISHIFT_X, L.FLIP_Y, L.FLIP_X, L.ISO, L.INVERSE, L.PHASE_IN, L.C2R_X, L.HALF_Y):
        assert status_of(**dict(good, flags=good["flags"] | f)) == L.BAD_ARG, hex(f)
    for f in (L.SHIFT_Y, L.ISHIFT_Y, L.SHIFT_X, L.SHIFT_Y | L.SHIFT_X | L.ISHIFT_Y):
        A.make(**dict(good, flags=good["flags"] | f))


def test_lengths_the_field_pass_declines_are_unsupported():
    assert status_of(**T.herm_field_kw((34, 4, 6), A.C128)) == L.UNSUPPORTED_LENGTH    # 2 x 17: no Rader form
    assert status_of(**T.herm_field_kw((103, 4, 6), A.C64)) == L.UNSUPPORTED_LENGTH    # a prime: no Bluestein form
    assert status_of(**T.herm_field_kw((2048, 4, 6), A.C64)) == L.UNSUPPORTED_LENGTH   # 1024 x 2: the tile of 128 output bytes per row (256 KB) does not fit the LDS
    for nt in (2, 7, 11, 13, 14, 77, 360, 1024):
        p = A.make(**T.herm_field_kw((nt, 4, 6), A.C128))
        assert A.family(p) == (L.K_FASTH, "fasth") and p.kernel_info()[1] == 8  # 8 complex128 columns = 128 bytes of an output row


# ---------------------------------------------------------------------------------- 4. fused against composed
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_fused_against_composed(shape, dtype):
    da, oa = T.field(shape, 2, dtype, seed=8)
    n = int(np.prod(shape))
    for det, win, shift, tp in itertools.product([None, "linear"], [None, "hann"], [True, False], [True, False]):
        kw = dict(dim=["t", "y", "x"], shift=shift, detrend=det, window=win, true_phase=tp)
        kap = A.kappa(oa.values, o.detrend(oa, kw["dim"], "linear").values) if det else 0.0
        fused = xa.fft(da, **kw)
        assert "[fasth]" in T.newest_plan()
        api._plan_cache.clear()
        comp = composed(lambda: xa.fft(da, **kw))
        assert api._plan_cache and T.no_fasth_plan()
        assert fused.dims == comp.dims
        A.assert_accurate(fused.values, comp.values, dtype, n, kap, what=f"fused vs composed {shape} {dtype} {kw}")


def test_labels_are_the_compositions():
    """Dims, coordinate names in their order, values and attributes (spacing, direct_lag) are what the composed stages give."""
    da, _ = T.field((8, 6, 10), 2, "float64")
    for dim, tp in itertools.product(ORDERS, [True, False]):
        call = lambda: xa.fft(da, dim=dim, window="hann", detrend="constant", true_phase=tp)  # noqa: E731
        fused = call()
        assert "[fasth]" in T.newest_plan()
        comp = composed(call)
        assert fused.dims == comp.dims and list(fused.coords) == list(comp.coords) and fused.name == comp.name and fused.attrs == comp.attrs
        for k in comp.coords:
            assert np.array_equal(fused[k].values, comp[k].values) and fused[k].attrs == comp[k].attrs and fused[k].dims == comp[k].dims, k


# ---------------------------------------------------------------------------------- 5. calls outside the route compose as before
def _declined(call):
    """The call's result with the switch on equals the composition's bits, and no plan of it is the last pass."""
    api._plan_cache.clear()
    on = call()
    assert api._plan_cache and T.no_fasth_plan()
    off = composed(call)
    assert on.dims == off.dims and np.array_equal(np.asarray(on.values), np.asarray(off.values), equal_nan=True)
    assert list(on.coords) == list(off.coords)


def test_a_descending_coordinate_composes():
    da, _ = T.field((8, 6, 10), 2, "float64")
    c = {k: v.values for k, v in da.coords.items()}
    c["y"] = c["y"][::-1].copy()
    dd = xa.DataArray(da.data, DIMS, c)
    _declined(lambda: xa.fft(dd, dim=["t", "y", "x"]))  # (true_phase: the flipped axis, xrft.py:436-441)


def test_complex_data_composes():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((2, 8, 6, 10)) + 1j * rng.standard_normal((2, 8, 6, 10))
    dc = xa.DataArray(torch.from_numpy(v), DIMS, T.coords((8, 6, 10), 2))
    _declined(lambda: xa.fft(dc, dim=["t", "y", "x"]))


def test_real_dim_composes():
    da, _ = T.field((8, 6, 10), 2, "float32")
    _declined(lambda: xa.fft(da, dim=["t", "y", "x"], real_dim="x", window="hann"))


def test_half_precision_input_composes():
    da, _ = T.field((8, 6, 10), 2, "float32")
    dh = xa.DataArray(torch.from_numpy(np.asarray(da.values)).to(torch.float16), DIMS, T.coords((8, 6, 10), 2))
    _declined(lambda: xa.fft(dh, dim=["t", "y", "x"]))


def test_other_than_the_trailing_three_axes_composes():
    rng = np.random.default_rng(3)
    c = dict(T.coords((8, 6, 10), 2))
    da = xa.DataArray(torch.from_numpy(rng.standard_normal((8, 6, 10, 2))), ("t", "y", "x", "b"), c)
    _declined(lambda: xa.fft(da, dim=["t", "y", "x"]))


def test_a_length_without_a_butterfly_composes():
    da, oa = T.field((34, 4, 6), 1, "float64")  # 34 = 2 x 17: the Rader form of the one-axis kernel is not carried over
    _declined(lambda: xa.fft(da, dim=["t", "y", "x"]))
    cases.check(xa.fft(da, dim=["t", "y", "x"]), o.fft(oa, dim=["t", "y", "x"]), cases.TOL["float64"])


def test_four_transform_dims_compose():
    da, _ = T.field((8, 6, 10), 4, "float64")
    _declined(lambda: xa.fft(da, dim=["b", "t", "y", "x"]))


# ---------------------------------------------------------------------------------- 6. a NaN stays in its own batch entry
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_nan_stays_in_its_batch_entry(dtype):
    da, _ = T.field((12, 7, 16), 3, dtype)
    v = np.asarray(da.values).copy()
    v[1, 5, 3, 9] = np.nan
    dn = xa.DataArray(v, DIMS, T.coords((12, 7, 16), 3))
    for kw in (dict(), dict(detrend="linear", window="hann", shift=False)):
        clean = np.asarray(xa.fft(da, dim=["t", "y", "x"], **kw).values)
        got = np.asarray(xa.fft(dn, dim=["t", "y", "x"], **kw).values)
        assert "[fasth]" in T.newest_plan()
        for b in (0, 2):
            assert np.array_equal(got[b], clean[b]), (b, kw)
