"""Isotropic spectra on non-trailing axes where the axes lie, on the emulated library: the per-element radial sums of the fused inner / mid
plans (csrc/fastn.h, fastn_irows_kernel<.., ISO>) at the plan level against long-double bin sums of the float64 spectrum, and
isotropic_power_spectrum / isotropic_cross_spectrum of (y, x, t) and (t, y, x) arrays against the oracle -- with no transposed copy: the plan
that ran is the "[inner layout]" one with a radial-sums line.  Calls the fused passes decline still answer through the transposing path."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

import xrft_amd as xa  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402
from xrft_amd import _lib, api  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402

import accuracy as A  # noqa: E402
import cases  # noqa: E402

TOL = {"float32": 2e-4, "float64": 1e-10}


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api._plan_cache.clear()
    _lib._load_for_testing(build_emu.build())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    api._plan_cache.clear()
    _lib._state.update(dll=None, path=None, device="cuda")


def newest_plan():
    return next(reversed(api._plan_cache.values())).describe()


def ran_in_place():
    d = newest_plan()
    return "[inner layout]" in d and any("[inner layout]" in line and "radial sums" in line for line in d.splitlines())


def element_bin_sums(spec, axes, bm, nbins):
    """Per-element bin sums of a 2-D spectrum held in `axes` of `spec` (long double, as accuracy.reference sums): [..other.., nbins]."""
    s = np.moveaxis(spec, axes, (-2, -1))
    flat = s.reshape(-1, s.shape[-2] * s.shape[-1])
    out = np.zeros((flat.shape[0], nbins), dtype=np.complex128 if np.iscomplexobj(spec) else np.float64)
    for i, row in enumerate(flat):
        for part in ("real", "imag") if np.iscomplexobj(spec) else ("real",):
            acc = np.zeros(nbins, dtype=np.longdouble)
            np.add.at(acc, bm.ravel(), getattr(row, part).astype(np.longdouble))
            out[i] += acc.astype(np.float64) * (1j if part == "imag" else 1.0)
    return out


# ---------------------------------------------------------------------------------- 1. the plan
@pytest.mark.parametrize("dtype", [A.F32, A.F64], ids=["float32", "float64"])
@pytest.mark.parametrize("mode", [L.OUT_POWER, L.OUT_CROSS], ids=["power", "cross"])
@pytest.mark.parametrize("lay", [dict(inner=6), dict(mid=5), dict(inner=7)], ids=["inner6", "mid5", "inner7"])
@pytest.mark.parametrize("store", [False, True], ids=["sums-only", "spectrum-too"])
def test_plan_radial_sums_per_element(lay, mode, dtype, store):
    """An ISO plan on an inner / mid layout (the parent: bad argument): its iso block [batch][ne][nbins] against per-element long-double bin
    sums of the float64 spectrum; with the spectrum stored too, that is the plain plan's."""
    flags = L.ISO | (0 if store else L.NO_SPECTRUM_OUT)
    kw = dict(ny=48, nx=40, out_mode=mode, dtype=dtype, detrend=L.DETREND_LINEAR, flags=flags, **lay)
    bm, nb = A.radial_map(48, 40)
    p = A.make(**kw, binmap=bm, nbins=nb)
    assert A.family(p) == (L.K_FASTN, "inner layout") and "radial sums" in p.describe()
    rng = np.random.default_rng(11)
    shape, axes, _ = A._axes(kw)
    x, x64 = A.tensor(rng.standard_normal(shape) + 0.1 * np.arange(48).reshape(1, 48, *([1] * (len(shape) - 2))), dtype)
    x1 = x164 = None
    if mode == L.OUT_CROSS:
        x1, x164 = A.tensor(rng.standard_normal(shape), dtype)
    out, iso = p.execute(x, x1)
    ref, _ = A.reference(dict(kw, flags=0), x64, x164)
    kap = A.kappa(x64.reshape(shape), A.detrended(x64.reshape(shape), axes, L.DETREND_LINEAR))
    ne = lay.get("inner", lay.get("mid"))
    assert tuple(iso.shape) == (2 * ne, nb)
    iref = element_bin_sums(ref, axes, bm, nb)
    A.assert_accurate(iso.numpy(), iref, dtype, 48 * 40, kap, what="per-element radial sums")
    if store:
        A.assert_accurate(out.numpy().reshape(ref.shape), ref, dtype, 48 * 40, kap, what="stored spectrum")
    else:
        assert out is None
    out2, iso2 = p.execute(x, x1)
    assert np.array_equal(iso2.numpy(), iso.numpy())  # (bit for bit: fixed order, no atomics)


def test_plan_workspace_counts_the_partial_table():
    bm, nb = A.radial_map(48, 40)
    plain = A.make(ny=48, nx=40, inner=6, batch=1)
    isop = A.make(ny=48, nx=40, inner=6, batch=1, flags=L.ISO | L.NO_SPECTRUM_OUT, binmap=bm, nbins=nb)
    assert isop.workspace_bytes >= plain.workspace_bytes + (48 // 2 + 1) * 6 * nb * 8
    crossp = A.make(ny=48, nx=40, inner=6, batch=1, out_mode=L.OUT_CROSS, flags=L.ISO | L.NO_SPECTRUM_OUT, binmap=bm, nbins=nb)
    plainc = A.make(ny=48, nx=40, inner=6, batch=1, out_mode=L.OUT_CROSS)
    assert crossp.workspace_bytes >= plainc.workspace_bytes + (48 // 2 + 1) * 6 * nb * 16


def test_plan_refuses_a_map_that_is_not_radial():
    bm, nb = A.radial_map(48, 40)
    sh = np.random.default_rng(0).permutation(bm.ravel()).reshape(bm.shape).astype(np.int32)
    with pytest.raises(_lib.XrftHipError) as e:
        A.make(ny=48, nx=40, inner=6, flags=L.ISO | L.NO_SPECTRUM_OUT, binmap=sh, nbins=nb)
    assert e.value.status == L.BAD_ARG


@pytest.mark.parametrize("kw", [dict(ny=48, nx=40, inner=6, mid=5), dict(ny=48, nx=51, inner=6), dict(ny=48, nx=40, inner=6, flags=L.HALF_X),
                                dict(ny=48, nx=40, inner=6, flags=L.FLIP_X, out_mode=L.OUT_CROSS), dict(ny=12, nx=40, inner=6)],
                         ids=["mid-and-inner", "prime17", "half", "flip", "short"])
def test_plan_declined_means_the_caller_transposes(kw):
    kw = dict(kw)
    kw["flags"] = kw.get("flags", 0) | L.ISO | L.NO_SPECTRUM_OUT
    with pytest.raises(_lib.XrftHipError) as e:
        A.make(**kw, binmap=A.radial_map(kw["ny"], kw["nx"])[0], nbins=A.radial_map(kw["ny"], kw["nx"])[1])
    assert e.value.status == L.UNSUPPORTED_LENGTH


# ---------------------------------------------------------------------------------- 2. the API
def field(order, ext, dtype, seed, plane=True):
    rng = np.random.default_rng(seed)
    shape = tuple(ext[d] for d in order)
    v = rng.standard_normal(shape)
    if plane:
        ii = {d: np.arange(ext[d]).reshape([-1 if e == d else 1 for e in order]) for d in order}
        a, b = [d for d in order if d != "t"][:2] if len(order) == 3 else ("y", "x")
        v = v + 0.05 * ii[a] - 0.03 * ii[b] + 2.0
    return v.astype(dtype)


def coords_of(ext, x0=0.0):
    return {"t": np.arange(ext["t"]) * 2.0, "y": np.arange(ext["y"]) * 0.5 + 1.0, "x": np.arange(ext["x"]) * 0.125 - 3.0 + x0}  # (anisotropic spacing)


LAYOUTS = [(("y", "x", "t"), ("y", "x")), (("t", "y", "x"), ("t", "x"))]
VARIANTS = [dict(), dict(detrend="constant"), dict(detrend="linear", window="hann")]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n0,n1", [(48, 40), (45, 40), (48, 35)])
@pytest.mark.parametrize("rev", [False, True], ids=["dim-in-order", "dim-reversed"])
@pytest.mark.parametrize("order,pair", LAYOUTS, ids=["yxt", "tyx"])
def test_isotropic_power_spectrum_where_the_axes_lie(order, pair, rev, n0, n1, dtype):
    other = [d for d in order if d not in pair][0]
    ext = {pair[0]: n0, pair[1]: n1, other: 6 if other == "t" else 5}
    v = field(order, ext, dtype, 3)
    da, od = cases.pair(v, order, coords_of(ext))
    dim = list(pair[::-1] if rev else pair)
    for var in VARIANTS:
        for truncate in (False, True):
            for nfactor in (1, 4):
                kw = dict(dim=dim, truncate=truncate, nfactor=nfactor, **var)
                api._plan_cache.clear()
                got = xa.isotropic_power_spectrum(da, **kw)
                assert ran_in_place(), (kw, newest_plan())
                ref = o.isotropic_power_spectrum(od, **kw)
                assert tuple(got.dims) == (other, "freq_r") == tuple(ref.dims)
                assert np.array_equal(np.asarray(got["freq_r"].values), np.asarray(ref.coord("freq_r")), equal_nan=True)
                cases.check(got, ref, TOL[dtype])
                A.assert_accurate(np.asarray(got.values), ref.values, dtype, n0 * n1,
                                  A.kappa(od.values, o.detrend(od, dim, var["detrend"]).transpose(*order).values) if var.get("detrend") else 0.0, what=str(kw))


# ---------------------------------------------------------------------------------- 3. cross spectra
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nt", [7, 9, 17])
@pytest.mark.parametrize("x0", [0.0, 0.375], ids=["same-coords", "offset-x"])
@pytest.mark.parametrize("order,pair", LAYOUTS, ids=["yxt", "tyx"])
def test_isotropic_cross_spectrum_where_the_axes_lie(order, pair, x0, nt, dtype):
    """Element counts that leave the last block of a row workgroup ragged; coordinates offset along x between the two fields: a true-phase
    factor that differs between a sample and its Hermitian twin (summed explicitly)."""
    other = [d for d in order if d not in pair][0]
    for n0, n1 in ((48, 40), (45, 35)):
        ext = {pair[0]: n0, pair[1]: n1, other: nt}
        da, od = cases.pair(field(order, ext, dtype, 5), order, coords_of(ext))
        db, ob = cases.pair(field(order, ext, dtype, 6, plane=False), order, coords_of(ext, x0))
        for var in (dict(), dict(detrend="linear", window="hann"), dict(true_phase=False)):
            kw = dict(dim=list(pair), **var)
            api._plan_cache.clear()
            got = xa.isotropic_cross_spectrum(da, db, **kw)
            assert ran_in_place(), (kw, newest_plan())
            ref = o.isotropic_cross_spectrum(od, ob, **kw)
            assert tuple(got.dims) == (other, "freq_r")
            cases.check(got, ref, TOL[dtype])
            if x0 and var.get("true_phase", True):
                noph = o.isotropic_cross_spectrum(od, ob, **dict(kw, true_phase=False))
                assert np.abs(noph.values - ref.values).max() > 1e-3 * np.abs(ref.values).max()  # (the factor is not trivial)


# ---------------------------------------------------------------------------------- 4. sum conservation, 5. repeats and layouts
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("order,pair", LAYOUTS, ids=["yxt", "tyx"])
def test_sum_conservation_repeats_and_the_transposed_call(order, pair, dtype):
    other = [d for d in order if d not in pair][0]
    ext = {pair[0]: 48, pair[1]: 40, other: 6}
    v = field(order, ext, dtype, 9)
    c = coords_of(ext)
    da, od = cases.pair(v, order, c)
    kw = dict(dim=list(pair), detrend="linear", window="hann")
    api._plan_cache.clear()
    got = xa.isotropic_power_spectrum(da, truncate=False, **kw)
    assert ran_in_place()
    # (test_xrft.py:963) the radial sums conserve the spectrum's total, per element
    ps = o.power_spectrum(od, **kw)
    tot = ps.values.sum(axis=tuple(ps.dims.index("freq_" + d) for d in pair))
    kap = A.kappa(od.values, o.detrend(od, list(pair), "linear").transpose(*order).values)
    A.assert_accurate(np.asarray(got.values).sum(axis=-1), tot, dtype, 48 * 40, kap, what="sum over freq_r")
    assert np.array_equal(np.asarray(xa.isotropic_power_spectrum(da, truncate=False, **kw).values), np.asarray(got.values))  # bit for bit
    # the same call on the array with the transform axes trailing (another plan family, another summation order): the same bound, not the same bits
    last = (other,) + tuple(pair)
    dt, odt = cases.pair(np.ascontiguousarray(v.transpose([order.index(d) for d in last])), last, c)
    api._plan_cache.clear()
    alt = xa.isotropic_power_spectrum(dt, truncate=False, **kw)
    assert "[inner layout]" not in newest_plan()
    ref = o.isotropic_power_spectrum(od, truncate=False, **kw)
    assert tuple(alt.dims) == tuple(got.dims)
    cases.check(alt, ref, TOL[dtype])
    cases.check(got, ref, TOL[dtype])
    A.assert_accurate(np.asarray(got.values), np.asarray(alt.values), dtype, 48 * 40, kap, what="in place against transposed")


# ---------------------------------------------------------------------------------- 6. what the fused passes decline
def test_fallbacks_still_answer_through_the_transposing_path():
    rng = np.random.default_rng(21)
    # (a, y, b, x, c): elements between AND behind the axes
    v = rng.standard_normal((2, 32, 3, 24, 2))
    c = {"a": np.arange(2.0), "y": np.arange(32) * 0.5, "b": np.arange(3.0), "x": np.arange(24) * 0.25, "c": np.arange(2.0)}
    da, od = cases.pair(v, ("a", "y", "b", "x", "c"), c)
    api._plan_cache.clear()
    got = xa.isotropic_power_spectrum(da, dim=["y", "x"], detrend="constant")
    assert not ran_in_place()
    cases.check(got, o.isotropic_power_spectrum(od, dim=["y", "x"], detrend="constant"), 1e-10)
    # a descending x coordinate with true_phase (a flipped axis), two fields
    ext = {"y": 48, "x": 40, "t": 4}
    cd = coords_of(ext)
    cd["x"] = cd["x"][::-1].copy()
    a, oa = cases.pair(field(("y", "x", "t"), ext, "float64", 1), ("y", "x", "t"), cd)
    b, ob = cases.pair(field(("y", "x", "t"), ext, "float64", 2), ("y", "x", "t"), cd)
    api._plan_cache.clear()
    got = xa.isotropic_cross_spectrum(a, b, dim=["y", "x"], true_phase=True)
    assert not ran_in_place()
    cases.check(got, o.isotropic_cross_spectrum(oa, ob, dim=["y", "x"], true_phase=True), 1e-10)
    # 51 = 3 x 17 on the second axis: no butterfly for 17 in the fused passes
    ext = {"y": 48, "x": 51, "t": 4}
    a, oa = cases.pair(field(("y", "x", "t"), ext, "float64", 3), ("y", "x", "t"), coords_of(ext))
    api._plan_cache.clear()
    got = xa.isotropic_power_spectrum(a, dim=["y", "x"], detrend="linear", window="hann")
    assert not ran_in_place()
    cases.check(got, o.isotropic_power_spectrum(oa, dim=["y", "x"], detrend="linear", window="hann"), 1e-10)
    # real_dim
    ext = {"y": 48, "x": 40, "t": 4}
    a, oa = cases.pair(field(("y", "x", "t"), ext, "float64", 4), ("y", "x", "t"), coords_of(ext))
    api._plan_cache.clear()
    try:
        ref = o.isotropic_power_spectrum(oa, dim=["y", "x"], real_dim="x")
    except Exception as e:  # (the oracle refuses: so must the product)
        with pytest.raises(type(e)):
            xa.isotropic_power_spectrum(a, dim=["y", "x"], real_dim="x")
    else:
        got = xa.isotropic_power_spectrum(a, dim=["y", "x"], real_dim="x")
        assert not ran_in_place()
        cases.check(got, ref, 1e-10)


# ---------------------------------------------------------------------------------- 7. a NaN stays in its element
@pytest.mark.parametrize("kw", [dict(), dict(detrend="linear", window="hann")], ids=["plain", "linear-hann"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nt", [6, 7])
@pytest.mark.parametrize("order,pair", LAYOUTS, ids=["yxt", "tyx"])
def test_a_nan_poisons_its_own_element_only(order, pair, nt, dtype, kw):
    """A NaN in element 2: every other element's sums finite and the oracle's, element 2 NaN wherever the oracle's are.  The column pass of the fused
    plans packs two adjacent columns of the view -- with the elements innermost, elements e and e + 1 of one x -- into one complex sequence; its guarded
    form (fastn_cols_kernel<.., GUARD>) keeps a sample that is not finite out of the shared transform and marks its own column instead."""
    other = [d for d in order if d not in pair][0]
    ext = {pair[0]: 48, pair[1]: 40, other: nt}
    v = field(order, ext, dtype, 13)
    idx = {pair[0]: 5, pair[1]: 7, other: 2}
    v[tuple(idx[d] for d in order)] = np.nan
    da, od = cases.pair(v, order, coords_of(ext))
    api._plan_cache.clear()
    got = np.asarray(xa.isotropic_power_spectrum(da, dim=list(pair), **kw).values)
    assert ran_in_place()
    ref = o.isotropic_power_spectrum(od, dim=list(pair), **kw).values
    keep = np.arange(nt) != 2
    assert np.all(np.isfinite(got[keep])), np.argwhere(~np.isfinite(got))[:, 0]
    assert np.abs(got[keep] - ref[keep]).max() < TOL[dtype] * np.abs(ref[keep]).max()
    assert np.all(np.isnan(got[2][np.isnan(ref[2])])) and np.isnan(ref[2]).any()
    # ... and in a cross spectrum, whichever field holds it
    w = field(order, ext, dtype, 14, plane=False)
    db, ob = cases.pair(w, order, coords_of(ext))
    for a, b, oa, ob_ in ((da, db, od, ob), (db, da, ob, od)):
        gc = np.asarray(xa.isotropic_cross_spectrum(a, b, dim=list(pair), **kw).values)
        assert ran_in_place()
        rc = o.isotropic_cross_spectrum(oa, ob_, dim=list(pair), **kw).values
        assert np.all(np.isfinite(gc[keep])) and np.abs(gc[keep] - rc[keep]).max() < TOL[dtype] * np.abs(rc[keep]).max()
        assert np.all(np.isnan(gc[2].real[np.isnan(rc[2].real)]))
