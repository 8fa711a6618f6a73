"""A NaN or an inf stays inside its own transform: shared by tests/test_nonfinite_emulated.py (CPU, the emulated library) and tests/test_gpu_nonfinite.py (GPU).
Not a conftest: imported by the tests that use it.

Several kernel families pack two INDEPENDENT real sequences into one complex transform (two rows, two columns, two elements of an inner layout) and split the
result afterwards; a sample that is not finite in one of them would fill the other's spectrum too.  The reference (numpy.fft along the axis) transforms every
sequence on its own.  The contract, for one call and a chosen set B of its independent transforms (rows of a 1-D plan; (batch, column) of AXIS_Y; (batch,
element) of an inner layout; (batch, mid, element); slabs of a plain two-axis plan), each holding one sample that is not finite:

  1. every transform NOT in B -- all of them, B is known by construction -- meets the rounding-level contract of tests/accuracy.py against the float64
     transform of the same samples;
  2. every output element of a transform in B is not finite (which of NaN / inf is not asserted: the guarded kernels store NaN); C2R_X: at least one is
     (numpy's irfft itself leaves half of such a transform finite);
  3. two fields (cross spectrum, cross phase): the same with the bad sample in field 0, and in field 1;
  4. two executions give the same bits (NaN payloads aside).

The routed family is asserted before anything is executed.  No leaking family reads strided or half-precision input (test: they decline), so the dense float
loader is the only one to guard."""
import numpy as np
import torch

from xrft_amd import _lib as L

import accuracy as A

F32, F64, C64, C128 = A.F32, A.F64, A.C64, A.C128
Y = L.AXIS_Y
C2R = L.INVERSE | L.C2R_X
BAD = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}

# (id, make() arguments without batch, environment, expected kind, expected tag): the forms that pack two independent transforms into one, at the smallest shape
# that still routes to the family and still exercises its pairing (fastm x-only at 1000 points: two -- float32 four -- row pairs per workgroup, at 100 points
# four; fastg y-only in its radix (96), chirp (103 float64), Rader (103 float32) and prime-factor Rader (365 = 5 x 73) forms)
PACKED = [
    ("fastmx", dict(ndim=1, nx=1000, dtype=F64), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-f32", dict(ndim=1, nx=1000), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-100", dict(ndim=1, nx=100, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-complex", dict(ndim=1, nx=1000, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-f32-half", dict(ndim=1, nx=1000, flags=L.HALF_X), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-half-x2", dict(ndim=1, nx=1000, dtype=F64, flags=L.HALF_X | L.REALDIM_X2), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-cross", dict(ndim=1, nx=1000, dtype=F64, out_mode=L.OUT_CROSS), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-phase", dict(ndim=1, nx=1000, out_mode=L.OUT_PHASE), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-c2r", dict(ndim=1, nx=1000, dtype=C128, out_mode=L.OUT_COMPLEX, flags=C2R), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-c2r-c64", dict(ndim=1, nx=100, dtype=C64, out_mode=L.OUT_COMPLEX, flags=C2R), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastgy-rows", dict(ndim=1, nx=365, dtype=F64), {}, L.K_FASTG_ROWS, "fastg rows Rader"),
    ("fastgy-rows-complex-f32", dict(ndim=1, nx=365, out_mode=L.OUT_COMPLEX), {}, L.K_FASTG_ROWS, "fastg rows Rader"),
    ("fastgy-rows-half", dict(ndim=1, nx=365, dtype=F64, flags=L.HALF_X | L.REALDIM_X2), {}, L.K_FASTG_ROWS, "fastg rows Rader"),
    ("fastgy-rows-cross", dict(ndim=1, nx=365, dtype=F64, out_mode=L.OUT_CROSS), {}, L.K_FASTG_ROWS, "fastg rows Rader"),
    ("fastmy", dict(ny=100, nx=200, dtype=F64, flags=Y), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastmy-complex-f32", dict(ny=100, nx=200, flags=Y, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastmy-half", dict(ny=100, nx=200, dtype=F64, flags=Y | L.HALF_X), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastmy-cross", dict(ny=100, nx=200, dtype=F64, flags=Y, out_mode=L.OUT_CROSS), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastmy-phase", dict(ny=100, nx=200, flags=Y, out_mode=L.OUT_PHASE), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastgy", dict(ny=103, nx=206, dtype=F64, flags=Y), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fastgy-complex-f32", dict(ny=103, nx=206, flags=Y, out_mode=L.OUT_COMPLEX), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fastgy-radix", dict(ny=96, nx=206, dtype=F64, flags=Y, out_mode=L.OUT_COMPLEX), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fastgy-rader", dict(ny=365, nx=16, flags=Y), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fastgy-half", dict(ny=96, nx=206, flags=Y | L.HALF_X | L.REALDIM_X2), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fastgy-cross", dict(ny=103, nx=206, dtype=F64, flags=Y, out_mode=L.OUT_CROSS), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fastgy-phase", dict(ny=96, nx=206, flags=Y, out_mode=L.OUT_PHASE), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fastmy-off", dict(ny=100, nx=200, dtype=F64, flags=Y), {"XRFTHIP_FASTM": "0"}, L.K_FASTG_Y, "fastg y-only"),
    ("fusedi-f32", dict(ny=33, nx=32, inner=4), {}, L.K_FASTN, "inner layout"),
    ("fusedi-complex-f64", dict(ny=33, nx=32, inner=4, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "inner layout"),
    ("fusedi-odd-inner", dict(ny=33, nx=32, inner=3, dtype=F64), {}, L.K_FASTN, "inner layout"),
    ("fusedi-128x256", dict(ny=128, nx=256, inner=4), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-x", dict(ny=32, nx=48, inner=4, flags=L.HALF_X), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-y-odd", dict(ny=33, nx=32, inner=4, dtype=F64, flags=L.HALF_Y, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-y-odd-power-x2", dict(ny=33, nx=32, inner=4, flags=L.HALF_Y | L.REALDIM_X2), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-y-odd-cross-x2", dict(ny=33, nx=32, inner=4, dtype=F64, out_mode=L.OUT_CROSS, flags=L.HALF_Y | L.REALDIM_X2), {}, L.K_FASTN, "inner layout"),
    ("fusedi-cross", dict(ny=32, nx=48, inner=4, dtype=F64, out_mode=L.OUT_CROSS), {}, L.K_FASTN, "inner layout"),
    ("fusedi-rader-cols", dict(ny=146, nx=16, inner=4, dtype=F64), {}, L.K_FASTN, "inner layout"),
]
# one representative of every family that does not pack independent transforms: a later change that starts pairing there is caught
CONTAINED = [
    ("fasts", dict(ny=64, nx=128), {}, L.K_FASTS, "fasts"),
    ("fastg", dict(ny=50, nx=50, dtype=F64), {}, L.K_FASTG, "fastg"),
    ("fastg-rows", dict(ndim=1, nx=50, dtype=F64), {}, L.K_FASTG_ROWS, "fastg rows"),
    ("fastr", dict(ndim=1, nx=65536), {}, L.K_FASTR, "fastr"),
    ("fasty-complex-rows", dict(ndim=1, nx=2048, dtype=C64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTR, "fasty complex rows"),
    ("fastn-small", dict(ny=125, nx=250, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "fastn"),
    ("fastm-small", dict(ny=180, nx=360, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM, "fastm"),
    ("fasty-small", dict(ny=256, nx=512), {}, L.K_FASTY, "fasty"),
    ("composite", dict(ny=128, nx=256, dtype=C64, out_mode=L.OUT_COMPLEX, mid=4), {}, L.K_COMPOSITE, "inner layout"),
    ("fusedm-complex", dict(ny=64, nx=96, mid=3, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "inner layout"),
    ("generic-prime", dict(ndim=1, nx=1031, dtype=F64), {}, L.K_GENERIC, "main"),
    ("fastmx-complex-in", dict(ndim=1, nx=1000, dtype=C128, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmy-inverse", dict(ny=100, nx=200, dtype=C128, flags=Y | L.INVERSE, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM_Y, "fastm y-only"),
    # an odd number of columns along a non-trailing axis leaves the y-only kernels (they take whole column pairs): the generic column tiles
    ("axis-y-odd-100x201", dict(ny=100, nx=201, dtype=F64, flags=Y), {}, L.K_GENERIC, "main"),
    ("axis-y-odd-103x205", dict(ny=103, nx=205, flags=Y), {}, L.K_GENERIC, "main"),
]
ROWS = {r[0]: r for r in PACKED + CONTAINED}


def tshape(kw):
    """The shape of the independent transforms of a make() descriptor: the input's shape without the transform axes."""
    shape, axes, _ = A._axes(dict(kw, batch=kw.get("batch", 2)))
    return tuple(n for a, n in enumerate(shape) if a not in axes)


def positions(kw):
    """{name: flat index of a transform}: the first, the second, the last (the unpaired tail of an odd count), one in the middle and -- transforms inside a batch
    entry -- the first of the LAST batch entry (its last is the last of all)."""
    ts = tshape(kw)
    n = int(np.prod(ts))
    pos = {"first": 0, "second": 1, "last": n - 1, "middle": n // 2}
    if len(ts) > 1 and ts[0] > 1:
        pos["first-of-last-entry"] = n - n // ts[0]
    return {k: v for k, v in pos.items() if 0 <= v < n}


def _two(kw):
    return kw.get("out_mode", L.OUT_POWER) in (L.OUT_CROSS, L.OUT_PHASE)


def params():
    """(id, row id, batch, B as flat transform indices, position inside the bad transform, bad value, detrend, field that holds it)"""
    out = []
    for rid, kw, _env, _kind, _tag in PACKED + CONTAINED:
        packed = rid in {r[0] for r in PACKED}
        c2r = bool(kw.get("flags", 0) & L.C2R_X)
        one_d = len(tshape(dict(kw, batch=5))) == 1
        for batch in (5,) if one_d or not packed else (5, 1):  # (one entry: pairing can only happen across columns or elements; rows and slabs have nothing else to check)
            k = dict(kw, batch=batch)
            for i, (pname, j) in enumerate(positions(k).items()):
                if not packed and pname not in ("second", "last"):
                    continue
                out.append((f"{rid}-b{batch}-{pname}", rid, batch, (j,), "first" if i % 2 == 0 else "last", "nan", L.DETREND_NONE, 0))
        if not packed:
            continue
        k = dict(kw, batch=5)
        n = int(np.prod(tshape(k)))
        out.append((f"{rid}-both-partners", rid, 5, (2, 3), "last", "nan", L.DETREND_NONE, 0))
        out.append((f"{rid}-pinf", rid, 5, (1,), "last", "pinf", L.DETREND_NONE, 0))
        out.append((f"{rid}-ninf", rid, 5, (n - 1,), "first", "ninf", L.DETREND_NONE, 0))
        if not c2r:  # (an inverse real transform takes no detrend)
            out.append((f"{rid}-constant", rid, 5, (1,), "first", "nan", L.DETREND_CONSTANT, 0))
            out.append((f"{rid}-linear", rid, 5, (n - 1,), "last", "nan", L.DETREND_LINEAR, 0))
            out.append((f"{rid}-linear-pinf", rid, 5, (0,), "last", "pinf", L.DETREND_LINEAR, 0))
        if _two(kw):
            for pname in ("first", "second", "last"):
                out.append((f"{rid}-field1-{pname}", rid, 5, (positions(k)[pname],), "last", "nan", L.DETREND_NONE, 1))
            out.append((f"{rid}-field1-linear", rid, 5, (1,), "first", "ninf", L.DETREND_LINEAR, 1))
    return out


def _same_bits(a, b):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a.cpu(), b.cpu()))
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na], b[~nb]))


def run_case(rid, batch, B, inpos, bad, detrend, field, dev, seed=0):
    """One case on `dev` ("cpu": the emulated library, "cuda": the real one), the caller having set the row's environment.  Returns the plan."""
    _rid, kw, _env, kind, tag = ROWS[rid]
    kw = dict(kw, batch=batch, detrend=detrend)
    p = A.make(**kw)
    assert A.family(p) == (kind, tag), (A.family(p), kind, tag)  # (first: a routing change must not move the case onto another kernel)
    dt = kw.get("dtype", F32)
    shape, axes, _ = A._axes(kw)
    mode, flags = kw.get("out_mode", L.OUT_POWER), kw.get("flags", 0)
    c2r = bool(flags & L.C2R_X)
    rng = np.random.default_rng(seed)
    fields = []
    for f in range(2 if _two(kw) else 1):
        v = A.signal(kw, "noise", rng)
        if c2r:
            v = np.fft.rfftn(A.signal(dict(kw, dtype=F64), "noise", rng), axes=axes)
        if f == field:
            t = v.copy() if c2r else _split_out(v, kw).copy()  # (c2r: 1-D plans only, [row][half spectrum])
            for j in B:
                t[j, 0 if inpos == "first" else -1] = BAD[bad]
            if c2r:
                v = t
            else:
                keep = [i for i in range(len(shape)) if i not in axes]
                v = np.transpose(t.reshape([shape[i] for i in keep] + [shape[i] for i in axes]), np.argsort(keep + list(axes)))
        fields.append(A.tensor(v, dt))
    x, x64 = fields[0]
    x1, x164 = fields[1] if len(fields) > 1 else (None, None)
    with np.errstate(all="ignore"):
        ref, _ = A.reference(dict(kw, out_mode=L.OUT_CROSS) if mode == L.OUT_PHASE else kw, x64, x164)
    out, _ = p.execute(x.to(dev), None if x1 is None else x1.to(dev))
    out2, _ = p.execute(x.to(dev), None if x1 is None else x1.to(dev))
    got = out.cpu().numpy().reshape(ref.shape)
    n_t = int(np.prod(tshape(kw)))
    inb = np.zeros(n_t, dtype=bool)
    inb[list(B)] = True
    r_t, g_t = _split_out(ref, kw), _split_out(got, kw)
    what = f"{rid} batch {batch} B {B} at the {inpos} sample = {bad}, detrend {detrend}, field {field}"
    assert np.isfinite(r_t[~inb]).all(), what  # (the reference keeps the sample in its own transform: numpy along the axis)
    # 1. containment: every transform outside B, none skipped, to rounding
    kap = 0.0
    if detrend:
        clean = np.where(np.isfinite(x64), x64, 0.0).reshape(shape)  # (the detrend is per transform: those of B are left out below)
        kap = A.kappa(_split_out(clean, kw)[~inb], _split_out(A.detrended(clean, axes, detrend), kw)[~inb])
    n = A.points(kw)
    if mode == L.OUT_PHASE:
        A.assert_accurate(np.abs(r_t[~inb]) * np.exp(1j * g_t[~inb].astype(np.float64)), r_t[~inb], dt, n, kap, what=what + " (phase)")
    else:
        A.assert_accurate(g_t[~inb], r_t[~inb], dt, n, kap, flat=(mode == L.OUT_COMPLEX and not c2r), what=what)
    # 2. no laundering: a transform in B comes out not finite
    if c2r:
        assert (~np.isfinite(g_t[inb])).any(axis=1).all(), what
    else:
        assert (~np.isfinite(g_t[inb])).all(), f"{what}: {int(np.isfinite(g_t[inb]).sum())} finite values in the transforms of B"
    # 4. repeatability
    assert _same_bits(out, out2), what
    return p


def _split_out(a, kw):
    """[transform][points] of a RESULT (a transform axis may be halved: the result's own extents)."""
    shape, axes, _ = A._axes(kw)
    a = np.asarray(a)
    keep = [i for i in range(len(shape)) if i not in axes]
    a = np.transpose(a, keep + list(axes))
    return a.reshape(int(np.prod([shape[i] for i in keep])), -1)


def run_declines_other_loaders(rid):
    """The packed families read dense input of the plan's own precision only, so there is no second loader to guard.  Held per row, by the status the library
    documents: a float16 / bfloat16 plan of a real row answers UNSUPPORTED_LENGTH ("the caller widens"); a strided 1-D plan (rows 8 samples apart: 16-byte
    multiples in every precision) answers UNSUPPORTED_LENGTH ("the caller copies") or is served by ANOTHER family; a strided plan of an AXIS_Y or inner layout
    answers BAD_ARG ("those layouts stay dense").  Returns what was tried."""
    _rid, kw, _env, kind, tag = ROWS[rid]
    real = kw.get("dtype", F32) in (F32, F64)
    tried = []
    if real:
        for h in (torch.float16, torch.bfloat16):
            try:
                p = A.make(batch=2, **dict(kw, dtype=h))
            except L.XrftHipError as e:
                assert e.status == L.UNSUPPORTED_LENGTH, (rid, h, e.status)
                tried.append((str(h), "declined"))
                continue
            assert A.family(p) != (kind, tag), (rid, h, A.family(p))
            tried.append((str(h), A.family(p)))
    if kw.get("ndim", 2) == 1:
        row = kw["nx"] // 2 + 1 if kw.get("flags", 0) & L.C2R_X else kw["nx"]
        try:
            p = A.make(batch=2, **dict(kw, in_stride_batch=row + 8))
        except L.XrftHipError as e:
            assert e.status == L.UNSUPPORTED_LENGTH, (rid, "strided", e.status)
            tried.append(("strided", "declined"))
        else:
            assert A.family(p) != (kind, tag), (rid, "strided", A.family(p))
            tried.append(("strided", A.family(p)))
    else:
        shape, _ax, _ = A._axes(dict(kw, batch=2))
        pitch = int(np.prod(shape[2:])) + 8
        try:
            A.make(batch=2, **dict(kw, in_stride_y=pitch, in_stride_batch=shape[1] * pitch))
        except L.XrftHipError as e:
            assert e.status == L.BAD_ARG, (rid, "strided", e.status)
            tried.append(("strided", "bad argument"))
        else:
            raise AssertionError(f"{rid}: a strided plan of a layout that stays dense was created")
    assert tried
    return tried


# ---------------------------------------------------------------------------------- the labelled API: a land mask on a (t, y, x) cube
# sizes: (24, 5, 7) -- the cube that leaked: t innermost over ["y", "x"] is the composite inner layout, one axis the fastg y-only kernel; (4, 33, 32) -- the fused
# inner-layout passes over ["y", "x"]; (100, 4, 6) -- the fastm y-only kernel along t, and with t innermost the fastm x-only kernel; (365, 3, 4) -- with t
# innermost the Rader rows of the fastg y-only kernel (a sequence = two rows), elsewhere its Rader columns
API_SIZES = [(24, 5, 7), (4, 33, 32), (100, 4, 6), (365, 3, 4)]
API_DIMS = [["t"], ["y"], ["x"], ["y", "x"]]
API_DETREND = [(None, None), ("constant", None), ("linear", None), (None, "hann"), ("constant", "hann"), ("linear", "hann")]


def api_params():
    out = []
    for size in API_SIZES:
        for order in A.ORDERS:
            for dim in API_DIMS:
                out.append((f"{'x'.join(map(str, size))}-{''.join(order)}-{''.join(dim)}", size, order, dim))
    return out


def run_api_land_mask(size, order, dim, dtype, seed=5):
    """fft / power_spectrum / cross_spectrum (the mask on either field) of a cube with one NaN element and one all-NaN transform, under every detrend and
    window: finite exactly where the oracle is, to rounding there; a refusal of the oracle is the product's refusal.  Returns the families that ran."""
    import pytest

    import xrft_amd as xa
    from oracle import xrft_oracle as o
    from xrft_amd import api

    import cases

    ext = dict(zip(("t", "y", "x"), size))
    shape = tuple(ext[d] for d in order)
    coords = {d: np.arange(ext[d]) * 0.5 for d in ext}
    rng = np.random.default_rng(seed)
    v0, v1 = rng.standard_normal(shape), rng.standard_normal(shape)
    rest = [d for d in order if d not in dim]
    masked = v0.copy()
    one = {d: (1 if ext[d] > 1 else 0) for d in order}
    masked[tuple(one[d] for d in order)] = np.nan                                        # one element
    masked[tuple(slice(None) if d in dim else ext[d] - 1 for d in order)] = np.nan       # one whole transform: the last
    n = int(np.prod([ext[d] for d in dim]))
    fams = set()
    api._plan_cache.clear()
    for det, win in API_DETREND:
        for op in ("fft", "power_spectrum", "cross_spectrum", "cross_spectrum_mask_on_field_1"):
            a, oa = cases.pair(masked.astype(dtype), order, coords)
            b, ob = cases.pair(v1.astype(dtype), order, coords)
            if op == "cross_spectrum_mask_on_field_1":
                a, oa, b, ob = b, ob, a, oa

            def call(mod, p, q):
                if op == "fft":
                    return mod.fft(p, dim=dim, detrend=det, window=win)
                if op == "power_spectrum":
                    return mod.power_spectrum(p, dim=dim, detrend=det, window=win)
                return mod.cross_spectrum(p, q, dim=dim, detrend=det, window=win)

            what = f"{op} {size} {order} dim={dim} detrend={det} window={win} {dtype}"
            try:
                with np.errstate(all="ignore"):
                    ref = call(o, oa, ob)
            except Exception as e:  # the oracle refuses: the product must refuse the same way
                with pytest.raises(type(e)):
                    call(xa, a, b)
                continue
            got = call(xa, a, b)
            assert tuple(got.dims) == tuple(ref.dims), what
            g, r = np.asarray(got.values), np.asarray(ref.values)
            fin = np.isfinite(r)
            assert np.array_equal(np.isfinite(g), fin), f"{what}: {int((np.isfinite(g) != fin).sum())} values finite on one side only"
            kap = 0.0
            if det:
                clean = np.where(np.isfinite(masked), masked, 0.0)
                kap = A.kappa(clean, o.detrend(o.OArr(clean, order, coords), dim, det).transpose(*order).values)
            A.assert_accurate(g[fin], r[fin], dtype, n, kap, what=what)
    for p in api._plan_cache.values():
        fams.add(A.family(p))
    assert rest and fams, (rest, fams)
    return fams


# the families that run for every cube, memory order and dim (api._plan_cache / describe(), the same in float64 and float32), as observed when the cases were
# written: a routing change fails the case instead of quietly testing another kernel.  Every packed family is reached: "fastm x-only" (100 samples along an innermost
# t), "fastg rows Rader" (365 along an innermost t), "fastm y-only", "fastg y-only" (radix and Rader columns) and the fused "inner layout" passes.
API_FAMILY = {
    "24x5x7-tyx-t": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-tyx-y": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-tyx-x": {(L.K_FASTG_ROWS, "fastg rows")},
    "24x5x7-tyx-yx": {(L.K_FASTG, "fastg")},
    "24x5x7-txy-t": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-txy-y": {(L.K_FASTG_ROWS, "fastg rows")},
    "24x5x7-txy-x": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-txy-yx": {(L.K_FASTG, "fastg")},
    "24x5x7-ytx-t": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-ytx-y": {(L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-ytx-x": {(L.K_FASTG_ROWS, "fastg rows")},
    "24x5x7-ytx-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "24x5x7-yxt-t": {(L.K_FASTG_ROWS, "fastg rows")},
    "24x5x7-yxt-y": {(L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-yxt-x": {(L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-yxt-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "24x5x7-xty-t": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-xty-y": {(L.K_FASTG_ROWS, "fastg rows")},
    "24x5x7-xty-x": {(L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-xty-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "24x5x7-xyt-t": {(L.K_FASTG_ROWS, "fastg rows")},
    "24x5x7-xyt-y": {(L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-xyt-x": {(L.K_FASTG_Y, "fastg y-only")},
    "24x5x7-xyt-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "4x33x32-tyx-t": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-tyx-y": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-tyx-x": {(L.K_FASTG_ROWS, "fastg rows")},
    "4x33x32-tyx-yx": {(L.K_FASTG, "fastg")},
    "4x33x32-txy-t": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-txy-y": {(L.K_FASTG_ROWS, "fastg rows")},
    "4x33x32-txy-x": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-txy-yx": {(L.K_FASTG, "fastg")},
    "4x33x32-ytx-t": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-ytx-y": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-ytx-x": {(L.K_FASTG_ROWS, "fastg rows")},
    "4x33x32-ytx-yx": {(L.K_FASTN, "inner layout")},
    "4x33x32-yxt-t": {(L.K_FASTG_ROWS, "fastg rows")},
    "4x33x32-yxt-y": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-yxt-x": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-yxt-yx": {(L.K_FASTN, "inner layout")},
    "4x33x32-xty-t": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-xty-y": {(L.K_FASTG_ROWS, "fastg rows")},
    "4x33x32-xty-x": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-xty-yx": {(L.K_FASTN, "inner layout")},
    "4x33x32-xyt-t": {(L.K_FASTG_ROWS, "fastg rows")},
    "4x33x32-xyt-y": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-xyt-x": {(L.K_FASTG_Y, "fastg y-only")},
    "4x33x32-xyt-yx": {(L.K_FASTN, "inner layout")},
    "100x4x6-tyx-t": {(L.K_FASTM_Y, "fastm y-only")},
    "100x4x6-tyx-y": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-tyx-x": {(L.K_FASTG_ROWS, "fastg rows")},
    "100x4x6-tyx-yx": {(L.K_FASTG, "fastg")},
    "100x4x6-txy-t": {(L.K_FASTM_Y, "fastm y-only")},
    "100x4x6-txy-y": {(L.K_FASTG_ROWS, "fastg rows")},
    "100x4x6-txy-x": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-txy-yx": {(L.K_FASTG, "fastg")},
    "100x4x6-ytx-t": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-ytx-y": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-ytx-x": {(L.K_FASTG_ROWS, "fastg rows")},
    "100x4x6-ytx-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "100x4x6-yxt-t": {(L.K_FASTM_X, "fastm x-only")},
    "100x4x6-yxt-y": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-yxt-x": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-yxt-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "100x4x6-xty-t": {(L.K_FASTM_Y, "fastm y-only"), (L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-xty-y": {(L.K_FASTG_ROWS, "fastg rows")},
    "100x4x6-xty-x": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-xty-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "100x4x6-xyt-t": {(L.K_FASTM_X, "fastm x-only")},
    "100x4x6-xyt-y": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-xyt-x": {(L.K_FASTG_Y, "fastg y-only")},
    "100x4x6-xyt-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "365x3x4-tyx-t": {(L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-tyx-y": {(L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-tyx-x": {(L.K_FASTG_ROWS, "fastg rows")},
    "365x3x4-tyx-yx": {(L.K_FASTG, "fastg")},
    "365x3x4-txy-t": {(L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-txy-y": {(L.K_FASTG_ROWS, "fastg rows")},
    "365x3x4-txy-x": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-txy-yx": {(L.K_FASTG, "fastg")},
    "365x3x4-ytx-t": {(L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-ytx-y": {(L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-ytx-x": {(L.K_FASTG_ROWS, "fastg rows")},
    "365x3x4-ytx-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "365x3x4-yxt-t": {(L.K_FASTG_ROWS, "fastg rows Rader")},
    "365x3x4-yxt-y": {(L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-yxt-x": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-yxt-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "365x3x4-xty-t": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-xty-y": {(L.K_FASTG_ROWS, "fastg rows")},
    "365x3x4-xty-x": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-xty-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
    "365x3x4-xyt-t": {(L.K_FASTG_ROWS, "fastg rows Rader")},
    "365x3x4-xyt-y": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-xyt-x": {(L.K_GENERIC, "main"), (L.K_FASTG_Y, "fastg y-only")},
    "365x3x4-xyt-yx": {(L.K_FASTG, "fastg"), (L.K_COMPOSITE, "inner layout")},
}
