"""float16 / bfloat16 input read where it lies (xrfthip_dtype XRFTHIP_F16 / XRFTHIP_BF16), on the emulated library: the kernels' index arithmetic, the host
routing and the fallback, with the float16 decode of the emulated build (integer arithmetic; the device uses the hardware convert -- tests/test_gpu_half_input.py).

1. a half plan gives the float32 plan's bits on the widened samples, per family, mode, detrend, window, shift and batch count (tests/half_input.py);
2. the public calls meet the oracle fed the samples widened to float64 at the float32 tolerance, and the rounding-level bound of tests/accuracy.py;
3. a numpy float16 array and the same data as a torch float16 tensor give identical bits, float32 / complex64 results and the float32 call's coordinates;
4. xrfthip_convert is exact on all 65 536 bit patterns of each format, and so is a plan's loader;
5. base pointers off the 16-byte boundary, rows not divisible by 8, a partial last workgroup: the plan's bits or a clean XRFTHIP_UNSUPPORTED_LENGTH;
7. families without a 2-byte loader, complex-only flags, repeated calls."""
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
import half_input as H  # noqa: E402


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


# ---------------------------------------------------------------------------------- 1. bit identity, per family
@pytest.mark.parametrize("hname", list(H.HALVES))
@pytest.mark.parametrize("rid", H.ROW_IDS)
def test_half_plan_gives_the_float32_plans_bits(rid, hname, monkeypatch):
    kw0, env, kind, tag = H.row(rid)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert A.family(A.make(**kw0, batch=1, dtype=torch.float32)) == (kind, tag)
    big = kw0.get("ny", 1) * kw0["nx"] > 65536  # (the emulated two-pass kernels: the covering set in every mode)
    taken = {}
    seed = 0
    for mode in H.MODES:
        for det, win, shift, batch in (H.COVER if (mode != "power" or big) else H.FULL):
            kw = H.mode_kw(kw0, mode, det, win, shift, batch)
            if kw is None:
                continue
            seed += 1
            taken.setdefault(mode, set()).add(H.run_plan_case(kw, hname, seed))
    assert taken["power"] == {"taken"}, taken  # (every row's own family serves plain power spectra)
    assert all(len(v) == 1 for v in taken.values()), taken  # (detrend, window, shift and batch never change who serves a mode)


# ---------------------------------------------------------------------------------- 2. oracle and contract
@pytest.mark.parametrize("hname", list(H.HALVES))
@pytest.mark.parametrize("rid", ["fasts-64x64", "fasty-256x512", "fastr-4096", "fastg-50x50", "fastg-15x9", "fastg-rows-50"])
def test_half_plan_meets_the_rounding_bound(rid, hname):
    kw, env, kind, tag = H.row(rid)
    kw.update(out_mode=L.OUT_POWER, detrend=L.DETREND_LINEAR, flags=0, batch=2)
    shape, axes, _ = A._axes(kw)
    x16, _x32 = H.field(shape, H.HALVES[hname], 9)
    p = A.make(**kw, dtype=H.HALVES[hname])
    assert A.family(p) == (kind, tag)
    out, _ = p.execute(x16)
    x64 = x16.to(torch.float64).numpy().reshape(shape)
    ref, _ = A.reference(kw, x64)
    kap = A.kappa(x64, A.detrended(x64, axes, L.DETREND_LINEAR))
    A.assert_accurate(out.numpy().reshape(ref.shape), ref, "float32", A.points(kw), kap, what=f"{tag} {hname} power spectrum")


def _cube(shape, seed=5):
    nt, ny, nx = shape
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v = (rng.standard_normal(shape) + 0.05 * ii - 0.03 * jj + 2.0).astype(np.float16)
    coords = {"time": np.arange(nt), "y": np.arange(ny) * 0.5, "x": np.arange(nx) * 2.0 + 3.0}
    return v, coords


D3 = ("time", "y", "x")
# (id, shape, call on (module, array[, second array])): the same public calls with half input, against the oracle and against the float32 call
API_CALLS = [
    ("ps-fasts", (3, 64, 64), lambda m, a, b: m.power_spectrum(a, dim=["y", "x"], detrend="linear", window="hann")),
    ("ps-fastg", (3, 50, 50), lambda m, a, b: m.power_spectrum(a, dim=["y", "x"], detrend="constant", window="hann")),
    ("ps-realdim", (3, 50, 50), lambda m, a, b: m.power_spectrum(a, dim=["y"], real_dim="x", detrend="linear", window="hann")),
    ("fft-fastg", (1, 6, 10), lambda m, a, b: m.fft(a, dim=["y", "x"], detrend="linear")),
    ("cs-fastg", (3, 50, 50), lambda m, a, b: m.cross_spectrum(a, b, dim=["y", "x"], detrend="linear", window="hann")),
    ("cp-fastg", (3, 50, 50), lambda m, a, b: m.cross_phase(a, b, dim=["y", "x"], detrend="linear", window="hann")),
    ("iso-fasts", (3, 64, 64), lambda m, a, b: m.isotropic_power_spectrum(a, dim=["y", "x"], detrend="constant", window="hann")),
    ("ps-fastm", (1, 360, 720), lambda m, a, b: m.power_spectrum(a, dim=["y", "x"], detrend="linear", window="hann")),
    ("ps-axis-y", (4, 50, 6), lambda m, a, b: m.power_spectrum(a, dim=["y"], detrend="linear", window="hann")),
    ("ps-inner", (16, 12, 3), lambda m, a, b: m.power_spectrum(a, dim=["time", "y"], detrend="linear")),
    ("ps-1d-rows", (3, 4, 50), lambda m, a, b: m.power_spectrum(a, dim=["x"], detrend="linear", window="hann")),
]


@pytest.mark.parametrize("cid,shape,call", API_CALLS, ids=[c[0] for c in API_CALLS])
def test_public_calls_meet_the_oracle_and_the_float32_call(cid, shape, call):
    v, coords = _cube(shape)
    w, _ = _cube(shape, seed=6)
    v64, w64 = v.astype(np.float64), w.astype(np.float64)
    ref = call(o, o.OArr(v64, D3, coords), o.OArr(w64, D3, coords))
    f32 = call(xa, xa.DataArray(torch.from_numpy(v.astype(np.float32)), D3, coords), xa.DataArray(torch.from_numpy(w.astype(np.float32)), D3, coords))
    for hname, hdt in H.HALVES.items():
        if hname == "float16":
            a16, b16 = torch.from_numpy(v), torch.from_numpy(w)
            a32, b32, r = None, None, ref
            want = f32
        else:  # the bfloat16 rounding of the same data: its own widened samples are the reference's input
            a16, b16 = torch.from_numpy(v.astype(np.float32)).to(hdt), torch.from_numpy(w.astype(np.float32)).to(hdt)
            r = call(o, o.OArr(a16.to(torch.float64).numpy(), D3, coords), o.OArr(b16.to(torch.float64).numpy(), D3, coords))
            want = call(xa, xa.DataArray(a16.float(), D3, coords), xa.DataArray(b16.float(), D3, coords))
        got = call(xa, xa.DataArray(a16, D3, coords), xa.DataArray(b16, D3, coords))
        iso = cid.startswith("iso")
        assert got.data.dtype == want.data.dtype and got.data.dtype in ((torch.float64,) if iso else (torch.float32, torch.complex64)), got.data.dtype
        assert torch.equal(got.data, want.data), f"{cid} {hname}: not the float32 call's bits"
        for d in want.dims:
            assert np.array_equal(np.asarray(got[d].values), np.asarray(want[d].values))
        if cid.startswith("cp-"):
            # an angle has no max-norm relative error across the +-pi cut: held as tests/cases.py run_cross_phase_cases holds float32 cross phases, modulo 2 pi at 2e-3
            # ("the angle of a near-zero cross spectrum amplifies rounding"); dims and coordinates as cases.check holds them
            assert tuple(got.dims) == tuple(r.dims) and all(np.array_equal(np.asarray(got[d].values), np.asarray(r.coord(d))) for d in r.dims if d in r.coords)
            dphi = np.abs(np.angle(np.exp(1j * (got.values - r.values)))).max()
            assert dphi < 2e-3, dphi
        else:
            cases.check(got, r, cases.TOL["float32"])


# ---------------------------------------------------------------------------------- 3. the front doors agree
def test_numpy_float16_and_torch_float16_agree():
    v, coords = _cube((3, 64, 64))
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    a = xa.power_spectrum(xa.DataArray(v, D3, coords), **kw)
    assert H.NOTE["float16"] in newest_plan() and "[fasts]" in newest_plan()
    b = xa.power_spectrum(xa.DataArray(torch.from_numpy(v), D3, coords), **kw)
    f = xa.power_spectrum(xa.DataArray(v.astype(np.float32), D3, coords), **kw)
    assert "input read where it lies" not in newest_plan()
    assert a.data.dtype == b.data.dtype == torch.float32 and torch.equal(a.data, b.data) and torch.equal(a.data, f.data)
    c = xa.fft(xa.DataArray(v, D3, coords), dim=["y", "x"])
    d = xa.fft(xa.DataArray(torch.from_numpy(v), D3, coords), dim=["y", "x"])
    assert c.data.dtype == d.data.dtype == torch.complex64 and torch.equal(c.data, d.data)
    for dname in f.dims:
        assert np.array_equal(np.asarray(a[dname].values), np.asarray(f[dname].values)) and np.array_equal(np.asarray(b[dname].values), np.asarray(f[dname].values))
    bf = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16)
    e = xa.power_spectrum(xa.DataArray(bf, D3, coords), **kw)
    assert H.NOTE["bfloat16"] in newest_plan()
    g = xa.power_spectrum(xa.DataArray(bf.float(), D3, coords), **kw)
    assert e.data.dtype == torch.float32 and torch.equal(e.data, g.data)


def test_mixed_precisions_promote_as_before():
    v, coords = _cube((2, 50, 50))
    w, _ = _cube((2, 50, 50), seed=6)
    kw = dict(dim=["y", "x"], detrend="linear")
    for other, rdt in ((np.float32, torch.complex64), (np.float64, torch.complex128)):
        got = xa.cross_spectrum(xa.DataArray(v, D3, coords), xa.DataArray(w.astype(other), D3, coords), **kw)
        want = xa.cross_spectrum(xa.DataArray(v.astype(np.float32), D3, coords), xa.DataArray(w.astype(other), D3, coords), **kw)
        assert got.data.dtype == rdt and torch.equal(got.data, want.data)
    bf = torch.from_numpy(w.astype(np.float32)).to(torch.bfloat16)
    got = xa.cross_spectrum(xa.DataArray(v, D3, coords), xa.DataArray(bf, D3, coords), **kw)  # float16 with bfloat16: both widened
    want = xa.cross_spectrum(xa.DataArray(v.astype(np.float32), D3, coords), xa.DataArray(bf.float(), D3, coords), **kw)
    assert got.data.dtype == torch.complex64 and torch.equal(got.data, want.data)


# ---------------------------------------------------------------------------------- 4. conversion is exact
@pytest.mark.parametrize("hname", list(H.HALVES))
def test_convert_is_exact_on_every_bit_pattern(hname):
    x = H.all_patterns(hname)
    want = x.float()
    for off in (0, 1):  # (a 4-byte aligned source: pairs per load, and the odd tail; a source 2 bytes off: sample by sample)
        src = x[off:]
        got = engine.convert(src, torch.float32)
        w = want[off:]
        nan = torch.isnan(w)
        assert got.dtype == torch.float32 and bool((torch.isnan(got) == nan).all())
        assert torch.equal(H.bits32(got)[~nan], H.bits32(w)[~nan])
    assert int(nan.sum()) == (2046 if hname == "float16" else 254)
    with pytest.raises(TypeError):
        engine.convert(x, torch.float64)
    with pytest.raises(L.XrftHipError):  # no other direction
        L.check(L.load().xrfthip_convert(L.F32, L.F16, 4, C.c_void_p(want.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(0)))


@pytest.mark.parametrize("hname", list(H.HALVES))
def test_a_plans_loader_is_exact_on_every_bit_pattern(hname):
    """The 65 536 patterns (NaN and inf replaced by 1) as ONE fastg row group of 1024 rows of 64 samples: the complex spectrum of the half plan against the float32
    plan's -- and the kx = 0 column (the sum of a row) says the samples themselves arrived as torch widens them."""
    x = H.all_patterns(hname).clone()
    bad = ~torch.isfinite(x.float())
    x[bad] = 1.0
    x = x.reshape(1024, 64)
    kw = dict(ndim=1, batch=1024, nx=64, out_mode=L.OUT_COMPLEX)
    ph, pf = A.make(**kw, dtype=H.HALVES[hname]), A.make(**kw, dtype=torch.float32)
    assert A.family(ph) == A.family(pf) == (L.K_FASTG_ROWS, "fastg rows")
    oh, _ = ph.execute(x)
    of, _ = pf.execute(x.float())
    # (the largest bfloat16 values overflow float32 inside the transform: inf and NaN results compare by their bits, which the same arithmetic gives both plans)
    assert torch.equal(H.bits32(torch.view_as_real(oh)), H.bits32(torch.view_as_real(of)))
    k0h, k0f = oh.reshape(1024, 64)[:, 0].real, x.float().sum(dim=1)
    small = torch.isfinite(k0f) & (x.float().abs().amax(dim=1) < 1e30)
    assert torch.allclose(k0h[small].double(), x.double().sum(dim=1)[small], rtol=1e-5, atol=0.0)  # (the samples themselves: the kx = 0 bin is their sum)


# ---------------------------------------------------------------------------------- 5. alignment and tails
@pytest.mark.parametrize("hname", list(H.HALVES))
@pytest.mark.parametrize("rid", ["fasts-64x64", "fasty-256x512", "fastr-4096", "fastg-6x10", "fastg-15x9", "fastg-rows-50"])
def test_misaligned_fields_fall_back_with_the_same_bits(rid, hname):
    """The field 2, 4 and 8 bytes past a 16-byte boundary, its last sample the last element of the buffer: xrfthip_exec answers XRFTHIP_UNSUPPORTED_LENGTH
    (include/xrft_hip.h: 16-byte aligned fields) and reads nothing; the public call widens the field and gives the aligned call's bits."""
    kw, env, kind, tag = H.row(rid)
    hdt = H.HALVES[hname]
    kw.update(batch=3, out_mode=L.OUT_POWER, detrend=L.DETREND_LINEAR, flags=0)
    shape = (3, kw["ny"], kw["nx"]) if kw.get("ndim", 2) == 2 else (3, kw["nx"])
    n = int(np.prod(shape))
    x16, x32 = H.field(shape, hdt, 21)
    p = A.make(**kw, dtype=hdt)
    ws = torch.empty(max(p.workspace_bytes, 256) + 256, dtype=torch.uint8)
    want, _ = p.execute(x16)
    for off in (1, 2, 4):  # elements = 2, 4, 8 bytes
        buf = torch.empty(n + 8 + off, dtype=hdt)
        base = (-(buf.data_ptr() // 2)) % 8  # first element on a 16-byte boundary
        view = buf[base + off:base + off + n]
        view.copy_(x16.reshape(-1))
        assert view.data_ptr() % 16 == 2 * off
        out = torch.empty_like(want)
        rc = L.load().xrfthip_exec(p._h, C.c_void_p(view.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(0),
                                   C.c_void_p((ws.data_ptr() + 255) & ~255), p.workspace_bytes, C.c_void_p(0))
        assert rc == L.UNSUPPORTED_LENGTH, rc
    if kw.get("ndim", 2) == 2:  # ... and through the front door
        coords = {"time": np.arange(3), "y": np.arange(shape[1]) * 0.5, "x": np.arange(shape[2]) * 2.0}
        ps = dict(dim=["y", "x"], detrend="linear", window="hann")
        buf = torch.empty(n + 16, dtype=hdt)
        base = (-(buf.data_ptr() // 2)) % 8
        view = buf[base + 1:base + 1 + n].reshape(shape)
        view.copy_(x16)
        a = xa.power_spectrum(xa.DataArray(view, D3, coords), **ps)
        assert "input read where it lies" not in newest_plan()
        b = xa.power_spectrum(xa.DataArray(x16, D3, coords), **ps)
        assert torch.equal(a.data, b.data)


@pytest.mark.parametrize("hname", list(H.HALVES))
def test_tails_and_partial_workgroups(hname):
    """Rows not divisible by 8 (10, 50, 9 samples), a batch that ends inside a row group (fastg rows: 301 rows) and the field's last sample on the last element of its
    buffer: the float32 plan's bits (a read past the buffer is scripts/run_emu_asan.sh's to catch)."""
    hdt = H.HALVES[hname]
    for kw in (dict(ndim=1, nx=50, batch=301), dict(ndim=1, nx=9, batch=301), dict(ny=6, nx=10, batch=5), dict(ny=15, nx=9, batch=5)):
        kw = dict(kw, out_mode=L.OUT_POWER, detrend=L.DETREND_LINEAR)
        assert H.run_plan_case(kw, hname, 33) == "taken"
        p = A.make(**kw, dtype=hdt)
        if kw.get("ndim", 2) == 1:
            assert p.kernel_info()[1] > 1 and kw["batch"] % p.kernel_info()[1] != 0, p.kernel_info()  # (the last workgroup's group of rows is short)


# ---------------------------------------------------------------------------------- 7. declines and repeats
def test_families_without_a_half_loader_decline(monkeypatch):
    hd = torch.float16
    for kw in (dict(ny=360, nx=720), dict(ny=100, nx=200, flags=L.AXIS_Y), dict(ny=128, nx=256, inner=4), dict(ny=128, nx=256, mid=4),
               dict(ny=64, nx=64, in_stride_y=72), dict(ndim=1, nx=1031), dict(ny=3000, nx=3000)):
        assert H.try_make(**kw, dtype=hd) is None and H.try_make(**kw, dtype=torch.bfloat16) is None, kw
    monkeypatch.setenv("XRFTHIP_NO_FAST", "1")
    assert H.try_make(ny=64, nx=64, dtype=hd) is None  # (the generic tiles)


@pytest.mark.parametrize("flags", [L.INVERSE, L.INVERSE | L.C2R_X, L.PHASE_IN], ids=["inverse", "c2r", "phase-in"])
def test_complex_only_flags_are_bad_arguments(flags):
    for hd in H.HALVES.values():
        with pytest.raises(L.XrftHipError) as e:
            A.make(ny=64, nx=64, dtype=hd, out_mode=L.OUT_COMPLEX, flags=flags)
        assert e.value.status == L.BAD_ARG  # (as for real float32 input)
    with pytest.raises(L.XrftHipError) as e:
        A.make(**A.herm_kw((8, 6, 10), torch.float16, L.OUT_POWER))
    assert e.value.status == L.BAD_ARG


def test_old_descriptor_sizes_and_the_version_stand():
    assert L.load().xrfthip_version() == 106
    d = L.Desc(64, 2, 2, 64, 64, L.F16, L.OUT_POWER, 0, 0, 1.0, 0, 0)  # (the first version of the struct: no inner / mid / strides / herm fields)
    h = C.c_void_p(0)
    assert L.load().xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
    buf = C.create_string_buffer(4096)
    L.load().xrfthip_plan_describe(h, buf, len(buf))
    assert H.NOTE["float16"] in buf.value.decode()
    L.load().xrfthip_plan_destroy(h)


def test_a_refusal_is_remembered_and_repeats_are_identical():
    v, coords = _cube((1, 360, 720))
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    api.clear_plan_cache()
    a = xa.power_spectrum(xa.DataArray(v, D3, coords), **kw)
    assert "[fastm]" in newest_plan() and "input read where it lies" not in newest_plan()
    assert len(api._HALF_REFUSED) == 1
    b = xa.power_spectrum(xa.DataArray(v, D3, coords), **kw)
    assert len(api._HALF_REFUSED) == 1 and torch.equal(a.data, b.data)
    f = xa.power_spectrum(xa.DataArray(v.astype(np.float32), D3, coords), **kw)
    assert torch.equal(a.data, f.data)


def test_column_pass_reuse_with_half_fields():
    """Half plans take part in the reuse of the column pass under the same key rules: the results with and without it are the float32 calls' bits."""
    shape = (2, 256, 512)
    a16, _ = H.field(shape, torch.float16, 41)
    b16, _ = H.field(shape, torch.float16, 42)
    coords = {"time": np.arange(2), "y": np.arange(256) * 0.5, "x": np.arange(512) * 2.0}
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    res = {}
    for reuse in (True, False):
        engine.reuse_column_pass(reuse)
        try:
            da, db = xa.DataArray(a16, D3, coords), xa.DataArray(b16, D3, coords)
            res[reuse] = (xa.cross_spectrum(da, db, **kw).data, xa.power_spectrum(da, **kw).data, xa.power_spectrum(db, **kw).data)
        finally:
            engine.reuse_column_pass(True)
    assert H.NOTE["float16"] in newest_plan() and "[fasty]" in newest_plan()
    fa, fb = xa.DataArray(a16.float(), D3, coords), xa.DataArray(b16.float(), D3, coords)
    want = (xa.cross_spectrum(fa, fb, **kw).data, xa.power_spectrum(fa, **kw).data, xa.power_spectrum(fb, **kw).data)
    for k in range(3):
        assert torch.equal(res[True][k], res[False][k]) and torch.equal(res[True][k], want[k])
