"""GPU (-m gpu): float16 / bfloat16 input read where it lies on an MI355X -- the hardware convert (v_cvt_f32_f16) and the 16-bit shift behind the 2-byte loads.

* a half plan gives the float32 plan's bits on the widened samples: every family with a 2-byte loader, every mode, detrend, window, shift and batch count
  (tests/half_input.py -- the same rows as tests/test_half_input_emulated.py);
* xrfthip_convert and a plan's loader are exact on all 65 536 bit patterns of each format;
* the front doors agree (numpy float16, torch float16, bfloat16), results are float32 / complex64 and meet the oracle;
* no copy: power_spectrum of a half tensor of a FastY shape allocates less than its result plus a float32 copy of the field;
* misaligned fields, families without a loader and repeated calls give the float32 route's bits."""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import accuracy as A  # noqa: E402
import cases  # noqa: E402
import half_input as H  # noqa: E402
from oracle import xrft_oracle as o  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402

D3 = ("time", "y", "x")


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


def _cube(shape, seed=5):
    nt, ny, nx = shape
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v = (rng.standard_normal(shape) + 0.05 * ii - 0.03 * jj + 2.0).astype(np.float16)
    return v, {"time": np.arange(nt), "y": np.arange(ny) * 0.5, "x": np.arange(nx) * 2.0 + 3.0}


@pytest.mark.parametrize("hname", list(H.HALVES))
@pytest.mark.parametrize("rid", H.ROW_IDS)
def test_half_plan_gives_the_float32_plans_bits(rid, hname, monkeypatch):
    kw0, env, kind, tag = H.row(rid)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert A.family(A.make(**kw0, batch=1, dtype=torch.float32)) == (kind, tag)
    taken, seed = {}, 0
    for mode in H.MODES:
        for det, win, shift, batch in (H.FULL if mode == "power" else H.COVER):
            kw = H.mode_kw(kw0, mode, det, win, shift, batch)
            if kw is None:
                continue
            seed += 1
            taken.setdefault(mode, set()).add(H.run_plan_case(kw, hname, seed, dev="cuda"))
    assert taken["power"] == {"taken"} and all(len(v) == 1 for v in taken.values()), taken


@pytest.mark.parametrize("hname", list(H.HALVES))
@pytest.mark.parametrize("rid,batch", [("fasts-64x64", 700), ("fasty-256x512", 3), ("fastr-4096", 300), ("fastg-50x50", 700), ("fastg-rows-50", 3001)])
def test_more_than_one_round_of_workgroups(rid, hname, batch):
    """Batches beyond one workgroup per CU (256 CUs), the last row group partial: the float32 plan's bits."""
    kw0, env, kind, tag = H.row(rid)
    kw = H.mode_kw(kw0, "power", L.DETREND_LINEAR, True, True, batch)
    assert H.run_plan_case(kw, hname, 77, dev="cuda") == "taken"


@pytest.mark.parametrize("hname", list(H.HALVES))
def test_the_headline_slab(hname):
    """One 4096 x 4096 slab (the largest instantiation of the column kernel, 512 threads): linear detrend + Hann, the float32 plan's bits."""
    kw = H.mode_kw(dict(ny=4096, nx=4096), "power", L.DETREND_LINEAR, True, True, 1)
    assert H.run_plan_case(kw, hname, 78, dev="cuda") == "taken"


@pytest.mark.parametrize("hname", list(H.HALVES))
def test_four_step_rows(hname):
    """The four-step 1-D form of the two-pass kernels (2^20 samples per row), with and without a window (the slab-shaped window table)."""
    for win in (False, True):
        kw = H.mode_kw(dict(ndim=1, nx=1 << 20), "power", L.DETREND_LINEAR, win, False, 2)
        p = A.make(**kw, dtype=torch.float32)
        assert A.family(p) == (L.K_FASTY, "fasty four-step")
        assert H.run_plan_case(kw, hname, 79, dev="cuda") == "taken"


@pytest.mark.parametrize("hname", list(H.HALVES))
def test_convert_and_loader_are_exact_on_every_bit_pattern(hname):
    from xrft_amd import engine

    x = H.all_patterns(hname, "cuda")
    want = x.cpu().float()  # (torch's CPU widening: the yardstick)
    for off in (0, 1):
        got = engine.convert(x[off:], torch.float32).cpu()
        w = want[off:]
        nan = torch.isnan(w)
        assert bool((torch.isnan(got) == nan).all()) and torch.equal(H.bits32(got)[~nan], H.bits32(w)[~nan])
    # the same patterns through a plan's loader: one fastg row group of 1024 rows of 64 samples, NaN and inf replaced
    y = H.all_patterns(hname).clone()
    y[~torch.isfinite(y.float())] = 1.0
    y = y.reshape(1024, 64).cuda()
    kw = dict(ndim=1, batch=1024, nx=64, out_mode=L.OUT_COMPLEX)
    ph, pf = A.make(**kw, dtype=H.HALVES[hname]), A.make(**kw, dtype=torch.float32)
    assert A.family(ph) == A.family(pf) == (L.K_FASTG_ROWS, "fastg rows")
    oh, _ = ph.execute(y)
    of, _ = pf.execute(y.cpu().float().cuda())  # (widened on the CPU: the yardstick above)
    assert torch.equal(H.bits32(torch.view_as_real(oh)), H.bits32(torch.view_as_real(of)))


def test_front_doors_agree_and_meet_the_oracle():
    import xrft_amd as xa

    v, coords = _cube((3, 256, 512))
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    a = xa.power_spectrum(xa.DataArray(v, D3, coords), **kw)
    assert H.NOTE["float16"] in _newest_plan() and "[fasty]" in _newest_plan()
    b = xa.power_spectrum(xa.DataArray(torch.from_numpy(v).cuda(), D3, coords), **kw)
    f = xa.power_spectrum(xa.DataArray(v.astype(np.float32), D3, coords), **kw)
    assert a.data.dtype == b.data.dtype == torch.float32 and torch.equal(a.data, b.data) and torch.equal(a.data, f.data)
    for d in f.dims:
        assert np.array_equal(np.asarray(a[d].values), np.asarray(f[d].values)) and np.array_equal(np.asarray(b[d].values), np.asarray(f[d].values))
    cases.check(a, o.power_spectrum(o.OArr(v.astype(np.float64), D3, coords), **kw), cases.TOL["float32"])
    c = xa.fft(xa.DataArray(torch.from_numpy(v).cuda(), D3, coords), dim=["y", "x"])
    assert c.data.dtype == torch.complex64
    bf = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).cuda()
    e = xa.power_spectrum(xa.DataArray(bf, D3, coords), **kw)
    assert H.NOTE["bfloat16"] in _newest_plan()
    g = xa.power_spectrum(xa.DataArray(bf.float(), D3, coords), **kw)
    assert e.data.dtype == torch.float32 and torch.equal(e.data, g.data)
    cases.check(e, o.power_spectrum(o.OArr(bf.cpu().to(torch.float64).numpy(), D3, coords), **kw), cases.TOL["float32"])
    # cross spectra of two half fields, isotropic spectra (float64 results, as for float32 input), a cross phase
    w, _ = _cube((3, 256, 512), seed=6)
    for fn, args in ((xa.cross_spectrum, 2), (xa.isotropic_power_spectrum, 1), (xa.cross_phase, 2)):
        h = [xa.DataArray(torch.from_numpy(z).cuda(), D3, coords) for z in (v, w)][:args]
        s = [xa.DataArray(torch.from_numpy(z.astype(np.float32)).cuda(), D3, coords) for z in (v, w)][:args]
        rh, rs = fn(*h, **kw), fn(*s, **kw)
        assert rh.data.dtype == rs.data.dtype and torch.equal(rh.data, rs.data), fn.__name__
    assert rs.data.dtype == torch.float32


def test_no_widened_copy_of_the_field():
    """After a warm-up call, power_spectrum of a float16 tensor of a FastY shape: the peak allocation above the input stays below (result + 4 bytes per input sample)
    -- what a float32 copy of the field alone would add."""
    import xrft_amd as xa

    shape = (8, 1024, 1024)
    g = torch.Generator(device="cuda").manual_seed(12)
    x = (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) + 1.0).to(torch.float16)
    coords = {"time": np.arange(shape[0]) * 1.0, "y": np.arange(shape[1]) * 0.5, "x": np.arange(shape[2]) * 0.25}
    da = xa.DataArray(x, D3, coords)
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    res = xa.power_spectrum(da, **kw)  # warm-up: plan, tables, scratch
    assert "[fasty]" in _newest_plan() and H.NOTE["float16"] in _newest_plan()
    del res
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = xa.power_spectrum(da, **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    out_bytes = res.data.numel() * res.data.element_size()
    print(f"power_spectrum float16 {shape}: peak {peak} B over the resident set, result {out_bytes} B, a float32 copy would be {4 * x.numel()} B")
    assert res.data.dtype == torch.float32 and peak < out_bytes + 4 * x.numel(), (peak, out_bytes)
    f = xa.power_spectrum(xa.DataArray(x.float(), D3, coords), **kw)
    assert torch.equal(res.data, f.data)


@pytest.mark.parametrize("hname", list(H.HALVES))
def test_misaligned_fields_and_families_without_a_loader(hname):
    import xrft_amd as xa

    hdt = H.HALVES[hname]
    # a field 2, 4 and 8 bytes past a 16-byte boundary: xrfthip_exec declines it unread; the public call widens it -- the aligned call's bits
    shape = (3, 256, 512)
    n = int(np.prod(shape))
    x16, _ = H.field(shape, hdt, 21, "cuda")
    coords = {"time": np.arange(3), "y": np.arange(256) * 0.5, "x": np.arange(512) * 2.0}
    kw = dict(dim=["y", "x"], detrend="linear", window="hann")
    want = xa.power_spectrum(xa.DataArray(x16, D3, coords), **kw)
    assert H.NOTE[hname] in _newest_plan()
    p = A.make(ny=256, nx=512, batch=3, dtype=hdt)
    ws = torch.empty(p.workspace_bytes + 256, dtype=torch.uint8, device="cuda")
    out = torch.empty((3, 256, 512), dtype=torch.float32, device="cuda")
    for off in (1, 2, 4):
        buf = torch.empty(n + 16, dtype=hdt, device="cuda")
        base = (-(buf.data_ptr() // 2)) % 8
        view = buf[base + off:base + off + n].reshape(shape)
        view.copy_(x16)
        assert view.data_ptr() % 16 == 2 * off
        rc = L.load().xrfthip_exec(p._h, C.c_void_p(view.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(0),
                                   C.c_void_p((ws.data_ptr() + 255) & ~255), p.workspace_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == L.UNSUPPORTED_LENGTH, rc
        got = xa.power_spectrum(xa.DataArray(view, D3, coords), **kw)
        assert "input read where it lies" not in _newest_plan() and torch.equal(got.data, want.data)
    # a FastM length, an AXIS_Y call, an inner-layout call: declined by the library, the float32 route's bits
    v, c2 = _cube((2, 720, 1440))
    h = torch.from_numpy(v.astype(np.float32)).to(hdt).cuda()
    vi, ci = _cube((16, 64, 8))
    hi = torch.from_numpy(vi.astype(np.float32)).to(hdt).cuda()
    for dims in (["y", "x"], ["y"], ["time", "y"]):
        sub, cc = (h, c2) if dims != ["time", "y"] else (hi, ci)
        a = xa.power_spectrum(xa.DataArray(sub, D3, cc), dim=dims, detrend="linear", window="hann")
        assert "input read where it lies" not in _newest_plan()
        b = xa.power_spectrum(xa.DataArray(sub.float(), D3, cc), dim=dims, detrend="linear", window="hann")
        a2 = xa.power_spectrum(xa.DataArray(sub, D3, cc), dim=dims, detrend="linear", window="hann")
        assert a.data.dtype == torch.float32 and torch.equal(a.data, b.data) and torch.equal(a.data, a2.data), dims
    for flags in (L.INVERSE, L.INVERSE | L.C2R_X, L.PHASE_IN):
        with pytest.raises(L.XrftHipError) as e:
            A.make(ny=64, nx=64, dtype=hdt, out_mode=L.OUT_COMPLEX, flags=flags)
        assert e.value.status == L.BAD_ARG
    for kwd in (dict(ny=720, nx=1440), dict(ny=100, nx=200, flags=L.AXIS_Y), dict(ny=128, nx=256, inner=4), dict(ny=64, nx=64, in_stride_y=72)):
        assert H.try_make(**kwd, dtype=hdt) is None, kwd
