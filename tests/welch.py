"""Shared by the tests of Welch spectra (xrfthip_desc.seg_hop, csrc/fastw.h; tests/test_welch_emulated.py on the emulated library, tests/test_gpu_welch.py on the
MI355X): the plan-level cases, their series, the float64 reference, the bound.  Not a conftest: imported by the tests that use it.

The reference is the oracle's power / cross spectrum of the float64 image of the same float32 samples, cut into segments ON THE HOST (segment s of a series starts at
s * hop), one spectrum per segment, then numpy's mean over the segments in float64.  The bound is the contract of one mean spectrum, tests/batch_mean.py::bound with
n = L: A.bound("float32", L, kappa) + 16 u -- a relative L2 error per output (per series); a cross spectrum's is taken against the mean of the terms' magnitudes;
kappa = max |x| / rms(x - fit) over the segments of the series, 0 without a detrend (B.kappa).

Every series carries its own amplitude (x1, x3, x9, x27, then again): a segment summed into the wrong series misses the bound."""
import ctypes as C

import numpy as np
import torch

from oracle import xrft_oracle as o
from xrft_amd import _lib as L
from xrft_amd import api, engine

import accuracy as A
import batch_mean as B

U32 = A.U["float32"]
DIMS = ("p", "s", "t")
FORMS = ["plain", "linear-hann-shift"]
# (L, hop, M, P, runs pinned (0 = the plan's choice), the longest run): the smallest and the largest length; hops L (no overlap), L / 2, 37 (odd, unaligned starts)
# and 1; 2 and 3 segments (an odd count: the last pair is half empty), 35 in ONE run (two full float32 chains of 16 and the hand-over to float64) and 36 in two
# runs of 18; 1, 3 and 300 series (more than the CUs)
CASES = [(64, 64, 2, 1, 0, None), (64, 32, 3, 3, 0, None), (64, 37, 35, 1, 1, 35), (64, 1, 36, 3, 2, 18), (256, 128, 3, 3, 0, None), (256, 37, 2, 300, 0, None),
         (256, 256, 35, 3, 1, 35), (256, 1, 5, 1, 0, None), (1024, 512, 5, 2, 0, None)]
LARGEST = (4096, 2048, 3, 2, 0, None)
CROSS_CASES = [(64, 37, 35, 1, 1, 35), (256, 128, 3, 3, 0, None), (256, 1, 36, 3, 2, 18)]
CROSS_LAG = 7.0  # origin of the second series' coordinate: the net true-phase factor is not 1


def case_id(c):
    return f"L{c[0]}-H{c[1]}-M{c[2]}-P{c[3]}" + (f"-runs{c[4]}" if c[4] else "")


def span(case):
    return (case[2] - 1) * case[1] + case[0]


def series(case, seed=41, pitch=None):
    """[P][pitch] float32 (pitch >= the span; default the span): seeded noise over a line, series p scaled by 3^(p mod 4)."""
    l, h, m, p = case[:4]
    n = span(case) if pitch is None else pitch
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((p, n)) + 0.01 * np.arange(n) + 1.5
    v *= (3.0 ** (np.arange(p) % 4)).reshape(p, 1)
    return v.astype(np.float32)


def second_series(x, seed=42):
    """The first rolled by 5 samples plus a tenth of its size in noise: the cross spectra of the segments do not cancel in the mean."""
    rng = np.random.default_rng(seed)
    amp = np.abs(x).mean(axis=1).reshape(-1, 1)
    return (np.roll(x, 5, axis=1) + 0.1 * amp * rng.standard_normal(x.shape)).astype(np.float32)


def segments(x, case):
    """[P][M][L] float64: the host's cut."""
    l, h, m, p = case[:4]
    x = np.asarray(x, dtype=np.float64)
    return np.stack([x[:, s * h:s * h + l] for s in range(m)], axis=1)


def form_kw(form):
    if form == "plain":
        return dict(detrend=L.DETREND_NONE, flags=0), dict(detrend=None, window=None, shift=False)
    if form == "constant":
        return dict(detrend=L.DETREND_CONSTANT, flags=0), dict(detrend="constant", window=None, shift=False)
    return dict(detrend=L.DETREND_LINEAR, flags=L.SHIFT_X, window="hann"), dict(detrend="linear", window="hann", shift=True)


def make_plan(case, form="plain", mode=L.OUT_POWER, pitch=0, lag=None, runs=None, **over):
    l, h, m, p = case[:4]
    runs = case[4] if runs is None else runs
    if runs:
        with B.env("XRFTHIP_MEAN_RUNS", runs):
            return make_plan(case, form, mode, pitch, lag, 0, **over)
    pkw, _ = form_kw(form)
    pkw = dict(pkw)
    win = pkw.pop("window", None)
    kw = dict(ndim=1, batch=p * m, ny=1, nx=l, dtype=torch.float32, out_mode=mode, scale=1.0, mean_batch=m, seg_hop=h, in_stride_batch=pitch, **pkw)
    if win:
        kw["window_x"] = api._window_vector(win, l)
    if mode == L.OUT_CROSS and lag is not None:  # true phase: both series ifftshifted, the net factor phase0 * conj(phase1) per unshifted frequency
        kw["flags"] |= L.ISHIFT_X
        f = np.fft.fftfreq(l, 1.0)
        kw["phase_x"] = np.exp(-2j * np.pi * f * api._lag_coord(np.arange(l) * 1.0)) * np.conj(np.exp(-2j * np.pi * f * api._lag_coord(lag + np.arange(l) * 1.0)))
    kw.update(over)
    return engine.SpectralPlan(**kw)


def run(plan, x0, x1=None):
    dev = L.device()
    t0 = torch.from_numpy(np.ascontiguousarray(x0)).to(dev)
    t1 = None if x1 is None else torch.from_numpy(np.ascontiguousarray(x1)).to(dev)
    out, _ = plan.execute(t0, t1)
    return out.cpu().numpy().reshape(out.shape[0], -1)


def reference(case, form, x0, x1=None, lag=None, half=0):
    """(mean over the segments of the oracle's spectra of the float64 samples, mean of their magnitudes).  half: 1 = k = 0 .. L / 2 of the unshifted spectrum
    (XRFTHIP_HALF_X), 2 = the oracle's real_dim (HALF_X | REALDIM_X2)."""
    l, h, m, p = case[:4]
    _, okw = form_kw(form)
    okw = dict(okw)
    if half:
        okw["shift"] = False
    crd = {"p": np.arange(p), "s": np.arange(m), "t": np.arange(l) * 1.0}
    kw = dict(dim=["t"], scaling="false_density", real_dim="t" if half == 2 else None, **okw)
    a0 = o.OArr(segments(x0, case), DIMS, crd)
    if x1 is None:
        ps = o.power_spectrum(a0, **kw).values
    else:
        crd1 = dict(crd, t=(0.0 if lag is None else lag) + np.arange(l) * 1.0)
        ps = o.cross_spectrum(a0, o.OArr(segments(x1, case), DIMS, crd1), true_phase=lag is not None, **kw).values
    if half == 1:
        ps = ps[..., :l // 2 + 1]
    return ps.mean(axis=1), np.abs(ps).mean(axis=1)


def kappa(case, form, x):
    """max |x| / rms(x - fit) over the segments of each series (0 without a detrend)."""
    kind = form_kw(form)[0]["detrend"]
    if kind == L.DETREND_NONE:
        return [0.0] * case[3]
    return [A.kappa(s, A.detrended(s, (1,), kind)) for s in segments(x, case)]


def bound(l, kap):
    return B.bound(1, l, kap)


def assert_outputs(case, got, ref, mag, kaps, what):
    """Every series within the bound, each against its own reference; finite; prints each figure before it asserts (the worst only for many series)."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rows = []
    for k in range(ref.shape[0]):
        rows.append((B.rel_error(got[k], ref[k], None if mag is None else mag[k]), bound(case[0], kaps[k]), k))
    for err, bnd, k in (rows if len(rows) <= 4 else [max(rows, key=lambda r: r[0] / r[1])]):
        print(f"{what} series {k}: error {err:.3e} bound {bnd:.3e}")
    assert np.isfinite(got).all(), what
    for err, bnd, k in rows:
        assert err <= bnd, f"{what} series {k}: error {err:.3e} > {bnd:.3e}"


def check_plan(case, form, mode=L.OUT_POWER, lag=None, half=0):
    l, h, m, p, runs, run_len = case
    x0 = series(case)
    x1 = second_series(x0) if mode == L.OUT_CROSS else None
    over = {}
    if half:
        pkw, _ = form_kw(form)
        over["flags"] = (pkw["flags"] & ~L.SHIFT_X) | L.HALF_X | (L.REALDIM_X2 if half == 2 else 0)
    plan = make_plan(case, form, mode, lag=lag, **over)
    assert plan.kernel_info()[0] == L.K_FASTW and "[fastw]" in plan.describe() and "[mean over the batch]" in plan.describe(), plan.describe()
    if run_len is not None:
        assert B.runs_per_output(plan) == runs and B.run_length(plan) == run_len, plan.describe()
    got = run(plan, x0, x1)
    nxo = l // 2 + 1 if half else l
    assert got.shape == (p, nxo) and got.dtype == (np.complex64 if mode == L.OUT_CROSS else np.float32)
    ref, mag = reference(case, form, x0, x1, lag, half)
    kaps = kappa(case, form, x0)
    if x1 is not None:
        kaps = [max(a, b) for a, b in zip(kaps, kappa(case, form, x1))]
    assert_outputs(case, got, ref, mag if x1 is not None else None, kaps, f"{'cross' if x1 is not None else 'power'} {case_id(case)} {form} half={half}")
    assert np.array_equal(got, run(plan, x0, x1))  # every addition in an order the plan fixes: the same bits
    return plan, got


def check_ishift_changes_no_bit(case):
    x0 = series(case)
    x1 = second_series(x0)
    for mode, b in ((L.OUT_POWER, None), (L.OUT_CROSS, x1)):
        pkw, _ = form_kw("linear-hann-shift")
        a = run(make_plan(case, "linear-hann-shift", mode), x0, b)
        c = run(make_plan(case, "linear-hann-shift", mode, flags=pkw["flags"] | L.ISHIFT_X), x0, b)
        assert np.array_equal(a, c), mode


def check_pitch_and_padding(case, form="linear-hann-shift"):
    """A pitch larger than the span (odd: the series start on 4-byte boundaries only), the samples beyond the span NaN: they must not reach the result."""
    sp = span(case)
    pitch = sp + 5
    x = series(case, pitch=pitch)
    dense = np.ascontiguousarray(x[:, :sp])
    x[:, sp:] = np.nan
    want = run(make_plan(case, form), dense)
    got = run(make_plan(case, form, pitch=pitch), x)
    assert np.isfinite(got).all() and np.array_equal(got, want)
    # ... and a view that starts one sample into a larger buffer (a 4-byte aligned pointer)
    buf = torch.full((case[3] * pitch + 1,), float("nan"), dtype=torch.float32, device=L.device())
    view = buf[1:].reshape(case[3], pitch)
    view[:, :sp] = torch.from_numpy(dense).to(L.device())
    assert view.data_ptr() % 16 == 4
    out, _ = make_plan(case, form, pitch=pitch).execute(view)
    assert np.array_equal(out.cpu().numpy().reshape(case[3], -1), want)


def check_no_overlap_is_the_plain_plan_and_reduce(case, form):
    """hop = L: within the bound of the existing plain 1-D plan followed by xrfthip_reduce_axis."""
    l, h, m, p = case[:4]
    assert h == l
    x = series(case)
    got = run(make_plan(case, form), x)
    pkw, _ = form_kw(form)
    pkw = dict(pkw)
    win = pkw.pop("window", None)
    plain = engine.SpectralPlan(ndim=1, batch=p * m, ny=1, nx=l, dtype=torch.float32, out_mode=L.OUT_POWER, scale=1.0,
                                window_x=api._window_vector(win, l) if win else None, **pkw)
    spec, _ = plain.execute(torch.from_numpy(x.reshape(p * m, l)).to(L.device()))
    comp = engine.reduce_axis(spec.reshape(p, m, l), 1, 1.0 / m).cpu().numpy()
    ref, _ = reference(case, form, x)
    kaps = kappa(case, form, x)
    for k in range(p):
        e1, e2, bnd = B.rel_error(got[k], ref[k]), B.rel_error(comp[k], ref[k]), bound(l, kaps[k])
        print(f"no overlap {case_id(case)} {form} series {k}: fused {e1:.3e} composed {e2:.3e} bound {bnd:.3e}; fused against composed {B.rel_error(got[k], comp[k]):.3e}")
        assert e1 <= bnd and e2 <= bnd and B.rel_error(got[k], comp[k]) <= 2 * bnd


def check_nan(case, form="linear-hann-shift"):
    l, h, m, p = case[:4]
    assert p == 3
    x = series(case)
    plan = make_plan(case, form)
    clean = run(plan, x)
    xn = x.copy()
    xn[1, span(case) // 2] = np.nan
    got = run(plan, xn)
    assert not np.isfinite(got[1]).any(), "series 1 has finite samples"
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    x1 = second_series(x)
    planc = make_plan(case, form, L.OUT_CROSS, lag=CROSS_LAG)
    cleanc = run(planc, x, x1)
    gotc = run(planc, x, np.where(np.isnan(xn), np.inf, x1).astype(np.float32))
    assert not (np.isfinite(gotc[1].real) | np.isfinite(gotc[1].imag)).any()
    assert np.array_equal(gotc[0], cleanc[0]) and np.array_equal(gotc[2], cleanc[2])


def _status(**kw):
    base = dict(ndim=1, batch=6, ny=1, nx=256, dtype=torch.float32, out_mode=L.OUT_POWER, mean_batch=3, seg_hop=128)
    base.update(kw)
    try:
        engine.SpectralPlan(**base)
    except L.XrftHipError as e:
        return e.status
    return 0


def check_status_codes():
    assert _status() == 0 and _status(seg_hop=1) == 0 and _status(seg_hop=256) == 0 and _status(out_mode=L.OUT_CROSS) == 0
    for fl in (L.SHIFT_X, L.ISHIFT_X, L.HALF_X, L.HALF_X | L.REALDIM_X2, L.SHIFT_X | L.ISHIFT_X):
        assert _status(flags=fl) == 0, fl
    for det in (L.DETREND_NONE, L.DETREND_CONSTANT, L.DETREND_LINEAR):
        assert _status(detrend=det) == 0
    bad = [dict(seg_hop=-1), dict(seg_hop=257), dict(ndim=2, ny=4), dict(ndim=2, ny=256, flags=L.AXIS_Y), dict(inner=4), dict(mid=4), dict(herm_ny=4, herm_nx=4),
           dict(flags=L.ISO), dict(in_stride_y=512), dict(mean_batch=0), dict(mean_batch=1), dict(batch=7), dict(out_mode=L.OUT_COMPLEX), dict(out_mode=L.OUT_PHASE),
           dict(out_mode=L.OUT_COHERENCE), dict(in_stride_batch=2 * 128 + 255), dict(flags=L.HALF_X | L.SHIFT_X)]
    for kw in bad:
        assert _status(**kw) == L.BAD_ARG, kw
    assert _status(in_stride_batch=2 * 128 + 256) == 0 and _status(in_stride_batch=2 * 128 + 257) == 0
    composes = [dict(nx=96, seg_hop=48), dict(nx=32, seg_hop=16), dict(nx=8192, seg_hop=4096), dict(dtype=torch.float64), dict(dtype=torch.complex64), dict(dtype=torch.float16),
                dict(dtype=torch.bfloat16), dict(flags=L.FLIP_X), dict(out_mode=L.OUT_CROSS, flags=L.FLIP0_X)]
    for kw in composes:
        assert _status(**kw) == L.UNSUPPORTED_LENGTH, kw
    # seg_hop = 0: everything as before -- a 1-D mean plan has no mean form
    assert _status(seg_hop=0) == L.UNSUPPORTED_LENGTH
    assert _status(seg_hop=0, mean_batch=0) == 0


def check_older_struct_sizes():
    """A descriptor with each of the six earlier struct_size values still creates its plan (the appended fields count as 0); seg_hop and seg_reserved came together:
    the size between the two, a larger one and a non-zero reserved word are XRFTHIP_BAD_ARG."""
    dll = L.load()
    D = L.DescSeg
    sizes = [getattr(D, f).offset for f in ("inner", "mid", "in_stride_y", "herm_ny", "mean_batch", "seg_hop")] + [C.sizeof(D)]
    assert sizes == sorted(set(sizes)) and sizes[-1] - sizes[-2] == 16 and len(sizes) == 7 and sizes[-2] == C.sizeof(L.Desc)
    for sz in sizes:
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        h = C.c_void_p(0)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0, sz
        dll.xrfthip_plan_destroy(h)
    # the field is read only from a descriptor that has it: the older size with garbage behind it is the plan without the field
    d = D(sizes[-2], 1, 6, 1, 256, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 128, 0)
    h = C.c_void_p(0)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.UNSUPPORTED_LENGTH
    for sz in (sizes[-2] + 8, sizes[-1] + 8):
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG, sz
    d = D(sizes[-1], 1, 6, 1, 256, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 128, 0)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
    dll.xrfthip_plan_destroy(h)
    d.seg_reserved = 1
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG


def check_workspace(case):
    """xrfthip_workspace_bytes is sufficient (the plan ran with exactly that above) and holds the partials; one byte less: XRFTHIP_WORKSPACE_TOO_SMALL."""
    l, h, m, p = case[:4]
    plan = make_plan(case, "plain")
    need = plan.workspace_bytes
    assert need >= p * B.runs_per_output(plan) * l * 8
    dev = L.device()
    x = torch.from_numpy(series(case)).to(dev)
    out = torch.empty((p, l), dtype=torch.float32, device=dev)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) & ~255
    dll = L.load()
    if dev != "cpu":
        torch.cuda.synchronize()
    args = (plan._h, C.c_void_p(x.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(0), C.c_void_p(base))
    assert dll.xrfthip_exec(*args, need - 1, C.c_void_p(0)) == -3  # XRFTHIP_WORKSPACE_TOO_SMALL
    assert dll.xrfthip_exec(*args, need, C.c_void_p(0)) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run(plan, series(case)))


# ---------------------------------------------------------------------------------- API level (both libraries)
import xrft_amd as xa  # noqa: E402


def api_series(shape, dims, dtype, seed, tdim="time", dt=0.5, t0=0.0, descending=False):
    """(the product's array, the float64 image of its samples, its coordinates)."""
    rng = np.random.default_rng(seed)
    n = shape[dims.index(tdim)]
    shp = [1] * len(shape)
    shp[dims.index(tdim)] = n
    v = rng.standard_normal(shape) + 0.01 * np.arange(n).reshape(shp) + 1.0
    t = torch.from_numpy(v).to({"float32": torch.float32, "float64": torch.float64}[dtype])
    crd = {d: np.arange(k) * 1.0 for d, k in zip(dims, shape)}
    crd[tdim] = t0 + np.arange(n) * dt
    if descending:
        crd[tdim] = crd[tdim][::-1].copy()
    return xa.DataArray(t.to(L.device()), dims, crd), t.to(torch.float64).numpy(), crd


def composed(da, da2, dim, nperseg, hop, **kw):
    """The expression the functions stand for: the segments unfolded, the public call, .mean."""
    seg = api._welch_segments(da, dim, nperseg, hop)
    if da2 is None:
        return xa.power_spectrum(seg, dim=[dim], **kw).mean(dim + "_segment")
    return xa.cross_spectrum(seg, api._welch_segments(da2, dim, nperseg, hop), dim=[dim], **kw).mean(dim + "_segment")


def oracle_welch(wide, crd, dims, dim, nperseg, hop, wide2=None, crd2=None, **kw):
    """The oracle's spectrum of the host's cut of the float64 samples, then the mean over the segments: (mean, mean of magnitudes) with ``dim`` last."""
    ax = dims.index(dim)
    n = wide.shape[ax]
    m = (n - nperseg) // hop + 1

    def cut(w):
        w = np.moveaxis(w, ax, -1)
        return np.stack([w[..., s * hop:s * hop + nperseg] for s in range(m)], axis=-2)

    sd = [d for d in dims if d != dim] + ["seg", dim]
    a = o.OArr(cut(wide), sd, {dim: crd[dim][:nperseg]})
    if wide2 is None:
        full = o.power_spectrum(a, dim=[dim], **kw).values
    else:
        full = o.cross_spectrum(a, o.OArr(cut(wide2), sd, {dim: (crd2 or crd)[dim][:nperseg]}), dim=[dim], **kw).values
    return full.mean(axis=-2), np.abs(full).mean(axis=-2)


def api_bound(dtype, nperseg, segs, detrend):
    kap = 0.0
    if detrend:
        s = segs.reshape(-1, nperseg)
        kap = A.kappa(s, A.detrended(s, (1,), L.DETREND_LINEAR if detrend == "linear" else L.DETREND_CONSTANT))
    return A.bound(dtype, nperseg, kap) + 16.0 * A.U[dtype]


# name -> (shape, dims, dtype, nperseg, noverlap, keyword arguments, fused?, descending)
LINHANN = dict(detrend="linear", window="hann", window_correction=True)
API_CASES = {
    "trailing-256": ((3, 1000), ("x", "time"), "float32", 256, None, LINHANN, True, False),
    "real-dim-64": ((2, 3, 300), ("y", "x", "time"), "float32", 64, 27, dict(LINHANN, real_dim="time"), True, False),
    "leading-time": ((700, 3), ("time", "x"), "float32", 128, 64, dict(detrend="constant", window="hann"), True, False),  # (arranged first, then fused)
    "float64": ((3, 600), ("x", "time"), "float64", 128, None, LINHANN, False, False),
    "length-96": ((3, 500), ("x", "time"), "float32", 96, None, LINHANN, False, False),
    "descending": ((3, 600), ("x", "time"), "float32", 128, None, LINHANN, True, True),  # (a power spectrum flips nothing: fused; the cross spectrum of check_api_cross_descending composes)
}


def check_api_case(name):
    shape, dims, dtype, nperseg, noverlap, kw, fused, desc = API_CASES[name]
    api.clear_plan_cache()
    da, wide, crd = api_series(shape, dims, dtype, seed=51, descending=desc)
    hop = nperseg - (nperseg // 2 if noverlap is None else noverlap)
    got = xa.welch_power_spectrum(da, "time", nperseg, noverlap, **kw)
    kinds = [p.kernel_info()[0] for p in api._plan_cache.values()]
    assert (B.newest_plan().kernel_info()[0] == L.K_FASTW) if fused else (L.K_FASTW not in kinds), B.newest_plan().describe()
    want = composed(da, None, "time", nperseg, hop, **kw)
    B.compare_labelled(got, want)
    assert tuple(got.dims) == tuple(d for d in dims if d != "time") + ("freq_time",)
    ref, _ = oracle_welch(wide, crd, list(dims), "time", nperseg, hop, **kw)
    m = (shape[dims.index("time")] - nperseg) // hop + 1
    segs = np.stack([np.moveaxis(wide, dims.index("time"), -1)[..., s * hop:s * hop + nperseg] for s in range(m)], axis=-2)
    err, bnd = B.rel_error(got.values, ref), api_bound(dtype, nperseg, segs, kw.get("detrend"))
    print(f"welch_power_spectrum {name}: error {err:.3e} bound {bnd:.3e} (fused: {fused}); composed {B.rel_error(want.values, ref):.3e}")
    assert np.isfinite(got.values).all() and err <= bnd, (err, bnd)
    assert B.rel_error(want.values, ref) <= bnd


def check_api_cross_and_coherence():
    api.clear_plan_cache()
    shape, dims, nperseg = (3, 1000), ("x", "time"), 256
    da, wide, crd = api_series(shape, dims, "float32", seed=52)
    rng = np.random.default_rng(53)
    w2 = (np.roll(wide, 5, axis=1) + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    crd2 = dict(crd, time=crd["time"] + 3.5)  # (another origin: the net true-phase factor is not 1)
    da2 = xa.DataArray(torch.from_numpy(w2).to(L.device()), dims, crd2)
    kw = dict(LINHANN)
    got = xa.welch_cross_spectrum(da, da2, "time", nperseg, **kw)
    assert B.newest_plan().kernel_info()[0] == L.K_FASTW, B.newest_plan().describe()
    want = composed(da, da2, "time", nperseg, nperseg // 2, **kw)
    B.compare_labelled(got, want)
    ref, mag = oracle_welch(wide, crd, list(dims), "time", nperseg, nperseg // 2, w2.astype(np.float64), crd2, **kw)
    segs = lambda w: np.stack([w[:, s * 128:s * 128 + 256] for s in range((1000 - 256) // 128 + 1)], axis=1)  # noqa: E731
    bnd = max(api_bound("float32", nperseg, segs(wide), "linear"), api_bound("float32", nperseg, segs(w2.astype(np.float64)), "linear"))
    err = B.rel_error(got.values, ref, mag)
    print(f"welch_cross_spectrum: error {err:.3e} bound {bnd:.3e}; composed {B.rel_error(want.values, ref, mag):.3e}")
    assert np.isfinite(got.values.real).all() and np.isfinite(got.values.imag).all() and err <= bnd
    # the coherence: the library's division of the three means
    coh = xa.welch_coherence(da, da2, "time", nperseg, **kw)
    p1, _ = oracle_welch(wide, crd, list(dims), "time", nperseg, 128, **kw)
    p2, _ = oracle_welch(w2.astype(np.float64), crd2, list(dims), "time", nperseg, 128, **kw)
    cref = np.abs(ref) ** 2 / (p1 * p2)
    assert coh.dims == got.dims and coh.values.dtype == np.float32
    cerr = float(np.abs(coh.values - cref).max())
    print(f"welch_coherence: max error {cerr:.3e}")
    assert cerr <= 64 * U32  # (a quotient of three means, each within a few u of values <= 1)
    assert coh.values.min() >= 0.0 and coh.values.max() <= 1.0 + 8 * U32


def check_api_cross_descending():
    """A descending coordinate under true_phase: the reference flips each field, the plan declines the flip, the call composes -- same labels, same values."""
    api.clear_plan_cache()
    shape, dims, nperseg = (2, 600), ("x", "time"), 128
    da, wide, crd = api_series(shape, dims, "float32", seed=55, descending=True)
    da2 = xa.DataArray(torch.from_numpy(np.roll(wide, 3, axis=1).astype(np.float32)).to(L.device()), dims, crd)
    got = xa.welch_cross_spectrum(da, da2, "time", nperseg, **LINHANN)
    assert L.K_FASTW not in [p.kernel_info()[0] for p in api._plan_cache.values()]
    want = composed(da, da2, "time", nperseg, nperseg // 2, **LINHANN)
    B.compare_labelled(got, want)
    assert np.array_equal(got.values, want.values)


def check_api_errors():
    import pytest

    da, _, _ = api_series((3, 300), ("x", "time"), "float32", seed=54)
    for kw in (dict(nperseg=301), dict(nperseg=0), dict(nperseg=64, noverlap=64), dict(nperseg=64, noverlap=-1)):
        with pytest.raises(ValueError):
            xa.welch_power_spectrum(da, "time", **kw)
        with pytest.raises(ValueError):
            xa.welch_cross_spectrum(da, da, "time", **kw)
    with pytest.raises(ValueError):
        xa.welch_power_spectrum(da, "nope", 64)
    with pytest.raises(ValueError):
        xa.welch_coherence(da, da, "time", 300)  # (one segment)
    with pytest.raises(ValueError):
        xa.welch_coherence(da, da, "time", 200, 50)  # (one segment: 150 more samples would be needed)
    # a linear detrend refuses non-finite samples (scipy.signal.detrend's refusal, as the composed call) -- in any segment, not beyond the last one
    v = da.data.clone()
    v[1, 299] = float("nan")
    dn = xa.DataArray(v, da.dims, da.coords)
    assert np.isfinite(xa.welch_power_spectrum(dn, "time", 64, detrend="linear").values).all()  # (sample 299 fills no segment: 9 x 32 + 64 = 288 + ... dropped)
    v[1, 200] = float("inf")
    for route in (dn, xa.DataArray(v.to(torch.float64), da.dims, da.coords)):
        with pytest.raises(ValueError):
            xa.welch_power_spectrum(route, "time", 64, detrend="linear")
    assert xa.welch_power_spectrum(da, "time", 300).dims == ("x", "freq_time")  # (one segment is a spectrum)
    assert xa.welch_power_spectrum(da, "time", 64).shape == (3, 64) and xa.welch_power_spectrum(da, "time", 64, real_dim="time").shape == (3, 33)
