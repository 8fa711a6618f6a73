"""Shared by the tests of Welch spectra along a leading axis (xrfthip_desc.seg_stride, the column layout of csrc/fastw.h; tests/test_welch_cols_emulated.py on the
emulated library, tests/test_gpu_welch_cols.py on the MI355X).  Not a conftest: imported by the tests that use it.

The reference and the bound are those of tests/welch.py: column e of block p is series p * inner + e of the rows case (L, H, M, P * inner), compared with the
oracle's spectra of the float64 image of the same samples, cut on the host and averaged in float64 (welch.reference), within welch.bound per output
(welch.assert_outputs); welch.api_bound at the API.  No tolerance of its own.

Every column carries its own amplitude, 3^(e mod 4), every block a further factor 5^p: a segment summed into the wrong column misses the bound.  The samples are
handed over as the view the plan addresses, inside a buffer that starts one float before them and holds NaN wherever the plan must not read (the gap between
inner and S, the space behind the span): every check is also a check that nothing else is read."""
import ctypes as C

import numpy as np
import torch

from xrft_amd import _lib as L
from xrft_amd import api, engine

import batch_mean as B
import welch as W

# (L, H, M, P, inner, S, runs pinned (0 = the plan's choice), the longest run, floats added to the dense block pitch (0 = in_stride_batch 0))
CASES = [
    (64, 32, 3, 1, 32, 32, 0, None, 0),        # exactly one full group, an odd segment count
    (64, 37, 35, 2, 33, 40, 1, 35, 5),         # a tail group of one column, a box (S > inner), two blocks with a pitch, 35 segments in ONE run
    (64, 1, 36, 1, 5, 5, 2, 18, 0),            # two runs of 18, fewer columns than a group
    (128, 64, 4, 1, 70, 70, 0, None, 0),       # three groups
    (256, 128, 3, 3, 17, 24, 0, None, 0),      # 16 columns per group: two groups, the second of one column; three dense blocks of a box
    (512, 256, 2, 1, 9, 9, 0, None, 0),        # 8 columns per group
    (64, 32, 2, 1, 1, 7, 0, None, 0),          # one column of a wide grid
    (64, 32, 2, 1, 9000, 9000, 0, None, 0),    # more workgroups than CUs
    # (not in the issue's list) one pair of segments per round at L = 512: 35 segments in one run are 18 rounds -- a full float32 chain of 16, the hand-over to
    # float64, and two more that ADD to the partial
    (512, 1, 35, 1, 9, 9, 1, 35, 0),
]
CROSS_CASES = [CASES[1], CASES[2], CASES[4]]
HALF_CASES = [CASES[1], CASES[4]]
CONSTANT_CASES = [CASES[0], CASES[3]]
GROUP = {64: 32, 128: 32, 256: 16, 512: 8}  # columns per workgroup (fastw.h)


def case_id(c):
    return f"L{c[0]}-H{c[1]}-M{c[2]}-P{c[3]}-in{c[4]}-S{c[5]}" + (f"-runs{c[6]}" if c[6] else "")


def rows_case(c):
    """The rows case of tests/welch.py whose series are the columns: series p * inner + e."""
    return (c[0], c[1], c[2], c[3] * c[4], c[6], c[7])


def span(c):
    return (c[2] - 1) * c[1] + c[0]


def pitch_of(c):
    """(in_stride_batch of the plan, floats between the blocks in memory)."""
    dense = span(c) * c[5]
    return (dense + c[8] if c[8] else 0), dense + c[8]


def cube(c, seed=43):
    """[P][span][inner] float32: seeded noise over a line along time, column e scaled by 3^(e mod 4), block p by 5^p."""
    l, h, m, p, inner = c[:5]
    n = span(c)
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((p, n, inner)) + (0.01 * np.arange(n) + 1.5).reshape(1, n, 1)
    v *= (3.0 ** (np.arange(inner) % 4)).reshape(1, 1, inner) * (5.0 ** np.arange(p)).reshape(p, 1, 1)
    return v.astype(np.float32)


def second_cube(x, seed=44):
    """The first rolled by 5 samples along time plus a tenth of its size in noise."""
    rng = np.random.default_rng(seed)
    amp = np.abs(x).mean(axis=1, keepdims=True)
    return (np.roll(x, 5, axis=1) + 0.1 * amp * rng.standard_normal(x.shape)).astype(np.float32)


def as_rows(x):
    """[P * inner][span]: the series of the rows case."""
    p, n, inner = x.shape
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1)).reshape(p * inner, n))


def view_of(c, x, fill=float("nan")):
    """The samples as the view (P, span, inner) with strides (pitch, S, 1) that starts ONE float into a buffer filled with ``fill`` (a 4-byte aligned pointer)."""
    l, h, m, p, inner, s = c[:6]
    n = span(c)
    _, pitch = pitch_of(c)
    dev = L.device()
    buf = torch.full((1 + p * pitch + 3,), fill, dtype=torch.float32, device=dev)
    v = torch.as_strided(buf, (p, n, inner), (pitch, s, 1), 1)
    v.copy_(torch.from_numpy(x).to(dev))
    return v


def make_plan(c, form="plain", mode=L.OUT_POWER, lag=None, **over):
    kw = dict(inner=c[4], seg_stride=c[5])
    kw.update(over)
    return W.make_plan((c[0], c[1], c[2], c[3], c[6], c[7]), form, mode, pitch=pitch_of(c)[0], lag=lag, **kw)


def run(plan, c, x0, x1=None):
    out, _ = plan.execute(view_of(c, x0), None if x1 is None else view_of(c, x1))
    assert tuple(out.shape[:2]) == (c[3], c[4])
    return out.cpu().numpy().reshape(c[3] * c[4], -1)


def assert_column_plan(plan, c):
    d = plan.describe()
    assert plan.kernel_info()[0] == L.K_FASTW and "[fastw]" in d and "[fastw columns]" in d and "[mean over the batch]" in d, d
    assert plan.seg_stride == c[5] and plan.inner == c[4]
    assert f"of {c[4]} adjacent columns, sample stride {c[5]} " in d and f"takes {GROUP[c[0]]} adjacent columns" in d, d


def check_plan(c, form, mode=L.OUT_POWER, lag=None, half=0):
    l, h, m, p, inner, s, runs, run_len, _ = c
    rc = rows_case(c)
    x0 = cube(c)
    x1 = second_cube(x0) if mode == L.OUT_CROSS else None
    over = {}
    if half:
        pkw, _ = W.form_kw(form)
        over["flags"] = (pkw["flags"] & ~L.SHIFT_X) | L.HALF_X | (L.REALDIM_X2 if half == 2 else 0)
    plan = make_plan(c, form, mode, lag=lag, **over)
    assert_column_plan(plan, c)
    if run_len is not None:
        assert B.runs_per_output(plan) == runs and B.run_length(plan) == run_len, plan.describe()
    got = run(plan, c, x0, x1)
    nxo = l // 2 + 1 if half else l
    assert got.shape == (p * inner, nxo) and got.dtype == (np.complex64 if mode == L.OUT_CROSS else np.float32)
    r0, r1 = as_rows(x0), None if x1 is None else as_rows(x1)
    ref, mag = W.reference(rc, form, r0, r1, lag, half)
    kaps = W.kappa(rc, form, r0)
    if r1 is not None:
        kaps = [max(a, b) for a, b in zip(kaps, W.kappa(rc, form, r1))]
    W.assert_outputs(rc, got, ref, mag if r1 is not None else None, kaps, f"columns {'cross' if r1 is not None else 'power'} {case_id(c)} {form} half={half}")
    assert np.array_equal(got, run(plan, c, x0, x1))  # every addition in an order the plan fixes: the same bits
    return plan, got


def check_unit_stride_is_the_rows_plan(case=W.CASES[1]):
    """seg_stride = 1 with inner = 1 is the rows form itself: the same plan (its describe text) and the same bits."""
    x = W.series(case)
    rows = W.make_plan(case, "linear-hann-shift")
    cols = W.make_plan(case, "linear-hann-shift", inner=1, seg_stride=1)
    assert rows.describe() == cols.describe() and "[fastw columns]" not in cols.describe()
    assert np.array_equal(W.run(rows, x), W.run(cols, x))


def check_nan(c=CASES[1], e=31, form="linear-hann-shift"):
    """A NaN in one sample of column e of block 1: exactly output (1, e) is non-finite, every other output keeps its bits (so e - 1 and e + 1 stay within the bound)."""
    l, h, m, p, inner = c[:5]
    x = cube(c)
    plan = make_plan(c, form)
    clean = run(plan, c, x)
    xn = x.copy()
    xn[1, span(c) // 2, e] = np.nan
    got = run(plan, c, xn)
    bad = inner + e
    assert not np.isfinite(got[bad]).any()
    keep = np.arange(p * inner) != bad
    assert np.isfinite(got[keep]).all() and np.array_equal(got[keep], clean[keep])
    rc = rows_case(c)
    ref, _ = W.reference(rc, form, as_rows(x))
    kaps = W.kappa(rc, form, as_rows(x))
    for k in (bad - 1, bad + 1):
        assert B.rel_error(got[k], ref[k]) <= W.bound(l, kaps[k])
    x1 = second_cube(x)
    planc = make_plan(c, form, L.OUT_CROSS, lag=W.CROSS_LAG)
    cleanc = run(planc, c, x, x1)
    gotc = run(planc, c, x, np.where(np.isnan(xn), np.inf, x1).astype(np.float32))
    assert not (np.isfinite(gotc[bad].real) | np.isfinite(gotc[bad].imag)).any()
    assert np.array_equal(gotc[keep], cleanc[keep])


def check_gap_is_never_read(form="linear-hann-shift"):
    """An odd S above inner, a pitch above the span and a base pointer one float into its buffer: the gap and the space behind the span hold NaN in one run and
    1e30 in another and change no bit -- and the bits are those of the dense cube (S = inner)."""
    c = (64, 37, 5, 2, 33, 41, 0, None, 7)
    x = cube(c)
    plan = make_plan(c, form)
    a, _ = plan.execute(view_of(c, x, float("nan")))
    b, _ = plan.execute(view_of(c, x, 1e30))
    assert view_of(c, x).data_ptr() % 16 == 4
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b)
    dense = c[:5] + (c[4],) + (0, None, 0)
    assert np.array_equal(a.reshape(c[3] * c[4], -1), run(make_plan(dense, form), dense, x))


def check_workspace(c=CASES[2]):
    """xrfthip_workspace_bytes is sufficient and holds the partials [P * inner][runs][L] float64; one byte less: XRFTHIP_WORKSPACE_TOO_SMALL."""
    l, h, m, p, inner = c[:5]
    plan = make_plan(c, "plain")
    need = plan.workspace_bytes
    assert need >= p * inner * B.runs_per_output(plan) * l * 8
    assert need < p * inner * B.runs_per_output(plan) * l * 8 + (1 << 16)
    dev = L.device()
    x = cube(c)
    v = view_of(c, x)
    out = torch.empty((p, inner, l), dtype=torch.float32, device=dev)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) & ~255
    dll = L.load()
    if dev != "cpu":
        torch.cuda.synchronize()
    args = (plan._h, C.c_void_p(v.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(0), C.c_void_p(base))
    assert dll.xrfthip_exec(*args, need - 1, C.c_void_p(0)) == -3  # XRFTHIP_WORKSPACE_TOO_SMALL
    assert dll.xrfthip_exec(*args, need, C.c_void_p(0)) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(p * inner, l), run(plan, c, x))


def _status(**kw):
    base = dict(ndim=1, batch=6, ny=1, nx=256, dtype=torch.float32, out_mode=L.OUT_POWER, mean_batch=3, seg_hop=128, inner=4, seg_stride=4)
    base.update(kw)
    try:
        engine.SpectralPlan(**base)
    except L.XrftHipError as e:
        return e.status
    return 0


def check_status_codes():
    sp = 2 * 128 + 256
    assert _status() == 0 and _status(seg_stride=9) == 0 and _status(inner=1, seg_stride=1) == 0 and _status(inner=1, seg_stride=5) == 0 and _status(out_mode=L.OUT_CROSS) == 0
    for fl in (L.SHIFT_X, L.ISHIFT_X, L.HALF_X, L.HALF_X | L.REALDIM_X2, L.SHIFT_X | L.ISHIFT_X):
        assert _status(flags=fl) == 0, fl
    for det in (L.DETREND_NONE, L.DETREND_CONSTANT, L.DETREND_LINEAR):
        assert _status(detrend=det) == 0
    for nx in (64, 128, 512):
        assert _status(nx=nx, seg_hop=nx // 2) == 0
    # the pitch: 0, or at least ((M - 1) H + L - 1) S + inner
    assert _status(seg_stride=7, in_stride_batch=(sp - 1) * 7 + 4) == 0 and _status(seg_stride=7, in_stride_batch=(sp - 1) * 7 + 3) == L.BAD_ARG
    bad = [dict(seg_stride=-1), dict(seg_hop=0), dict(seg_hop=0, mean_batch=0), dict(seg_stride=3), dict(seg_stride=0), dict(inner=2, seg_stride=1), dict(mid=2),
           dict(ndim=2, ny=4), dict(ndim=2, ny=256, flags=L.AXIS_Y), dict(herm_ny=4, herm_nx=4), dict(flags=L.ISO), dict(in_stride_y=512), dict(mean_batch=1), dict(batch=7),
           dict(out_mode=L.OUT_COMPLEX), dict(out_mode=L.OUT_COHERENCE), dict(seg_hop=257), dict(flags=L.HALF_X | L.SHIFT_X)]
    for kw in bad:
        assert _status(**kw) == L.BAD_ARG, kw
    arranges = [dict(nx=1024, seg_hop=512), dict(nx=4096, seg_hop=2048), dict(nx=96, seg_hop=48), dict(nx=32, seg_hop=16), dict(dtype=torch.float64), dict(dtype=torch.complex64),
                dict(dtype=torch.float16), dict(dtype=torch.bfloat16), dict(flags=L.FLIP_X), dict(out_mode=L.OUT_CROSS, flags=L.FLIP0_X)]
    for kw in arranges:
        assert _status(**kw) == L.UNSUPPORTED_LENGTH, kw
    with B.env("XRFTHIP_FASTW_COLS", 0):
        assert _status() == L.UNSUPPORTED_LENGTH
        assert _status(inner=1, seg_stride=1) == 0  # (the rows form)
    assert L.load().xrfthip_version() == 106


def check_struct_sizes():
    """The seven earlier struct_size values still create their plans (the appended words count as 0); seg_stride and seg_reserved2 came together: the size between
    the two, a larger one and a non-zero reserved word (either) are XRFTHIP_BAD_ARG."""
    dll = L.load()
    D = L.DescCols
    sizes = [getattr(D, f).offset for f in ("inner", "mid", "in_stride_y", "herm_ny", "mean_batch", "seg_hop", "seg_stride")] + [C.sizeof(D)]
    assert sizes == sorted(set(sizes)) and len(sizes) == 8 and sizes[-1] - sizes[-2] == 16 and sizes[-2] == C.sizeof(L.DescSeg) and sizes[-3] == C.sizeof(L.Desc)
    h = C.c_void_p(0)
    for sz in sizes:
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0, sz
        dll.xrfthip_plan_destroy(h)
    for sz in (sizes[-2] + 8, sizes[-1] + 8):
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG, sz

    def welch(sz, inner, stride, r1=0, r2=0):
        return D(sz, 1, 6, 1, 256, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, inner, 0, 0, 0, 0, 0, 3, 128, r1, stride, r2)

    # the words are read only from a descriptor that has them: the older size with a stride behind it is the rows plan (inner = 4 without a stride: BAD_ARG)
    buf = C.create_string_buffer(8192)
    d = welch(sizes[-2], 1, 7)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
    dll.xrfthip_plan_describe(h, buf, len(buf))
    assert b"[fastw]" in buf.value and b"[fastw columns]" not in buf.value
    dll.xrfthip_plan_destroy(h)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(welch(sizes[-2], 4, 7))) == L.BAD_ARG
    d = welch(sizes[-1], 4, 7)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
    dll.xrfthip_plan_describe(h, buf, len(buf))
    assert b"[fastw columns]" in buf.value
    dll.xrfthip_plan_destroy(h)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(welch(sizes[-1], 4, 7, r2=1))) == L.BAD_ARG
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(welch(sizes[-1], 4, 7, r1=1))) == L.BAD_ARG


# ---------------------------------------------------------------------------------- API level (both libraries)
import xrft_amd as xa  # noqa: E402

LINHANN = W.LINHANN
# name -> (shape, dims, nperseg, noverlap, keyword arguments, isel of the array or None, (seg_stride, inner) of the newest plan)
API_CASES = {
    "cube": ((300, 5, 7), ("time", "y", "x"), 64, 27, LINHANN, None, (35, 35)),
    "members": ((2, 300, 3, 5), ("member", "time", "y", "x"), 64, 27, LINHANN, None, (15, 15)),
    "box": ((300, 8), ("time", "x"), 64, 27, LINHANN, dict(x=slice(1, 6)), (8, 5)),
    "real-dim": ((300, 5, 7), ("time", "y", "x"), 64, 27, dict(LINHANN, real_dim="time"), None, (35, 35)),
}


def _sliced(da, wide, crd, dims, isel):
    if not isel:
        return da, wide, crd
    idx = tuple(isel.get(d, slice(None)) for d in dims)
    return da.isel(**isel), wide[idx], {d: (v[isel[d]] if d in isel else v) for d, v in crd.items()}


def assert_newest_is_column_plan(want):
    p = B.newest_plan()
    assert p.kernel_info()[0] == L.K_FASTW and "[fastw columns]" in p.describe() and (p.seg_stride, p.inner) == want, p.describe()


def assert_within_api_bound(what, got, wide, crd, dims, nperseg, hop, kw, dtype="float32", also=None):
    """``got`` (and ``also``, the composed expression) against the oracle's Welch spectrum of the float64 samples, within welch.api_bound."""
    ref, _ = W.oracle_welch(wide, crd, list(dims), "time", nperseg, hop, **kw)
    t = dims.index("time")
    m = (wide.shape[t] - nperseg) // hop + 1
    segs = np.stack([np.moveaxis(wide, t, -1)[..., s * hop:s * hop + nperseg] for s in range(m)], axis=-2)
    err, bnd = B.rel_error(got.values, ref), W.api_bound(dtype, nperseg, segs, kw.get("detrend"))
    print(f"welch_power_spectrum {what}: error {err:.3e} bound {bnd:.3e}" + ("" if also is None else f"; composed {B.rel_error(also.values, ref):.3e}"))
    assert np.isfinite(got.values).all() and err <= bnd, (err, bnd)
    assert also is None or B.rel_error(also.values, ref) <= bnd


def check_api_case(name):
    shape, dims, nperseg, noverlap, kw, isel, want = API_CASES[name]
    api.clear_plan_cache()
    da, wide, crd = W.api_series(shape, dims, "float32", seed=71)
    da, wide, crd = _sliced(da, wide, crd, dims, isel)
    hop = nperseg - noverlap
    before = da.data.clone()
    got = xa.welch_power_spectrum(da, "time", nperseg, noverlap, **kw)
    assert_newest_is_column_plan(want)
    assert torch.equal(da.data, before)
    want_da = W.composed(da, None, "time", nperseg, hop, **kw)
    B.compare_labelled(got, want_da)
    assert tuple(got.dims) == tuple(d for d in dims if d != "time") + ("freq_time",)
    assert_within_api_bound(f"in place {name}", got, wide, crd, dims, nperseg, hop, kw, also=want_da)
    return got


def check_api_cross_and_coherence():
    api.clear_plan_cache()
    shape, dims, nperseg, hop = (300, 5, 7), ("time", "y", "x"), 64, 32
    da, wide, crd = W.api_series(shape, dims, "float32", seed=72)
    rng = np.random.default_rng(73)
    w2 = (np.roll(wide, 5, axis=0) + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    crd2 = dict(crd, time=crd["time"] + 3.5)  # (another origin: the net true-phase factor is not 1)
    da2 = xa.DataArray(torch.from_numpy(w2).to(L.device()), dims, crd2)
    kw = dict(LINHANN)
    got = xa.welch_cross_spectrum(da, da2, "time", nperseg, **kw)
    assert_newest_is_column_plan((35, 35))
    want = W.composed(da, da2, "time", nperseg, hop, **kw)
    B.compare_labelled(got, want)
    ref, mag = W.oracle_welch(wide, crd, list(dims), "time", nperseg, hop, w2.astype(np.float64), crd2, **kw)
    m = (300 - nperseg) // hop + 1
    segs = lambda w: np.stack([np.moveaxis(w, 0, -1)[..., s * hop:s * hop + nperseg] for s in range(m)], axis=-2)  # noqa: E731
    bnd = max(W.api_bound("float32", nperseg, segs(wide), "linear"), W.api_bound("float32", nperseg, segs(w2.astype(np.float64)), "linear"))
    err = B.rel_error(got.values, ref, mag)
    print(f"welch_cross_spectrum in place: error {err:.3e} bound {bnd:.3e}; composed {B.rel_error(want.values, ref, mag):.3e}")
    assert np.isfinite(got.values.real).all() and np.isfinite(got.values.imag).all() and err <= bnd
    assert B.rel_error(want.values, ref, mag) <= bnd
    coh = xa.welch_coherence(da, da2, "time", nperseg, **kw)
    assert_newest_is_column_plan((35, 35))
    p1, _ = W.oracle_welch(wide, crd, list(dims), "time", nperseg, hop, **kw)
    p2, _ = W.oracle_welch(w2.astype(np.float64), crd2, list(dims), "time", nperseg, hop, **kw)
    cref = np.abs(ref) ** 2 / (p1 * p2)
    assert coh.dims == got.dims and coh.values.dtype == np.float32
    cerr = float(np.abs(coh.values - cref).max())
    print(f"welch_coherence in place: max error {cerr:.3e}")
    assert cerr <= 64 * W.U32  # (the bound of tests/welch.py: a quotient of three means, each within a few u of values <= 1)
    assert coh.values.min() >= 0.0 and coh.values.max() <= 1.0 + 8 * W.U32
    # two fields with different strides: both arranged, the rows plan, the same labels
    da3 = xa.DataArray(torch.from_numpy(np.ascontiguousarray(np.moveaxis(w2, 0, -1))).to(L.device()).movedim(-1, 0), dims, crd2)
    assert da3.data.stride() != da.data.stride()
    got3 = xa.welch_cross_spectrum(da, da3, "time", nperseg, **kw)
    assert B.newest_plan().kernel_info()[0] == L.K_FASTW and "[fastw columns]" not in B.newest_plan().describe()
    B.compare_labelled(got3, want)
    assert B.rel_error(got3.values, ref, mag) <= bnd


def check_api_not_the_column_plan():
    """A float64 cube composes and nperseg = 1024 is arranged first (the rows plan), as before: no column plan, values within the bound."""
    for dtype, nperseg, n in (("float64", 64, 300), ("float32", 1024, 2500)):
        api.clear_plan_cache()
        shape, dims = (n, 2, 3), ("time", "y", "x")
        da, wide, crd = W.api_series(shape, dims, dtype, seed=74)
        got = xa.welch_power_spectrum(da, "time", nperseg, **LINHANN)
        descs = [p.describe() for p in api._plan_cache.values()]
        assert not any("[fastw columns]" in d for d in descs)
        assert any("[fastw]" in d for d in descs) == (dtype == "float32")
        hop = nperseg // 2
        want = W.composed(da, None, "time", nperseg, hop, **LINHANN)
        B.compare_labelled(got, want)
        assert_within_api_bound(f"{dtype} nperseg {nperseg} over a leading axis", got, wide, crd, dims, nperseg, hop, LINHANN, dtype, also=want)
    # a view whose trailing dims are not one unit-stride run (every second x): arranged, the rows plan
    api.clear_plan_cache()
    da, wide, crd = W.api_series((300, 4, 6), ("time", "y", "x"), "float32", seed=75)
    dv = da.isel(x=slice(0, 6, 2))
    got = xa.welch_power_spectrum(dv, "time", 64, **LINHANN)
    assert "[fastw columns]" not in B.newest_plan().describe() and B.newest_plan().kernel_info()[0] == L.K_FASTW
    B.compare_labelled(got, W.composed(dv, None, "time", 64, 32, **LINHANN))
    assert_within_api_bound("every second x", got, wide[:, :, ::2], dict(crd, x=crd["x"][::2]), dims, 64, 32, LINHANN)


def check_api_column_blocks(monkeypatch):
    """The cap patched small: (300, 1, 70) runs as blocks of 32, 32 and a tail of 6 columns -- two plans -- and returns the bits of the unblocked call (7 segments:
    three runs per output in either call)."""
    shape, dims = (300, 1, 70), ("time", "y", "x")
    da, _, _ = W.api_series(shape, dims, "float32", seed=76)
    for two in (False, True):
        call = (lambda: xa.welch_cross_spectrum(da, da, "time", 64, 27, **LINHANN)) if two else (lambda: xa.welch_power_spectrum(da, "time", 64, 27, **LINHANN))
        api.clear_plan_cache()
        whole = call()
        assert_newest_is_column_plan((70, 70))
        assert len(api._plan_cache) == 1
        api.clear_plan_cache()
        monkeypatch.setattr(api, "_WELCH_COLS_WS_CAP", 1)
        blocked = call()
        monkeypatch.undo()
        plans = list(api._plan_cache.values())
        assert sorted((p.seg_stride, p.inner) for p in plans) == [(70, 6), (70, 32)], [p.describe() for p in plans]
        assert all(B.runs_per_output(p) == 3 for p in plans)
        B.compare_labelled(blocked, whole)
        assert np.array_equal(blocked.values, whole.values)
    # ... and with blocks in front of time (the blocks of a (member, time, x) array are copied into the result)
    da, _, _ = W.api_series((2, 300, 40), ("member", "time", "x"), "float32", seed=77)
    api.clear_plan_cache()
    whole = xa.welch_power_spectrum(da, "time", 64, 27, **LINHANN)
    api.clear_plan_cache()
    monkeypatch.setattr(api, "_WELCH_COLS_WS_CAP", 1)
    blocked = xa.welch_power_spectrum(da, "time", 64, 27, **LINHANN)
    monkeypatch.undo()
    assert sorted((p.seg_stride, p.inner) for p in api._plan_cache.values()) == [(40, 8), (40, 32)]
    assert np.array_equal(blocked.values, whole.values)
