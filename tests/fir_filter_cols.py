"""Shared by the tests of the FIR filter's column layout (xrfthip_desc.seg_filter_cols, csrc/fastf.h fastf_kernel<.., true>, xrft_amd.fir_filter along a leading
dim; tests/test_fir_filter_cols_emulated.py on the emulated library, tests/test_gpu_fir_filter_cols.py on the MI355X).  Not a conftest: imported by the tests that
use it.

The model, the bound and the taps are those of tests/fir_filter.py: scipy.signal.convolve in float64 per column, || got - ref ||_2 <= (2 b + 4 u) Hmax A.  Nothing
here has a tolerance of its own: besides the bound, every comparison is np.array_equal -- against the rows plan on the transposed contiguous copy, against a column
run alone, a shorter record, a second execution, the knob-off call.

A case is (L, K, N, blocks, inner, S): `blocks` blocks of N time rows of `inner` adjacent columns whose samples lie S elements apart.  The input of every plan-level
check lives in a buffer filled with NaN: what lies between the columns (S > inner) and behind a block (blocks > 1: the pitch is 11 elements beyond what a block
reaches) would show in the result."""
import ctypes as C

import numpy as np
import torch

import xrft_amd as xa
from xrft_amd import _lib as L
from xrft_amd import _segments as SEG
from xrft_amd import api, engine

import batch_mean as B
import fir_filter as F
import spectrogram as S
import welch_cols as WC
from fir_filter import assert_within, model, offsets, taps_of, the_bound

MODES = F.MODES
TAPS = F.TAPS
# L = 64: spr = 4 segments of a column per tile, M = 13 ("same"), 6, 16 | 17; 128: spr 2; 256 and 512: spr 1, 512 with C = 16.  K = 1, a mid K and K - 1 = L / 2 at
# every L but 256 / 64 where two of the three stand.  inner = 1 inside S = 7 (one column of a wider array), 5, 32 (one full group), 33 (a second group of one live
# column), 40 (a last group of 8 live columns; C = 16: three groups).  S = inner and S > inner; one block, and three with a pitch beyond the block
CASES = [(64, 9, 700, 1, 5, 5), (64, 1, 300, 3, 1, 7), (64, 33, 500, 1, 33, 40), (128, 65, 600, 3, 40, 40), (128, 17, 450, 1, 32, 33), (256, 31, 900, 1, 33, 33),
         (256, 129, 1500, 3, 5, 9), (512, 65, 1300, 1, 40, 64), (512, 257, 1100, 3, 1, 7), (512, 1, 600, 1, 5, 5)]
PLAN_PARAMS = [(c, m, t) for c in CASES for m in MODES for t in TAPS]
PREFIX_CASES = [((64, 9, 700, 1, 5, 5), 500), ((128, 65, 600, 3, 40, 40), 450), ((512, 65, 1300, 1, 40, 64), 1000)]
GAP_CASES = [c for c in CASES if c[5] > c[4] and c[3] > 1]
CONTAIN = (256, 65, 700, 3, 5, 9)
GROUP = {64: 32, 128: 32, 256: 32, 512: 16}  # columns per workgroup (fastf.h)
SPR = {64: 4, 128: 2, 256: 1, 512: 1}        # segments of a column per tile


def case_id(c):
    return f"L{c[0]}-K{c[1]}-N{c[2]}-B{c[3]}-I{c[4]}-S{c[5]}"


def param_id(p):
    return f"{case_id(p[0])}-{p[1]}-{p[2]}"


def pitch_of(c):
    """(the descriptor's in_stride_batch, the elements between blocks): dense for one block, else 11 elements beyond what a block reaches."""
    l, k, n, blocks, inner, s = c
    if blocks == 1:
        return 0, n * s
    p = (n - 1) * s + inner + 11
    return p, p


def cube(c, seed=101):
    """[blocks][N][inner] float32: seeded noise over a line along time, column e scaled by 3^(e mod 4), block b by 5^b (a result stored under another column's or
    block's index misses the bound)."""
    l, k, n, blocks, inner, s = c
    v = np.random.default_rng(seed).standard_normal((blocks, n, inner)) + 0.01 * np.arange(n).reshape(1, n, 1) + 0.5
    return (v * (3.0 ** (np.arange(inner) % 4)).reshape(1, 1, inner) * (5.0 ** np.arange(blocks)).reshape(blocks, 1, 1)).astype(np.float32)


def as_rows(x):
    """[blocks * inner][time]: the transposed contiguous copy, the series first as the rows plan has them."""
    x = np.asarray(x)
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1))).reshape(x.shape[0] * x.shape[2], x.shape[1])


def view_of(c, x, fill=float("nan")):
    """The (blocks, N, inner) device view with strides (pitch, S, 1) of a buffer filled with `fill`; only the columns are written."""
    l, k, n, blocks, inner, s = c
    x = np.asarray(x)
    n = x.shape[1]
    pitch = pitch_of(c)[1] if blocks > 1 else n * s
    total = (blocks - 1) * pitch + (n - 1) * s + inner
    buf = torch.full((total,), fill, dtype=torch.float32, device=L.device())
    view = torch.as_strided(buf, (blocks, n, inner), (pitch, s, 1))
    view.copy_(torch.from_numpy(x).to(L.device()))
    return view


def plan_kw(c, mode, **over):
    l, k, n, blocks, inner, s = c
    kw = F.plan_kw((l, k, n, blocks), mode, inner=inner, seg_stride=s, seg_filter_cols=1, in_stride_batch=pitch_of(c)[0])
    kw.update(over)
    return kw


def narrow(l, inner):
    """At most half of the groups' columns live: the class the library declines by default (profiles/r30_fir_filter_cols.txt) and takes with XRFTHIP_MEAN_ALL=1."""
    g = GROUP[l]
    return 2 * inner <= -(-inner // g) * g


def make_plan(c, mode, taps=None, **over):
    """The column plan of the case; a narrow grid's under XRFTHIP_MEAN_ALL=1 (the variable is read when the plan is created)."""
    resp = None if taps is None else np.fft.rfft(np.asarray(taps, dtype=np.float64), c[0])
    kw = plan_kw(c, mode, phase_x=resp, **over)
    if narrow(kw["nx"], kw["inner"]):
        with B.env("XRFTHIP_MEAN_ALL", 1):
            return engine.SpectralPlan(**kw)
    return engine.SpectralPlan(**kw)


def check_narrow_grids_are_declined_by_default():
    """2 inner <= groups C answers XRFTHIP_UNSUPPORTED_LENGTH (the caller arranges) unless XRFTHIP_MEAN_ALL=1; one live column more and the plan is taken."""
    for l, g in GROUP.items():
        for inner, declined in ((1, True), (5, True), (g // 2, True), (g // 2 + 1, False), (g, False), (g + 1, False), (g + g // 2, False), (2 * g + 1, False), (3 * g, False)):
            assert narrow(l, inner) == declined, (l, inner)
            kw = dict(nx=l, seg_hop=l - 32, seg_lead=16, mean_batch=-(-700 // (l - 32)), batch=3 * -(-700 // (l - 32)), inner=inner, seg_stride=inner + 3, in_stride_batch=0)
            with B.env("XRFTHIP_MEAN_ALL", None):
                assert _status(**kw) == (L.UNSUPPORTED_LENGTH if declined else 0), (l, inner)
            with B.env("XRFTHIP_MEAN_ALL", 1):
                assert _status(**kw) == 0, (l, inner)


def rows_plan(c, mode, taps):
    l, k, n, blocks, inner, s = c
    return F.make_plan((l, k, n, blocks * inner), mode, taps)


def run(plan, view):
    out, _ = plan.execute(view)
    return out.cpu().numpy()


def assert_column_plan(plan, c):
    """The filter's plan in its column layout: the family and the lines of the rows form, and the column geometry."""
    l, k, n, blocks, inner, s = c
    F.assert_filter_plan(plan)
    d = plan.describe()
    g = GROUP[l]
    assert plan.seg_filter_cols == 1 and plan.seg_stride == s and plan.inner == inner
    assert "[fastw columns]" in d and f"a workgroup takes {g} adjacent columns ({-(-inner // g)} groups per block; {4 * g} bytes of one time row per wave-load)" in d, d
    assert f"sample stride {s}" in d and f"and {min(SPR[l], 1 << max(0, (plan.mean_batch - 1).bit_length()))} segments of each per round" in d, d


def check_plan(c, mode, kind):
    l, k, n, blocks, inner, s = c
    a, n_out = offsets(mode, n, k)
    x, taps = cube(c), taps_of(kind, k)
    view = view_of(c, x)
    plan = make_plan(c, mode, taps)
    assert_column_plan(plan, c)
    got = run(plan, view)
    assert got.shape == (blocks, n_out, inner) and got.dtype == np.float32
    rows = as_rows(x)
    assert_within(f"column plan {case_id(c)} {mode} {kind}", as_rows(got), model(rows, taps, mode), the_bound(rows, taps, l, a, n_out))
    # the rows plan on the transposed contiguous copy: the same bits
    assert np.array_equal(as_rows(got), F.run(rows_plan(c, mode, taps), rows)), "the column plan differs from the rows plan on the arranged copy"
    assert np.array_equal(got, run(plan, view))  # a second execution
    # one column cut out and run alone as inner = 1, where it lies
    b, e = blocks - 1, inner // 2
    alone = run(make_plan((l, k, n, 1, 1, s), mode, taps, in_stride_batch=0), view[b:b + 1, :, e:e + 1])
    assert np.array_equal(alone[0, :, 0], got[b, :, e]), (b, e)
    return got


def check_prefix(c, fewer, mode):
    """A record cut to N' time rows: every output whose segment's L inputs lie wholly below N' keeps its bits (fir_filter.check_prefix, per column)."""
    l, k, n, blocks, inner, s = c
    x, taps = cube(c), taps_of("normal", k)
    a, n_out = offsets(mode, n, k)
    a2, n_out2 = offsets(mode, fewer, k)
    assert a2 == a
    full = run(make_plan(c, mode, taps), view_of(c, x))
    c2 = (l, k, fewer, blocks, inner, s)
    part = run(make_plan(c2, mode, taps), view_of(c2, x[:, :fewer]))
    v = l - k + 1
    whole = (fewer - (a - (k - 1)) - l) // v + 1
    cnt = min(whole * v, n_out, n_out2)
    assert cnt > v and np.array_equal(full[:, :cnt], part[:, :cnt])


def check_nothing_outside_is_read(c, mode):
    """S > inner and a pitch beyond the block, NaN in the unseen columns and in the gap: finite, and the bits of the dense cube (S = inner, no pitch)."""
    l, k, n, blocks, inner, s = c
    assert s > inner and blocks > 1
    x, taps = cube(c), taps_of("firwin", k)
    got = run(make_plan(c, mode, taps), view_of(c, x))
    dense = (l, k, n, blocks, inner, inner)
    want = run(make_plan(dense, mode, taps, in_stride_batch=0), torch.from_numpy(x).to(L.device()))
    assert np.isfinite(got).all() and np.array_equal(got, want)


def check_containment(bad, mode, where, c=CONTAIN):
    """One non-finite sample, time row `where` of column 2 of block 1: the outputs of that column in the (at most two) segments that hold it are non-finite;
    every other output -- the other columns of the same group among them -- keeps its bits."""
    l, k, n, blocks, inner, s = c
    a, n_out = offsets(mode, n, k)
    v = l - k + 1
    m = -(-n_out // v)
    x, taps = cube(c), taps_of("normal", k)
    plan = make_plan(c, mode, taps)
    clean = run(plan, view_of(c, x))
    xb = x.copy()
    xb[1, where, 2] = bad
    got = run(plan, view_of(c, xb))
    segs = [sg for sg in range(m) if 0 <= where - (sg * v + a - (k - 1)) < l]
    assert 1 <= len(segs) <= 2, segs
    hit = np.zeros(got.shape, dtype=bool)
    for sg in segs:
        hit[1, sg * v:min((sg + 1) * v, n_out), 2] = True
    print(f"time row {where} ({mode}): segments {segs}, {int(hit.sum())} outputs")
    assert (~np.isfinite(got[hit])).all(), "an output of a segment that holds the sample is finite"
    assert np.isfinite(got[~hit]).all() and np.array_equal(got[~hit], clean[~hit])


STATUS_CASE = (256, 65, 700, 3, 40, 64)  # (40 of the 64 columns of two groups live: not a narrow grid)


def _status(**kw):
    base = plan_kw(STATUS_CASE, "same")
    base.update(kw)
    try:
        engine.SpectralPlan(**base)
    except L.XrftHipError as e:
        return e.status
    return 0


def _raw_status(cols, reserved, **over):
    """xrfthip_plan_create on a descriptor of the library's own size with the two new words as given (engine.SpectralPlan always writes reserved = 0)."""
    kw = plan_kw(STATUS_CASE, "same")
    kw.update(over)
    d = L.DescFiltCols(C.sizeof(L.DescFiltCols), 1, kw["batch"], 1, kw["nx"], L.F32, L.OUT_COMPLEX, 0, 0, kw["scale"], 0, 0, kw["inner"], 0, 0, kw["in_stride_batch"], 0, 0,
                       kw["mean_batch"], kw["seg_hop"], 0, kw["seg_stride"], 0, 0, 0, 0, 0, kw["seg_filter"], kw["seg_lead"], kw["seg_in_len"], kw["seg_out_len"], 0, 0, cols, reserved)
    h = C.c_void_p(0)
    rc = L.load().xrfthip_plan_create(C.byref(h), C.byref(d))
    if rc == 0:
        L.load().xrfthip_plan_destroy(h)
    return rc


def check_status_codes():
    big = (1 << 31) - 1
    reach = 699 * 64 + 40  # what a block reaches: (N - 1) S + inner
    assert _status() == 0 and _status(seg_stride=40) == 0 and _status(in_stride_batch=0) == 0 and _status(in_stride_batch=reach) == 0
    with B.env("XRFTHIP_MEAN_ALL", 1):  # (one column: a narrow grid.  S = 1: still the column layout)
        assert _status(inner=1, seg_stride=1, in_stride_batch=0) == 0 and _status(inner=1, seg_stride=7, in_stride_batch=0) == 0
    assert _status(seg_stride=big, in_stride_batch=0) == 0 and _status(phase_x=np.fft.rfft(taps_of("normal", 65), 256)) == 0
    for nx in (64, 128, 512):  # (K = 33)
        assert _status(nx=nx, seg_hop=nx - 32, seg_lead=16, mean_batch=-(-700 // (nx - 32)), batch=3 * -(-700 // (nx - 32))) == 0, nx
    assert _raw_status(1, 0) == 0 and _raw_status(0, 0, seg_stride=0, inner=1, in_stride_batch=0) == 0
    for cols, res in ((2, 0), (-1, 0), (1, 1), (0, 1), (1, -1)):
        assert _raw_status(cols, res) == L.BAD_ARG, (cols, res)
    assert _raw_status(0, 1, seg_stride=0, inner=1, in_stride_batch=0) == L.BAD_ARG  # (the reserved word alone, on the rows form)
    bad = [dict(seg_filter_cols=2), dict(seg_filter_cols=-1), dict(seg_filter=0, seg_lead=0, seg_in_len=0, seg_out_len=0), dict(seg_filter=0), dict(seg_stride=0),
           dict(seg_stride=39), dict(seg_stride=-9), dict(seg_stride=big + 1, in_stride_batch=0), dict(inner=big + 1, seg_stride=big + 2, in_stride_batch=0),
           dict(in_stride_batch=reach - 1), dict(seg_in_len=big + 1, in_stride_batch=0), dict(seg_out_len=big + 1, seg_in_len=big + 1, in_stride_batch=0),
           # ... and what the rows form refuses
           dict(seg_keep=1), dict(seg_synth=1), dict(seg_hop=0), dict(seg_hop=127), dict(ndim=2, ny=4), dict(mid=4), dict(dtype=torch.float64), dict(dtype=torch.float16),
           dict(out_mode=L.OUT_POWER), dict(flags=L.SHIFT_X), dict(detrend=L.DETREND_LINEAR), dict(window_x=api._window_vector("hann", 256)), dict(seg_lead=65),
           dict(seg_out_len=733), dict(mean_batch=3, batch=9), dict(batch=13)]
    for kw in bad:
        assert _status(**kw) == L.BAD_ARG, kw
    # seg_filter_cols on the other forms
    assert S._status(seg_filter_cols=1) == L.BAD_ARG and WC._status(seg_filter_cols=1) == L.BAD_ARG and B._status(seg_filter_cols=1) == L.BAD_ARG
    one = dict(nx=64, seg_hop=64, seg_lead=0, seg_in_len=64, seg_out_len=64, mean_batch=1, in_stride_batch=0)  # (K = 1, one segment: a workgroup per group of columns)
    arranges = [dict(nx=1024, seg_hop=960, mean_batch=1, batch=3), dict(nx=4096, seg_hop=4032, mean_batch=1, batch=3),
                dict(one, batch=1 << 31, inner=1, seg_stride=1), dict(one, batch=1 << 26, inner=993, seg_stride=993),  # 2^31 and 32 x 2^26 workgroups
                dict(nx=100, seg_hop=60, seg_lead=20, mean_batch=12, batch=36), dict(nx=32, seg_hop=24, seg_lead=4, mean_batch=30, batch=90)]
    with B.env("XRFTHIP_MEAN_ALL", 1):  # (so that it is the launch that declines the single column)
        for kw in arranges:
            assert _status(**kw) == L.UNSUPPORTED_LENGTH, kw
        assert _status(**dict(one, batch=big, inner=1, seg_stride=1)) == 0 and _status(**dict(one, batch=1 << 26, inner=992, seg_stride=992)) == 0  # (31 groups)
    for knob in ("XRFTHIP_FASTW", "XRFTHIP_FASTW_FILTER", "XRFTHIP_FASTW_COLS", "XRFTHIP_FASTW_FILTER_COLS"):
        with B.env(knob, 0):
            assert _status() == L.UNSUPPORTED_LENGTH, knob
    with B.env("XRFTHIP_FASTW_FILTER_COLS", 0):  # (the knob is this layout's alone)
        assert F._status() == 0 and S._status() == 0 and S._status(inner=4, seg_stride=4) == 0 and WC._status() == 0
    for knob in ("XRFTHIP_FASTW_KEEP", "XRFTHIP_FASTW_SYNTH", "XRFTHIP_FASTW_TAPERS"):
        with B.env(knob, 0):
            assert _status() == 0
    assert L.load().xrfthip_version() == 106


def check_struct_sizes():
    """Every struct_size the descriptor ever had is accepted; the two new words came together: the size between them and a larger one are XRFTHIP_BAD_ARG; a
    DescTaper-sized descriptor with garbage behind it is read without the two words."""
    dll = L.load()
    D = L.DescFiltCols
    sizes = [getattr(D, f).offset for f in ("inner", "mid", "in_stride_y", "herm_ny", "mean_batch", "seg_hop", "seg_stride", "seg_keep", "seg_synth", "seg_filter",
                                            "seg_tapers", "seg_filter_cols")] + [C.sizeof(D)]
    assert len(sizes) == 13 and sizes == sorted(set(sizes)) and sizes[-1] - sizes[-2] == 16 and sizes[-2] == C.sizeof(L.DescTaper) and sizes[-3] == C.sizeof(L.DescFilt)
    assert [f[0] for f in D._fields_[:len(L.DescTaper._fields_)]] == [f[0] for f in L.DescTaper._fields_]
    assert [f[0] for f in D._fields_[-2:]] == ["seg_filter_cols", "seg_reserved5"]
    h = C.c_void_p(0)
    zeros = (0,) * 25
    for sz in sizes:
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *zeros)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0, sz
        dll.xrfthip_plan_destroy(h)
    for sz in (sizes[-2] + 8, sizes[-1] + 8):
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *zeros)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG, sz

    def filt(sz, inner, stride, cols, res=0):  # 3 blocks (series) of 700 samples, K = 65 at L = 256, "same"
        return D(sz, 1, 12, 1, 256, L.F32, L.OUT_COMPLEX, 0, 0, 1.0 / 256, 0, 0, inner, 0, 0, 0, 0, 0, 4, 192, 0, stride, 0, 0, 0, 0, 0, 1, 32, 700, 700, 0, 0, cols, res)

    def describe(d):
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
        buf = C.create_string_buffer(8192)
        dll.xrfthip_plan_describe(h, buf, len(buf))
        dll.xrfthip_plan_destroy(h)
        return buf.value.decode()

    d = describe(filt(sizes[-1], 40, 64, 1))
    assert "[fastw overlap-save]" in d and "[fastw columns]" in d
    # the words are read only from a descriptor that has them: the older size with garbage behind it is the rows filter ...
    d = describe(filt(sizes[-2], 1, 0, 1, 7))
    assert "[fastw overlap-save]" in d and "[fastw columns]" not in d
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(filt(sizes[-1], 1, 0, 1, 7))) == L.BAD_ARG
    # ... and columns under the older size are refused as ever (seg_stride with seg_filter)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(filt(sizes[-2], 40, 64, 1))) == L.BAD_ARG
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(filt(sizes[-1], 40, 64, 0))) == L.BAD_ARG


def check_workspace(c=(64, 33, 500, 1, 33, 40), mode="same"):
    """xrfthip_workspace_bytes is 0 and the plan runs without a workspace."""
    l, k, n, blocks, inner, s = c
    taps = taps_of("normal", k)
    plan = make_plan(c, mode, taps)
    assert plan.workspace_bytes == 0
    dev = L.device()
    view = view_of(c, cube(c))
    out = torch.empty((blocks, offsets(mode, n, k)[1], inner), dtype=torch.float32, device=dev)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert L.load().xrfthip_exec(plan._h, C.c_void_p(view.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(0), C.c_void_p(0), 0, C.c_void_p(0)) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run(plan, view))


# ---------------------------------------------------------------------------------- API level (both libraries)
# name -> (shape, dims, slice of the last dim or None, K, nfft, seg_stride of the column plan | "arranged" | None (composes), dtype[, XRFTHIP_MEAN_ALL])
API_CASES = {
    "time-y-x": ((700, 3, 5), ("time", "y", "x"), None, 17, None, 15, "float32"),
    "y-time-x": ((4, 300, 5), ("y", "time", "x"), None, 9, None, "arranged", "float32"),  # 5 of a group's 16 columns: a narrow grid, declined by default ...
    "y-time-x-every-class": ((4, 300, 5), ("y", "time", "x"), None, 9, None, 5, "float32", 1),  # ... and taken with XRFTHIP_MEAN_ALL=1
    "y-time-x-wide": ((4, 300, 12), ("y", "time", "x"), None, 9, None, 12, "float32"),
    "member-time-lat-lon": ((2, 400, 6, 7), ("member", "time", "lat", "lon"), None, 31, None, 42, "float32"),
    "sliced-last-dim": ((500, 24), ("time", "x"), slice(2, 17), 17, None, 24, "float32"),  # S = 24 > inner = 15
    "does-not-collapse": ((500, 3, 12), ("time", "y", "x"), slice(2, 9), 17, None, "arranged", "float32"),  # (y, x) is no longer one unit-stride run
    "stepped-last-dim": ((3, 300, 8), ("y", "time", "x"), slice(None, None, 2), 9, None, "arranged", "float32"),  # columns two elements apart
    "k150-default-nfft": ((900, 2, 5), ("time", "y", "x"), None, 150, None, "arranged", "float32"),
    "k150-nfft-512": ((900, 2, 5), ("time", "y", "x"), None, 150, 512, 10, "float32"),
    "float64": ((300, 2, 5), ("time", "y", "x"), None, 17, None, None, "float64"),
}


def api_array(name, seed=105):
    """(the DataArray the call sees -- a view where the case slices --, its values as numpy)."""
    shape, dims, cut, k, nfft, route, dtype = API_CASES[name][:7]
    da, vals, crd = F.api_array(shape, dims, dtype, seed)
    if cut is None:
        return da, vals
    t = da.data[..., cut]
    crd = dict(crd, **{dims[-1]: crd[dims[-1]][cut]})
    return xa.DataArray(t, dims, crd, "field", {"units": "K"}), vals[..., cut]


def check_api_case(name, mode):
    with B.env("XRFTHIP_MEAN_ALL", 1 if len(API_CASES[name]) > 7 else None):
        return _check_api_case(name, mode)


def _check_api_case(name, mode):
    shape, dims, cut, k, nfft, route, dtype = API_CASES[name][:7]
    api.clear_plan_cache()
    api._MEAN_REFUSED.clear()
    da, vals = api_array(name)
    taps = taps_of("firwin", k)
    got = xa.fir_filter(da, "time", taps, mode, nfft=nfft)
    plans = F.filter_plans()
    assert bool(plans) == (route is not None), [p.describe() for p in api._plan_cache.values()]
    ax = dims.index("time")
    n = vals.shape[ax]
    l = SEG._fir_default_nfft(k, n) if nfft is None else nfft
    if route is not None:
        F.assert_filter_plan(plans[-1])
        assert plans[-1].nx == l
        if route == "arranged":
            assert plans[-1].seg_filter_cols == 0 and plans[-1].seg_stride == 0
        else:
            assert plans[-1].seg_filter_cols == 1 and plans[-1].seg_stride == route and "[fastw columns]" in plans[-1].describe(), plans[-1].describe()
            assert got.data.is_contiguous()
    a, n_out = offsets(mode, n, k)
    assert tuple(got.dims) == tuple(dims) and got.shape == tuple(n_out if d == "time" else s for d, s in zip(dims, vals.shape))
    assert np.asarray(got.values).dtype == {"float32": np.float32, "float64": np.float64}[dtype]
    x = F.series_first(vals, ax)
    ref, bnd = model(x, taps, mode), the_bound(x, taps, l, a, n_out, dtype)
    assert_within(f"fir_filter {name} {mode}", F.series_first(got.values, ax), ref, bnd)
    if route is not None:  # the knob-off call on the same build: the arranged rows, the same segments, the same arithmetic
        with B.env("XRFTHIP_FASTW_FILTER_COLS", 0):
            off = xa.fir_filter(da, "time", taps, mode, nfft=nfft)
            assert F.filter_plans()[-1].seg_filter_cols == 0
        B.compare_labelled(got, off)
        assert np.array_equal(np.asarray(got.values), np.asarray(off.values))
    return got


def check_api_other_dtypes():
    """complex data run as two real calls, half precision is widened first: both through the column plan, contiguous, within the float32 bound of their parts."""
    api.clear_plan_cache()
    da, vals, _ = F.api_array((400, 3, 5), ("time", "y", "x"), "float32", seed=106)
    taps = taps_of("firwin", 17)
    l = SEG._fir_default_nfft(17, 400)
    a, n_out = offsets("same", 400, 17)
    z = torch.complex(da.data, torch.flip(da.data, dims=(1,)))
    got = xa.fir_filter(xa.DataArray(z, da.dims, da.coords), "time", taps)
    assert F.filter_plans() and all(p.seg_filter_cols == 1 for p in F.filter_plans())
    assert np.asarray(got.values).dtype == np.complex64 and got.data.is_contiguous()
    x = F.series_first(vals, 0)
    xf = F.series_first(vals[:, ::-1], 0)
    assert_within("complex data, real part", F.series_first(np.asarray(got.values).real, 0), model(x, taps, "same"), the_bound(x, taps, l, a, n_out))
    assert_within("complex data, imaginary part", F.series_first(np.asarray(got.values).imag, 0), model(xf, taps, "same"), the_bound(xf, taps, l, a, n_out))
    half = da.data.to(torch.float16)
    gh = xa.fir_filter(xa.DataArray(half, da.dims, da.coords), "time", taps)
    xh = F.series_first(half.cpu().to(torch.float64).numpy(), 0)
    assert np.asarray(gh.values).dtype == np.float32 and gh.data.is_contiguous() and F.filter_plans()[-1].seg_filter_cols == 1
    assert_within("float16 data", F.series_first(gh.values, 0), model(xh, taps, "same"), the_bound(xh, taps, l, a, n_out))


def check_api_refusal_is_remembered():
    """XRFTHIP_FASTW=0 is a knob the API does not read: the library declines the column plan and then the rows plan, once each (XRFTHIP_UNSUPPORTED_LENGTH, remembered),
    and the second call composes without building a plan with seg_filter_cols.  float64, L beyond 512, a trailing dim and the three knobs the API reads: never asked."""
    api.clear_plan_cache()
    api._MEAN_REFUSED.clear()
    made = []
    real = engine.SpectralPlan

    class Counting(real):
        def __init__(self, *a, **kw):
            if kw.get("seg_filter_cols"):
                made.append(kw)
            super().__init__(*a, **kw)

    engine.SpectralPlan = Counting
    try:
        da, _, _ = F.api_array((700, 3, 5), ("time", "y", "x"), "float32", seed=107)
        taps = taps_of("firwin", 17)
        refused = len(api._MEAN_REFUSED)
        with B.env("XRFTHIP_FASTW", 0):
            first = xa.fir_filter(da, "time", taps)
            assert len(made) == 1 and len(api._MEAN_REFUSED) == refused + 2 and not F.filter_plans()
            second = xa.fir_filter(da, "time", taps)
            assert len(made) == 1 and np.array_equal(first.values, second.values)
        d64, _, _ = F.api_array((700, 3, 5), ("time", "y", "x"), "float64", seed=107)
        xa.fir_filter(d64, "time", taps)
        xa.fir_filter(da, "time", taps_of("firwin", 150))  # (the default nfft: 1024)
        xa.fir_filter(da, "time", taps, nfft=100)
        xa.fir_filter(xa.DataArray(da.data.movedim(0, -1).contiguous(), ("y", "x", "time")), "time", taps)
        for knob in ("XRFTHIP_FASTW_FILTER", "XRFTHIP_FASTW_COLS", "XRFTHIP_FASTW_FILTER_COLS"):
            with B.env(knob, 0):
                xa.fir_filter(da, "time", taps)
        assert len(made) == 1
        api._MEAN_REFUSED.clear()
        third = xa.fir_filter(da, "time", taps)
        assert len(made) == 2 and F.filter_plans()[-1].seg_filter_cols == 1 and third.data.is_contiguous()
    finally:
        engine.SpectralPlan = real


# ---------------------------------------------------------------------------------- extents (GPU: the buffer is allocated and never filled)
def run_huge_sample_stride(dev, c=(256, 65, 2300, 1, 32, 1 << 20), mode="same", kind="normal", beyond=1 << 31):
    """Columns whose samples lie 2^20 elements apart: the input offsets pass 2^31 elements inside ONE block.  Only the 32 live columns are written; a band of 32
    columns next to them holds NaN.  Within the bound, and the bits of the rows plan on the gathered columns."""
    import extents as E

    l, k, n, blocks, inner, s = c
    a, n_out = offsets(mode, n, k)
    total = (n - 1) * s + 2 * inner
    assert (n - 1) * s + inner > beyond and blocks == 1
    need = total * 4 + (1 << 30)
    print(f"sample stride {s}: the last sample at element {(n - 1) * s + inner - 1}, {need / 2 ** 30:.2f} GiB of device memory")
    ok, why = E.enough_memory(need, dev)
    if not ok:
        raise E.NeedsMemory(why)
    x, taps = cube(c), taps_of(kind, k)
    plan = make_plan(c, mode, taps)
    assert_column_plan(plan, c)
    try:
        buf = torch.empty(total, dtype=torch.float32, device=dev)
        torch.as_strided(buf, (n, inner), (s, 1), inner).fill_(float("nan"))
        view = torch.as_strided(buf, (1, n, inner), (n * s, s, 1))
        view.copy_(torch.from_numpy(x).to(dev))
        got = run(plan, view)
        del view, buf
        rows = as_rows(x)
        assert_within(f"column plan {case_id(c)} {mode} {kind}", as_rows(got), model(rows, taps, mode), the_bound(rows, taps, l, a, n_out))
        assert np.array_equal(as_rows(got), F.run(rows_plan(c, mode, taps), rows)), "the strided column plan differs from the rows plan on the gathered columns"
    finally:
        E.release(dev)
