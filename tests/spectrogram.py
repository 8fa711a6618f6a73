"""Shared by the tests of spectrograms (xrfthip_desc.seg_keep, csrc/fastk.h; tests/test_spectrogram_emulated.py on the emulated library, tests/test_gpu_spectrogram.py
on the MI355X): the plan-level cases, their series, the float64 reference, the bound.  Not a conftest: imported by the tests that use it.

The reference is the oracle's power_spectrum / fft of the float64 image of each segment, cut ON THE HOST (segment s of a series starts at s * hop) -- what
tests/welch.py builds before its mean.  The bound is the existing contract of ONE transform, per segment: accuracy.assert_accurate(got[p, s], ref[p, s], "float32" |
"complex64", L, kappa of that segment).  No tolerance of its own.

Every series carries its own amplitude (x 3^(p mod 4), welch.series) and every hop-long stretch of samples a further factor 1 + (i // hop) mod 3, so that
neighbouring segments differ in size and shape: a spectrum stored under the wrong series or segment index misses the bound."""
import ctypes as C

import numpy as np
import torch

from oracle import xrft_oracle as o
from xrft_amd import _lib as L
from xrft_amd import api, engine

import accuracy as A
import batch_mean as B
import welch as W
import welch_cols as WC

DIMS = ("p", "s", "t")
FORMS = ["plain", "linear-hann-shift"]
MODES = [L.OUT_POWER, L.OUT_COMPLEX]
# (L, hop, M, P): the smallest and the largest length; hops L, L / 2, 37 (unaligned starts) and 1; 130 segments of 64 samples (128 fill a round: a second, almost
# empty round), 33 of 256 (32 fill a round); 300 series (more than the CUs); one segment
CASES = [(64, 64, 2, 1), (64, 32, 3, 3), (64, 37, 130, 1), (64, 1, 5, 3), (256, 128, 3, 300), (256, 37, 33, 3), (1024, 512, 5, 2), (4096, 2048, 3, 2), (256, 128, 1, 2)]
EXTRA_CASES = [CASES[1], CASES[4]]  # ... also with a constant detrend and the half outputs
# (L, hop, M, blocks, inner, S, -, -, floats added to the dense block pitch): the tuples of tests/welch_cols.py.  One column more than a group in a box of a wider grid
# with a block pitch; a full group; 16 columns per group and one more
COL_CASES = [(64, 32, 3, 1, 5, 5, 0, None, 0), (64, 37, 9, 2, 33, 40, 0, None, 5), (256, 128, 3, 1, 32, 32, 0, None, 0), (512, 256, 3, 2, 17, 17, 0, None, 0)]
GROUP = {64: 32, 128: 32, 256: 32, 512: 16}  # columns per workgroup (fastk.h: min(32, 8192 / L))
CONTAIN = (256, 128, 5, 3)
CONTAIN_COLS = (256, 128, 5, 1, 3, 3, 0, None, 0)


def case_id(c):
    return f"L{c[0]}-H{c[1]}-M{c[2]}-P{c[3]}" + (f"-in{c[4]}-S{c[5]}" if len(c) > 4 else "")


def mode_id(m):
    return "power" if m == L.OUT_POWER else "complex"


def envelope(n, hop):
    return 1.0 + (np.arange(n) // hop) % 3


def series(case, seed=71, pitch=None):
    """[P][pitch] float32: welch.series (series p scaled by 3^(p mod 4)) under the envelope."""
    x = W.series(case + (0, None), seed, pitch)
    return (x * envelope(x.shape[1], case[1])).astype(np.float32)


def cube(c, seed=73):
    """[blocks][span][inner] float32: welch_cols.cube (column e scaled by 3^(e mod 4), block p by 5^p) under the envelope along time."""
    x = WC.cube(c, seed)
    return (x * envelope(x.shape[1], c[1]).reshape(1, -1, 1)).astype(np.float32)


def make_plan(case, form="plain", mode=L.OUT_POWER, pitch=0, **over):
    l, h, m, p = case[:4]
    pkw = dict(W.form_kw(form)[0])
    win = pkw.pop("window", None)
    kw = dict(ndim=1, batch=p * m, ny=1, nx=l, dtype=torch.float32, out_mode=mode, scale=1.0, mean_batch=m, seg_hop=h, seg_keep=1, in_stride_batch=pitch, **pkw)
    if win:
        kw["window_x"] = api._window_vector(win, l)
    kw.update(over)
    return engine.SpectralPlan(**kw)


def make_col_plan(c, form="plain", mode=L.OUT_POWER, **over):
    return make_plan(c[:4], form, mode, pitch=WC.pitch_of(c)[0], **dict(dict(inner=c[4], seg_stride=c[5]), **over))


def run(plan, x):
    out, _ = plan.execute(torch.from_numpy(np.ascontiguousarray(x)).to(L.device()))
    return out.cpu().numpy()


def run_cols(plan, c, x):
    """(blocks * inner, M, nx_out): the column plan's [block][segment][frequency][column] result with the series first, as the rows plan has them."""
    out, _ = plan.execute(WC.view_of(c, x))
    assert tuple(out.shape) == (c[3], c[2], plan.nx_out, c[4]), out.shape
    return np.ascontiguousarray(np.transpose(out.cpu().numpy(), (0, 3, 1, 2))).reshape(c[3] * c[4], c[2], plan.nx_out)


def half_flags(form, half):
    return (W.form_kw(form)[0]["flags"] & ~L.SHIFT_X) | L.HALF_X | (L.REALDIM_X2 if half == 2 else 0)


def reference(case, form, x, mode, half=0):
    """[P][M][nx_out] float64 / complex128: the oracle's spectrum of every host-cut segment.  half: 1 = k = 0 .. L / 2 of the unshifted spectrum (XRFTHIP_HALF_X),
    2 = the oracle's real_dim (HALF_X | REALDIM_X2, POWER)."""
    l, h, m, p = case[:4]
    okw = dict(W.form_kw(form)[1])
    if half:
        okw["shift"] = False
    crd = {"p": np.arange(p), "s": np.arange(m), "t": np.arange(l) * 1.0}
    a = o.OArr(W.segments(x, case), DIMS, crd)
    if mode == L.OUT_POWER:
        ref = o.power_spectrum(a, dim=["t"], scaling="false_density", real_dim="t" if half == 2 else None, **okw).values
    else:
        ref = o.fft(a, dim=["t"], true_phase=False, true_amplitude=False, **okw).values
    return ref[..., :l // 2 + 1] if half == 1 else ref


def kappas(case, form, x):
    """[P][M]: max |x| / rms(x - fit) of every segment (0 without a detrend)."""
    kind = W.form_kw(form)[0]["detrend"]
    segs = W.segments(x, case)
    if kind == L.DETREND_NONE:
        return np.zeros(segs.shape[:2])
    return np.array([[A.kappa(s[None], A.detrended(s[None], (1,), kind)) for s in ser] for ser in segs])


def assert_segments(case, got, ref, kaps, mode, what):
    """Every (series, segment) within the bound of one transform, each against its own reference; prints the worst figure before it asserts."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    dt = "float32" if mode == L.OUT_POWER else "complex64"
    assert np.isfinite(got).all(), what
    worst = (0.0, None)
    for p in range(ref.shape[0]):
        for s in range(ref.shape[1]):
            e = A.errors(got[p, s], ref[p, s])[0] / A.bound(dt, case[0], kaps[p, s])
            worst = max(worst, (e, (p, s)))
    print(f"{what}: worst error / bound {worst[0]:.3f} at (series, segment) {worst[1]}")
    for p in range(ref.shape[0]):
        for s in range(ref.shape[1]):
            A.assert_accurate(got[p, s], ref[p, s], dt, case[0], kaps[p, s], what=f"{what} series {p} segment {s}")


def assert_keep_plan(plan, cols=None):
    d = plan.describe()
    assert plan.kernel_info()[0] == L.K_FASTW and "[fastw segments kept]" in d and "[mean over the batch]" not in d and "[fastw]" not in d, d
    assert plan.workspace_bytes == 0
    if cols is not None:
        assert "[fastw columns]" in d and f"of {cols[4]} adjacent columns, sample stride {cols[5]} " in d and f"takes {GROUP[cols[0]]} adjacent columns" in d, d


def check_plan(case, form, mode, half=0):
    l, h, m, p = case
    x = series(case)
    over = {"flags": half_flags(form, half)} if half else {}
    plan = make_plan(case, form, mode, **over)
    assert_keep_plan(plan)
    got = run(plan, x)
    nxo = l // 2 + 1 if half else l
    assert got.shape == (p, m, nxo) and got.dtype == (np.float32 if mode == L.OUT_POWER else np.complex64)
    assert_segments(case, got, reference(case, form, x, mode, half), kappas(case, form, x), mode, f"{mode_id(mode)} {case_id(case)} {form} half={half}")
    assert np.array_equal(got, run(plan, x), equal_nan=True)  # a second execution: the same bits
    return plan, got


def check_col_plan(c, form, mode, half=0):
    l, h, m, p, inner = c[:5]
    rc = (l, h, m, p * inner)
    x = cube(c)
    over = {"flags": half_flags(form, half)} if half else {}
    plan = make_col_plan(c, form, mode, **over)
    assert_keep_plan(plan, c)
    got = run_cols(plan, c, x)  # (the gap between inner and S and the space behind the span hold NaN: welch_cols.view_of)
    rows = WC.as_rows(x)
    assert_segments(rc, got, reference(rc, form, rows, mode, half), kappas(rc, form, rows), mode, f"columns {mode_id(mode)} {case_id(c)} {form} half={half}")
    assert np.array_equal(got, run_cols(plan, c, x))
    # ... and the rows plan on the arranged series writes the same bits: one kernel, two loaders
    assert np.array_equal(got, run(make_plan(rc, form, mode, **over), rows))


def check_ishift_changes_no_bit(case):
    x = series(case)
    fl = W.form_kw("linear-hann-shift")[0]["flags"]
    a = run(make_plan(case, "linear-hann-shift"), x)
    b = run(make_plan(case, "linear-hann-shift", flags=fl | L.ISHIFT_X), x)
    assert np.array_equal(a, b)


def check_pitch_and_padding(case, mode, form="linear-hann-shift"):
    """A pitch larger than the span (odd: the series start on 4-byte boundaries only), the samples beyond the span NaN; then a pointer aligned to 4 bytes only: the
    bits of the dense call."""
    sp = W.span(case)
    pitch = sp + 5
    x = series(case, pitch=pitch)
    dense = np.ascontiguousarray(x[:, :sp])
    x[:, sp:] = np.nan
    want = run(make_plan(case, form, mode), dense)
    got = run(make_plan(case, form, mode, pitch=pitch), x)
    assert np.isfinite(got).all() and np.array_equal(got, want)
    buf = torch.full((case[3] * pitch + 1,), float("nan"), dtype=torch.float32, device=L.device())
    view = buf[1:].reshape(case[3], pitch)
    view[:, :sp] = torch.from_numpy(dense).to(L.device())
    assert view.data_ptr() % 16 == 4
    out, _ = make_plan(case, form, mode, pitch=pitch).execute(view)
    assert np.array_equal(out.cpu().numpy(), want)


def check_no_overlap_is_the_plain_plan(case, form, mode):
    """hop = L: both within the bound against the oracle, and the two within twice the bound of each other, per segment."""
    l, h, m, p = case
    assert h == l
    x = series(case)
    got = run(make_plan(case, form, mode), x)
    pkw = dict(W.form_kw(form)[0])
    win = pkw.pop("window", None)
    plain = engine.SpectralPlan(ndim=1, batch=p * m, ny=1, nx=l, dtype=torch.float32, out_mode=mode, scale=1.0, window_x=api._window_vector(win, l) if win else None, **pkw)
    comp = plain.execute(torch.from_numpy(x.reshape(p * m, l)).to(L.device()))[0].cpu().numpy().reshape(p, m, l)
    ref, kaps = reference(case, form, x, mode), kappas(case, form, x)
    dt = "float32" if mode == L.OUT_POWER else "complex64"
    for k in range(p):
        for s in range(m):
            bnd = A.bound(dt, l, kaps[k, s])
            e1, e2, e12 = A.errors(got[k, s], ref[k, s])[0], A.errors(comp[k, s], ref[k, s])[0], A.errors(got[k, s], comp[k, s])[0]
            print(f"no overlap {case_id(case)} {form} {mode_id(mode)} ({k}, {s}): kept {e1:.3e} plain {e2:.3e} bound {bnd:.3e}; against each other {e12:.3e}")
            assert e1 <= bnd and e2 <= bnd and e12 <= 2 * bnd


def _nonfinite(v):
    return ~np.isfinite(v)  # (a complex element: either part)


def check_containment(mode, form, bad):
    """A non-finite sample at sample 300 of series 1 (L = 256, hop = 128, M = 5): exactly segments 1 and 2 of series 1 are non-finite in every element, every other
    (series, segment) keeps the bits of the clean run -- the check a kernel that packs neighbouring segments into one transform fails."""
    case = CONTAIN
    x = series(case)
    plan = make_plan(case, form, mode)
    clean = run(plan, x)
    xb = x.copy()
    xb[1, 300] = bad
    got = run(plan, xb)
    hit = np.zeros(got.shape[:2], dtype=bool)
    hit[1, 1] = hit[1, 2] = True
    assert _nonfinite(got[hit]).all(), "a segment that holds the sample has finite elements"
    assert np.isfinite(got[~hit]).all() and np.array_equal(got[~hit], clean[~hit])


def check_containment_cols(mode, form, bad):
    c = CONTAIN_COLS
    x = cube(c)
    plan = make_col_plan(c, form, mode)
    clean = run_cols(plan, c, x)
    xb = x.copy()
    xb[0, 300, 1] = bad
    got = run_cols(plan, c, xb)
    hit = np.zeros(got.shape[:2], dtype=bool)
    hit[1, 1] = hit[1, 2] = True
    assert _nonfinite(got[hit]).all()
    assert np.isfinite(got[~hit]).all() and np.array_equal(got[~hit], clean[~hit])


def _status(**kw):
    base = dict(ndim=1, batch=6, ny=1, nx=256, dtype=torch.float32, out_mode=L.OUT_POWER, mean_batch=3, seg_hop=128, seg_keep=1)
    base.update(kw)
    try:
        engine.SpectralPlan(**base)
    except L.XrftHipError as e:
        return e.status
    return 0


def check_status_codes():
    assert _status() == 0 and _status(out_mode=L.OUT_COMPLEX) == 0 and _status(seg_hop=1) == 0 and _status(seg_hop=256) == 0
    assert _status(mean_batch=1, batch=2) == 0 and _status(mean_batch=1, batch=2, out_mode=L.OUT_COMPLEX) == 0  # (one segment)
    for fl in (L.SHIFT_X, L.HALF_X, L.HALF_X | L.REALDIM_X2, L.ISHIFT_X, L.SHIFT_X | L.ISHIFT_X):
        assert _status(flags=fl) == 0, fl
    for fl in (L.SHIFT_X, L.HALF_X):
        assert _status(flags=fl, out_mode=L.OUT_COMPLEX) == 0, fl
    for det in (L.DETREND_NONE, L.DETREND_CONSTANT, L.DETREND_LINEAR):
        assert _status(detrend=det) == 0 and _status(detrend=det, out_mode=L.OUT_COMPLEX) == 0
    assert _status(inner=3, seg_stride=3, in_stride_batch=0) == 0 and _status(inner=3, seg_stride=7, out_mode=L.OUT_COMPLEX) == 0
    bad = [dict(seg_keep=2), dict(seg_keep=-1), dict(seg_hop=0), dict(seg_hop=0, mean_batch=0), dict(out_mode=L.OUT_CROSS), dict(out_mode=L.OUT_PHASE),
           dict(out_mode=L.OUT_COHERENCE), dict(out_mode=L.OUT_COMPLEX, flags=L.HALF_X | L.REALDIM_X2), dict(flags=L.REALDIM_X2),
           # ... and what seg_hop / seg_stride refuse
           dict(seg_hop=-1), dict(seg_hop=257), dict(ndim=2, ny=4), dict(inner=4), dict(mid=4), dict(herm_ny=4, herm_nx=4), dict(flags=L.ISO), dict(in_stride_y=512),
           dict(mean_batch=0), dict(batch=7), dict(in_stride_batch=2 * 128 + 255), dict(flags=L.HALF_X | L.SHIFT_X), dict(seg_stride=-1), dict(inner=4, seg_stride=3),
           dict(inner=3, seg_stride=3, in_stride_batch=(2 * 128 + 255) * 3 + 2)]
    for kw in bad:
        assert _status(**kw) == L.BAD_ARG, kw
    composes = [dict(nx=96, seg_hop=48), dict(nx=32, seg_hop=16), dict(nx=8192, seg_hop=4096), dict(nx=1024, seg_hop=512, inner=3, seg_stride=3), dict(dtype=torch.float64),
                dict(dtype=torch.complex64, out_mode=L.OUT_COMPLEX), dict(dtype=torch.float16), dict(dtype=torch.bfloat16), dict(flags=L.FLIP_X),
                dict(out_mode=L.OUT_COMPLEX, flags=L.ISHIFT_X), dict(out_mode=L.OUT_COMPLEX, phase_x=np.exp(-2j * np.pi * np.fft.fftfreq(256) * 3.0))]
    for kw in composes:
        assert _status(**kw) == L.UNSUPPORTED_LENGTH, kw
    assert _status(nx=512, seg_hop=256, inner=3, seg_stride=3) == 0
    for knob in ("XRFTHIP_FASTW", "XRFTHIP_FASTW_KEEP"):
        with B.env(knob, 0):
            assert _status() == L.UNSUPPORTED_LENGTH, knob
    with B.env("XRFTHIP_FASTW_COLS", 0):
        assert _status(inner=3, seg_stride=3) == L.UNSUPPORTED_LENGTH and _status() == 0
    with B.env("XRFTHIP_FASTW_KEEP", 0):  # (the knob is this form's alone)
        assert _status(seg_keep=0) == 0
    # the class that measured slower than its composition (L = 4096 without overlap, profiles/r21_spectrogram.txt) composes by default
    assert _status(nx=4096, seg_hop=4096) == L.UNSUPPORTED_LENGTH and _status(nx=4096, seg_hop=2048) == 0 and _status(nx=2048, seg_hop=2048) == 0
    with B.env("XRFTHIP_MEAN_ALL", 1):
        assert _status(nx=4096, seg_hop=4096) == 0
    # seg_keep = 0: everything as before
    assert _status(seg_keep=0) == 0 and _status(seg_keep=0, out_mode=L.OUT_CROSS) == 0
    assert _status(seg_keep=0, mean_batch=1, batch=2) == L.BAD_ARG and _status(seg_keep=0, out_mode=L.OUT_COMPLEX) == L.BAD_ARG


def check_struct_sizes():
    """The nine struct_size values are accepted (the words a shorter one lacks count as 0); seg_keep and seg_reserved3 came together: the size between the two, a
    larger one and a non-zero reserved word are XRFTHIP_BAD_ARG; a DescCols-sized descriptor with garbage behind it is the Welch plan."""
    dll = L.load()
    D = L.DescKeep
    sizes = [getattr(D, f).offset for f in ("inner", "mid", "in_stride_y", "herm_ny", "mean_batch", "seg_hop", "seg_stride", "seg_keep")] + [C.sizeof(D)]
    assert sizes == sorted(set(sizes)) and len(sizes) == 9 and sizes[-1] - sizes[-2] == 16 and sizes[-2] == C.sizeof(L.DescCols) and sizes[-3] == C.sizeof(L.DescSeg)
    h = C.c_void_p(0)
    for sz in sizes:
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0, sz
        dll.xrfthip_plan_destroy(h)
    for sz in (sizes[-2] + 8, sizes[-1] + 8):
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG, sz

    def seg(sz, keep, res3):
        return D(sz, 1, 6, 1, 256, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 128, 0, 0, 0, keep, res3)

    def describe(d):
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
        buf = C.create_string_buffer(8192)
        dll.xrfthip_plan_describe(h, buf, len(buf))
        dll.xrfthip_plan_destroy(h)
        return buf.value.decode()

    assert "[fastw segments kept]" in describe(seg(sizes[-1], 1, 0))
    # the words are read only from a descriptor that has them: the older size with garbage behind it is the Welch plan
    text = describe(seg(sizes[-2], 1, 77))
    assert "[fastw]" in text and "[mean over the batch]" in text and "segments kept" not in text
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(seg(sizes[-1], 1, 1))) == L.BAD_ARG
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(seg(sizes[-1], 0, 1))) == L.BAD_ARG


def check_workspace(case=CASES[1]):
    """xrfthip_workspace_bytes is 0 and the plan runs without a workspace."""
    l, h, m, p = case
    plan = make_plan(case, "linear-hann-shift")
    assert plan.workspace_bytes == 0
    dev = L.device()
    x = torch.from_numpy(series(case)).to(dev)
    out = torch.empty((p, m, l), dtype=torch.float32, device=dev)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert L.load().xrfthip_exec(plan._h, C.c_void_p(x.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(0), C.c_void_p(0), 0, C.c_void_p(0)) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run(plan, series(case)))


# ---------------------------------------------------------------------------------- API level (both libraries)
import xrft_amd as xa  # noqa: E402


def composed(da, dim, nperseg, hop, complex_, **kw):
    """The expression the functions stand for: the segments unfolded, the public call along their samples, the dims moved so that (<dim>_segment, freq_<dim>) lie
    where ``dim`` lay, and the <dim>_segment coordinate -- the middle of each segment's samples."""
    seg = api._welch_segments(da, dim, nperseg, hop)
    full = xa.fft(seg, dim=[dim], true_phase=False, **dict(dict(true_amplitude=False), **kw)) if complex_ else xa.power_spectrum(seg, dim=[dim], **kw)
    sname, fname = dim + "_segment", "freq_" + dim
    final = [x for d in da.dims for x in ((sname, fname) if d == dim else (d,))]
    full = full.transpose(*final)
    t = np.asarray(da[dim].values)
    m = (len(t) - nperseg) // hop + 1
    mid = np.array([t[s * hop] + (t[s * hop + nperseg - 1] - t[s * hop]) / 2 for s in range(m)])
    coords = dict(full.coords)
    coords[sname] = xa.Coordinate((sname,), mid, None, sname)
    return xa.DataArray(full.data, final, coords, full.name, full.attrs)


def oracle_segments(wide, crd, dims, dim, nperseg, hop, complex_, **kw):
    """(the oracle's spectrum of every host-cut float64 segment, the segments): [series][M][nx_out] and [series][M][nperseg], the series in the order of the other dims."""
    ax = dims.index(dim)
    m = (wide.shape[ax] - nperseg) // hop + 1
    w = np.moveaxis(wide, ax, -1)
    segs = np.stack([w[..., s * hop:s * hop + nperseg] for s in range(m)], axis=-2)
    a = o.OArr(segs, [d for d in dims if d != dim] + ["seg", dim], {dim: crd[dim][:nperseg]})
    if complex_:
        full = o.fft(a, dim=[dim], true_phase=False, **dict(dict(true_amplitude=False), **kw)).values
    else:
        full = o.power_spectrum(a, dim=[dim], **kw).values
    return full.reshape(-1, m, full.shape[-1]), segs.reshape(-1, m, nperseg)


def series_first(values, ax):
    """[series][M][nx_out] of a result whose (<dim>_segment, freq_<dim>) lie at axes (ax, ax + 1)."""
    v = np.moveaxis(np.asarray(values), (ax, ax + 1), (-2, -1))
    return v.reshape(-1, v.shape[-2], v.shape[-1])


def assert_api_accurate(what, got, wide, crd, dims, nperseg, hop, complex_, kw, dtype="float32"):
    ref, segs = oracle_segments(wide, crd, list(dims), "time", nperseg, hop, complex_, **kw)
    g = series_first(got.values, list(dims).index("time"))
    assert g.shape == ref.shape, (g.shape, ref.shape)
    det = kw.get("detrend")
    kind = L.DETREND_LINEAR if det == "linear" else L.DETREND_CONSTANT
    dt = {"float32": "complex64", "float64": "complex128"}[dtype] if complex_ else dtype
    worst = 0.0
    for p in range(ref.shape[0]):
        for s in range(ref.shape[1]):
            kap = A.kappa(segs[p, s][None], A.detrended(segs[p, s][None], (1,), kind)) if det else 0.0
            worst = max(worst, A.errors(g[p, s], ref[p, s])[0] / A.bound(dt, nperseg, kap))
            A.assert_accurate(g[p, s], ref[p, s], dt, nperseg, kap, what=f"{what} series {p} segment {s}")
    print(f"{what}: worst error / bound {worst:.3f}")


def keep_plans():
    return [p for p in api._plan_cache.values() if getattr(p, "seg_keep", 0)]


LINHANN = dict(detrend="linear", window="hann", window_correction=True)
# name -> (shape, dims, slices of the array or None, nperseg, noverlap, keyword arguments, "rows" | "columns" (the fused form) | None (composes), dtype, stft?)
API_CASES = {
    "trailing-64-half-overlap": ((3, 1000), ("x", "time"), None, 64, 32, LINHANN, "rows", "float32", False),
    "trailing-64-noverlap-27": ((3, 1000), ("x", "time"), None, 64, 27, dict(detrend="constant", window="hann"), "rows", "float32", False),
    "trailing-256-real-dim": ((3, 1000), ("x", "time"), None, 256, None, dict(LINHANN, real_dim="time"), "rows", "float32", False),
    "trailing-sliced": ((3, 1000), ("x", "time"), (slice(None), slice(100, 900)), 64, None, LINHANN, "rows", "float32", False),
    "leading-time": ((600, 4, 5), ("time", "y", "x"), None, 64, None, LINHANN, "columns", "float32", False),
    "middle-time": ((2, 600, 7), ("e", "time", "x"), None, 64, None, dict(detrend="constant"), "columns", "float32", False),
    "leading-time-sliced": ((600, 8), ("time", "x"), (slice(None), slice(1, 6)), 64, None, LINHANN, "columns", "float32", False),
    "stft-trailing": ((3, 1000), ("x", "time"), None, 64, None, dict(detrend="linear", window="hann"), "rows", "float32", True),
    "stft-true-amplitude-real-dim": ((3, 1000), ("x", "time"), None, 256, 100, dict(window="hann", true_amplitude=True, real_dim="time"), "rows", "float32", True),
    "stft-leading-time": ((600, 4, 5), ("time", "y", "x"), None, 64, None, dict(detrend="linear", window="hann", shift=False), "columns", "float32", True),
    "float64": ((3, 600), ("x", "time"), None, 128, None, LINHANN, None, "float64", False),
    "length-100": ((3, 500), ("x", "time"), None, 100, None, LINHANN, None, "float32", False),
    "stft-length-100": ((3, 500), ("x", "time"), None, 100, None, dict(detrend="linear"), None, "float32", True),
}


def check_api_case(name):
    shape, dims, isel, nperseg, noverlap, kw, form, dtype, complex_ = API_CASES[name]
    api.clear_plan_cache()
    da, wide, crd = W.api_series(shape, dims, dtype, seed=81)
    if isel is not None:
        da = xa.DataArray(da.data[isel], dims, {d: crd[d][s] for d, s in zip(dims, isel)})
        wide, crd = wide[isel], {d: crd[d][s] for d, s in zip(dims, isel)}
        assert not da.data.is_contiguous()
    hop = nperseg - (nperseg // 2 if noverlap is None else noverlap)
    fn = xa.stft if complex_ else xa.spectrogram
    got = fn(da, "time", nperseg, noverlap, **kw)
    if form is None:
        assert not keep_plans() and L.K_FASTW not in [p.kernel_info()[0] for p in api._plan_cache.values()]
    else:
        d = B.newest_plan().describe()
        assert B.newest_plan().kernel_info()[0] == L.K_FASTW and "[fastw segments kept]" in d, d
        assert ("[fastw columns]" in d and "read where they lie" in d and "no transposed copy" in d) == (form == "columns"), d
    want = composed(da, "time", nperseg, hop, complex_, **kw)
    B.compare_labelled(got, want)
    ax = dims.index("time")
    m = (da.shape[ax] - nperseg) // hop + 1
    assert tuple(got.dims) == tuple(dims[:ax]) + ("time_segment", "freq_time") + tuple(dims[ax + 1:])
    assert got.shape[ax] == m and got.shape[ax + 1] == (nperseg // 2 + 1 if kw.get("real_dim") else nperseg)
    t = np.asarray(crd["time"])
    assert np.array_equal(got["time_segment"].values, [t[s * hop] + (t[s * hop + nperseg - 1] - t[s * hop]) / 2 for s in range(m)])
    if form is None:
        assert np.array_equal(got.values, want.values)
    assert_api_accurate(f"{fn.__name__} {name}", got, wide, crd, dims, nperseg, hop, complex_, kw, dtype)
    return da, got


def check_api_refusal_is_remembered():
    """nperseg = 100: the library declines once (XRFTHIP_UNSUPPORTED_LENGTH); the second call composes without building a plan with seg_keep.  float64: never asked."""
    api.clear_plan_cache()
    api._MEAN_REFUSED.clear()
    made = []
    real = engine.SpectralPlan

    class Counting(real):
        def __init__(self, *a, **kw):
            if kw.get("seg_keep"):
                made.append(kw)
            super().__init__(*a, **kw)

    engine.SpectralPlan = Counting
    try:
        da, _, _ = W.api_series((3, 500), ("x", "time"), "float32", seed=82)
        first = xa.spectrogram(da, "time", 100, **LINHANN)
        assert len(made) == 1 and len(api._MEAN_REFUSED) == 1 and not keep_plans()
        second = xa.spectrogram(da, "time", 100, **LINHANN)
        assert len(made) == 1 and np.array_equal(first.values, second.values)
        d64, _, _ = W.api_series((3, 500), ("x", "time"), "float64", seed=82)
        xa.spectrogram(d64, "time", 128, **LINHANN)
        assert len(made) == 1
        with B.env("XRFTHIP_FASTW_KEEP", 0):  # (the knob: the composed route on a call the plan would take, the same labels)
            off = xa.spectrogram(da, "time", 128, **LINHANN)
        assert len(made) == 1
        on = xa.spectrogram(da, "time", 128, **LINHANN)
        assert len(made) == 2 and keep_plans()
        B.compare_labelled(on, off)
    finally:
        engine.SpectralPlan = real


def check_api_labels():
    """Dims order, kept coordinates, and the <dim>_segment coordinate of a datetime64 axis."""
    api.clear_plan_cache()
    n = 300
    rng = np.random.default_rng(83)
    t = np.datetime64("2001-01-01T00:00") + np.arange(n) * np.timedelta64(30, "m")
    crd = {"time": t, "y": np.arange(4) * 2.0, "x": np.arange(5) * 0.5}
    da = xa.DataArray(torch.from_numpy(rng.standard_normal((n, 4, 5)).astype(np.float32)).to(L.device()), ("time", "y", "x"), crd)
    got = xa.spectrogram(da, "time", 64, 16, window="hann")
    m = (n - 64) // 48 + 1
    assert got.dims == ("time_segment", "freq_time", "y", "x") and got.shape == (m, 64, 4, 5)
    assert np.array_equal(got["y"].values, crd["y"]) and np.array_equal(got["x"].values, crd["x"])
    mid = got["time_segment"].values
    assert mid.dtype.kind == "M" and np.array_equal(mid, np.array([t[s * 48] + (t[s * 48 + 63] - t[s * 48]) / 2 for s in range(m)]))
    B.compare_labelled(got, composed(da, "time", 64, 48, False, window="hann"))
    one = xa.stft(da, "time", n, window="hann")  # (one segment is a spectrum)
    assert one.dims == ("time_segment", "freq_time", "y", "x") and one.shape == (1, n, 4, 5)


def check_api_errors():
    import pytest

    da, _, _ = W.api_series((3, 300), ("x", "time"), "float32", seed=84)
    for fn in (xa.spectrogram, xa.stft):
        for kw in (dict(nperseg=301), dict(nperseg=0), dict(nperseg=64, noverlap=64), dict(nperseg=64, noverlap=-1)):
            with pytest.raises(ValueError):
                fn(da, "time", **kw)
        with pytest.raises(ValueError):
            fn(da, ["time"], 64)
        with pytest.raises(ValueError):
            fn(da, "nope", 64)
        with pytest.raises(ValueError):
            fn(da, "time", 64, real_dim="x")
        # a linear detrend refuses non-finite samples (scipy.signal.detrend's refusal, as the composed call) -- in any segment, not beyond the last one
        v = da.data.clone()
        v[1, 299] = float("nan")
        dn = xa.DataArray(v, da.dims, da.coords)
        assert np.isfinite(fn(dn, "time", 64, detrend="linear").values).all()  # (sample 299 fills no segment)
        v[1, 200] = float("inf")
        for route in (dn, xa.DataArray(v.to(torch.float64), da.dims, da.coords)):
            with pytest.raises(ValueError):
                fn(route, "time", 64, detrend="linear")
        assert not np.isfinite(fn(dn, "time", 64).values).all()  # (no detrend: the sample goes through, into its own segments)
    with pytest.raises(TypeError):
        xa.stft(da, "time", 64, true_phase=True)
