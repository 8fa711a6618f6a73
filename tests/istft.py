"""Shared by the tests of the synthesis (xrfthip_desc.seg_synth, csrc/fasto.h, xrft_amd.istft; tests/test_istft_emulated.py on the emulated library,
tests/test_gpu_istft.py on the MI355X): the model, the bound, the plan-level cases and the API-level checks.  Not a conftest: imported by the tests that use it.

The model is plain numpy in float64, per series: numpy.fft.irfft (numpy.fft.ifft of a two-sided spectrum) of each segment's values cast exactly to complex128, times
`scale`, times the window w, overlap-added at s * hop, divided by D[n] = sum_s w^2[n - s hop] where D > 1e-10.  test_the_model_is_the_inverse shows that it inverts
the float64 analysis.

The bound has no constant of its own.  With b = accuracy.bound(dtype, L) (the contract of ONE transform, norm-wise), u the unit roundoff, D' = D where D > 1e-10
else 1, R = ceil(L / hop) and A^2 = sum over series and segments of ||x_s||^2 (the model's unwindowed inverse segments):

    || (got - ref) D' ||_2  <=  sqrt(R) (b + (R + 2) u) A

-- each inverse segment is within b of the model's norm-wise; at most R of them meet in a sample (Cauchy-Schwarz) and |w| <= 1; R + 2 roundings come from the
products, the adds and the division."""
import ctypes as C

import numpy as np
import torch

from xrft_amd import _lib as L
from xrft_amd import api, engine

import accuracy as A
import batch_mean as B
import spectrogram as S
import welch as W

FLAGS = L.INVERSE | L.C2R_X
WINDOWS = [None, "hann"]
# (L, hop, M, P), each the smallest shape that reaches its hazard: R = 1; basic overlap; an unaligned hop and two workgroups per series; R = 64, the admitted extreme
# (F = 65); R = 4 and two workgroups; more series than CUs; F = 7; NS = 2, F = 1 (every owned range fed by two tiles); one segment
CASES = [(64, 64, 2, 1), (64, 32, 3, 3), (64, 37, 130, 1), (64, 1, 70, 2), (256, 64, 40, 3), (256, 128, 3, 300), (1024, 512, 9, 2), (4096, 2048, 4, 2), (256, 128, 1, 2)]
PREFIX_CASES = [((64, 37, 130, 1), 100), ((4096, 2048, 4, 2), 3)]  # the first (M' - R + 1) hop samples of an M-segment run are those of the M'-segment run
CONTAIN = (256, 128, 5, 3)
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}


def win_id(w):
    return w or "boxcar"


def window(name, l):
    return np.ones(l) if name is None else np.asarray(api._window_vector(name, l), dtype=np.float64)


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------- the model and the bound
def envelope(w, hop, m):
    """D[n] = sum_s w^2[n - s hop], float64."""
    l = len(w)
    d = np.zeros((m - 1) * hop + l)
    for s in range(m):
        d[s * hop:s * hop + l] += w ** 2
    return d


def inverse_segments(spec, l, scale, two_sided=False):
    """[P][M][L] float64 (complex128: two_sided): the unwindowed inverse transform of every segment, times scale.  numpy's irfft / ifft divide by L: undone, the
    library's inverse is unnormalised and `scale` carries the 1 / L."""
    z = np.asarray(spec).astype(np.complex128)
    return (np.fft.ifft(z, n=l, axis=-1) if two_sided else np.fft.irfft(z, n=l, axis=-1)) * (l * scale)


def overlap_add(segs, w, hop):
    """[P][span]: the segments times w, added at s * hop, in float64."""
    p, m, l = segs.shape
    out = np.zeros((p, (m - 1) * hop + l), dtype=segs.dtype)
    for s in range(m):
        out[:, s * hop:s * hop + l] += segs[:, s] * w
    return out


def model(spec, l, hop, w, scale, two_sided=False):
    """(ref [P][span], D' [span], A): the model, the divisor with 1 where D <= 1e-10, the norm of the unwindowed inverse segments."""
    segs = inverse_segments(spec, l, scale, two_sided)
    d = envelope(w, hop, segs.shape[1])
    dp = np.where(d > 1e-10, d, 1.0)
    return overlap_add(segs, w, hop) / dp, dp, float(np.sqrt(np.sum(np.abs(segs) ** 2)))


def the_bound(l, hop, a, dtype="float32"):
    r = ceil_div(l, hop)
    real = {"float32": "float32", "complex64": "float32", "float64": "float64", "complex128": "float64"}[dtype]
    return np.sqrt(r) * (A.bound(dtype, l) + (r + 2) * U[real]) * a


def figure(got, ref, dp):
    return float(np.sqrt(np.sum(np.abs((np.asarray(got).astype(ref.dtype) - ref) * dp) ** 2)))


def assert_within(what, got, ref, dp, l, hop, a, dtype="float32", factor=1.0):
    """|| (got - ref) D' ||_2 within the bound; prints the figure before it asserts."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    f, b = figure(got, ref, dp), factor * the_bound(l, hop, a, dtype)
    print(f"{what}: || (got - ref) D' || = {f:.3e}, bound {b:.3e} (ratio {f / b:.3f})")
    assert f <= b, f"{what}: {f:.3e} > {b:.3e}"


def analysis(x, case, w, dtype=np.complex64):
    """[P][M][L / 2 + 1]: the half spectrum of every host-cut, windowed segment, computed in float64 and rounded to `dtype`."""
    return np.fft.rfft(W.segments(x, case) * w, axis=-1).astype(dtype)


def spectra(case, wname, seed=71):
    """The input of a plan-level case: the complex64 stft of spectrogram.series (amplitudes differ per series and per hop)."""
    return analysis(S.series(case, seed), case, window(wname, case[0]))


def check_the_model_is_the_inverse():
    """A float64 series, its float64 analysis (cut, window, rfft) and the model: the series, to 1e-12 relative (2-norm) over the samples where D > 1e-10."""
    rng = np.random.default_rng(5)
    for l in (64, 256):
        for wname in WINDOWS:
            for hop in (l, l // 2, l // 4, 37):
                m = 7
                case = (l, hop, m, 2)
                x = rng.standard_normal((2, W.span(case))) + 0.5
                w = window(wname, l)
                got, dp, _ = model(analysis(x, case, w, np.complex128), l, hop, w, 1.0 / l)
                ok = envelope(w, hop, m) > 1e-10
                rel = np.linalg.norm((got - x)[:, ok]) / np.linalg.norm(x[:, ok])
                print(f"L = {l} {win_id(wname)} hop {hop}: {rel:.2e} over {ok.sum()} of {ok.size} samples")
                assert rel <= 1e-12 and ok.sum() >= ok.size - m - 1
                assert np.array_equal(got[:, ~ok], overlap_add(inverse_segments(analysis(x, case, w, np.complex128), l, 1.0 / l), w, hop)[:, ~ok])  # (undivided)


def check_the_bound_is_sensitive():
    """A result with ONE segment shifted by one sample, and one with D computed from w instead of w^2, both miss the bound."""
    case, wname = (256, 128, 5, 3), "hann"
    l, hop, m, p = case
    w = window(wname, l)
    spec = spectra(case, wname)
    ref, dp, a = model(spec, l, hop, w, 1.0 / l)
    b = the_bound(l, hop, a)
    segs = inverse_segments(spec, l, 1.0 / l)
    shifted = segs.copy()
    shifted[0, 2] = np.roll(segs[0, 2], 1)  # (series 0 is the SMALLEST: amplitude 1 of 1, 3, 9)
    f1 = figure(overlap_add(shifted, w, hop) / dp, ref, dp)
    d1 = np.zeros_like(dp)
    for s in range(m):
        d1[s * hop:s * hop + l] += w
    f2 = figure(overlap_add(segs, w, hop) / np.where(d1 > 1e-10, d1, 1.0), ref, dp)
    print(f"one segment shifted by a sample: {f1:.3e}; D from w: {f2:.3e}; bound {b:.3e}")
    assert f1 > b and f2 > b


# ---------------------------------------------------------------------------------- plan level (both libraries)
def make_plan(case, wname=None, pitch=0, **over):
    l, h, m, p = case
    kw = dict(ndim=1, batch=p * m, ny=1, nx=l, dtype=torch.complex64, out_mode=L.OUT_COMPLEX, flags=FLAGS, scale=1.0 / l, mean_batch=m, seg_hop=h, seg_synth=1,
              in_stride_batch=pitch, window_x=None if wname is None else api._window_vector(wname, l))
    kw.update(over)
    return engine.SpectralPlan(**kw)


def run(plan, spec):
    t = spec if isinstance(spec, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(spec)).to(L.device())
    out, _ = plan.execute(t)
    return out.cpu().numpy()


def assert_synth_plan(plan):
    d = plan.describe()
    assert plan.kernel_info()[0] == L.K_FASTW and "[fastw overlap-add]" in d and "[mean over the batch]" not in d and "[fastw segments kept]" not in d and "[fastw]" not in d, d
    assert plan.workspace_bytes == 0


def check_plan(case, wname):
    l, h, m, p = case
    spec = spectra(case, wname)
    plan = make_plan(case, wname)
    assert_synth_plan(plan)
    got = run(plan, spec)
    assert got.shape == (p, W.span(case)) and got.dtype == np.float32
    ref, dp, a = model(spec, l, h, window(wname, l), 1.0 / l)
    assert_within(f"plan {S.case_id(case)} {win_id(wname)}", got, ref, dp, l, h, a)
    assert np.array_equal(got, run(plan, spec))  # a second execution: the same bits
    # series k of the P-series plan has the bits of the same series run alone
    for k in sorted({0, p // 2, p - 1}):
        assert np.array_equal(got[k], run(make_plan((l, h, m, 1), wname), spec[k:k + 1])[0]), k
    # the imaginary parts of bins 0 and L / 2 are ignored
    odd = spec.copy()
    odd[..., 0] += 1j
    odd[..., -1] += 1j
    assert np.array_equal(got, run(plan, odd))
    return got


def check_prefix(case, fewer, wname):
    """The first (M' - R + 1) hop samples of the M-segment run are those of the M'-segment run: a sample's bits depend on its covering segments only."""
    l, h, m, p = case
    spec = spectra(case, wname)
    full = run(make_plan(case, wname), spec)
    part = run(make_plan((l, h, fewer, p), wname), spec[:, :fewer])
    n = (fewer - ceil_div(l, h) + 1) * h
    assert n > 0 and np.array_equal(full[:, :n], part[:, :n])


def check_pitch_and_padding(case, wname):
    """A pitch larger than M (L / 2 + 1), NaN in the padding: the bits of the dense call."""
    l, h, m, p = case
    spec = spectra(case, wname)
    nb = l // 2 + 1
    pitch = m * nb + 5
    buf = torch.full((p * pitch,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=L.device())
    view = torch.as_strided(buf, (p, m, nb), (pitch, nb, 1))
    view.copy_(torch.from_numpy(spec).to(L.device()))
    want = run(make_plan(case, wname), spec)
    got = run(make_plan(case, wname, pitch=pitch), view)
    assert np.isfinite(got).all() and np.array_equal(got, want)


def check_containment(wname, bad):
    """A non-finite bin in segment 2 of series 1 (L = 256, hop = 128, M = 5): exactly the samples [256, 512) of series 1 are non-finite, every other keeps its bits."""
    case = CONTAIN
    spec = spectra(case, wname)
    plan = make_plan(case, wname)
    clean = run(plan, spec)
    sb = spec.copy()
    sb[1, 2, 17] = bad
    got = run(plan, sb)
    hit = np.zeros(got.shape, dtype=bool)
    hit[1, 256:512] = True
    assert (~np.isfinite(got[hit])).all(), "a sample of the segment that holds the bin is finite"
    assert np.isfinite(got[~hit]).all() and np.array_equal(got[~hit], clean[~hit])


def _status(**kw):
    base = dict(ndim=1, batch=6, ny=1, nx=256, dtype=torch.complex64, out_mode=L.OUT_COMPLEX, flags=FLAGS, mean_batch=3, seg_hop=128, seg_synth=1)
    base.update(kw)
    try:
        engine.SpectralPlan(**base)
    except L.XrftHipError as e:
        return e.status
    return 0


def check_status_codes():
    assert _status() == 0 and _status(seg_hop=256) == 0 and _status(seg_hop=37) == 0 and _status(mean_batch=1, batch=2) == 0
    assert _status(window_x=api._window_vector("hann", 256)) == 0 and _status(in_stride_batch=3 * 129) == 0 and _status(in_stride_batch=3 * 129 + 5) == 0
    assert _status(nx=64, seg_hop=1) == 0 and _status(nx=4096, seg_hop=2048) == 0 and _status(nx=2048, seg_hop=1024) == 0 and _status(inner=1) == 0
    bad = [dict(seg_synth=2), dict(seg_synth=-1), dict(seg_hop=0), dict(seg_keep=1), dict(out_mode=L.OUT_POWER), dict(out_mode=L.OUT_CROSS), dict(dtype=torch.float32),
           dict(dtype=torch.float64), dict(dtype=torch.complex128), dict(dtype=torch.float16), dict(detrend=L.DETREND_CONSTANT), dict(detrend=L.DETREND_LINEAR),
           dict(flags=0), dict(flags=L.INVERSE), dict(flags=L.C2R_X), dict(flags=FLAGS | L.SHIFT_X), dict(flags=FLAGS | L.ISHIFT_X), dict(flags=FLAGS | L.PHASE_IN),
           dict(flags=FLAGS | L.HALF_X), dict(flags=FLAGS | L.ISO), dict(phase_x=np.exp(-2j * np.pi * np.fft.rfftfreq(256) * 3.0)), dict(in_stride_batch=3 * 129 - 1),
           # ... and what seg_hop refuses
           dict(seg_hop=-1), dict(seg_hop=257), dict(ndim=2, ny=4), dict(inner=4), dict(mid=4), dict(herm_ny=4, herm_nx=4), dict(in_stride_y=512), dict(mean_batch=0),
           dict(batch=7), dict(seg_stride=-1), dict(inner=4, seg_stride=3)]
    for kw in bad:
        assert _status(**kw) == L.BAD_ARG, kw
    composes = [dict(nx=100, seg_hop=50), dict(nx=32, seg_hop=16), dict(nx=8192, seg_hop=4096), dict(nx=2048, seg_hop=512), dict(nx=4096, seg_hop=1024),
                dict(nx=256, seg_hop=1), dict(inner=3, seg_stride=3), dict(seg_stride=7),
                dict(nx=64, seg_hop=64, mean_batch=1 << 25, batch=1 << 25),  # span = 2^31
                dict(nx=64, seg_hop=64, mean_batch=1, batch=1 << 31)]        # 2^31 workgroups
    for kw in composes:
        assert _status(**kw) == L.UNSUPPORTED_LENGTH, kw
    assert _status(nx=64, seg_hop=64, mean_batch=(1 << 25) - 1, batch=(1 << 25) - 1) == 0 and _status(nx=64, seg_hop=64, mean_batch=1, batch=(1 << 31) - 1) == 0
    for knob in ("XRFTHIP_FASTW", "XRFTHIP_FASTW_SYNTH"):
        with B.env(knob, 0):
            assert _status() == L.UNSUPPORTED_LENGTH, knob
    with B.env("XRFTHIP_FASTW_SYNTH", 0):  # (the knob is this form's alone)
        assert S._status() == 0
    with B.env("XRFTHIP_FASTW_KEEP", 0):
        assert _status() == 0
    # seg_synth = 0: everything as before -- seg_hop with XRFTHIP_INVERSE stays XRFTHIP_BAD_ARG
    assert _status(seg_synth=0) == L.BAD_ARG and _status(seg_synth=0, seg_keep=1) != 0 and S._status() == 0


def check_struct_sizes():
    """Every struct_size the descriptor ever had is accepted (the words a shorter one lacks count as 0); seg_synth and seg_reserved4 came together: the size between
    the two, a larger one and a non-zero reserved word are XRFTHIP_BAD_ARG; a DescKeep-sized descriptor with garbage behind it is read without the two words."""
    dll = L.load()
    D = L.DescSynth
    sizes = [getattr(D, f).offset for f in ("inner", "mid", "in_stride_y", "herm_ny", "mean_batch", "seg_hop", "seg_stride", "seg_keep", "seg_synth")] + [C.sizeof(D)]
    assert sizes == sorted(set(sizes)) and sizes[-1] - sizes[-2] == 16 and sizes[-2] == C.sizeof(L.DescKeep) and sizes[-3] == C.sizeof(L.DescCols)
    assert [f[0] for f in D._fields_[:len(L.DescKeep._fields_)]] == [f[0] for f in L.DescKeep._fields_] and [f[0] for f in D._fields_[-2:]] == ["seg_synth", "seg_reserved4"]
    h = C.c_void_p(0)
    zeros = (0,) * 17
    for sz in sizes:
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *zeros)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0, sz
        dll.xrfthip_plan_destroy(h)
    for sz in (sizes[-2] + 8, sizes[-1] + 8):
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *zeros)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG, sz

    def synth(sz, on, res4, keep=0):
        return D(sz, 1, 6, 1, 256, L.C64, L.OUT_COMPLEX, 0, FLAGS, 1.0 / 256, 0, 0, 0, 0, 0, 0, 0, 0, 3, 128, 0, 0, 0, keep, 0, on, res4)

    assert dll.xrfthip_plan_create(C.byref(h), C.byref(synth(sizes[-1], 1, 0))) == 0
    buf = C.create_string_buffer(8192)
    dll.xrfthip_plan_describe(h, buf, len(buf))
    dll.xrfthip_plan_destroy(h)
    assert "[fastw overlap-add]" in buf.value.decode()
    # the words are read only from a descriptor that has them: the older size with garbage behind it is seg_hop with XRFTHIP_INVERSE, refused as ever
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(synth(sizes[-2], 1, 77))) == L.BAD_ARG
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(synth(sizes[-1], 1, 1))) == L.BAD_ARG
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(synth(sizes[-1], 0, 1))) == L.BAD_ARG
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(synth(sizes[-1], 1, 0, keep=1))) == L.BAD_ARG


def check_workspace(case=CASES[1]):
    """xrfthip_workspace_bytes is 0 and the plan runs without a workspace."""
    l, h, m, p = case
    plan = make_plan(case, "hann")
    assert plan.workspace_bytes == 0
    dev = L.device()
    spec = spectra(case, "hann")
    x = torch.from_numpy(spec).to(dev)
    out = torch.empty((p, W.span(case)), dtype=torch.float32, device=dev)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert L.load().xrfthip_exec(plan._h, C.c_void_p(x.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(0), C.c_void_p(0), 0, C.c_void_p(0)) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run(plan, spec))


# ---------------------------------------------------------------------------------- API level (both libraries)
import xrft_amd as xa  # noqa: E402


def synth_plans():
    return [p for p in api._plan_cache.values() if getattr(p, "seg_synth", 0)]


# name -> (shape, dims, nperseg, noverlap, keyword arguments of stft and istft, "fused" | "arranged" | None (composes), dtype)
API_CASES = {
    "trailing-256-hann": ((3, 1000), ("x", "time"), 256, None, dict(window="hann", real_dim="time"), "fused", "float32"),
    "trailing-256-no-overlap-true-amplitude": ((3, 1000), ("x", "time"), 256, 0, dict(window="hann", real_dim="time", true_amplitude=True), "fused", "float32"),
    "leading-time-cube": ((700, 3, 5), ("time", "y", "x"), 256, None, dict(window="hann", real_dim="time"), "arranged", "float32"),
    "length-100": ((3, 500), ("x", "time"), 100, None, dict(window="hann", real_dim="time"), None, "float32"),
    "float64": ((3, 1000), ("x", "time"), 256, None, dict(window="hann", real_dim="time"), None, "float64"),
    "two-sided-shifted": ((3, 600), ("x", "time"), 128, None, dict(window="hann", shift=True), None, "float32"),
    "two-sided-unshifted": ((3, 600), ("x", "time"), 128, None, dict(window="hann", shift=False), None, "float32"),
}


def api_model(st, dims, nperseg, hop, kw, dt):
    """(the model of the library's own stft output, series first; D'; A; the result's values, series first -> a function of them)."""
    ax = list(dims).index("time")
    v = np.moveaxis(np.asarray(st.values), (ax, ax + 1), (-2, -1))
    spec = v.reshape(-1, v.shape[-2], v.shape[-1])
    two = kw.get("real_dim") is None
    if two and kw.get("shift", True):
        spec = np.fft.ifftshift(spec, axes=-1)
    scale = (1.0 / dt if kw.get("true_amplitude") else 1.0) / nperseg
    return model(spec, nperseg, hop, window(kw.get("window"), nperseg), scale, two)


def series_first(values, ax):
    v = np.moveaxis(np.asarray(values), ax, -1)
    return v.reshape(-1, v.shape[-1])


def check_api_case(name):
    shape, dims, nperseg, noverlap, kw, route, dtype = API_CASES[name]
    api.clear_plan_cache()
    api._MEAN_REFUSED.clear()
    da, wide, crd = W.api_series(shape, dims, dtype, seed=85, t0=3.0)
    dt = 0.5
    hop = nperseg - (nperseg // 2 if noverlap is None else noverlap)
    st = xa.stft(da, "time", nperseg, noverlap, **kw)
    ikw = dict(kw)
    got = xa.istft(st, "time", noverlap=noverlap, **ikw)
    assert bool(synth_plans()) == (route is not None), [p.describe() for p in api._plan_cache.values()]
    if route is not None:
        assert synth_plans()[-1].kernel_info()[0] == L.K_FASTW and "[fastw overlap-add]" in synth_plans()[-1].describe()
    ax = list(dims).index("time")
    m = (shape[ax] - nperseg) // hop + 1
    span = (m - 1) * hop + nperseg
    assert tuple(got.dims) == tuple(dims) and got.shape == tuple(span if d == "time" else k for d, k in zip(dims, shape))
    two = kw.get("real_dim") is None
    want_dt = {("float32", False): np.float32, ("float32", True): np.complex64, ("float64", False): np.float64, ("float64", True): np.complex128}[(dtype, two)]
    assert np.asarray(got.values).dtype == want_dt
    ref, dp, a = api_model(st, dims, nperseg, hop, kw, dt)
    g = series_first(got.values, ax)
    bdt = {np.float32: "float32", np.complex64: "complex64", np.float64: "float64", np.complex128: "complex128"}[want_dt]
    assert_within(f"istft {name}", g, ref, dp, nperseg, hop, a, bdt)
    # ... and, away from the two ends (where D is one window's own small tail), it is the series again: a plausibility check, held loosely -- the contract is the model's
    if noverlap is None:
        x = series_first(wide, ax)[:, nperseg:span - nperseg]
        rel = np.linalg.norm(g[:, nperseg:span - nperseg] - x) / np.linalg.norm(x)
        print(f"istft(stft) {name}: {rel:.2e} of the series")
        assert rel < (1e-5 if dtype == "float32" else 1e-13)
    # the rebuilt coordinate, the kept ones
    assert np.allclose(got["time"].values, crd["time"][:span], rtol=1e-12, atol=0) and got["time"].values.shape == (span,)
    for d in dims:
        if d != "time":
            assert np.array_equal(got[d].values, crd[d])
    assert got.name is None and not got.attrs
    if route is not None:  # the fused and the composed result of one call lie within twice the bound of each other
        with B.env("XRFTHIP_FASTW_SYNTH", 0):
            n0 = len(synth_plans())
            comp = xa.istft(st, "time", noverlap=noverlap, **ikw)
            assert len(synth_plans()) == n0
        B.compare_labelled(got, comp)
        assert_within(f"istft {name} fused against composed", g, series_first(comp.values, ax).astype(np.float64), dp, nperseg, hop, a, bdt, factor=2.0)
    return da, st, got


def check_api_labels():
    """Dims order, t0 and dt, kept coordinates, a datetime64 <dim>_segment (t0 = 0), a segment dim without a coordinate, fewer segments than stft wrote."""
    api.clear_plan_cache()
    n = 600
    rng = np.random.default_rng(86)
    crd = {"time": 7.0 + np.arange(n) * 0.25, "y": np.arange(4) * 2.0, "x": np.arange(5) * 0.5}
    da = xa.DataArray(torch.from_numpy(rng.standard_normal((4, n, 5)).astype(np.float32)).to(L.device()), ("y", "time", "x"), crd)
    st = xa.stft(da, "time", 64, 16, window="hann", real_dim="time")
    got = xa.istft(st, "time", noverlap=16, window="hann", real_dim="time")
    m = (n - 64) // 48 + 1
    span = (m - 1) * 48 + 64
    assert got.dims == ("y", "time", "x") and got.shape == (4, span, 5)
    assert np.allclose(got["time"].values, crd["time"][:span], rtol=1e-12, atol=0) and got["time"].attrs["spacing"] == 0.25
    assert np.array_equal(got["y"].values, crd["y"]) and np.array_equal(got["x"].values, crd["x"]) and list(got.coords) == ["y", "x", "time"]
    # a datetime64 time axis: the middles are datetime64, t0 = 0, dt from freq_time
    t = np.datetime64("2001-01-01T00:00") + np.arange(n) * np.timedelta64(30, "m")
    dd = xa.DataArray(da.data, ("y", "time", "x"), dict(crd, time=t))
    sd = xa.stft(dd, "time", 64, window="hann", real_dim="time")
    assert sd["time_segment"].values.dtype.kind == "M"
    gd = xa.istft(sd, "time", window="hann", real_dim="time")
    dt = 1.0 / (64 * (sd["freq_time"].values[1] - sd["freq_time"].values[0]))
    assert gd["time"].values[0] == 0.0 and np.allclose(gd["time"].values, dt * np.arange(gd.shape[1]), rtol=1e-12, atol=0)
    # no coordinate on the segment dim: t0 = 0; and a shorter <dim>_segment stays as it is (no length is inferred)
    bare = xa.DataArray(st.data[:, :5], st.dims, {k: v for k, v in st.coords.items() if k != "time_segment"})
    gb = xa.istft(bare, "time", 64, 16, window="hann", real_dim="time")
    assert gb.shape == (4, 4 * 48 + 64, 5) and gb["time"].values[0] == 0.0
    assert np.array_equal(gb.values[:, :4 * 48], got.values[:, :4 * 48])  # (the samples whose covering segments are the same: the same bits)


def check_api_refusal_is_remembered():
    """nperseg = 100: the library declines once (XRFTHIP_UNSUPPORTED_LENGTH); the second call composes without building a plan with seg_synth.  float64 and two-sided
    spectra: never asked."""
    api.clear_plan_cache()
    api._MEAN_REFUSED.clear()
    made = []
    real = engine.SpectralPlan

    class Counting(real):
        def __init__(self, *a, **kw):
            if kw.get("seg_synth"):
                made.append(kw)
            super().__init__(*a, **kw)

    engine.SpectralPlan = Counting
    try:
        da, _, _ = W.api_series((3, 500), ("x", "time"), "float32", seed=87)
        kw = dict(window="hann", real_dim="time")
        st = xa.stft(da, "time", 100, **kw)
        refused = len(api._MEAN_REFUSED)
        first = xa.istft(st, "time", **kw)
        assert len(made) == 1 and len(api._MEAN_REFUSED) == refused + 1 and not synth_plans()
        second = xa.istft(st, "time", **kw)
        assert len(made) == 1 and np.array_equal(first.values, second.values)
        d64, _, _ = W.api_series((3, 500), ("x", "time"), "float64", seed=87)
        xa.istft(xa.stft(d64, "time", 128, **kw), "time", **kw)
        xa.istft(xa.stft(da, "time", 128, window="hann"), "time", window="hann")
        assert len(made) == 1
        s128 = xa.stft(da, "time", 128, **kw)
        with B.env("XRFTHIP_FASTW_SYNTH", 0):
            xa.istft(s128, "time", **kw)
        assert len(made) == 1
        xa.istft(s128, "time", **kw)
        assert len(made) == 2 and synth_plans()
    finally:
        engine.SpectralPlan = real


def check_api_errors():
    import pytest

    da, _, _ = W.api_series((3, 600), ("x", "time"), "float32", seed=88)
    st = xa.stft(da, "time", 64, real_dim="time")
    two = xa.stft(da, "time", 64)
    for kw in (dict(nperseg=66), dict(nperseg=33), dict(noverlap=64), dict(noverlap=-1), dict(real_dim="x")):
        with pytest.raises(ValueError):
            xa.istft(st, "time", **dict(dict(real_dim="time"), **kw))
    with pytest.raises(ValueError):
        xa.istft(two, "time", nperseg=126)
    with pytest.raises(ValueError):
        xa.istft(st, ["time"], real_dim="time")
    with pytest.raises(ValueError):
        xa.istft(st, "x", real_dim="x")  # (no x_segment / freq_x)
    with pytest.raises(ValueError):
        xa.istft(da, "time")
    swapped = xa.DataArray(st.data.transpose(1, 2), ("x", "freq_time", "time_segment"), st.coords)
    with pytest.raises(ValueError):
        xa.istft(swapped, "time", real_dim="time")
    apart = xa.DataArray(st.data.permute(1, 0, 2), ("time_segment", "x", "freq_time"), st.coords)
    with pytest.raises(ValueError):
        xa.istft(apart, "time", real_dim="time")
    with pytest.raises(TypeError):
        xa.istft(st, "time", real_dim="time", detrend="linear")
