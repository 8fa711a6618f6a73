"""Shared by the tests of the FIR filter (xrfthip_desc.seg_filter, csrc/fastf.h, xrft_amd.fir_filter; tests/test_fir_filter_emulated.py on the emulated library,
tests/test_gpu_fir_filter.py on the MI355X): the model, the bound, the plan-level cases and the API-level checks.  Not a conftest: imported by the tests that use it.

The model is scipy.signal.convolve(x.astype(float64), taps[None], mode, method="direct") in float64, per series.

The bound has no constant of its own.  With b = accuracy.bound(dtype, L) (the contract of ONE transform, norm-wise; overlap-save runs two), u the unit roundoff,
Hmax = max |rfft(taps, L)| in float64 and A^2 = the sum over series and segments of the squared norm of each segment's L zero-filled inputs (rebuilt here from L,
V = L - K + 1 and a):

    || got - ref ||_2  <=  (2 b + 4 u) Hmax A

-- the spectrum of a segment is within b of its norm, the product with H (rounded to the data's precision: u, the product: u) at most Hmax times larger, the way
back adds b again, `scale` one more u (4 u with the store)."""
import ctypes as C

import numpy as np
import scipy.signal
import torch

import xrft_amd as xa
from xrft_amd import _lib as L
from xrft_amd import _segments as SEG
from xrft_amd import api, engine

import accuracy as A
import batch_mean as B
import istft as I
import spectrogram as S

MODES = ["full", "same", "valid"]
TAPS = ["normal", "firwin"]
# (L, K, N, P), each the smallest shape that reaches its hazard: K = 1, V = L, one exact segment; K - 1 = L / 2, the admitted extreme, a partial last segment;
# V = 57 unaligned and M = 141 > NS = 128, two workgroups per series; basic overlap; more series than CUs; longer segments; NS = 2, three workgroups; long segments
# with short taps; a series shorter than the taps ("full" and "same" only)
CASES = [(64, 1, 64, 1), (64, 33, 100, 3), (64, 8, 8000, 1), (256, 65, 700, 3), (256, 31, 300, 300), (1024, 257, 5000, 2), (4096, 2049, 9000, 2), (4096, 2, 5000, 1),
         (64, 33, 10, 2)]
PLAN_PARAMS = [(c, m, t) for c in CASES for m in MODES for t in TAPS if not (m == "valid" and c[2] < c[1])]
PREFIX_CASES = [((64, 8, 8000, 1), 5000), ((256, 65, 700, 3), 500), ((4096, 2049, 9000, 2), 7000)]
PITCH_CASES = [(64, 33, 100, 3), (256, 65, 700, 3)]
CONTAIN = (256, 65, 700, 3)
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
ZERO_LAST_TAP = (31, "firwin")  # firwin(31, 0.2) ends in sinc(0.2 * 15) = sinc(3) = 0 but for rounding


def case_id(c):
    return f"L{c[0]}-K{c[1]}-N{c[2]}-P{c[3]}"


def param_id(p):
    return f"{case_id(p[0])}-{p[1]}-{p[2]}"


def offsets(mode, n, k):
    """(a, n_out): output sample n' is y_full[n' + a]."""
    return {"full": (0, n + k - 1), "same": ((k - 1) // 2, n), "valid": (k - 1, n - k + 1)}[mode]


def taps_of(kind, k, seed=97):
    if kind == "firwin":
        return np.asarray(scipy.signal.firwin(k, 0.2), dtype=np.float64)
    return np.random.default_rng(seed + k).standard_normal(k)


def series(case, seed=91):
    """[P][N] float32: seeded noise over a line, series p scaled by 3^(p mod 4) (a result stored under another series' index misses the bound)."""
    l, k, n, p = case
    v = np.random.default_rng(seed).standard_normal((p, n)) + 0.01 * np.arange(n) + 0.5
    return (v * (3.0 ** (np.arange(p) % 4)).reshape(p, 1)).astype(np.float32)


# ---------------------------------------------------------------------------------- the model and the bound
_MODELS = {}


def model(x, taps, mode):
    """The reference, computed once per (series, taps, mode) and shared by the tests that need it; read-only."""
    x, taps = np.asarray(x), np.asarray(taps, dtype=np.float64)
    key = (x.shape, str(x.dtype), hash(x.tobytes()), hash(taps.tobytes()), mode)
    if key not in _MODELS:
        ref = scipy.signal.convolve(x.astype(np.float64), taps[None], mode, method="direct")
        ref.setflags(write=False)
        _MODELS[key] = ref
    return _MODELS[key]


def segment_inputs(x, l, k, a, n_out):
    """[P][M][L] float64: the zero-filled inputs of every segment -- sample j of segment s is x[s V + a - (K - 1) + j] inside [0, N), else 0."""
    x = np.asarray(x, dtype=np.float64)
    p, n = x.shape
    v = l - k + 1
    m = -(-n_out // v)
    idx = (np.arange(m) * v)[:, None] + (a - (k - 1)) + np.arange(l)[None, :]
    ok = (idx >= 0) & (idx < n)
    return np.where(ok[None], x[:, np.clip(idx, 0, n - 1)], 0.0)


def the_bound(x, taps, l, a, n_out, dtype="float32"):
    k = len(taps)
    amp = float(np.sqrt(np.sum(segment_inputs(x, l, k, a, n_out) ** 2)))
    hmax = float(np.abs(np.fft.rfft(np.asarray(taps, dtype=np.float64), l)).max())
    return (2.0 * A.bound(dtype, l) + 4.0 * U[dtype]) * hmax * amp


def figure(got, ref):
    return float(np.sqrt(np.sum((np.asarray(got).astype(np.float64) - ref) ** 2)))


def assert_within(what, got, ref, bound):
    """|| got - ref ||_2 within the bound; prints the figure before it asserts."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    f = figure(got, ref)
    print(f"{what}: || got - ref || = {f:.3e}, bound {bound:.3e} (ratio {f / bound:.4f})")
    assert f <= bound, f"{what}: {f:.3e} > {bound:.3e}"


def restatement(x, taps, l, a, n_out):
    """The algorithm in float32 numpy: the segments, rfft, the product with the complex64 response, irfft, the kept samples."""
    k = len(taps)
    v = l - k + 1
    seg = segment_inputs(x, l, k, a, n_out).astype(np.float32)
    h = np.fft.rfft(np.asarray(taps, dtype=np.float64), l).astype(np.complex64)
    y = np.fft.irfft((np.fft.rfft(seg, axis=-1).astype(np.complex64) * h).astype(np.complex64), n=l, axis=-1).astype(np.float32)
    return y[..., k - 1:].reshape(seg.shape[0], -1)[:, :n_out]


def check_the_bound_is_sensitive():
    """On the cases with N >= K: a float32 restatement of the algorithm lies far inside the bound; a result shifted by one sample and one with the last tap dropped
    miss it."""
    for case in CASES:
        l, k, n, p = case
        if n < k:
            continue
        x = series(case)
        for kind in TAPS:
            taps = taps_of(kind, k)
            for mode in MODES:
                a, n_out = offsets(mode, n, k)
                ref = model(x, taps, mode)
                b = the_bound(x, taps, l, a, n_out)
                f0 = figure(restatement(x, taps, l, a, n_out), ref)
                f1 = figure(np.roll(ref, 1, axis=1), ref)
                idx = np.arange(n_out) + a - (k - 1)  # (the convolution is linear: without the last tap the result lacks taps[K - 1] x[n' + a - (K - 1)])
                f2 = figure(ref - taps[-1] * np.where((idx >= 0) & (idx < n), x.astype(np.float64)[:, np.clip(idx, 0, n - 1)], 0.0), ref)
                print(f"{case_id(case)} {mode} {kind}: restated {f0 / b:.4f}, shifted by a sample {f1 / b:.3g}, last tap dropped {f2 / b:.3g} of the bound {b:.3e}")
                assert f0 <= b and f1 > b, (case, mode, kind)
                if (k, kind) == ZERO_LAST_TAP:  # (dropping that tap changes nothing, as on a series shorter than the taps: this one (K, taps) alone is left out)
                    assert abs(taps[-1]) < 1e-15 and f2 < 1e-6 * b
                    continue
                assert f2 > b, (case, mode, kind)


# ---------------------------------------------------------------------------------- plan level (both libraries)
def plan_kw(case, mode, **over):
    l, k, n, p = case
    a, n_out = offsets(mode, n, k)
    v = l - k + 1
    m = -(-n_out // v)
    kw = dict(ndim=1, batch=p * m, ny=1, nx=l, dtype=torch.float32, out_mode=L.OUT_COMPLEX, flags=0, scale=1.0 / l, mean_batch=m, seg_hop=v, seg_filter=1, seg_lead=a,
              seg_in_len=n, seg_out_len=n_out)
    kw.update(over)
    return kw


def make_plan(case, mode, taps=None, pitch=0, **over):
    resp = None if taps is None else np.fft.rfft(np.asarray(taps, dtype=np.float64), case[0])
    return engine.SpectralPlan(**plan_kw(case, mode, phase_x=resp, in_stride_batch=pitch, **over))


def run(plan, x):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(L.device())
    out, _ = plan.execute(t)
    return out.cpu().numpy()


def assert_filter_plan(plan):
    d = plan.describe()
    assert plan.kernel_info()[0] == L.K_FASTW and "[fastw overlap-save]" in d and "[fastw overlap-add]" not in d and "[fastw segments kept]" not in d and "[fastw]" not in d, d
    assert "4 algorithmic bytes per sample read and 4 per sample written" in d, d
    assert plan.workspace_bytes == 0


def check_plan(case, mode, kind):
    l, k, n, p = case
    a, n_out = offsets(mode, n, k)
    x, taps = series(case), taps_of(kind, k)
    plan = make_plan(case, mode, taps)
    assert_filter_plan(plan)
    got = run(plan, x)
    assert got.shape == (p, n_out) and got.dtype == np.float32
    assert_within(f"plan {case_id(case)} {mode} {kind}", got, model(x, taps, mode), the_bound(x, taps, l, a, n_out))
    assert np.array_equal(got, run(plan, x))  # a second execution: the same bits
    for s in sorted({0, p // 2, p - 1}):  # series s of the P-series plan has the bits of the same series run alone
        assert np.array_equal(got[s], run(make_plan((l, k, n, 1), mode, taps), x[s:s + 1])[0]), s
    # the imaginary parts of entries 0 and L / 2 are ignored
    resp = np.fft.rfft(taps, l)
    resp[0] += 1j
    resp[-1] -= 2j
    assert np.array_equal(got, run(engine.SpectralPlan(**plan_kw(case, mode, phase_x=resp)), x))
    return got


def check_prefix(case, fewer, mode):
    """A series cut to N' samples: every output whose segment's L inputs lie wholly below N' keeps its bits."""
    l, k, n, p = case
    x, taps = series(case), taps_of("normal", k)
    a, n_out = offsets(mode, n, k)
    a2, n_out2 = offsets(mode, fewer, k)
    assert a2 == a
    full = run(make_plan(case, mode, taps), x)
    part = run(make_plan((l, k, fewer, p), mode, taps), np.ascontiguousarray(x[:, :fewer]))
    v = l - k + 1
    whole = (fewer - (a - (k - 1)) - l) // v + 1  # segments s with s V + a - (K - 1) + L - 1 < N'
    cnt = min(whole * v, n_out, n_out2)
    assert cnt > v and np.array_equal(full[:, :cnt], part[:, :cnt])


def check_pitch_and_gap(case, mode):
    """A pitch beyond N, NaN in the gap: the bits of the dense call."""
    l, k, n, p = case
    x, taps = series(case), taps_of("firwin", k)
    pitch = n + 7
    buf = torch.full((p * pitch,), float("nan"), dtype=torch.float32, device=L.device())
    view = torch.as_strided(buf, (p, n), (pitch, 1))
    view.copy_(torch.from_numpy(x).to(L.device()))
    want = run(make_plan(case, mode, taps), x)
    got = run(make_plan(case, mode, taps, pitch=pitch), view)
    assert np.isfinite(got).all() and np.array_equal(got, want)


def check_containment(bad, mode, where):
    """One non-finite sample i of series 1: every output of the (at most two) segments whose L inputs include i is non-finite, every other keeps its bits."""
    case = CONTAIN
    l, k, n, p = case
    a, n_out = offsets(mode, n, k)
    v = l - k + 1
    m = -(-n_out // v)
    x, taps = series(case), taps_of("normal", k)
    plan = make_plan(case, mode, taps)
    clean = run(plan, x)
    xb = x.copy()
    xb[1, where] = bad
    got = run(plan, xb)
    segs = [s for s in range(m) if 0 <= where - (s * v + a - (k - 1)) < l]
    assert 1 <= len(segs) <= 2, segs
    hit = np.zeros(got.shape, dtype=bool)
    for s in segs:
        hit[1, s * v:min((s + 1) * v, n_out)] = True
    print(f"sample {where} ({mode}): segments {segs}, {int(hit.sum())} outputs")
    assert (~np.isfinite(got[hit])).all(), "an output of a segment that holds the sample is finite"
    assert np.isfinite(got[~hit]).all() and np.array_equal(got[~hit], clean[~hit])


def check_no_table_is_ones(case=(256, 65, 700, 3), mode="same"):
    """Without a table the response counts as 1: the bits of the all-ones table, and the series delayed -- out[n'] = x[n' + a - (K - 1) + (K - 1)] = x[n' + a]."""
    l, k, n, p = case
    a, n_out = offsets(mode, n, k)
    x = series(case)
    none = run(make_plan(case, mode), x)
    ones = run(engine.SpectralPlan(**plan_kw(case, mode, phase_x=np.ones(l // 2 + 1, dtype=np.complex128))), x)
    assert np.array_equal(none, ones)
    delta = np.zeros(k)
    delta[0] = 1.0
    assert_within("no table: a delay", none, model(x, delta, mode), the_bound(x, delta, l, a, n_out))
    # ... and the table can be cleared again
    plan = make_plan(case, mode, taps_of("normal", k))
    L.check(L.load().xrfthip_plan_set_phase(plan._h, 1, C.c_void_p(0), 0))
    assert np.array_equal(run(plan, x), none)


def _status(**kw):
    base = plan_kw((256, 65, 700, 3), "same")
    base.update(kw)
    try:
        engine.SpectralPlan(**base)
    except L.XrftHipError as e:
        return e.status
    return 0


def check_status_codes():
    resp = np.fft.rfft(taps_of("normal", 65), 256)
    assert _status() == 0 and _status(phase_x=resp) == 0 and _status(in_stride_batch=700) == 0 and _status(in_stride_batch=707) == 0 and _status(inner=1) == 0
    assert _status(seg_lead=0) == 0 and _status(seg_lead=64, seg_out_len=636, mean_batch=4, batch=12) == 0  # ("valid")
    assert _status(seg_lead=0, seg_out_len=764) == 0  # ("full": ceil(764 / 192) = 4 as well)
    assert _status(nx=64, seg_hop=64, seg_lead=0, seg_in_len=64, seg_out_len=64, mean_batch=1, batch=1) == 0  # (K = 1)
    assert _status(nx=64, seg_hop=32, seg_lead=32, seg_in_len=100, seg_out_len=68, mean_batch=3, batch=3) == 0  # (K - 1 = L / 2)
    bad = [dict(seg_filter=2), dict(seg_filter=-1), dict(seg_filter=0), dict(seg_filter=0, seg_lead=0, seg_in_len=0), dict(seg_filter=0, seg_lead=0, seg_out_len=0),
           dict(seg_filter=0, seg_in_len=0, seg_out_len=0), dict(seg_hop=0), dict(seg_hop=127), dict(seg_hop=257), dict(seg_keep=1), dict(seg_synth=1), dict(seg_stride=1),
           dict(seg_stride=3, inner=3), dict(inner=4), dict(ndim=2, ny=4), dict(mid=4), dict(dtype=torch.float64), dict(dtype=torch.complex64), dict(dtype=torch.float16),
           dict(out_mode=L.OUT_POWER), dict(out_mode=L.OUT_CROSS), dict(flags=L.SHIFT_X), dict(flags=L.HALF_X), dict(flags=L.INVERSE), dict(flags=L.ISO),
           dict(detrend=L.DETREND_CONSTANT), dict(detrend=L.DETREND_LINEAR), dict(window_x=api._window_vector("hann", 256)), dict(seg_in_len=0), dict(seg_out_len=0),
           dict(seg_in_len=-5), dict(seg_lead=-1), dict(seg_lead=65), dict(seg_out_len=733), dict(mean_batch=3, batch=9), dict(mean_batch=5, batch=15),
           dict(batch=13), dict(in_stride_batch=699), dict(phase_x=resp[:-1]), dict(phase_x=np.ones(256, dtype=np.complex128)), dict(phase_y=resp)]
    for kw in bad:
        assert _status(**kw) == L.BAD_ARG, kw
    composes = [dict(nx=100, seg_hop=60, seg_lead=20, mean_batch=12, batch=36), dict(nx=32, seg_hop=24, seg_lead=4, mean_batch=30, batch=90),
                dict(nx=8192, seg_hop=8128, seg_lead=32, mean_batch=1, batch=3),
                dict(nx=64, seg_hop=64, seg_lead=0, seg_in_len=64, seg_out_len=64, mean_batch=1, batch=1 << 31)]  # 2^31 workgroups
    for kw in composes:
        assert _status(**kw) == L.UNSUPPORTED_LENGTH, kw
    assert _status(nx=64, seg_hop=64, seg_lead=0, seg_in_len=64, seg_out_len=64, mean_batch=1, batch=(1 << 31) - 1) == 0
    for knob in ("XRFTHIP_FASTW", "XRFTHIP_FASTW_FILTER"):
        with B.env(knob, 0):
            assert _status() == L.UNSUPPORTED_LENGTH, knob
    with B.env("XRFTHIP_FASTW_FILTER", 0):  # (the knob is this form's alone)
        assert S._status() == 0 and I._status() == 0
    for knob in ("XRFTHIP_FASTW_KEEP", "XRFTHIP_FASTW_SYNTH"):
        with B.env(knob, 0):
            assert _status() == 0
    # seg_filter = 0 leaves the spectrogram and synthesis descriptors' answers alone, and a companion word alone is refused on them too
    assert S._status() == 0 and I._status() == 0 and S._status(seg_hop=0) == L.BAD_ARG and I._status(seg_keep=1) == L.BAD_ARG
    assert S._status(seg_lead=1) == L.BAD_ARG and I._status(seg_in_len=1) == L.BAD_ARG and S._status(seg_out_len=1) == L.BAD_ARG


def check_struct_sizes():
    """Every struct_size the descriptor ever had is accepted (the words a shorter one lacks count as 0); the four new words came together: the sizes between them and
    a larger one are XRFTHIP_BAD_ARG; a DescSynth-sized descriptor with garbage behind it is read without the four words."""
    dll = L.load()
    D = L.DescFilt
    sizes = [getattr(D, f).offset for f in ("inner", "mid", "in_stride_y", "herm_ny", "mean_batch", "seg_hop", "seg_stride", "seg_keep", "seg_synth", "seg_filter")] + [C.sizeof(D)]
    assert len(sizes) == 11 and sizes == sorted(set(sizes)) and sizes[-1] - sizes[-2] == 32 and sizes[-2] == C.sizeof(L.DescSynth) and sizes[-3] == C.sizeof(L.DescKeep)
    assert [f[0] for f in D._fields_[:len(L.DescSynth._fields_)]] == [f[0] for f in L.DescSynth._fields_]
    assert [f[0] for f in D._fields_[-4:]] == ["seg_filter", "seg_lead", "seg_in_len", "seg_out_len"]
    h = C.c_void_p(0)
    zeros = (0,) * 21
    for sz in sizes:
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *zeros)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0, sz
        dll.xrfthip_plan_destroy(h)
    for sz in (sizes[-2] + 8, sizes[-2] + 16, sizes[-2] + 24, sizes[-1] + 8):
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *zeros)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG, sz

    def filt(sz, on, lead=32, n_in=700, n_out=700):
        return D(sz, 1, 12, 1, 256, L.F32, L.OUT_COMPLEX, 0, 0, 1.0 / 256, 0, 0, 0, 0, 0, 0, 0, 0, 4, 192, 0, 0, 0, 0, 0, 0, 0, on, lead, n_in, n_out)

    assert dll.xrfthip_plan_create(C.byref(h), C.byref(filt(sizes[-1], 1))) == 0
    buf = C.create_string_buffer(8192)
    dll.xrfthip_plan_describe(h, buf, len(buf))
    dll.xrfthip_plan_destroy(h)
    assert "[fastw overlap-save]" in buf.value.decode()
    # the words are read only from a descriptor that has them: the older size with garbage behind it is seg_hop with OUT_COMPLEX and no seg_keep, refused as ever
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(filt(sizes[-2], 1))) == L.BAD_ARG
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(filt(sizes[-1], 0))) == L.BAD_ARG
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(filt(sizes[-1], 1, lead=65))) == L.BAD_ARG
    # ... and, power spectra of slabs, it is accepted with the garbage behind it
    d = D(sizes[-2], 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *((0,) * 17), 1, 2, 3, 4)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0
    dll.xrfthip_plan_destroy(h)


def check_workspace(case=(64, 33, 100, 3), mode="same"):
    """xrfthip_workspace_bytes is 0 and the plan runs without a workspace."""
    l, k, n, p = case
    taps = taps_of("normal", k)
    plan = make_plan(case, mode, taps)
    assert plan.workspace_bytes == 0
    dev = L.device()
    x = series(case)
    xd = torch.from_numpy(x).to(dev)
    out = torch.empty((p, offsets(mode, n, k)[1]), dtype=torch.float32, device=dev)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert L.load().xrfthip_exec(plan._h, C.c_void_p(xd.data_ptr()), C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(0), C.c_void_p(0), 0, C.c_void_p(0)) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run(plan, x))


# ---------------------------------------------------------------------------------- API level (both libraries)
def filter_plans():
    return [p for p in api._plan_cache.values() if getattr(p, "seg_filter", 0)]


# name -> (shape, dims, K, nfft, "fused" | "arranged" | None (composes), dtype)
API_CASES = {
    "trailing-default-nfft": ((3, 1000), ("x", "time"), 31, None, "fused", "float32"),
    "trailing-nfft-256": ((3, 1000), ("x", "time"), 65, 256, "fused", "float32"),
    "leading-time-cube": ((700, 3, 5), ("time", "y", "x"), 17, None, "arranged", "float32"),
    "nfft-100": ((3, 500), ("x", "time"), 9, 100, None, "float32"),
    "long-taps": ((2, 700), ("x", "time"), 150, 256, None, "float32"),
    "float64": ((3, 1000), ("x", "time"), 31, None, None, "float64"),
}


def series_first(values, ax):
    v = np.moveaxis(np.asarray(values), ax, -1)
    return v.reshape(-1, v.shape[-1])


def api_array(shape, dims, dtype, seed):
    rng = np.random.default_rng(seed)
    ax = dims.index("time")
    shp = [1] * len(shape)
    shp[ax] = shape[ax]
    v = rng.standard_normal(shape) + 0.01 * np.arange(shape[ax]).reshape(shp) + 1.0
    t = torch.from_numpy(v).to({"float32": torch.float32, "float64": torch.float64}[dtype])
    crd = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    crd["time"] = 3.0 + np.arange(shape[ax]) * 0.5
    return xa.DataArray(t.to(L.device()), dims, crd, "field", {"units": "K"}), t.numpy(), crd


def check_api_case(name, mode):
    shape, dims, k, nfft, route, dtype = API_CASES[name]
    api.clear_plan_cache()
    api._MEAN_REFUSED.clear()
    da, vals, crd = api_array(shape, dims, dtype, seed=95)
    taps = taps_of("firwin", k)
    got = xa.fir_filter(da, "time", taps, mode, nfft=nfft)
    assert bool(filter_plans()) == (route is not None), [p.describe() for p in api._plan_cache.values()]
    l = SEG._fir_default_nfft(k, shape[dims.index("time")]) if nfft is None else nfft
    if route is not None:
        assert_filter_plan(filter_plans()[-1])
        assert filter_plans()[-1].nx == l and l & (l - 1) == 0 and 64 <= l <= 4096 and l >= 4 * (k - 1)
    ax = dims.index("time")
    n = shape[ax]
    a, n_out = offsets(mode, n, k)
    assert tuple(got.dims) == tuple(dims) and got.shape == tuple(n_out if d == "time" else s for d, s in zip(dims, shape))
    assert np.asarray(got.values).dtype == {"float32": np.float32, "float64": np.float64}[dtype]
    x = series_first(vals, ax)
    ref, bnd = model(x, taps, mode), the_bound(x, taps, l, a, n_out, dtype)
    g = series_first(got.values, ax)
    assert_within(f"fir_filter {name} {mode}", g, ref, bnd)
    if route is not None:  # the composed route of the same call, on the same build
        with B.env("XRFTHIP_FASTW_FILTER", 0):
            n0 = len(filter_plans())
            comp = xa.fir_filter(da, "time", taps, mode, nfft=nfft)
            assert len(filter_plans()) == n0
        B.compare_labelled(got, comp)
        assert_within(f"fir_filter {name} {mode} composed", series_first(comp.values, ax), ref, bnd)
    return got


def check_api_labels():
    """Dims, coordinates, name and attrs in the three modes, K even and odd; a dim without a coordinate; a descending coordinate; an uneven one."""
    import pytest

    api.clear_plan_cache()
    da, _, crd = api_array((4, 300, 5), ("y", "time", "x"), "float32", seed=96)
    t = crd["time"]
    for k in (8, 9):
        taps = taps_of("normal", k)
        for mode in MODES:
            got = xa.fir_filter(da, "time", taps, mode)
            a, n_out = offsets(mode, 300, k)
            assert got.dims == ("y", "time", "x") and got.shape == (4, n_out, 5) and got.name == "field" and got.attrs == {"units": "K"}
            assert list(got.coords) == list(da.coords) and np.array_equal(got["y"].values, crd["y"]) and np.array_equal(got["x"].values, crd["x"])
            want = {"same": t, "valid": t[k // 2:k // 2 + 300 - k + 1], "full": t[0] + 0.5 * (np.arange(300 + k - 1) - (k - 1) // 2)}[mode]
            assert got["time"].values.shape == (n_out,) and np.allclose(got["time"].values, want, rtol=1e-12, atol=1e-12), (k, mode)
    bare = xa.DataArray(da.data, da.dims, {d: v for d, v in crd.items() if d != "time"})
    for mode in MODES:
        assert "time" not in xa.fir_filter(bare, "time", taps, mode).coords
    down = xa.DataArray(da.data, da.dims, dict(crd, time=t[::-1].copy()))
    full = xa.fir_filter(down, "time", taps, "full")
    assert np.allclose(np.diff(full["time"].values), -0.5) and full["time"].values[(9 - 1) // 2] == t[-1]
    uneven = xa.DataArray(da.data, da.dims, dict(crd, time=np.cumsum(1.0 + (np.arange(300) % 2))))
    assert xa.fir_filter(uneven, "time", taps, "same")["time"].values.shape == (300,)
    with pytest.raises(ValueError):
        xa.fir_filter(uneven, "time", taps, "full")


def check_api_refusal_is_remembered():
    """nfft = 100: the library declines once (XRFTHIP_UNSUPPORTED_LENGTH); the second call composes without building a plan with seg_filter.  float64, taps longer
    than L / 2 + 1 and the knob: never asked."""
    api.clear_plan_cache()
    api._MEAN_REFUSED.clear()
    made = []
    real = engine.SpectralPlan

    class Counting(real):
        def __init__(self, *a, **kw):
            if kw.get("seg_filter"):
                made.append(kw)
            super().__init__(*a, **kw)

    engine.SpectralPlan = Counting
    try:
        da, _, _ = api_array((3, 500), ("x", "time"), "float32", seed=97)
        taps = taps_of("firwin", 9)
        refused = len(api._MEAN_REFUSED)
        first = xa.fir_filter(da, "time", taps, nfft=100)
        assert len(made) == 1 and len(api._MEAN_REFUSED) == refused + 1 and not filter_plans()
        second = xa.fir_filter(da, "time", taps, nfft=100)
        assert len(made) == 1 and np.array_equal(first.values, second.values)
        d64, _, _ = api_array((3, 500), ("x", "time"), "float64", seed=97)
        xa.fir_filter(d64, "time", taps)
        xa.fir_filter(da, "time", taps_of("firwin", 40), nfft=64)
        with B.env("XRFTHIP_FASTW_FILTER", 0):
            xa.fir_filter(da, "time", taps)
        assert len(made) == 1
        xa.fir_filter(da, "time", taps)
        assert len(made) == 2 and filter_plans()
    finally:
        engine.SpectralPlan = real


def check_api_errors():
    import pytest

    da, _, _ = api_array((3, 60), ("x", "time"), "float32", seed=98)
    taps = taps_of("firwin", 9)
    for args, kw in (((da, "time", taps.astype(np.complex128)), {}), ((da, "time", []), {}), ((da, "time", taps.reshape(3, 3)), {}), ((da, "time", taps, "reflect"), {}),
                     ((da, ["time"], taps), {}), ((da, ("x", "time"), taps), {}), ((da, "time", taps), dict(nfft=8)), ((da, "time", taps_of("normal", 61), "valid"), {}),
                     ((da, "nowhere", taps), {})):
        with pytest.raises(ValueError):
            xa.fir_filter(*args, **kw)
    assert xa.fir_filter(da, "time", taps_of("normal", 60), "valid").shape == (3, 1)
    assert xa.fir_filter(da, "time", list(taps)).shape == (3, 60) and xa.fir_filter(da, "time", taps_of("normal", 61), "full").shape == (3, 120)


def check_default_nfft():
    """The default segment length: the smallest power of two >= max(512, 4 (K - 1)), capped at 4096 -- K = 2049 included, the longest taps the one pass takes
    (K - 1 = L / 2 at 4096) --, shorter where one shorter segment holds the series whole; longer taps compose at the smallest power of two >= 2 (K - 1).  A default
    call with 2049 taps builds a filter plan of 4096-sample segments and stays within the bound."""
    rule = SEG._fir_default_nfft
    assert [rule(k) for k in (1, 2, 17, 65, 129, 130, 257, 513, 1025, 2049)] == [512, 512, 512, 512, 512, 1024, 1024, 2048, 4096, 4096]
    assert rule(2049, 4194304) == 4096 and rule(2049, 10) == 4096 and rule(2050) == 8192 and rule(4097) == 8192 and rule(4098) == 16384
    assert rule(9, 100) == 128 and rule(9, 20) == 64 and rule(17, 700) == 512 and rule(17, 240) == 256 and rule(65, 10) == 256
    api.clear_plan_cache()
    api._MEAN_REFUSED.clear()
    x = series((4096, 2049, 9000, 2))
    taps = taps_of("firwin", 2049)
    da = xa.DataArray(torch.from_numpy(x).to(L.device()), ("x", "time"), {"x": np.arange(2) * 1.0, "time": np.arange(9000) * 0.5})
    got = xa.fir_filter(da, "time", taps)
    assert filter_plans() and filter_plans()[-1].nx == 4096 and filter_plans()[-1].seg_hop == 2048
    assert_filter_plan(filter_plans()[-1])
    a, n_out = offsets("same", 9000, 2049)
    assert_within("fir_filter K = 2049 at the default nfft", np.asarray(got.values), model(x, taps, "same"), the_bound(x, taps, 4096, a, n_out))


def check_api_sliced_view():
    """A view sliced along the trailing dim is read where it lies -- the plan carries the batch pitch -- and returns the bits of its contiguous copy; so does a
    slice of the leading dim; an empty array returns an empty one."""
    api.clear_plan_cache()
    da, _, crd = api_array((3, 1000), ("x", "time"), "float32", seed=94)
    taps = taps_of("firwin", 31)
    view = da.data[:, 50:950]
    assert not view.is_contiguous()
    sub = {"x": crd["x"], "time": crd["time"][50:950]}
    got = xa.fir_filter(xa.DataArray(view, da.dims, sub), "time", taps)
    assert filter_plans() and filter_plans()[-1].in_stride_batch == 1000 and filter_plans()[-1].seg_in_len == 900
    want = xa.fir_filter(xa.DataArray(view.contiguous(), da.dims, sub), "time", taps)
    assert np.array_equal(got.values, want.values)
    rows = xa.fir_filter(xa.DataArray(da.data[1:], da.dims, dict(crd, x=crd["x"][1:])), "time", taps)
    assert np.array_equal(rows.values, xa.fir_filter(da, "time", taps).values[1:])
    empty = xa.fir_filter(xa.DataArray(da.data[:0], da.dims, dict(crd, x=crd["x"][:0])), "time", taps, "full")
    assert empty.shape == (0, 1030)


def check_other_dtypes():
    """complex data run as two real calls; half precision is widened: both within the float32 bound of their parts."""
    da, vals, _ = api_array((3, 400), ("x", "time"), "float32", seed=99)
    taps = taps_of("firwin", 17)
    l = SEG._fir_default_nfft(17, 400)
    z = torch.complex(da.data, torch.flip(da.data, dims=(0,)))
    got = xa.fir_filter(xa.DataArray(z, da.dims, da.coords), "time", taps)
    assert np.asarray(got.values).dtype == np.complex64
    a, n_out = offsets("same", 400, 17)
    assert_within("complex data, real part", np.asarray(got.values).real, model(vals, taps, "same"), the_bound(vals, taps, l, a, n_out))
    assert_within("complex data, imaginary part", np.asarray(got.values).imag, model(vals[::-1], taps, "same"), the_bound(vals, taps, l, a, n_out))
    half = da.data.to(torch.float16)
    gh = xa.fir_filter(xa.DataArray(half, da.dims, da.coords), "time", taps)
    xh = half.cpu().to(torch.float64).numpy()
    assert np.asarray(gh.values).dtype == np.float32
    assert_within("float16 data", np.asarray(gh.values), model(xh, taps, "same"), the_bound(xh, taps, l, a, n_out))
