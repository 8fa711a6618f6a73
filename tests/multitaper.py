"""Shared by the tests of multitaper spectra (xrfthip_desc.seg_tapers, csrc/fastt.h; xrft_amd.multitaper_*; tests/test_multitaper_emulated.py on the emulated
library, tests/test_gpu_multitaper.py on the MI355X): the plan-level cases, their series, the float64 reference, the bound.  Not a conftest: imported by the tests.

The reference is float64 numpy on the float64 image of the same float32 samples: scipy.signal.windows.dpss(N, NW, K, return_ratios=True), numpy's detrend over the N
samples, np.fft.fft(d * y, L) and S[k] = scale sum_j w_j |X_j[k]|^2 (cross: sum_j w_j X0_j conj(X1_j), times the phase table).  The bound is the contract of one
mean spectrum, tests/batch_mean.py::bound(1, L, kappa) -- a relative L2 error per output (per series); a cross spectrum's is taken against the weighted mean of the
terms' magnitudes; kappa = max |x| / rms(x - fit) over the N samples of the series, 0 without a detrend.

Every series carries its own amplitude (x1, x3, x9, x27, then again): a sum into the wrong series misses the bound."""
import ctypes as C

import numpy as np
import torch

from xrft_amd import _lib as L
from xrft_amd import api, engine

import accuracy as A
import batch_mean as B

U32 = A.U["float32"]
FORMS = ["plain", "constant", "linear-shift"]
# (L, N, K, P): one taper (a half-empty pair); zero padding, odd K, three series in one tile; K at its cap, NS = 4, a last workgroup with one live series; more
# workgroups than CUs; ...; two rounds; three rounds, the last half empty; sixteen rounds, the longest float32 chain
CASES = [(64, 64, 1, 1), (64, 50, 3, 3), (64, 64, 32, 5), (256, 250, 7, 300), (1024, 1000, 7, 2), (2048, 2048, 8, 2), (4096, 3000, 5, 2), (4096, 4096, 32, 1)]
CROSS_CASES = [(64, 50, 3, 3), (256, 250, 7, 300), (4096, 3000, 5, 2)]
HALF_CASES = [(64, 50, 3, 3), (1024, 1000, 7, 2)]
ALONE_CASES = [(64, 64, 32, 5), (256, 250, 7, 300)]
CROSS_LAG = 7.0  # origin of the second series' coordinate: the net true-phase factor is not 1


def case_id(c):
    return f"L{c[0]}-N{c[1]}-K{c[2]}-P{c[3]}"


def nw_of(k):
    return max(4.0, 0.5 * (k + 1))  # (K <= 2 NW - 1: every taper well concentrated)


_TAPERS = {}


def tapers(case, weights="unity"):
    """(d [K][N] float64 from scipy, w [K])."""
    from scipy.signal.windows import dpss

    l, n, k, p = case
    key = (n, k)
    if key not in _TAPERS:
        d, lam = dpss(n, nw_of(k), k, return_ratios=True)
        _TAPERS[key] = (np.atleast_2d(d), np.atleast_1d(lam))
    d, lam = _TAPERS[key]
    return d, (np.full(k, 1.0 / k) if weights == "unity" else lam / lam.sum())


def table(case, weights="unity"):
    d, w = tapers(case, weights)
    return (np.sqrt(w).reshape(-1, 1) * d).astype(np.float32)


def series(case, seed=61, pitch=None):
    """[P][pitch] float32 (pitch >= N; default N): seeded noise over a line, series p scaled by 3^(p mod 4)."""
    l, n, k, p = case
    m = n if pitch is None else pitch
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((p, m)) + 0.01 * np.arange(m) + 1.5
    v *= (3.0 ** (np.arange(p) % 4)).reshape(p, 1)
    return v.astype(np.float32)


def second_series(x, seed=62):
    rng = np.random.default_rng(seed)
    amp = np.abs(x).mean(axis=1).reshape(-1, 1)
    return (np.roll(x, 5, axis=1) + 0.1 * amp * rng.standard_normal(x.shape)).astype(np.float32)


def form_kw(form):
    if form == "plain":
        return dict(detrend=L.DETREND_NONE, flags=0)
    if form == "constant":
        return dict(detrend=L.DETREND_CONSTANT, flags=0)
    return dict(detrend=L.DETREND_LINEAR, flags=L.SHIFT_X)


def phase_table(l, lag):
    f = np.fft.fftfreq(l, 1.0)
    return np.exp(-2j * np.pi * f * api._lag_coord(np.arange(l) * 1.0)) * np.conj(np.exp(-2j * np.pi * f * api._lag_coord(lag + np.arange(l) * 1.0)))


def make_plan(case, form="plain", mode=L.OUT_POWER, pitch=0, lag=None, weights="unity", batch=None, tab=True, **over):
    l, n, k, p = case
    kw = dict(ndim=1, batch=p if batch is None else batch, ny=1, nx=l, dtype=torch.float32, out_mode=mode, scale=1.0, in_stride_batch=pitch, seg_tapers=k, seg_taper_len=n,
              tapers=table(case, weights) if tab else None, **form_kw(form))
    if mode == L.OUT_CROSS and lag is not None:  # true phase: both series ifftshifted, the net factor phase0 * conj(phase1) per unshifted frequency
        kw["flags"] |= L.ISHIFT_X
        kw["phase_x"] = phase_table(l, lag)
    kw.update(over)
    return engine.SpectralPlan(**kw)


def run(plan, x0, x1=None):
    dev = L.device()
    t0 = torch.from_numpy(np.ascontiguousarray(x0)).to(dev)
    t1 = None if x1 is None else torch.from_numpy(np.ascontiguousarray(x1)).to(dev)
    out, _ = plan.execute(t0, t1)
    return out.cpu().numpy().reshape(out.shape[0], -1)


def detrended(x, kind, over=None):
    """numpy's detrend of [P][N] float64 over its N samples (``over`` = L: the WRONG detrend, over the zero-extended series -- the checker's own test)."""
    x = np.asarray(x, dtype=np.float64)
    if over is not None:
        x = np.concatenate([x, np.zeros((x.shape[0], over - x.shape[1]))], axis=1)
    y = A.detrended(x, (1,), kind)
    return y


def reference(case, form, x0, x1=None, lag=None, half=0, weights="unity", drop_last=False, detrend_over_l=False, shift_second=False):
    """(S, the weighted mean of the terms' magnitudes), float64.  half: 1 = k <= L / 2 of the unshifted spectrum, 2 = with the real-dim factor.  The last three
    arguments build the WRONG references of check_the_checker_bites."""
    l, n, k, p = case
    d, w = tapers(case, weights)
    if shift_second:
        d = d.copy()
        d[1] = np.roll(d[1], 1)
    if drop_last:
        d, w = d[:-1], w[:-1]
    kind = form_kw(form)["detrend"]

    def spectra(x):
        y = detrended(x, kind, l if detrend_over_l else None)[:, :n]
        return np.fft.fft(d[None] * y[:, None, :], l)  # [P][K][L]

    xa_ = spectra(x0)
    if x1 is None:
        terms = np.abs(xa_) ** 2
    else:
        terms = xa_ * np.conj(spectra(x1))
    s = (w.reshape(1, -1, 1) * terms).sum(axis=1)
    mag = (w.reshape(1, -1, 1) * np.abs(terms)).sum(axis=1)
    if x1 is not None and lag is not None:
        s = s * phase_table(l, lag)
    if half:
        s, mag = s[:, :l // 2 + 1].copy(), mag[:, :l // 2 + 1].copy()
        if half == 2:
            s[:, 1:(l + 1) // 2] *= 2
            mag[:, 1:(l + 1) // 2] *= 2
    elif form_kw(form)["flags"] & L.SHIFT_X:
        s, mag = np.fft.fftshift(s, axes=-1), np.fft.fftshift(mag, axes=-1)
    return s, mag


def kappa(case, form, x):
    """max |x| / rms(x - fit) over the N samples of each series (0 without a detrend)."""
    kind = form_kw(form)["detrend"]
    if kind == L.DETREND_NONE:
        return [0.0] * x.shape[0]
    x = np.asarray(x, dtype=np.float64)[:, :case[1]]
    return [A.kappa(s, A.detrended(s.reshape(1, -1), (1,), kind)) for s in x]


def bound(l, kap):
    return B.bound(1, l, kap)


def errors(case, got, ref, mag, kaps):
    return [(B.rel_error(got[i], ref[i], None if mag is None else mag[i]), bound(case[0], kaps[i]), i) for i in range(ref.shape[0])]


def assert_outputs(case, got, ref, mag, kaps, what):
    """Every series within the bound, each against its own reference; finite; prints each figure before it asserts (the worst only for many series)."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rows = errors(case, got, ref, mag, kaps)
    for err, bnd, i in (rows if len(rows) <= 5 else [max(rows, key=lambda r: r[0] / r[1])]):
        print(f"{what} series {i}: error {err:.3e} bound {bnd:.3e}")
    assert np.isfinite(got).all(), what
    for err, bnd, i in rows:
        assert err <= bnd, f"{what} series {i}: error {err:.3e} > {bnd:.3e}"


def is_taper_plan(plan):
    return plan.kernel_info()[0] == L.K_FASTW and "[fastw tapers]" in plan.describe() and plan.workspace_bytes == 0


def check_plan(case, form, mode=L.OUT_POWER, lag=None, half=0, weights="unity"):
    l, n, k, p = case
    x0 = series(case)
    x1 = second_series(x0) if mode == L.OUT_CROSS else None
    over = {}
    if half:
        over["flags"] = (form_kw(form)["flags"] & ~L.SHIFT_X) | L.HALF_X | (L.REALDIM_X2 if half == 2 else 0)
    plan = make_plan(case, form, mode, lag=lag, weights=weights, **over)
    assert is_taper_plan(plan), plan.describe()
    got = run(plan, x0, x1)
    nxo = l // 2 + 1 if half else l
    assert got.shape == (p, nxo) and got.dtype == (np.complex64 if mode == L.OUT_CROSS else np.float32)
    ref, mag = reference(case, form, x0, x1, lag, half, weights)
    kaps = kappa(case, form, x0)
    if x1 is not None:
        kaps = [max(a, b) for a, b in zip(kaps, kappa(case, form, x1))]
    assert_outputs(case, got, ref, mag if x1 is not None else None, kaps, f"{'cross' if x1 is not None else 'power'} {case_id(case)} {form} half={half} {weights}")
    assert np.array_equal(got, run(plan, x0, x1))  # every addition in an order the plan fixes: the same bits
    return plan, got


def check_every_series_alone(case, form="linear-shift"):
    """Every series of the batch equals the series run alone (a plan of one series), bit for bit: its bits depend on its own samples only, not on its place in a tile."""
    l, n, k, p = case
    x = series(case)
    got = run(make_plan(case, form), x)
    one = make_plan(case, form, batch=1)
    for i in range(p):
        assert np.array_equal(run(one, x[i:i + 1])[0], got[i]), i
    x1 = second_series(x)
    gotc = run(make_plan(case, form, L.OUT_CROSS, lag=CROSS_LAG), x, x1)
    onec = make_plan(case, form, L.OUT_CROSS, lag=CROSS_LAG, batch=1)
    for i in sorted({0, 1, p // 2, p - 1}):
        assert np.array_equal(run(onec, x[i:i + 1], x1[i:i + 1])[0], gotc[i]), i


def check_ishift_changes_no_bit(case):
    x0 = series(case)
    x1 = second_series(x0)
    for mode, b in ((L.OUT_POWER, None), (L.OUT_CROSS, x1)):
        a = run(make_plan(case, "linear-shift", mode), x0, b)
        c = run(make_plan(case, "linear-shift", mode, flags=form_kw("linear-shift")["flags"] | L.ISHIFT_X), x0, b)
        assert np.array_equal(a, c), mode


def check_nan(case, form="linear-shift"):
    """A NaN in one series of a shared tile leaves every other output's bits unchanged and makes its own non-finite."""
    l, n, k, p = case
    assert p == 3 and l == 64
    x = series(case)
    plan = make_plan(case, form)
    clean = run(plan, x)
    xn = x.copy()
    xn[1, n // 2] = np.nan
    got = run(plan, xn)
    assert not np.isfinite(got[1]).any(), "series 1 has finite outputs"
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    x1 = second_series(x)
    planc = make_plan(case, form, L.OUT_CROSS, lag=CROSS_LAG)
    cleanc = run(planc, x, x1)
    gotc = run(planc, x, np.where(np.isnan(xn), np.inf, x1).astype(np.float32))
    assert not (np.isfinite(gotc[1].real) | np.isfinite(gotc[1].imag)).any()
    assert np.array_equal(gotc[0], cleanc[0]) and np.array_equal(gotc[2], cleanc[2])


def check_pitch_and_pointer(case, form="linear-shift"):
    """A pitch beyond N (odd: the series start on 4-byte boundaries only), the samples in the gap NaN: they must not reach the result; and a view that starts one
    sample into a larger buffer (a pointer on a 4-byte boundary only)."""
    l, n, k, p = case
    pitch = n + 5
    x = series(case, pitch=pitch)
    dense = np.ascontiguousarray(x[:, :n])
    x[:, n:] = np.nan
    want = run(make_plan(case, form), dense)
    dev = L.device()
    full = torch.from_numpy(x).to(dev)
    out, _ = make_plan(case, form, pitch=pitch).execute(full[:, :n])
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, want)
    buf = torch.full((p * pitch + 1,), float("nan"), dtype=torch.float32, device=dev)
    view = buf[1:].reshape(p, pitch)
    view[:, :n] = torch.from_numpy(dense).to(dev)
    assert view.data_ptr() % 16 == 4
    out, _ = make_plan(case, form, pitch=pitch).execute(view[:, :n])
    assert np.array_equal(out.cpu().numpy(), want)


def _status(**kw):
    base = dict(ndim=1, batch=6, ny=1, nx=256, dtype=torch.float32, out_mode=L.OUT_POWER, seg_tapers=7, seg_taper_len=250)
    base.update(kw)
    try:
        engine.SpectralPlan(**base)
    except L.XrftHipError as e:
        return e.status
    return 0


def check_status_codes():
    assert _status() == 0 and _status(out_mode=L.OUT_CROSS) == 0 and _status(seg_taper_len=256) == 0 and _status(seg_taper_len=1) == 0 and _status(seg_tapers=32) == 0
    assert _status(mean_batch=1) == 0 and _status(inner=1) == 0 and _status(in_stride_batch=250) == 0 and _status(in_stride_batch=251) == 0 and _status(batch=0) == 0
    for fl in (L.SHIFT_X, L.ISHIFT_X, L.HALF_X, L.HALF_X | L.REALDIM_X2, L.SHIFT_X | L.ISHIFT_X):
        assert _status(flags=fl) == 0, fl
    for det in (L.DETREND_NONE, L.DETREND_CONSTANT, L.DETREND_LINEAR):
        assert _status(detrend=det) == 0
    bad = [dict(seg_tapers=-1), dict(seg_taper_len=0), dict(seg_taper_len=257), dict(seg_tapers=0), dict(seg_hop=128), dict(seg_hop=128, mean_batch=3), dict(seg_keep=1),
           dict(seg_stride=4), dict(seg_synth=1), dict(seg_filter=1), dict(seg_lead=1), dict(seg_in_len=5), dict(seg_out_len=5), dict(ndim=2, ny=4), dict(inner=4), dict(mid=4),
           dict(herm_ny=4, herm_nx=4), dict(flags=L.ISO), dict(flags=L.INVERSE), dict(in_stride_y=512), dict(mean_batch=2), dict(mean_batch=3), dict(out_mode=L.OUT_COMPLEX),
           dict(out_mode=L.OUT_PHASE), dict(out_mode=L.OUT_COHERENCE), dict(in_stride_batch=249), dict(flags=L.HALF_X | L.SHIFT_X), dict(flags=L.REALDIM_X2), dict(detrend=3),
           dict(dtype=torch.float64), dict(dtype=torch.complex64), dict(dtype=torch.float16), dict(flags=L.FLIP0_X), dict(window_x=np.ones(256))]
    for kw in bad:
        assert _status(**kw) == L.BAD_ARG, kw
    composes = [dict(nx=96, seg_taper_len=90), dict(nx=32, seg_taper_len=32), dict(nx=8192), dict(seg_tapers=33), dict(flags=L.FLIP_X), dict(out_mode=L.OUT_CROSS, flags=L.FLIP0_X)]
    for kw in composes:
        assert _status(**kw) == L.UNSUPPORTED_LENGTH, kw
    for knob in ("XRFTHIP_FASTW_TAPERS", "XRFTHIP_FASTW"):
        with B.env(knob, 0):
            assert _status() == L.UNSUPPORTED_LENGTH, knob
    # the table: only a multitaper plan takes one; executing without it is XRFTHIP_BAD_ARG
    dll = L.load()
    plain = engine.SpectralPlan(ndim=1, batch=2, ny=1, nx=256, dtype=torch.float32, out_mode=L.OUT_POWER)
    tab = np.zeros((7, 250), dtype=np.float32)
    assert dll.xrfthip_plan_set_tapers(plain._h, tab.ctypes.data_as(C.c_void_p)) == L.BAD_ARG
    assert dll.xrfthip_plan_set_tapers(None, tab.ctypes.data_as(C.c_void_p)) == L.BAD_ARG
    case = (256, 250, 7, 2)
    bare = make_plan(case, tab=False)
    assert "NO TABLE" in bare.describe()
    try:
        run(bare, series(case))
        raise AssertionError("executed without a taper table")
    except L.XrftHipError as e:
        assert e.status == L.BAD_ARG
    assert dll.xrfthip_plan_set_tapers(bare._h, table(case).ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(run(bare, series(case)), run(make_plan(case), series(case)))
    assert dll.xrfthip_plan_set_tapers(bare._h, None) == 0 and "NO TABLE" in bare.describe()


def check_struct_sizes():
    """Every struct_size the descriptor ever had is accepted (the words a shorter one lacks count as 0); seg_tapers and seg_taper_len came together: the size between
    the two and a larger one are XRFTHIP_BAD_ARG; a DescFilt-sized descriptor with garbage behind it is read without the two words."""
    dll = L.load()
    D = L.DescTaper
    sizes = [getattr(D, f).offset for f in ("inner", "mid", "in_stride_y", "herm_ny", "mean_batch", "seg_hop", "seg_stride", "seg_keep", "seg_synth", "seg_filter", "seg_tapers")] + [C.sizeof(D)]
    assert len(sizes) == 12 and sizes == sorted(set(sizes)) and sizes[-1] - sizes[-2] == 16 and sizes[-2] == C.sizeof(L.DescFilt) and sizes[-3] == C.sizeof(L.DescSynth)
    assert [f[0] for f in D._fields_[:len(L.DescFilt._fields_)]] == [f[0] for f in L.DescFilt._fields_] and [f[0] for f in D._fields_[-2:]] == ["seg_tapers", "seg_taper_len"]
    h = C.c_void_p(0)
    zeros = (0,) * 23
    for sz in sizes:
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *zeros)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0, sz
        dll.xrfthip_plan_destroy(h)
    for sz in (sizes[-2] + 8, sizes[-1] + 8):
        d = D(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, *zeros)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG, sz

    def taper(sz, k, n):
        return D(sz, 1, 3, 1, 256, L.F32, L.OUT_POWER, 0, 0, 1.0, *((0,) * 21), k, n)

    buf = C.create_string_buffer(8192)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(taper(sizes[-1], 7, 250))) == 0
    dll.xrfthip_plan_describe(h, buf, len(buf))
    assert b"[fastw tapers]" in buf.value
    dll.xrfthip_plan_destroy(h)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(taper(sizes[-2], 7, 250))) == 0  # (the words are read only from a descriptor that has them: the plain 1-D plan)
    dll.xrfthip_plan_describe(h, buf, len(buf))
    assert b"[fastw tapers]" not in buf.value
    dll.xrfthip_plan_destroy(h)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(taper(sizes[-1], 0, 250))) == L.BAD_ARG


# ---------------------------------------------------------------------------------- the checker bites (numpy and scipy only)
def check_the_checker_bites():
    """The comparison of assert_outputs holds the float32 image of the right reference far inside the bound and misses it for a reference built with K - 1 tapers, with
    the detrend taken over L instead of N, and with the pair's second taper shifted by one sample."""
    for case, form in (((64, 50, 3, 3), "constant"), ((256, 250, 7, 4), "linear-shift"), ((1024, 1000, 7, 2), "constant")):
        x = series(case)
        ref, _ = reference(case, form, x)
        got = ref.astype(np.float32)
        kaps = kappa(case, form, x)
        for err, bnd, i in errors(case, got, ref, None, kaps):
            assert err <= 0.1 * bnd, (case, i, err, bnd)
        for wrong in (dict(drop_last=True), dict(detrend_over_l=True), dict(shift_second=True)):
            bad, _ = reference(case, form, x, **wrong)
            for err, bnd, i in errors(case, got, bad, None, kaps):
                print(f"{case_id(case)} {form} {wrong} series {i}: error {err:.3e} bound {bnd:.3e}")
                assert err > bnd, (case, wrong, i, err, bnd)


# ---------------------------------------------------------------------------------- API level (both libraries)
import xrft_amd as xa  # noqa: E402
from xrft_amd import _segments as S  # noqa: E402


def api_series(shape, dims, dtype, seed, tdim="time", dt=0.5, t0=2.0):
    """(the product's array, the float64 image of its samples, its coordinates)."""
    rng = np.random.default_rng(seed)
    n = shape[dims.index(tdim)]
    shp = [1] * len(shape)
    shp[dims.index(tdim)] = n
    v = rng.standard_normal(shape) + 0.01 * np.arange(n).reshape(shp) + 1.0
    t = torch.from_numpy(v).to({"float32": torch.float32, "float64": torch.float64}[dtype])
    crd = {d: np.arange(k) * 1.0 for d, k in zip(dims, shape)}
    crd[tdim] = t0 + np.arange(n) * dt
    return xa.DataArray(t.to(L.device()), dims, crd), t.to(torch.float64).numpy(), crd


def definition(wide, ax, dt, nw, k, l, weights="unity", detrend=None, real_dim=False, shift=True, wide2=None):
    """S[k] = dt sum_j w_j |sum_n d_j[n] y[n] e^{-2 pi i k n / L}|^2 from scipy's tapers and numpy, ``dim`` last (cross: X1 conj X2, no phase factor)."""
    from scipy.signal.windows import dpss

    kind = {None: L.DETREND_NONE, "constant": L.DETREND_CONSTANT, "linear": L.DETREND_LINEAR}[detrend]
    n = wide.shape[ax]
    d, lam = dpss(n, nw, k, return_ratios=True)
    d, lam = np.atleast_2d(d), np.atleast_1d(lam)
    w = np.full(k, 1.0 / k) if weights == "unity" else lam / lam.sum()

    def spectra(v):
        y = np.moveaxis(np.asarray(v, dtype=np.float64), ax, -1)
        y = A.detrended(y, (y.ndim - 1,), kind)
        return np.fft.fft(d * y[..., None, :], l)

    x = spectra(wide)
    terms = np.abs(x) ** 2 if wide2 is None else x * np.conj(spectra(wide2))
    s = dt * (w.reshape(-1, 1) * terms).sum(axis=-2)
    mag = dt * (w.reshape(-1, 1) * np.abs(terms)).sum(axis=-2)
    if real_dim:
        s, mag = s[..., :l // 2 + 1].copy(), mag[..., :l // 2 + 1].copy()
        s[..., 1:(l + 1) // 2] *= 2
        mag[..., 1:(l + 1) // 2] *= 2
    elif shift:
        s, mag = np.fft.fftshift(s, axes=-1), np.fft.fftshift(mag, axes=-1)
    return s, mag


def api_bound(dtype, l, series_, detrend):
    kap = 0.0
    if detrend:
        s = series_.reshape(-1, series_.shape[-1])
        kap = A.kappa(s, A.detrended(s, (1,), L.DETREND_LINEAR if detrend == "linear" else L.DETREND_CONSTANT))
    return A.bound(dtype, l, kap) + 16.0 * A.U[dtype]


def taper_plans():
    return [p for p in api._plan_cache.values() if getattr(p, "seg_tapers", 0)]


def composed(fn, *a, **kw):
    with B.env("XRFTHIP_FASTW_TAPERS", 0):
        return fn(*a, **kw)


# name -> (shape, dims, dtype, keyword arguments, the transform length, fused?)
API_CASES = {
    "trailing-250": ((3, 250), ("x", "time"), "float32", dict(detrend="linear"), 256, True),
    "real-dim-eigen": ((2, 3, 100), ("y", "x", "time"), "float32", dict(detrend="constant", real_dim="time", weights="eigen", NW=3.0, K=4), 128, True),
    "unshifted-nfft-512": ((3, 250), ("x", "time"), "float32", dict(shift=False, nfft=512), 512, True),
    "leading-time": ((300, 3), ("time", "x"), "float32", dict(detrend="linear", NW=2.5), 512, True),  # (arranged first, then fused)
    "float64": ((3, 250), ("x", "time"), "float64", dict(detrend="linear"), 256, False),
    "nfft-96": ((3, 90), ("x", "time"), "float32", dict(detrend="linear", nfft=96), 96, False),
    "K-40": ((2, 250), ("x", "time"), "float32", dict(detrend="constant", NW=20.5, K=40), 256, False),
}


def check_api_case(name):
    shape, dims, dtype, kw, l, fused = API_CASES[name]
    api.clear_plan_cache()
    da, wide, crd = api_series(shape, dims, dtype, seed=71)
    got = xa.multitaper_power_spectrum(da, "time", **kw)
    assert bool(taper_plans()) == fused, [p.describe() for p in api._plan_cache.values()]
    if fused:
        assert is_taper_plan(taper_plans()[-1])
    want = composed(xa.multitaper_power_spectrum, da, "time", **kw)
    B.compare_labelled(got, want)
    ax = dims.index("time")
    nw, k = kw.get("NW", 4.0), kw.get("K", int(2 * kw.get("NW", 4.0)) - 1)
    assert tuple(got.dims) == tuple(d for d in dims if d != "time") + ("freq_time",) and got.attrs == {"tapers": k}
    ref, _ = definition(wide, ax, 0.5, nw, k, l, kw.get("weights", "unity"), kw.get("detrend"), kw.get("real_dim") is not None, kw.get("shift", True))
    assert got.shape == ref.shape
    f = np.asarray(got.coords["freq_time"].values)
    assert np.allclose(f, np.fft.rfftfreq(l, 0.5) if kw.get("real_dim") else (np.fft.fftshift(np.fft.fftfreq(l, 0.5)) if kw.get("shift", True) else np.fft.fftfreq(l, 0.5)))
    bnd = api_bound(dtype, l, np.moveaxis(wide, ax, -1), kw.get("detrend"))
    flat = lambda v: np.asarray(v).reshape(-1, ref.shape[-1])  # noqa: E731
    for g, r in zip(flat(got.values), flat(ref)):
        err, errc = B.rel_error(g, r), None
        assert np.isfinite(g).all() and err <= bnd, (name, err, bnd)
    for g, r in zip(flat(want.values), flat(ref)):
        errc = B.rel_error(g, r)
        assert errc <= bnd, (name, errc, bnd)
    print(f"multitaper_power_spectrum {name}: last series error {err:.3e} composed {errc:.3e} bound {bnd:.3e} (fused: {fused})")


def check_api_cross_and_coherence():
    api.clear_plan_cache()
    shape, dims = (3, 250), ("x", "time")
    da, wide, crd = api_series(shape, dims, "float32", seed=72)
    rng = np.random.default_rng(73)
    w2 = (np.roll(wide, 5, axis=1) + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    crd2 = dict(crd, time=crd["time"] + 3.5)  # (another origin: the net true-phase factor is not 1)
    da2 = xa.DataArray(torch.from_numpy(w2).to(L.device()), dims, crd2)
    kw = dict(detrend="linear")
    got = xa.multitaper_cross_spectrum(da, da2, "time", **kw)
    assert taper_plans() and is_taper_plan(taper_plans()[-1])
    want = composed(xa.multitaper_cross_spectrum, da, da2, "time", **kw)
    B.compare_labelled(got, want)
    assert "direct_lag" in got.coords["freq_time"].attrs and got.values.dtype == np.complex64
    ref, mag = definition(wide, 1, 0.5, 4.0, 7, 256, detrend="linear", wide2=w2.astype(np.float64))
    f = np.fft.fftshift(np.fft.fftfreq(256, 0.5))
    lag0, lag1 = api._lag_coord(crd["time"][0] + 0.5 * np.arange(256)), api._lag_coord(crd2["time"][0] + 0.5 * np.arange(256))
    ref = ref * np.exp(-2j * np.pi * f * lag0) * np.conj(np.exp(-2j * np.pi * f * lag1))
    bnd = max(api_bound("float32", 256, wide, "linear"), api_bound("float32", 256, w2.astype(np.float64), "linear"))
    for i in range(3):
        err, errc = B.rel_error(got.values[i], ref[i], mag[i]), B.rel_error(want.values[i], ref[i], mag[i])
        print(f"multitaper_cross_spectrum series {i}: error {err:.3e} composed {errc:.3e} bound {bnd:.3e}")
        assert err <= bnd and errc <= bnd
    nophase = xa.multitaper_cross_spectrum(da, da2, "time", true_phase=False, **kw)
    ref0, mag0 = definition(wide, 1, 0.5, 4.0, 7, 256, detrend="linear", wide2=w2.astype(np.float64))
    assert all(B.rel_error(nophase.values[i], ref0[i], mag0[i]) <= bnd for i in range(3)) and "direct_lag" not in nophase.coords["freq_time"].attrs
    # the coherence: the library's division of the three spectra
    coh = xa.multitaper_coherence(da, da2, "time", **kw)
    p1, _ = definition(wide, 1, 0.5, 4.0, 7, 256, detrend="linear")
    p2, _ = definition(w2.astype(np.float64), 1, 0.5, 4.0, 7, 256, detrend="linear")
    cref = np.abs(ref) ** 2 / (p1 * p2)
    assert coh.dims == got.dims and coh.values.dtype == np.float32 and coh.attrs == {"tapers": 7}
    cerr = float(np.abs(coh.values - cref).max())
    print(f"multitaper_coherence: max error {cerr:.3e}")
    assert cerr <= 64 * U32  # (a quotient of three sums, each within a few u of values <= 1)
    assert coh.values.min() >= 0.0 and coh.values.max() <= 1.0 + 8 * U32
    wantc = composed(xa.multitaper_coherence, da, da2, "time", **kw)
    B.compare_labelled(coh, wantc)
    assert float(np.abs(wantc.values - cref).max()) <= 64 * U32


def check_float64_against_the_definition():
    api.clear_plan_cache()
    da, wide, _ = api_series((3, 250), ("x", "time"), "float64", seed=74)
    for kw in (dict(detrend="linear"), dict(detrend="constant", weights="eigen", real_dim="time"), dict(NW=2.5, nfft=300, shift=False)):
        got = xa.multitaper_power_spectrum(da, "time", **kw)
        nw = kw.get("NW", 4.0)
        ref, _ = definition(wide, 1, 0.5, nw, int(2 * nw) - 1, kw.get("nfft", 256), kw.get("weights", "unity"), kw.get("detrend"), "real_dim" in kw, kw.get("shift", True))
        err = float(np.abs(got.values - ref).max() / np.abs(ref).max())
        print(f"float64 {kw}: max error / max {err:.3e}")
        assert got.values.dtype == np.float64 and err <= 1e-12 and not taper_plans()


def check_parseval():
    """sum_k S[k] / (L dt) = sum_j w_j sum_n (d_j y)^2[n], fused and composed."""
    da, wide, _ = api_series((3, 250), ("x", "time"), "float32", seed=75)
    for weights in ("unity", "eigen"):
        d, lam = S._dpss(250, 4.0, 7)
        w = np.full(7, 1 / 7) if weights == "unity" else lam / lam.sum()
        y = A.detrended(wide, (1,), L.DETREND_CONSTANT)
        rhs = (w.reshape(1, -1, 1) * (d[None] * y[:, None, :]) ** 2).sum(axis=(1, 2))
        for route in (lambda *a, **k: xa.multitaper_power_spectrum(*a, **k), lambda *a, **k: composed(xa.multitaper_power_spectrum, *a, **k)):
            got = route(da, "time", detrend="constant", weights=weights)
            lhs = got.values.astype(np.float64).sum(axis=-1) / (256 * 0.5)
            assert np.allclose(lhs, rhs, rtol=64 * U32), (lhs, rhs)


def check_leading_dim_equals_trailing():
    api.clear_plan_cache()
    da, wide, crd = api_series((100, 3, 4), ("time", "y", "x"), "float32", seed=76)
    a = xa.multitaper_power_spectrum(da, "time", detrend="linear")
    assert taper_plans()
    tr = xa.DataArray(da.data.permute(1, 2, 0).contiguous(), ("y", "x", "time"), crd)
    b = xa.multitaper_power_spectrum(tr, "time", detrend="linear")
    assert a.dims == b.dims == ("y", "x", "freq_time") and np.array_equal(a.values, b.values)
    # a trailing dim with a pitch between the series is read where it lies: the same bits as the dense copy
    big, _, crdb = api_series((5, 300), ("x", "time"), "float32", seed=77)
    view = xa.DataArray(big.data[:, :250], ("x", "time"), dict(crdb, time=crdb["time"][:250]))
    dense = xa.DataArray(big.data[:, :250].contiguous(), ("x", "time"), dict(crdb, time=crdb["time"][:250]))
    api.clear_plan_cache()
    v = xa.multitaper_power_spectrum(view, "time")
    assert [p.in_stride_batch for p in taper_plans()] == [300]
    assert np.array_equal(v.values, xa.multitaper_power_spectrum(dense, "time").values)


def check_dpss_against_scipy():
    import pytest

    pytest.importorskip("scipy")
    from scipy.signal.windows import dpss

    for n, nw, k in ((50, 2.5, 4), (64, 4.0, 7), (1000, 4.0, 7), (64, 4.0, 1)):
        d, lam = S._dpss_compute(n, nw, k)
        ds, ls = dpss(n, nw, k, return_ratios=True)
        ds, ls = np.atleast_2d(ds), np.atleast_1d(ls)
        assert d.shape == (k, n) and np.abs(d - ds).max() <= 1e-10 and np.abs(lam - ls).max() <= 1e-10, (n, np.abs(d - ds).max())
        assert ((d * ds).sum(axis=1) > 0.99).all()  # (equal signs: every taper against scipy's, not against its negative)
        d2, lam2 = S._dpss_compute(n, nw, k, use_scipy=False)  # the numpy fallback
        assert np.abs(d2 - d).max() <= 1e-10 and np.abs(lam2 - lam).max() <= 1e-10, (n, np.abs(d2 - d).max())
    assert S._dpss(64, 4.0, 7)[0] is S._dpss(64, 4.0, 7)[0]  # (remembered)


def check_api_tapers_argument_and_half_precision():
    api.clear_plan_cache()
    da, wide, _ = api_series((3, 250), ("x", "time"), "float32", seed=78)
    d, _ = S._dpss(250, 4.0, 7)
    a = xa.multitaper_power_spectrum(da, "time")
    b = xa.multitaper_power_spectrum(da, "time", tapers=3.0 * np.array(d))  # (rows normalised: the same table)
    assert B.rel_error(b.values, a.values) <= 4 * U32 and b.attrs == {"tapers": 7}  # (the normalisation may move a float64 taper value by an ulp)
    one = xa.multitaper_power_spectrum(da, "time", tapers=np.hanning(250), detrend="constant")
    h = np.hanning(250) / np.sqrt((np.hanning(250) ** 2).sum())
    ref = 0.5 * np.abs(np.fft.fft(h * A.detrended(wide, (1,), L.DETREND_CONSTANT), 256)) ** 2
    assert one.attrs == {"tapers": 1} and B.rel_error(one.values, np.fft.fftshift(ref, axes=-1)) <= api_bound("float32", 256, wide, "constant")
    half = xa.DataArray(da.data.to(torch.bfloat16), da.dims, da.coords)
    g = xa.multitaper_power_spectrum(half, "time")
    w = xa.multitaper_power_spectrum(xa.DataArray(da.data.to(torch.bfloat16).to(torch.float32), da.dims, da.coords), "time")
    assert g.values.dtype == np.float32 and np.array_equal(g.values, w.values)


def check_api_refusal_is_remembered():
    """A descending coordinate under true_phase: the plan declines the flip (XRFTHIP_UNSUPPORTED_LENGTH), the refusal is remembered, the call composes."""
    from xrft_amd import _plans

    api.clear_plan_cache()
    da, wide, crd = api_series((2, 250), ("x", "time"), "float32", seed=79)
    crd = dict(crd, time=crd["time"][::-1].copy())
    d1 = xa.DataArray(da.data, da.dims, crd)
    d2 = xa.DataArray(torch.roll(da.data, 3, 1), da.dims, crd)
    before = len(_plans._MEAN_REFUSED)
    got = xa.multitaper_cross_spectrum(d1, d2, "time")
    assert not taper_plans() and len(_plans._MEAN_REFUSED) == before + 1
    again = xa.multitaper_cross_spectrum(d1, d2, "time")
    assert len(_plans._MEAN_REFUSED) == before + 1 and np.array_equal(got.values, again.values)
    want = composed(xa.multitaper_cross_spectrum, d1, d2, "time")
    B.compare_labelled(got, want)
    assert np.array_equal(got.values, want.values)


def check_api_errors():
    import pytest

    da, _, _ = api_series((3, 100), ("x", "time"), "float32", seed=80)
    for kw in (dict(K=0), dict(K=101), dict(nfft=99), dict(NW=0.0), dict(NW=51.0), dict(weights="adaptive"), dict(tapers=np.ones((2, 99))), dict(tapers=np.zeros((2, 100))),
               dict(tapers=np.ones((2, 100)), weights="eigen"), dict(tapers=np.ones((2, 100)) * 1j), dict(real_dim="x")):
        with pytest.raises(ValueError):
            xa.multitaper_power_spectrum(da, "time", **kw)
        with pytest.raises(ValueError):
            xa.multitaper_cross_spectrum(da, da, "time", **kw)
    with pytest.raises(ValueError):
        xa.multitaper_power_spectrum(da, "nope")
    with pytest.raises(ValueError):
        xa.multitaper_power_spectrum(da, ["time"])
    with pytest.raises(NotImplementedError):
        xa.multitaper_power_spectrum(da, "time", detrend="quadratic")
    with pytest.raises(ValueError):
        xa.multitaper_coherence(da, da, "time", K=1)
    with pytest.raises(ValueError):
        xa.multitaper_cross_spectrum(da, xa.DataArray(da.data[:2], da.dims, dict(da.coords, x=np.arange(2.0))), "time")
    with pytest.raises(TypeError):
        xa.multitaper_power_spectrum(da, "time", scaling="spectrum")
    # a linear detrend refuses non-finite samples (scipy.signal.detrend's refusal, as the composed call), on both routes
    v = da.data.clone()
    v[1, 50] = float("inf")
    for route in (xa.DataArray(v, da.dims, da.coords), xa.DataArray(v.to(torch.float64), da.dims, da.coords)):
        with pytest.raises(ValueError):
            xa.multitaper_power_spectrum(route, "time", detrend="linear")
    assert xa.multitaper_power_spectrum(da, "time").shape == (3, 128) and xa.multitaper_power_spectrum(da, "time", real_dim="time").shape == (3, 65)
    assert xa.multitaper_power_spectrum(da, "time", K=1).attrs == {"tapers": 1}
