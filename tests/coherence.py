"""Shared by the tests of the magnitude-squared coherence (XRFTHIP_OUT_COHERENCE, xrfthip_coherence, xrft_amd.coherence; tests/test_coherence_emulated.py on the
emulated library, tests/test_gpu_coherence.py on the MI355X).  Not a conftest: imported by the tests that use it.  Fields, plans, the environment block, the float64
reference of a mean spectrum and its bound are those of tests/batch_mean.py (`B`).

    gamma^2(k) = |<F0 conj F1>|^2 / (<|F0|^2> <|F1|^2>),   <.> the mean over the M slabs of an output

Fields.  The first is B.field(case).  The second is the first rolled by (3, 5) plus noise COLOURED along x (n + roll(n, 1) halved: its spectrum falls to zero at
kx = nx / 2), as large as the field: gamma^2 depends on the frequency (about 1e-6 ... 1.0, median 0.24 - 0.57 over the cases here, 1 at kx = nx / 2) and the two powers have different
shapes, so a kernel that forms A^2 or B^2 for A B fails.  No bin has a zero denominator: no bin is left out of any comparison.

Reference, float64: |mean_m cs_m|^2 / (mean_m ps0_m  mean_m ps1_m), the spectra from the oracle's cross_spectrum / power_spectrum of the float64 image of the same
samples (B.reference).

Bound.  err = rms(got - ref) over one output, absolute (gamma^2 is O(1)), and  err <= 4 B.bound(ny, nx, kappa) + 3 u:  to first order
d gamma^2 = gamma^2 (2 Re dC / C - dA / A - dB / B) with gamma <= 1, each of the three means holds B.bound (the project's contract for one mean spectrum), and 3 u
covers the final product, quotient and rounding.  Every value is finite, >= 0 and <= 1 + 4 B.bound."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from oracle import xrft_oracle as o
from xrft_amd import _lib as L
from xrft_amd import api, engine
import xrft_amd as xa

import batch_mean as B
import ops as O

U32 = B.U32
LAG = B.CROSS_LAG


# ---------------------------------------------------------------------------------- fields, reference, bound
@functools.lru_cache(maxsize=None)
def fields(case, same=False):
    """(x0, x1) of a case, read-only (shared by the tests of the case)."""
    x0 = B.field(case)
    if same:
        x1 = x0.copy()
    else:
        n = np.random.default_rng(12).standard_normal(x0.shape)
        n = 0.5 * (n + np.roll(n, 1, axis=2))
        amp = np.abs(x0).reshape(x0.shape[0], -1).mean(axis=1).reshape(-1, 1, 1)
        x1 = (np.roll(x0, (3, 5), axis=(1, 2)) + amp * n).astype(np.float32)
    x0.setflags(write=False)
    x1.setflags(write=False)
    return x0, x1


@functools.lru_cache(maxsize=None)
def reference(case, form, same=False):
    """(gamma^2 in float64 [b / M][ny][nx], kappa per output), computed once per case and form, read-only."""
    x0, x1 = fields(case, same)
    cs, _ = B.reference(case, form, x0, x1, LAG)
    p0, _ = B.reference(case, form, x0)
    p1, _ = B.reference(case, form, x1)
    den = p0 * p1
    assert (den > 0).all()  # (no bin is left out)
    ref = np.abs(cs) ** 2 / den
    ref.setflags(write=False)
    kaps = tuple(max(a, c) for a, c in zip(B.kappa(case, form, x0), B.kappa(case, form, x1)))
    return ref, kaps


def run(plan, x0, x1=None):
    """B.run on the shared read-only fields (torch warns that it cannot mark a tensor read-only; nothing here writes to one)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return B.run(plan, x0, x1)


def bound(ny, nx, kap):
    return 4.0 * B.bound(ny, nx, kap) + 3.0 * U32


def assert_outputs(case, got, ref, kaps, what):
    """Every output: finite, >= 0, <= 1 + 4 B.bound, rms(got - ref) within the bound; prints err, the bound and the largest single-bin error before it asserts."""
    ny, nx = case[:2]
    assert got.shape == ref.shape and got.dtype == np.float32, (got.shape, ref.shape, got.dtype)
    for k in range(ref.shape[0]):
        d = np.abs(got[k].astype(np.float64) - ref[k])
        err, bnd = float(np.sqrt(np.mean(d ** 2))), bound(ny, nx, kaps[k])
        print(f"{what} output {k}: rms error {err:.3e} bound {bnd:.3e} largest bin {float(np.nanmax(d)):.3e} (gamma^2 {ref[k].min():.2e} .. {ref[k].max():.3f}, median {np.median(ref[k]):.2f})")
        assert np.isfinite(got[k]).all() and (got[k] >= 0).all() and (got[k] <= 1.0 + 4.0 * B.bound(ny, nx, kaps[k])).all(), f"{what} output {k}: outside [0, 1]"
        assert err <= bnd, f"{what} output {k}: rms error {err:.3e} > {bnd:.3e}"


def make_plan(case, form, mode=L.OUT_COHERENCE, phases=True, runs=0, **over):
    """The plan of B.make_plan(mode=CROSS) -- both fields ifftshifted, the true-phase tables of B.CROSS_LAG -- with out_mode `mode`; phases=False: without the tables."""
    ny, nx = case[:2]
    kw = dict(flags=B.form_kw(form)[0]["flags"] | L.ISHIFT_Y | L.ISHIFT_X)
    if phases:
        c0, c1 = B.coords(ny, nx, 1), B.coords(ny, nx, 1, *LAG)
        for ax, n in (("y", ny), ("x", nx)):
            f = np.fft.fftfreq(n, 1.0)
            kw["phase_" + ax] = np.exp(-2j * np.pi * f * api._lag_coord(c0[ax])) * np.conj(np.exp(-2j * np.pi * f * api._lag_coord(c1[ax])))
    kw.update(over)
    return B.make_plan(case, form, mode=mode, runs=runs, x0_lag=LAG, **kw)


def is_coherence_plan(p):
    d = p.describe()
    return p.kernel_info()[0] == L.K_FASTY and "[mean over the batch]" in d and "coherence" in d


# ---------------------------------------------------------------------------------- plan level
def check_plan(case, form, runs=0, run_len=None):
    ny, nx, b, m, _ = case
    x0, x1 = fields(case)
    p = make_plan(case, form, runs=runs)
    assert is_coherence_plan(p), p.describe()
    if run_len is not None:
        assert B.runs_per_output(p) == runs and B.run_length(p) == run_len, p.describe()
    got = run(p, x0, x1)
    assert got.shape == (b // m, ny, nx) and got.dtype == np.float32
    ref, kaps = reference(case, form)
    assert_outputs(case, got, ref, kaps, f"coherence {B.case_id(case)} {form}")
    assert np.array_equal(got, run(p, x0, x1))  # every addition in an order the plan fixes: the same bits
    return p, got


def check_workspace(case, form):
    """At most the CROSS mean plan's and 16 bytes more per sample of the P half spectra of every output (4 doubles where CROSS has 2)."""
    ny, nx, b, m, _ = case
    p = make_plan(case, form)
    cross = make_plan(case, form, mode=L.OUT_CROSS)
    assert B.runs_per_output(p) == B.runs_per_output(cross)
    extra = B.runs_per_output(p) * (b // m) * (ny // 2 + 1) * nx * 16
    assert cross.workspace_bytes < p.workspace_bytes <= cross.workspace_bytes + extra, (p.workspace_bytes, cross.workspace_bytes, extra)


def check_invariance(case, form):
    """Phase tables have no effect, and a power of two as `scale` is exact in every product: the same bits."""
    x0, x1 = fields(case)
    base = run(make_plan(case, form), x0, x1)
    assert np.array_equal(base, run(make_plan(case, form, phases=False), x0, x1)), "phase tables change the coherence"
    assert np.array_equal(base, run(make_plan(case, form, scale=2.0 ** -10), x0, x1)), "scale = 2^-10 changes the coherence"


def check_identical_fields(case, form):
    """x1 = x0: every bin within the bound of 1."""
    ny, nx = case[:2]
    x0, x1 = fields(case, same=True)
    got = run(make_plan(case, form), x0, x1)
    ref, kaps = reference(case, form, same=True)
    assert np.abs(ref - 1.0).max() < 1e-9
    for k in range(got.shape[0]):
        worst = float(np.abs(got[k].astype(np.float64) - 1.0).max())
        print(f"coherence of a field with itself {B.case_id(case)} {form} output {k}: largest |gamma^2 - 1| {worst:.3e} bound {bound(ny, nx, kaps[k]):.3e}")
        assert worst <= bound(ny, nx, kaps[k])


def check_against_existing_forms(case, form):
    """engine.coherence(CROSS mean plan, POWER mean plan of x0, of x1) -- the plans of before this mode -- and the fused plan differ by at most the bound."""
    ny, nx = case[:2]
    x0, x1 = fields(case)
    fused = run(make_plan(case, form), x0, x1)
    dev = L.device()
    cs = torch.from_numpy(run(make_plan(case, form, mode=L.OUT_CROSS), x0, x1)).to(dev)
    pw = [torch.from_numpy(run(B.make_plan(case, form), x)).to(dev) for x in (x0, x1)]
    composed = engine.coherence(cs, pw[0], pw[1]).cpu().numpy()
    assert composed.dtype == np.float32 and composed.shape == fused.shape
    _, kaps = reference(case, form)
    for k in range(fused.shape[0]):
        err = float(np.sqrt(np.mean((fused[k].astype(np.float64) - composed[k]) ** 2)))
        print(f"fused against composed {B.case_id(case)} {form} output {k}: rms difference {err:.3e} bound {bound(ny, nx, kaps[k]):.3e}")
        assert err <= bound(ny, nx, kaps[k])


def check_nan(case):
    """One NaN in one slab of field 1: every value of its own output non-finite, every other output bit-identical to the clean run."""
    ny, nx, b, m, _ = case
    form = "linear-hann-shift"
    x0, x1 = fields(case)
    p = make_plan(case, form)
    clean = run(p, x0, x1)
    for bad in range(b // m):
        xn = x1.copy()
        xn[bad * m + 2, ny // 3, nx // 5] = np.nan
        got = run(p, x0, xn)
        assert not np.isfinite(got[bad]).any(), f"output {bad} has finite samples"
        for k in range(b // m):
            if k != bad:
                assert np.array_equal(got[k], clean[k]), (bad, k)


def _status(**kw):
    return B._status(**dict(dict(out_mode=L.OUT_COHERENCE), **kw))


def check_status_codes():
    assert _status(mean_batch=0) == L.BAD_ARG and _status(mean_batch=1) == L.BAD_ARG
    assert _status(batch=10, mean_batch=4) == L.BAD_ARG
    assert _status(flags=L.ISO, binmap=np.zeros((256, 256), np.int32), nbins=1) == L.BAD_ARG
    for kw in (dict(flags=L.INVERSE), dict(detrend=7)):  # every descriptor to which CROSS answers BAD_ARG
        assert B._status(out_mode=L.OUT_CROSS, **kw) == L.BAD_ARG and _status(**kw) == L.BAD_ARG, kw
    assert _status(dtype=torch.complex64) == B._status(out_mode=L.OUT_CROSS, dtype=torch.complex64) == L.UNSUPPORTED_LENGTH  # (complex fields: as the CROSS mean plan)
    assert _status(dtype=torch.float64) == L.UNSUPPORTED_LENGTH
    assert _status(flags=L.HALF_X) == L.UNSUPPORTED_LENGTH
    assert _status(flags=L.AXIS_Y) == L.UNSUPPORTED_LENGTH
    assert _status(inner=4) == L.UNSUPPORTED_LENGTH
    for ny, nx in ((64, 64), (128, 128), (256, 64)):
        assert _status(ny=ny, nx=nx) == L.UNSUPPORTED_LENGTH, (ny, nx)
    assert _status() == 0
    assert _status(out_mode=5) == L.BAD_ARG
    B.check_status_codes()  # every other (out_mode, mean_batch) pair answers what it did


def check_exec_needs_two_fields():
    """xrfthip_exec with d_in1 == NULL answers as CROSS does."""
    case = B.FASTY[0]
    dll = L.load()
    x0 = torch.from_numpy(np.ascontiguousarray(fields(case)[0])).to(L.device())
    answers = []
    for mode in (L.OUT_CROSS, L.OUT_COHERENCE):
        p = make_plan(case, "plain", mode=mode)
        ws = torch.empty(max(p.workspace_bytes, 16), dtype=torch.uint8, device=x0.device)
        out = torch.empty((case[2] // case[3], case[0], case[1]), dtype=p.out_dtype(), device=x0.device)
        answers.append(dll.xrfthip_exec(p._h, C.c_void_p(x0.data_ptr()), None, C.c_void_p(out.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws.numel(), O.stream()))
    assert answers[0] == answers[1] == L.BAD_ARG, answers


# ---------------------------------------------------------------------------------- the stand-alone operation
OP_N = [1, 63, 4099]


def check_op(n, name):
    """xrfthip_coherence against |c|^2 / (p0 p1) in long double, to 2 u of the output precision (guard bands, two runs: ops.run_twice)."""
    dll = L.load()
    rng = np.random.default_rng(8000 + n)
    c, cw = O.samples(rng, (n,), name)
    real = O.REAL[name]
    p0 = (rng.random(n) + 0.1).astype(real)
    p1 = (rng.random(n) * 3.0 + 0.1).astype(real)
    dc, d0, d1 = O.dev_bytes(c), O.dev_bytes(p0), O.dev_bytes(p1)
    got = O.run_twice((n,), real, lambda out: dll.xrfthip_coherence(O.CODE[name], n, dc.data_ptr(), d0.data_ptr(), d1.data_ptr(), out, O.stream()))
    ld = np.longdouble
    ref = (cw.real.astype(ld) ** 2 + cw.imag.astype(ld) ** 2) / (p0.astype(ld) * p1.astype(ld))
    fig = O.rel_u(np.abs(got.astype(ld) - ref), ref, name)
    print(f"xrfthip_coherence {name} n = {n}: {fig:.3f} u")
    assert fig <= 2.0, f"coherence {name} n = {n}: {fig:.3f} u > 2"


def check_op_zero_denominator(name):
    """p0 p1 = 0 gives NaN (0 / 0) or inf exactly as numpy's division does."""
    dll = L.load()
    real = O.REAL[name]
    c = np.array([0.0, 1.0 + 2.0j, 3.0, 0.0, 1.0j, 2.0], dtype=name)
    p0 = np.array([0.0, 0.0, 2.0, 1.0, 0.0, 4.0], dtype=real)
    p1 = np.array([1.0, 1.0, 0.0, 0.0, 0.0, 0.5], dtype=real)
    dc, d0, d1 = O.dev_bytes(c), O.dev_bytes(p0), O.dev_bytes(p1)
    got = O.run_twice(c.shape, real, lambda out: dll.xrfthip_coherence(O.CODE[name], c.size, dc.data_ptr(), d0.data_ptr(), d1.data_ptr(), out, O.stream()))
    with np.errstate(divide="ignore", invalid="ignore"):
        want = ((c.real.astype(np.float64) ** 2 + c.imag.astype(np.float64) ** 2) / (p0.astype(np.float64) * p1.astype(np.float64))).astype(real)
    assert np.array_equal(got, want, equal_nan=True), (got, want)
    assert np.isnan(want[[0, 3]]).all() and np.isinf(want[[1, 2, 4]]).all() and want[5] == 2.0  # (0 / 0, x / 0, and a finite bin beside them)


def check_op_status_and_wrapper():
    dll = L.load()
    t = torch.zeros(4, dtype=torch.complex64, device=L.device())
    r = torch.ones(4, dtype=torch.float32, device=L.device())
    args = (t.data_ptr(), r.data_ptr(), r.data_ptr(), r.data_ptr())
    assert dll.xrfthip_coherence(L.F32, 4, *args, O.stream()) == L.BAD_ARG
    assert dll.xrfthip_coherence(L.C64, -1, *args, O.stream()) == L.BAD_ARG
    assert dll.xrfthip_coherence(L.C64, 4, t.data_ptr(), None, r.data_ptr(), r.data_ptr(), O.stream()) == L.BAD_ARG
    assert dll.xrfthip_coherence(L.C64, 0, *args, O.stream()) == 0
    with pytest.raises(ValueError):
        engine.coherence(r, r, r)
    with pytest.raises(ValueError):
        engine.coherence(t, r.double(), r)
    assert engine.coherence(t + 2.0, r, r * 2).cpu().tolist() == [2.0] * 4


# ---------------------------------------------------------------------------------- API level
# name -> (shape, dims, dtype, mean_dim, chunks, keyword arguments, fused?)
API_CASES = {
    "time-256": ((6, 256, 256), ("time", "y", "x"), "float32", "time", None, B.LINHANN, True),
    "float16": ((6, 256, 256), ("time", "y", "x"), "float16", "time", None, B.LINHANN, True),
    # B.API_CASES["segments-inner"]: the POWER form of these 128 x 128 slabs is fused (the one-pass kernel), but that kernel has no two-field form: the coherence COMPOSES
    "segments-inner": ((2, 256, 512), ("time", "y", "x"), "float32", ["y_segment", "x_segment"], {"y": 128, "x": 128}, dict(window="hann", chunks_to_segments=True), False),
    "float64": ((4, 48, 40), ("time", "y", "x"), "float64", "time", None, dict(window="hann"), False),
    "odd-50": ((5, 50, 50), ("time", "y", "x"), "float32", "time", None, dict(window="hann"), False),
    "outer-batch-dim": ((2, 3, 256, 256), ("a", "b", "y", "x"), "float32", "a", None, dict(window="hann"), False),
    "real-dim": ((4, 256, 256), ("time", "y", "x"), "float32", "time", None, dict(window="hann", real_dim="x"), False),
}


def api_fields(shape, dims, dtype, chunks, seed=41):
    """Two (product array, oracle array, float64 image) of B._api_field's kind: the second is the first rolled by (3, 5) plus coloured noise of its size."""
    da, oa, wide = B._api_field(shape, dims, dtype, chunks, seed)
    n = np.random.default_rng(seed + 1).standard_normal(shape)
    n = 0.5 * (n + np.roll(n, 1, axis=-1))
    tdt = {"float32": torch.float32, "float64": torch.float64, "float16": torch.float16}[dtype]
    t2 = torch.from_numpy(np.roll(wide, (3, 5), axis=(-2, -1)) + np.abs(wide).mean() * n).to(tdt)
    wide2 = t2.to(torch.float64).numpy()
    crd = {d: np.asarray(da[d].values) for d in dims}
    da2 = xa.DataArray(t2.to(L.device()), dims, crd)
    if chunks is not None:
        da2 = da2.chunk(chunks)
    oa2 = o.OArr(wide2, dims, {d: oa.coord(d) for d in dims}, chunks=oa.chunks if chunks is not None else None)
    return (da, oa, wide), (da2, oa2, wide2)


def coherence_plans():
    return [p for p in api._plan_cache.values() if p.out_mode == L.OUT_COHERENCE]


def compare_labels(got, want):
    """dims, coordinate names, order, dims, values and attrs are those of mean_cross_spectrum of the same call (not the dtype, not the name)."""
    assert tuple(got.dims) == tuple(want.dims), (got.dims, want.dims)
    assert list(got.coords) == list(want.coords), (list(got.coords), list(want.coords))
    for k in want.coords:
        assert tuple(got.coords[k].dims) == tuple(want.coords[k].dims), k
        assert np.array_equal(np.asarray(got.coords[k].values), np.asarray(want.coords[k].values)), k
        assert dict(got.coords[k].attrs) == dict(want.coords[k].attrs), (k, got.coords[k].attrs, want.coords[k].attrs)
    assert np.asarray(got.values).shape == np.asarray(want.values).shape


def check_api_case(name):
    shape, dims, dtype, mean_dim, chunks, kw, fused = API_CASES[name]
    api.clear_plan_cache()
    (da, oa, wide), (da2, oa2, wide2) = api_fields(shape, dims, dtype, chunks)
    kw = dict(kw, dim=["y", "x"])
    got = xa.coherence(da, da2, mean_dim, **kw)
    if fused:
        assert B.ran_mean_form() and B.newest_plan().out_mode == L.OUT_COHERENCE and "coherence" in B.newest_plan().describe(), B.newest_plan().describe()
    else:
        assert not coherence_plans(), [p.describe() for p in coherence_plans()]
    assert isinstance(got, xa.DataArray) and got.name is None  # (the caller's type; unnamed inputs)
    compare_labels(got, xa.mean_cross_spectrum(da, da2, mean_dim, **kw))
    dt = "float64" if dtype == "float64" else "float32"
    assert np.asarray(got.values).dtype == np.dtype(dt)
    cs = B._oracle_mean(o.cross_spectrum(oa, oa2, **kw), mean_dim).values
    den = B._oracle_mean(o.power_spectrum(oa, **kw), mean_dim).values * B._oracle_mean(o.power_spectrum(oa2, **kw), mean_dim).values
    assert (den > 0).all()
    ref = np.abs(cs) ** 2 / den
    yx = (chunks["y"], chunks["x"]) if chunks else shape[-2:]
    one = max(B._api_bound(dtype, yx, wide, kw.get("detrend")), B._api_bound(dtype, yx, wide2, kw.get("detrend")))
    bnd = 4.0 * one + 3.0 * B.A.U[dt]
    g = np.asarray(got.values, dtype=np.float64)
    assert g.shape == ref.shape
    err = float(np.sqrt(np.mean((g - ref) ** 2)))
    print(f"coherence {name}: rms error {err:.3e} bound {bnd:.3e} largest bin {np.abs(g - ref).max():.3e} (fused: {fused}; gamma^2 {ref.min():.2e} .. {ref.max():.3f})")
    assert np.isfinite(g).all() and (g >= 0).all() and (g <= 1.0 + 4.0 * one).all()
    assert err <= bnd, (err, bnd)


def check_api_name_and_errors():
    api.clear_plan_cache()
    (da, _, _), (da2, _, _) = api_fields((3, 256, 256), ("time", "y", "x"), "float32", None, seed=43)
    kw = dict(dim=["y", "x"])
    da.name, da2.name = "u", "v"
    assert xa.coherence(da, da2, "time", **kw).name == "u_v_coherence"
    da2.name = None
    assert xa.coherence(da, da2, "time", **kw).name is None
    # the value does not depend on scaling, window_correction or true_phase
    base = xa.coherence(da, da2, "time", window="hann", **kw).values
    other = xa.coherence(da, da2, "time", window="hann", scaling="spectrum", window_correction=True, true_phase=False, **kw).values
    assert np.abs(base - other).max() <= 64 * U32
    for shape, dtype in (((3, 256, 256), "float32"), ((3, 12, 10), "float64")):  # (the fused route and the composition)
        (a, _, _), (b, _, _) = api_fields(shape, ("time", "y", "x"), dtype, None, seed=45)
        for bad in ("y", "nope", ["time", "x"]):
            with pytest.raises(ValueError):
                xa.coherence(a, b, bad, **kw)
    for shape, dtype in (((1, 256, 256), "float32"), ((1, 12, 10), "float64")):  # fewer than two spectra: gamma^2 of one spectrum is 1 everywhere
        (a, _, _), (b, _, _) = api_fields(shape, ("time", "y", "x"), dtype, None, seed=47)
        with pytest.raises(ValueError, match="at least two"):
            xa.coherence(a, b, "time", **kw)
    api.clear_plan_cache()


def check_refused_plan_is_remembered():
    """A plan the library declines (128 x 128: the one-pass kernel has no two-field form) is asked for once."""
    api.clear_plan_cache()
    (da, _, _), (da2, _, _) = api_fields((4, 128, 128), ("time", "y", "x"), "float32", None, seed=49)
    xa.coherence(da, da2, "time", dim=["y", "x"])
    assert not coherence_plans() and len(api._MEAN_REFUSED) >= 1
    n = len(api._MEAN_REFUSED)
    xa.coherence(da, da2, "time", dim=["y", "x"])
    assert len(api._MEAN_REFUSED) == n
    api.clear_plan_cache()
