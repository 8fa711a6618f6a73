"""Shared by the tests of the mean over the batch inside the last pass (xrfthip_desc.mean_batch; tests/test_batch_mean_emulated.py on the emulated library,
tests/test_gpu_batch_mean.py on the MI355X): the plan-level cases, their fields, the float64 reference, the bound.  Not a conftest: imported by the tests that use it.

The reference is the oracle's power / cross spectrum of the float64 copy of the same samples, one spectrum per slab, averaged over every M consecutive slabs with
numpy in float64.  The bound is the rounding-level contract of tests/accuracy.py for ONE spectrum plus 16 u: the sequential-sum bound of a 16-term float32 chain of
same-signed terms (the kernels add at most 16 float32 terms in a row; everything beyond is float64).  A mean of complex terms can cancel and an FFT's error bound is
norm-wise on the terms, so a cross spectrum's error is normalised by the rms of mean_m |ref_m|.

Every output of a case carries its own amplitude (x1, x3, x9, ...: powers x1, x9, x81, ...): a slab summed into the wrong output misses the bound."""
import os

import numpy as np
import torch

from oracle import xrft_oracle as o
from xrft_amd import _lib as L
from xrft_amd import api, engine

import accuracy as A

U32 = A.U["float32"]
DIMS = ("b", "y", "x")
# (ny, nx, batch, M, slabs_per_group): groups of 3 slabs straddle the outputs of 7; 20 slabs per output in ONE group
FASTY = [(256, 256, 14, 7, 3), (256, 512, 14, 7, 3), (256, 256, 40, 20, 0)]
# 64 | 128 points per axis; 5 and 37 slabs per output
FASTS = [(ny, nx, b, m, 0) for ny, nx in ((64, 64), (64, 128), (128, 128)) for b, m in ((15, 5), (74, 37))]
# The library splits the slabs of an output into P runs, one workgroup each, to fill the card: with the few outputs above no workgroup walks more than three slabs
# and every float32 chain ends with the run.  These cases pin P (XRFTHIP_MEAN_RUNS) so that ONE workgroup walks the whole output, and say how long its run is:
# (case, runs per output, slabs per run): 20 = a full chain of 16, a flush, and 4 more; 35 and 37 = two full chains and a remainder -- the staging of the sums in the
# transforms' LDS between two slabs, the second and third flush adding to the partial, the 16-term contract.  The default-routed production shapes run like this
# ((4096, 256, 256): 64 slabs per workgroup)
LONG_FASTY = [((256, 256, 40, 20, 0), 1, 20), ((256, 256, 35, 35, 0), 1, 35), ((256, 256, 36, 36, 0), 2, 18)]
LONG_FASTS = [((ny, nx, 74, 37, 0), 1, 37) for ny, nx in ((64, 64), (64, 128), (128, 128))] + [((128, 128, 70, 70, 0), 2, 35)]
# the row kernels above 512 points (other thread counts, sequences per workgroup and LDS strides; declined by default, see check_default_routing)
LARGE_FASTY = [(1024, 1024, 2, 2, 0)]
FORMS = ["plain", "linear-hann-shift"]


def case_id(c):
    return "x".join(map(str, c[:2])) + f"-b{c[2]}-M{c[3]}" + (f"-g{c[4]}" if c[4] else "")


def coords(ny, nx, batch, y0=0.0, x0=0.0):
    return {"b": np.arange(batch), "y": y0 + np.arange(ny) * 1.0, "x": x0 + np.arange(nx) * 1.0}


def field(case, seed=11):
    """[batch][ny][nx] float32: seeded noise over a plane, output o scaled by 3^o."""
    ny, nx, batch, m, _ = case
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v = rng.standard_normal((batch, ny, nx)) + 0.02 * ii - 0.01 * jj + 1.5
    v *= (3.0 ** (np.arange(batch) // m)).reshape(batch, 1, 1)
    return v.astype(np.float32)


def second_field(x, seed=12):
    """The first field rolled by (3, 5) plus a tenth of its size in noise: the cross spectra of the slabs do not cancel in the mean."""
    rng = np.random.default_rng(seed)
    amp = np.abs(x).reshape(x.shape[0], -1).mean(axis=1).reshape(-1, 1, 1)
    return (np.roll(x, (3, 5), axis=(1, 2)) + 0.1 * amp * rng.standard_normal(x.shape)).astype(np.float32)


def form_kw(form):
    """(plan arguments, oracle arguments) of a form."""
    if form == "plain":
        return dict(detrend=L.DETREND_NONE, flags=0), dict(detrend=None, window=None, shift=False)
    return dict(detrend=L.DETREND_LINEAR, flags=L.SHIFT_Y | L.SHIFT_X, window="hann"), dict(detrend="linear", window="hann", shift=True)


class env:
    """An environment variable of the library (read when a plan is created) set while the block runs, then put back as it was."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.saved = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = str(self.value)

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.saved


def make_plan(case, form="plain", mode=L.OUT_POWER, mean=True, dtype=torch.float32, batch=None, mean_batch=None, x0_lag=None, runs=0, **over):
    """runs > 0: the plan's runs per output pinned (XRFTHIP_MEAN_RUNS)."""
    if runs:
        with env("XRFTHIP_MEAN_RUNS", runs):
            return make_plan(case, form, mode, mean, dtype, batch, mean_batch, x0_lag, 0, **over)
    ny, nx, b, m, spg = case
    pkw, _ = form_kw(form)
    pkw = dict(pkw)
    win = pkw.pop("window", None)
    kw = dict(ndim=2, batch=b if batch is None else batch, ny=ny, nx=nx, dtype=dtype, out_mode=mode, scale=1.0, slabs_per_group=spg,
              mean_batch=(m if mean else 0) if mean_batch is None else mean_batch, **pkw)
    if win:
        kw.update(window_y=api._window_vector(win, ny), window_x=api._window_vector(win, nx))
    if mode == L.OUT_CROSS:  # true phase: both fields ifftshifted, the net factor phase0 * conj(phase1) per unshifted frequency (api._flags_tables)
        kw["flags"] |= L.ISHIFT_Y | L.ISHIFT_X
        c0, c1 = coords(ny, nx, 1), coords(ny, nx, 1, *x0_lag)
        for ax, n in (("y", ny), ("x", nx)):
            f = np.fft.fftfreq(n, 1.0)
            kw["phase_" + ax] = np.exp(-2j * np.pi * f * api._lag_coord(c0[ax])) * np.conj(np.exp(-2j * np.pi * f * api._lag_coord(c1[ax])))
    kw.update(over)
    return engine.SpectralPlan(**kw)


def run(plan, x0, x1=None):
    dev = L.device()
    t0 = torch.from_numpy(np.ascontiguousarray(x0)).to(dev)
    t1 = None if x1 is None else torch.from_numpy(np.ascontiguousarray(x1)).to(dev)
    out, _ = plan.execute(t0, t1)
    return out.cpu().numpy()


def runs_per_output(plan):
    """P of a mean plan, as xrfthip_plan_describe prints it."""
    d = plan.describe()
    assert "[mean over the batch]" in d, d
    return int(d.split("P=")[1].split()[0])


def run_length(plan):
    """The most slabs one workgroup of a mean plan walks, as xrfthip_plan_describe prints it."""
    return int(plan.describe().split("run=")[1].split()[0])


def reference(case, form, x0, x1=None, x0_lag=None):
    """(mean over every M slabs of the oracle's spectra of the float64 samples, mean of their magnitudes)."""
    ny, nx, b, m, _ = case
    _, okw = form_kw(form)
    x0 = np.asarray(x0, dtype=np.float64)
    b = x0.shape[0]
    if x1 is None:
        ps = o.power_spectrum(o.OArr(x0, DIMS, coords(ny, nx, b)), dim=["y", "x"], scaling="false_density", **okw).values
    else:
        ps = o.cross_spectrum(o.OArr(x0, DIMS, coords(ny, nx, b)), o.OArr(np.asarray(x1, dtype=np.float64), DIMS, coords(ny, nx, b, *x0_lag)), dim=["y", "x"],
                              scaling="false_density", true_phase=True, **okw).values
    ps = ps.reshape(b // m, m, ny, nx)
    return ps.mean(axis=1), np.abs(ps).mean(axis=1)


def kappa(case, form, x):
    """max |x| / rms(x - plane) over the slabs of each output (0 without a detrend)."""
    ny, nx, b, m, _ = case
    if form == "plain":
        return [0.0] * (x.shape[0] // m)
    xs = np.asarray(x, dtype=np.float64).reshape(-1, m, ny, nx)
    return [A.kappa(xo, A.detrended(xo, (1, 2), L.DETREND_LINEAR)) for xo in xs]


def bound(ny, nx, kap):
    return A.bound("float32", ny * nx, kap) + 16.0 * U32


def rel_error(got, ref, mag=None):
    """|| got - ref ||_2 / || ref ||_2, or / || mag ||_2 (a cross spectrum: the mean of the terms' magnitudes)."""
    g, r = np.asarray(got).astype(np.complex128 if np.iscomplexobj(ref) else np.float64), np.asarray(ref)
    if mag is None:
        return A.errors(g, r)[0]
    return float(np.sqrt(np.mean(np.abs(g - r) ** 2)) / np.sqrt(np.mean(np.asarray(mag) ** 2)))


def assert_outputs(case, form, got, ref, mag, kaps, what):
    """Every output within the bound, each against its own reference (its own amplitude); prints each figure before it asserts."""
    ny, nx = case[:2]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for k in range(ref.shape[0]):
        err, bnd = rel_error(got[k], ref[k], None if mag is None else mag[k]), bound(ny, nx, kaps[k])
        print(f"{what} output {k}: error {err:.3e} bound {bound(ny, nx, kaps[k]):.3e}")
        assert np.isfinite(got[k]).all() and err <= bnd, f"{what} output {k}: error {err:.3e} > {bnd:.3e}"


def newest_plan():
    return next(reversed(api._plan_cache.values()))


def ran_mean_form():
    p = newest_plan()
    return p.mean_batch > 1 and "[mean over the batch]" in p.describe()


def no_mean_plan():
    return all(p.mean_batch <= 1 for p in api._plan_cache.values())


def compare_labelled(got, want):
    """dims, coordinate names, order and values, attrs and name of the fused result are those of power_spectrum(...).mean(...), exactly."""
    assert tuple(got.dims) == tuple(want.dims), (got.dims, want.dims)
    assert list(got.coords) == list(want.coords), (list(got.coords), list(want.coords))
    for k in want.coords:
        assert tuple(got.coords[k].dims) == tuple(want.coords[k].dims), k
        assert np.array_equal(np.asarray(got.coords[k].values), np.asarray(want.coords[k].values)), k
        assert dict(got.coords[k].attrs) == dict(want.coords[k].attrs), (k, got.coords[k].attrs, want.coords[k].attrs)
    assert got.attrs == want.attrs and got.name == want.name, (got.attrs, want.attrs, got.name, want.name)
    assert np.asarray(got.values).shape == np.asarray(want.values).shape and np.asarray(got.values).dtype == np.asarray(want.values).dtype


# ---------------------------------------------------------------------------------- plan-level checks (both libraries)
def expected_kind(case):
    return L.K_FASTY if case[0] >= 256 else L.K_FASTS


def check_power_plan(case, form, runs=0, run_len=None):
    ny, nx, b, m, _ = case
    x = field(case)
    p = make_plan(case, form, runs=runs)
    assert p.kernel_info()[0] == expected_kind(case) and "[mean over the batch]" in p.describe(), p.describe()
    if run_len is not None:
        assert runs_per_output(p) == runs and run_length(p) == run_len, p.describe()
    got = run(p, x)
    assert got.shape == (b // m, ny, nx) and got.dtype == np.float32
    ref, _ = reference(case, form, x)
    assert_outputs(case, form, got, ref, None, kappa(case, form, x), f"power {case_id(case)} {form}")
    assert np.array_equal(got, run(p, x))  # every addition in an order the plan fixes: the same bits
    # the workspace: the plain plan's and at most (P + 1) results -- P float64 half spectra per output
    plain = make_plan(case, form, mean=False)
    if plain.kernel_info()[0] != p.kernel_info()[0]:
        # 256 x 256: the plain plan is the one-pass slab kernel, which has no workspace at all, and the mean form is the two-pass pipeline, whose intermediate alone
        # (one group of slabs) is larger than a result: the partial sums are held against the plain plan of the SAME pipeline (XRFTHIP_FASTS=0 selects it)
        assert (ny, nx) == (256, 256) and plain.kernel_info()[0] == L.K_FASTS
        with env("XRFTHIP_FASTS", 0):
            plain = make_plan(case, form, mean=False)
    runs = runs_per_output(p)
    assert plain.kernel_info()[0] == p.kernel_info()[0]
    assert p.workspace_bytes <= plain.workspace_bytes + (runs + 1) * got.nbytes, (p.workspace_bytes, plain.workspace_bytes, runs, got.nbytes)


CROSS_LAG = (2.0, 7.0)  # origin of the second field's coordinates: the net true-phase factor is not 1


def check_cross_plan(case, runs=0, run_len=None):
    ny, nx, b, m, _ = case
    form = "linear-hann-shift"
    x0 = field(case)
    x1 = second_field(x0)
    p = make_plan(case, form, mode=L.OUT_CROSS, x0_lag=CROSS_LAG, runs=runs)
    assert p.kernel_info()[0] == L.K_FASTY and "[mean over the batch]" in p.describe(), p.describe()
    if run_len is not None:
        assert runs_per_output(p) == runs and run_length(p) == run_len, p.describe()
    got = run(p, x0, x1)
    assert got.shape == (b // m, ny, nx) and got.dtype == np.complex64
    ref, mag = reference(case, form, x0, x1, CROSS_LAG)
    kaps = [max(a, c) for a, c in zip(kappa(case, form, x0), kappa(case, form, x1))]
    assert_outputs(case, form, got, ref, mag, kaps, f"cross {case_id(case)}")
    assert np.array_equal(got, run(p, x0, x1))


def check_bit_identities(case):
    ny, nx, _, _, spg = case
    x = field((ny, nx, 3, 1, spg), seed=21)
    modes = [(L.OUT_POWER, None)] + ([(L.OUT_CROSS, second_field(x, 22))] if case[0] >= 256 else [])
    for form in FORMS:
        for mode, x1 in modes:
            kw = dict(mode=mode, x0_lag=CROSS_LAG)
            plain = make_plan((ny, nx, 3, 0, spg), form, mean=False, **kw)
            want = run(plain, x, x1)
            # M = 1 is the plain plan itself
            one = make_plan((ny, nx, 3, 1, spg), form, **kw)
            assert "[mean over the batch]" not in one.describe() and one.describe() == plain.describe()
            assert np.array_equal(run(one, x, x1), want)
            # M = 2 with every slab stored twice: x + x and the halving are exact
            two = make_plan((ny, nx, 6, 2, spg), form, **kw)
            assert "[mean over the batch]" in two.describe()
            got = run(two, np.repeat(x, 2, axis=0), None if x1 is None else np.repeat(x1, 2, axis=0))
            assert np.array_equal(got, want), f"{case_id(case)} {form} mode {mode}: doubled slabs differ from the plain plan"


def check_nan(case):
    ny, nx, b, m, _ = case
    form = "linear-hann-shift"
    x = field(case)
    p = make_plan(case, form)
    clean = run(p, x)
    ref, _ = reference(case, form, x)
    kaps = kappa(case, form, x)
    for bad in range(b // m):
        xn = x.copy()
        xn[bad * m + 2, ny // 3, nx // 5] = np.nan
        got = run(p, xn)
        assert not np.isfinite(got[bad]).any(), f"output {bad} has finite samples"
        for k in range(b // m):
            if k != bad:
                assert np.array_equal(got[k], clean[k]), (bad, k)
                assert rel_error(got[k], ref[k]) <= bound(ny, nx, kaps[k])


def _status(**kw):
    base = dict(ndim=2, batch=4, ny=256, nx=256, dtype=torch.float32, out_mode=L.OUT_POWER, mean_batch=2)
    base.update(kw)
    try:
        engine.SpectralPlan(**base)
    except L.XrftHipError as e:
        return e.status
    return 0


def check_status_codes():
    assert _status() == 0 and _status(ny=64, nx=128) == 0
    assert _status(batch=10, mean_batch=4) == L.BAD_ARG
    assert _status(mean_batch=-1) == L.BAD_ARG
    assert _status(out_mode=L.OUT_COMPLEX) == L.BAD_ARG
    assert _status(out_mode=L.OUT_PHASE) == L.BAD_ARG
    assert _status(flags=L.ISO, binmap=np.zeros((256, 256), np.int32), nbins=1) == L.BAD_ARG
    assert _status(flags=L.HALF_X) == L.UNSUPPORTED_LENGTH
    assert _status(flags=L.AXIS_Y) == L.UNSUPPORTED_LENGTH
    assert _status(inner=4) == L.UNSUPPORTED_LENGTH
    assert _status(dtype=torch.float64) == L.UNSUPPORTED_LENGTH
    assert _status(ny=50, nx=50) == L.UNSUPPORTED_LENGTH
    assert _status(ny=256, nx=64) == L.UNSUPPORTED_LENGTH  # (the one-pass slabs of 256 points on an axis have no mean form, and the two passes start at 256 x 256)
    assert _status(ny=256, nx=256, mean_batch=2, out_mode=L.OUT_CROSS) == 0


def every_mean_form():
    """XRFTHIP_MEAN_ALL=1 while the block runs: a mean plan takes the mean form of EVERY class the kernels serve.  By default the library keeps a mean form only where
    it measured faster than the composition it replaces (profiles/r15_batch_mean.txt) -- check_default_routing holds that -- and the kernels of the declined classes
    are tested all the same."""
    return env("XRFTHIP_MEAN_ALL", 1)


def check_default_routing():
    """Without the knob: the classes that measured faster keep their mean form, the others answer "the caller composes", and the API composes them."""
    with env("XRFTHIP_MEAN_ALL", None):
        for kw in (dict(), dict(ny=128, nx=128), dict(ny=128, nx=64), dict(ny=256, nx=512), dict(ny=1024, nx=1024), dict(out_mode=L.OUT_CROSS)):
            assert _status(**kw) == 0, kw
        for kw in (dict(ny=64, nx=64), dict(ny=64, nx=128)):
            assert _status(**kw) == L.UNSUPPORTED_LENGTH, kw
        api.clear_plan_cache()
        da, _, _ = _api_field((3, 64, 64), ("time", "y", "x"), "float32", None, seed=36)
        got = xa.mean_power_spectrum(da, "time", dim=["y", "x"])
        assert no_mean_plan()
        compare_labelled(got, xa.power_spectrum(da, dim=["y", "x"]).mean("time"))
    api.clear_plan_cache()


def check_older_struct_sizes():
    """A descriptor with each of the five earlier struct_size values still creates its plan (the appended fields count as 0)."""
    import ctypes as C

    dll = L.load()
    sizes = [getattr(L.Desc, f).offset for f in ("inner", "mid", "in_stride_y", "herm_ny", "mean_batch")] + [C.sizeof(L.Desc)]
    assert sizes == sorted(set(sizes)) and sizes[-1] - sizes[-2] == 8
    for sz in sizes:
        d = L.Desc(sz, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        h = C.c_void_p(0)
        assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == 0, sz
        dll.xrfthip_plan_destroy(h)
    d = L.Desc(sizes[-1] + 8, 2, 2, 64, 64, L.F32, L.OUT_POWER, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    h = C.c_void_p(0)
    assert dll.xrfthip_plan_create(C.byref(h), C.byref(d)) == L.BAD_ARG


# ---------------------------------------------------------------------------------- API-level checks (both libraries)
import xrft_amd as xa  # noqa: E402

import cases  # noqa: E402

LINHANN = dict(detrend="linear", window="hann")
# name -> (shape, dims, dtype, mean_dim, chunks, keyword arguments, fused?)
API_CASES = {
    "time-256": ((6, 256, 256), ("time", "y", "x"), "float32", "time", None, LINHANN, True),
    "inner-batch-dim": ((2, 3, 128, 64), ("a", "b", "y", "x"), "float32", "b", None, dict(window="hann"), True),
    "outer-batch-dim": ((2, 3, 128, 64), ("a", "b", "y", "x"), "float32", "a", None, dict(window="hann"), False),
    "segments-inner": ((2, 256, 512), ("time", "y", "x"), "float32", ["y_segment", "x_segment"], {"y": 128, "x": 128}, dict(window="hann", chunks_to_segments=True), True),
    "segments-all": ((2, 256, 512), ("time", "y", "x"), "float32", ["time", "y_segment", "x_segment"], {"y": 128, "x": 128}, dict(window="hann", chunks_to_segments=True), True),
    "float64": ((4, 48, 40), ("time", "y", "x"), "float64", "time", None, dict(window="hann"), False),
    "odd-50": ((5, 50, 50), ("time", "y", "x"), "float32", "time", None, dict(window="hann"), False),
    "float16": ((4, 256, 256), ("time", "y", "x"), "float16", "time", None, LINHANN, True),
}


def _api_field(shape, dims, dtype, chunks, seed):
    """(the product's array -- device data of `dtype` --, the oracle's over the float64 image of the same samples, that image)."""
    rng = np.random.default_rng(seed)
    ny, nx = shape[-2:]
    ii, jj = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v = rng.standard_normal(shape) + 0.02 * ii - 0.01 * jj + 1.0
    tdt = {"float32": torch.float32, "float64": torch.float64, "float16": torch.float16}[dtype]
    t = torch.from_numpy(v).to(tdt)
    wide = t.to(torch.float64).numpy()
    crd = {d: np.arange(n) * (0.5 if d == "x" else 1.0) for d, n in zip(dims, shape)}
    da = xa.DataArray(t.to(L.device()), dims, crd)
    oa = o.OArr(wide, dims, crd, chunks=None if chunks is None else {d: tuple([c] * (n // c)) for (d, c), n in ((kv, shape[dims.index(kv[0])]) for kv in chunks.items())})
    if chunks is not None:
        da = da.chunk(chunks)
    return da, oa, wide


def _oracle_mean(ref, names, mag=False):
    names = [names] if isinstance(names, str) else list(names)
    axes = tuple(ref.dims.index(d) for d in names)
    kept = [d for d in ref.dims if d not in names]
    vals = (np.abs(ref.values) if mag else ref.values).mean(axis=axes)
    return o.OArr(vals, kept, {d: ref.coord(d) for d in kept if d in ref.coords}, coord_attrs={d: ref.coord_attrs.get(d, {}) for d in kept})


def _api_bound(dtype, shape_yx, x, detrend):
    dt = "float32" if dtype == "float16" else dtype
    kap = 0.0
    if detrend:
        xs = x.reshape((-1,) + tuple(shape_yx))
        kap = A.kappa(xs, A.detrended(xs, (1, 2), L.DETREND_LINEAR))
    return A.bound(dt, int(np.prod(shape_yx)), kap) + 16.0 * A.U[dt]


def check_api_case(name):
    shape, dims, dtype, mean_dim, chunks, kw, fused = API_CASES[name]
    api.clear_plan_cache()
    da, oa, wide = _api_field(shape, dims, dtype, chunks, seed=31)
    kw = dict(kw, dim=["y", "x"])
    want = xa.power_spectrum(da, **kw).mean(mean_dim)
    got = xa.mean_power_spectrum(da, mean_dim, **kw)
    assert ran_mean_form() if fused else no_mean_plan(), newest_plan().describe()
    compare_labelled(got, want)
    ref = _oracle_mean(o.power_spectrum(oa, **kw), mean_dim)
    dt = "float32" if dtype == "float16" else dtype
    cases.check(got, ref, cases.TOL[dt])
    yx = (chunks["y"], chunks["x"]) if chunks else shape[-2:]
    err, bnd = rel_error(got.values, ref.values), _api_bound(dtype, yx, wide, kw.get("detrend"))
    print(f"mean_power_spectrum {name}: error {err:.3e} bound {bnd:.3e} (fused: {fused})")
    assert err <= bnd, (err, bnd)
    # ... and the composition it stands for holds the same bound
    assert rel_error(want.values, ref.values) <= bnd


def check_api_cross():
    api.clear_plan_cache()
    shape, dims = (6, 256, 256), ("time", "y", "x")
    da, oa, wide = _api_field(shape, dims, "float32", None, seed=33)
    rng = np.random.default_rng(34)
    w2 = (np.roll(wide, (3, 5), axis=(1, 2)) + 0.1 * rng.standard_normal(shape)).astype(np.float32)
    da2 = xa.DataArray(torch.from_numpy(w2).to(L.device()), dims, {d: np.asarray(da[d].values) for d in dims})
    oa2 = o.OArr(w2.astype(np.float64), dims, {d: oa.coord(d) for d in dims})
    kw = dict(dim=["y", "x"], **LINHANN)
    want = xa.cross_spectrum(da, da2, **kw).mean("time")
    got = xa.mean_cross_spectrum(da, da2, "time", **kw)
    assert ran_mean_form(), newest_plan().describe()
    compare_labelled(got, want)
    full = o.cross_spectrum(oa, oa2, **kw)
    ref, mag = _oracle_mean(full, "time"), _oracle_mean(full, "time", mag=True)
    cases.check(got, ref, cases.TOL["complex64"])
    err = rel_error(got.values, ref.values, mag.values)
    bnd = max(_api_bound("float32", shape[-2:], wide, True), _api_bound("float32", shape[-2:], w2.astype(np.float64), True))
    print(f"mean_cross_spectrum: error {err:.3e} bound {bnd:.3e}")
    assert err <= bnd, (err, bnd)


def check_api_errors():
    import pytest

    for dtype, shape in (("float32", (3, 64, 64)), ("float64", (3, 12, 10))):  # (the fused route and the composition)
        da, _, _ = _api_field(shape, ("time", "y", "x"), dtype, None, seed=35)
        for bad in ("y", "nope", ["time", "x"]):
            with pytest.raises(ValueError):
                xa.mean_power_spectrum(da, bad, dim=["y", "x"])
            with pytest.raises(ValueError):
                xa.mean_cross_spectrum(da, da, bad, dim=["y", "x"])
        assert xa.mean_power_spectrum(da, "time", dim=["y", "x"]).dims == ("freq_y", "freq_x")
