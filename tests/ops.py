"""Rounding-level checks of the stand-alone C-ABI operations (csrc/ops.cpp, csrc/aux_kernels.h), shared by tests/test_ops_emulated.py (the
emulated library) and tests/test_gpu_ops.py (the MI355X).  Not a conftest: imported by the tests that use it.

Every check calls the C ABI itself, not the engine.* wrapper, because the wrappers allocate their own result: here each output lies inside
an allocation with GUARD elements of a sentinel byte pattern in front of it and behind it, the library gets the interior pointer, and the
bands must come back untouched (an out-of-range store inside an allocation is silent on the GPU: this is how a tail written one element too
far shows).  Every call runs twice on fresh buffers and the two buffers must hold the same bytes, bands included.

The reference of every operation is the same operation written plainly in numpy on the exact float64 / complex128 image of the rounded
input -- in float64 where the output is single precision, in numpy.longdouble where it is double (a float64 reference carries 1-3 u of its
own: spectrum_tail on complex128 read 6.6 u against float64 numpy, 3 u of them the reference's).

u = 2^-24 or 2^-53, the unit roundoff of the OUTPUT precision.  The bounds, per operation:

  gather_axis             the bytes of numpy.roll / numpy.take (a copy)
  convert                 the bits of ndarray.astype (IEEE round to nearest even); NaN stays NaN
  table_mul, padding      exactly +0
  table_mul, product      |got - ref| <= C_TABLE_MUL u |x| |table| per element
                            one complex product: sqrt(2) gamma_2 = 2.83 u  ->  3
  spectrum_tail(_axis)    |got - ref| <= C_POWER u ref per element, power
                            re^2 + im^2: two squares (u each) and an add of positive terms (u): 2 u to first order; the cast of `scale` to T: u; the product: u  ->  4
                          |got - ref| <= C_CROSS u |a| |b| f per element, cross (f = |scale|, doubled where the real-dim factor is 2)
                            one complex product (2.83 u), the cast of `scale`, the product  ->  5
  angle, float32          within 1 float32 ulp of the long-double arctan2 (the kernel rounds a float64 result once: 1/2 ulp + the float64 error)
  angle, float64          within C_ANGLE_F64 ulp of the long-double arctan2 (measured: below)
  angle, specials         numpy.angle in value, sign of zero and NaN-ness
  detrend, detrend3,      max |got - ref| <= C_OP[dtype] u max |x| per fit (one slab / block / inner element, one component of a complex field)
  detrend_inner             (measured on the reference side: below)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from xrft_amd import _lib as L
from xrft_amd import engine

NAMES = ["float32", "float64", "complex64", "complex128"]
CNAMES = ["complex64", "complex128"]
U = {"float32": 2.0 ** -24, "complex64": 2.0 ** -24, "float64": 2.0 ** -53, "complex128": 2.0 ** -53}
CODE = {"float32": L.F32, "float64": L.F64, "complex64": L.C64, "complex128": L.C128}
REAL = {"float32": "float32", "float64": "float64", "complex64": "float32", "complex128": "float64"}
CPLX = {"float32": "complex64", "float64": "complex128", "complex64": "complex64", "complex128": "complex128"}
WIDE = {"float32": np.float64, "float64": np.float64, "complex64": np.complex128, "complex128": np.complex128}
KINDS = {"constant": L.DETREND_CONSTANT, "linear": L.DETREND_LINEAR}

# worst figures measured over the cases below, in the units of each bound (emulator / MI355X):
C_TABLE_MUL = 3.0  # single 1.58 / 1.34, double 1.71 / 1.71
C_POWER = 4.0      # single 2.79 / 2.73, double 2.30 / 2.30
C_CROSS = 5.0      # single 2.73 / 2.68, double 1.84 / 1.58
# angle in float64, in ulp of the result, against arctan2 in long double on the 5000 samples of check_angle: numpy's own float64 arctan2 (glibc) reads 0.720; the
# kernel gets 4x that (a device math library documents a couple of ulp where glibc gives under one).  Measured: emulator 0.504 (glibc's atan2), MI355X 1.344.
# (float32, bound 1 ulp: 0.500 on both -- a float64 result rounded once.)
ANGLE_F64_NUMPY = 0.720
C_ANGLE_F64 = 4.0 * ANGLE_F64_NUMPY
# The detrends, in units of u max |x| per fit.  The constants are measured on the REFERENCE side: the same formula (centred moments, the fit subtracted) written plainly
# at working precision in numpy (plain_detrend: numpy.sum in the data's precision) reads, against the long-double reference over every case of DETREND + DETREND3 +
# INNER below (reference_rendering_figures()),
#     float32 / complex64    3.90        float64 / complex128    3.21
# and C_OP is 4x that, rounded up to one decimal.  The faults these tests are after are thousands of u at these shapes: a centre off by a half, n^2 for n^2 - 1 in a
# slope's denominator, one slab's coefficients applied to its neighbour (check_sensitivity).
# The kernels keep float64 moments and coefficients and round x - fit once to the data's precision: float32 data sit near half an ulp, float64 data carry the float64
# sums' own error.  Measured worst over the same cases (emulator without the four cases of EMU_SKIP / MI355X):
#     float32    detrend 0.42 / 0.63    detrend3 0.48 / 0.62    detrend_inner 0.55 / 0.65
#     float64    detrend 2.17 / 3.42    detrend3 3.40 / 3.91    detrend_inner 4.48 / 4.48
# (detrend3 on a 65 x 64 x 3 float64 block read 20.0 while finalize_coef3_kernel added its 4096 chunks in one chain; in runs of 64 it reads 2.44.)
C_OP_REFERENCE = {"float32": 3.90, "float64": 3.21}
C_OP = {"float32": 15.6, "complex64": 15.6, "float64": 12.9, "complex128": 12.9}

GUARD = 64   # elements of the output's type in front of and behind every output
SENT = 0xA5  # every byte of a band, and of the output before the call (0xa5a5a5a5 is -2.9e-16 as a float32: an element not written fails its bound)

# the launch caps of csrc/ops.cpp that the cases below are sized to cross (each check asserts its own by arithmetic)
DETREND_SLABS_PER_LAUNCH = 32768      # xrfthip_detrend / xrfthip_detrend3: grid.y
DETREND_APPLY_GRID = 2048 * 256       # detrend_apply_kernel: threads of the capped grid
DETREND3_ROW_BLOCKS = 4096            # block3_moments_kernel / detrend3_apply_kernel: grid.x
FLUSH_TERMS = 64                      # slab_moments_kernel / block3_moments_kernel: working-precision terms per thread between two flushes
INNER_SLABS_PER_LAUNCH = 65535        # run_detrend_inner: grid.z
INNER_APPLY_GRID = 8 * 256 * 4        # plane_inner_apply_kernel: workgroups
INNER_LDS_COEF_BYTES = 40 * 1024      # ... whose coefficient table of 24 bytes per inner component must fit
INNER_THREADS = 1024                  # plane_inner_moments_kernel: lanes across the inner index
TAIL_GRID = 16384 * 256               # spectrum_tail / angle / gather_axis: threads of the capped grid
CONVERT_GRID = 8 * 256 * 4 * 256      # xrfthip_convert
REDUCE_GRID = 8 * 256 * 8 * 256       # xrfthip_reduce_axis / xrfthip_table_mul

WORST = {}  # what the checks measured, in the units of their bounds: {(operation, precision): figure}, for the figures written next to the constants


def note(op, name, fig):
    key = (op, REAL[name] if name in REAL else name)
    WORST[key] = max(WORST.get(key, 0.0), float(fig))
    return float(fig)


# ---------------------------------------------------------------------------------- buffers
def dev():
    return torch.device(engine.device_type())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if engine.device_type() == "cuda" else C.c_void_p(0)


def dev_bytes(a):
    """The bytes of a numpy array on the library's device (a uint8 tensor: whatever the dtype, no conversion on the way)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(dev())


def scratch(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev())


class Guarded:
    """An output of `shape` x `dtype` (numpy) with GUARD elements of the sentinel on either side, in one allocation."""

    def __init__(self, shape, dtype, fill=None):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        esz, n = self.dtype.itemsize, int(np.prod(shape, dtype=np.int64))
        self.lo, self.hi = GUARD * esz, (GUARD + n) * esz
        self.buf = torch.full((self.hi + GUARD * esz,), SENT, dtype=torch.uint8, device=dev())
        if fill is not None:
            self.buf[self.lo:self.hi] = dev_bytes(fill)
        self.ptr = self.buf.data_ptr() + self.lo  # (allocations are 256-byte aligned and a band is a multiple of 256 bytes for every type here)

    def result(self):
        host = self.buf.cpu().numpy()  # (a copy on the stream the library ran on: waits for it)
        assert (host[:self.lo] == SENT).all(), f"the band in front of the output was written: {np.flatnonzero(host[:self.lo] != SENT)[:8] - self.lo} (bytes from its start)"
        assert (host[self.hi:] == SENT).all(), f"the band behind the output was written: {np.flatnonzero(host[self.hi:] != SENT)[:8]} (bytes past its end)"
        return host[self.lo:self.hi].view(self.dtype).reshape(self.shape).copy()


def run_twice(shape, dtype, call, fill=None):
    """call(pointer to the output) -> status, on two fresh guarded outputs: status OK both times, the same bytes, bands untouched.  Returns the numpy result."""
    outs = []
    for _ in range(2):
        g = Guarded(shape, dtype, fill)
        st = call(g.ptr)
        assert st == 0, f"status {st}: {L.load().xrfthip_strerror(st).decode()}"
        outs.append(g)
    assert torch.equal(outs[0].buf, outs[1].buf), "two runs differ in their bits"
    return outs[0].result()


def samples(rng, shape, name):
    """Seeded noise rounded to `name`, and its exact float64 / complex128 image."""
    v = rng.standard_normal(shape)
    if name.startswith("complex"):
        v = v + 1j * rng.standard_normal(shape)
    x = v.astype(name)
    return x, x.astype(WIDE[name])


def hp(name):
    """The reference's precision: float64 under a single-precision result, long double under a double-precision one."""
    dbl = REAL[name] == "float64"
    return (np.longdouble, np.clongdouble) if dbl else (np.float64, np.complex128)


def rel_u(err, scale, name):
    """max err / scale in units of u (0 / 0 counts as 0)."""
    err, scale = np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / scale)
    return float(r.max(initial=0.0)) / U[name]


# ---------------------------------------------------------------------------------- detrend: references and the bound
def trend_field(rng, shape, fit_axes, name):
    """Noise over a plane plus an offset of several sigma along `fit_axes`, every independent element (the other axes) at a scale of its own."""
    def one():
        v = rng.standard_normal(shape) + 5.0 + 2.0 * rng.random()
        for k, ax in enumerate(fit_axes):
            s = [1] * len(shape)
            s[ax] = shape[ax]
            rise = (3.0 + rng.random()) * (-1.0) ** k  # (of the plane across the whole extent, in sigma of the noise: the same conditioning at 3 rows and at 8200)
            v = v + rise / max(shape[ax] - 1, 1) * np.arange(shape[ax], dtype=np.float64).reshape(s)
        return v
    v = one() + (1j * -one() if name.startswith("complex") else 0.0)
    free = [n if ax not in fit_axes else 1 for ax, n in enumerate(shape)]
    scale = 1.0 + (np.arange(int(np.prod(free))) % 5).reshape(free) * 0.75
    x = (v * scale).astype(name)
    return x, x.astype(WIDE[name])


def ref_detrend(xw, fit_axes, kind, centre_off=0.0, square_denominator=False):
    """x - fit over `fit_axes` in long double: the mean, or the least-squares hyperplane by centred coordinates (mutually orthogonal on a full grid: exact).
    centre_off / square_denominator: the two faults of check_sensitivity (a centre (n - 1) / 2 + off; n^2 for n^2 - 1 in a slope's denominator)."""
    fit_axes = tuple(fit_axes)
    a = xw.astype(np.clongdouble if np.iscomplexobj(xw) else np.longdouble)
    m = np.longdouble(int(np.prod([a.shape[ax] for ax in fit_axes])))
    out = a - a.sum(axis=fit_axes, keepdims=True) / m
    if kind == L.DETREND_LINEAR:
        for ax in fit_axes:
            n = a.shape[ax]
            if n == 1:
                continue
            s = [1] * a.ndim
            s[ax] = n
            c = (np.arange(n, dtype=np.longdouble) - (np.longdouble(n - 1) / 2 + np.longdouble(centre_off))).reshape(s)
            den = m * np.longdouble(n * n if square_denominator else n * n - 1) / 12
            out = out - c * ((a * c).sum(axis=fit_axes, keepdims=True) / den)
    return out


def plain_detrend(x, fit_axes, kind):
    """The same formula at WORKING precision: centred moments with numpy.sum in the data's precision, the fit subtracted in that precision.  Every fit is laid out
    contiguously first (the fit axes last, flattened), so that numpy.sum is its pairwise sum whatever the layout of the case (summed where they lie, the 16400 strided
    samples of a (8200, 2) fit with 3 inner elements are added one by one: 39 u against 3).  The yardstick C_OP is measured on (reference_rendering_figures), never a reference."""
    fit_axes = tuple(fit_axes)
    nf = len(fit_axes)
    rt = np.dtype(REAL[x.dtype.name]).type
    a = np.ascontiguousarray(np.moveaxis(x, fit_axes, tuple(range(-nf, 0))))
    fshape = a.shape[-nf:]
    m = rt(int(np.prod(fshape)))

    def total(v):
        return v.reshape(v.shape[:-nf] + (-1,)).sum(axis=-1, dtype=x.dtype).reshape(v.shape[:-nf] + (1,) * nf)

    out = a - total(a) / m
    if kind == L.DETREND_LINEAR:
        for k, n in enumerate(fshape):
            if n == 1:
                continue
            s = [1] * nf
            s[k] = n
            c = (np.arange(n, dtype=rt) - rt(0.5 * (n - 1))).reshape(s)
            den = m * rt(n * n - 1) / rt(12)
            out = out - c * (total(a * c) / den)
    assert out.dtype == x.dtype
    return np.moveaxis(out, tuple(range(-nf, 0)), fit_axes)


def fit_error(got, ref, xw, fit_axes, name):
    """The worst of max |got - ref| / max |x| over the fits (one per independent element and per component), in units of u."""
    fit_axes = tuple(fit_axes)
    g = got.astype(ref.dtype)
    worst = 0.0
    for part in ((np.real, np.imag) if np.iscomplexobj(xw) else (np.asarray,)):
        d = np.abs(part(g) - part(ref)).max(axis=fit_axes)
        s = np.abs(part(xw)).max(axis=fit_axes)
        worst = max(worst, rel_u(d, s, name))
    return worst


def assert_fit(got, ref, xw, fit_axes, name, what=""):
    c = fit_error(got, ref, xw, fit_axes, name)
    assert c <= C_OP[name], f"{what}: max |got - ref| = {c:.2f} u max |x| in some fit > C_OP = {C_OP[name]}"
    return c


# ---------------------------------------------------------------------------------- detrend over trailing axes (xrfthip_detrend)
# (id, ndim, (batch, ny, nx) or (batch, nx), what the shape reaches -- asserted by arithmetic in check_detrend)
DETREND = [
    ("1x1", 2, (3, 1, 1), "degenerate"),
    ("1x2", 2, (3, 1, 2), "degenerate"),
    ("1x5", 2, (3, 1, 5), "degenerate"),
    ("5x1", 2, (3, 5, 1), "degenerate"),
    ("row257", 1, (2, 257), "row-tail"),
    ("row1025", 1, (2, 1025), "unroll-tail"),
    ("row20000", 1, (2, 20000), "flush"),
    ("63x7", 2, (2, 63, 7), "few-chunks"),
    ("65x1030", 2, (2, 65, 1030), "ragged-deal"),
    ("130x3", 2, (2, 130, 3), "ragged-deal"),
    ("700x750", 2, (1, 700, 750), "apply-wrap"),
    ("32774-of-2x3", 2, (32774, 2, 3), "second-launch"),
    ("32774-rows-of-5", 1, (32774, 5), "second-launch"),
]
EMU_SKIP = {"32774-of-2x3", "32774-rows-of-5", "32770-of-2x2x3", "65540-of-2x2x2"}  # the second launch of a batch loop: 10^5 workgroups of fibers, 30 s a call on the emulator; the GPU suite runs them


def _reaches_detrend(batch, ny, nx, what):
    chunks = max(1, min(ny, 64, DETREND_SLABS_PER_LAUNCH // min(batch, DETREND_SLABS_PER_LAUNCH)))
    if what == "degenerate":
        return ny == 1 or nx == 1
    if what == "row-tail":
        return 256 < nx < 2 * 256
    if what == "unroll-tail":
        return nx > 4 * 256 and nx % (4 * 256) != 0
    if what == "flush":
        return (nx + 255) // 256 > FLUSH_TERMS
    if what == "few-chunks":
        return chunks == ny < 64
    if what == "ragged-deal":
        return chunks == 64 and ny % chunks != 0
    if what == "apply-wrap":
        return ny * nx > DETREND_APPLY_GRID
    if what == "second-launch":
        return batch > DETREND_SLABS_PER_LAUNCH and chunks == 1
    raise ValueError(what)


def check_detrend(case, name, kind):
    cid, ndim, shape, what = case
    batch, ny, nx = (shape[0], 1, shape[1]) if ndim == 1 else shape
    assert _reaches_detrend(batch, ny, nx, what), (cid, what)
    dll = L.load()
    rng = np.random.default_rng(1000 + len(cid) + 7 * ndim)
    fit = tuple(range(1, len(shape)))
    x, xw = trend_field(rng, shape, fit, name)
    ref = ref_detrend(xw, fit, KINDS[kind])
    xin = dev_bytes(x)
    nws = int(dll.xrfthip_detrend_workspace_bytes(batch))
    ws = scratch(nws)
    got = run_twice(shape, name, lambda out: dll.xrfthip_detrend(CODE[name], ndim, batch, ny, nx, KINDS[kind], xin.data_ptr(), out, ws.data_ptr(), nws, stream()))
    c = assert_fit(got, ref, xw, fit, name, f"detrend {cid} {name} {kind}")
    # in place (d_in == d_out): the bits of the out-of-place result
    inplace = run_twice(shape, name, lambda out: dll.xrfthip_detrend(CODE[name], ndim, batch, ny, nx, KINDS[kind], out, out, ws.data_ptr(), nws, stream()), fill=x)
    assert inplace.tobytes() == got.tobytes(), f"detrend {cid} {name} {kind}: in place differs from out of place"
    return note("detrend", name, c)


# ---------------------------------------------------------------------------------- detrend over three trailing axes (xrfthip_detrend3)
DETREND3 = [
    ("2x3x4", (2, 2, 3, 4), "small"),
    ("1x1x7", (2, 1, 1, 7), "degenerate-leading"),
    ("70x1x1", (1, 70, 1, 1), "degenerate-trailing"),
    ("5x3x300", (2, 5, 3, 300), "rows"),
    ("65x64x3", (1, 65, 64, 3), "row-cap"),
    ("2x2x20000", (1, 2, 2, 20000), "flush"),
    ("32770-of-2x2x3", (32770, 2, 2, 3), "second-launch"),
]


def check_detrend3(case, name, kind):
    cid, shape, what = case
    batch, n0, n1, n2 = shape
    reaches = {"small": True, "degenerate-leading": n0 == n1 == 1, "degenerate-trailing": n1 == n2 == 1, "rows": n2 > 256,
               "row-cap": n0 * n1 > DETREND3_ROW_BLOCKS, "flush": (n2 + 255) // 256 > FLUSH_TERMS, "second-launch": batch > DETREND_SLABS_PER_LAUNCH}
    assert reaches[what], (cid, what)
    dll = L.load()
    rng = np.random.default_rng(2000 + len(cid))
    x, xw = trend_field(rng, shape, (1, 2, 3), name)
    ref = ref_detrend(xw, (1, 2, 3), KINDS[kind])
    xin = dev_bytes(x)
    nws = int(dll.xrfthip_detrend_workspace_bytes(batch))
    ws = scratch(nws)
    got = run_twice(shape, name, lambda out: dll.xrfthip_detrend3(CODE[name], batch, n0, n1, n2, KINDS[kind], xin.data_ptr(), out, ws.data_ptr(), nws, stream()))
    return note("detrend3", name, assert_fit(got, ref, xw, (1, 2, 3), name, f"detrend3 {cid} {name} {kind}"))


# ---------------------------------------------------------------------------------- detrend with the independent elements innermost (xrfthip_detrend_inner)
# (id, shape, first fit axis, fit axes, what).  Inner extents 1, 3, 300, 700, 1030, 1800 real components -- twice that for a complex field.
INNER = [
    ("5x7-inner1", (2, 5, 7, 1), 1, 2, "inner1"),
    ("9x4-inner300", (1, 9, 4, 300), 1, 2, "inner-over-256"),
    ("5x3-inner700", (1, 5, 3, 700), 1, 2, "inner-over-256"),
    ("6x5-inner1030", (1, 6, 5, 1030), 1, 2, "two-tiles"),
    ("4x3-inner1800", (1, 4, 3, 1800), 1, 2, "coef-from-memory"),
    ("33-inner257", (2, 33, 257), 1, 1, "one-axis"),
    ("1x1-inner5", (3, 1, 1, 5), 1, 2, "degenerate"),
    ("300x2-inner2", (1, 300, 2, 2), 1, 2, "many-rows"),
    ("8200x2x3", (1, 8200, 2, 3), 1, 2, "apply-cap"),
    ("65540-of-2x2x2", (65540, 2, 2, 2), 1, 2, "second-launch"),
]


def check_detrend_inner(case, name, kind):
    cid, shape, axis0, naxes, what = case
    cplx = name.startswith("complex")
    batch = int(np.prod(shape[:axis0]))
    ny = shape[axis0] if naxes == 2 else 1
    nx = shape[axis0 + naxes - 1]
    inner = int(np.prod(shape[axis0 + naxes:]))
    i2 = inner * (2 if cplx else 1)
    reaches = {"inner1": inner == 1, "inner-over-256": i2 > 256 and 256 % i2 != 0, "two-tiles": i2 > INNER_THREADS and i2 % INNER_THREADS != 0,
               "coef-from-memory": i2 * 24 > INNER_LDS_COEF_BYTES, "one-axis": naxes == 1 and 256 % i2 != 0, "degenerate": ny == nx == 1,
               "many-rows": ny > 256, "apply-cap": batch * ny > INNER_APPLY_GRID and INNER_THREADS % i2 != 0,  # (and not every lane of the moments kernel is live: 1023 of 1024 at 3 components)
               "second-launch": batch > INNER_SLABS_PER_LAUNCH}
    assert reaches[what], (cid, what)
    dll = L.load()
    rng = np.random.default_rng(3000 + len(cid))
    fit = tuple(range(axis0, axis0 + naxes))
    x, xw = trend_field(rng, shape, fit, name)
    ref = ref_detrend(xw, fit, KINDS[kind])
    xin = dev_bytes(x)
    nws = int(dll.xrfthip_detrend_inner_workspace_bytes(CODE[name], batch, inner))
    ws = scratch(nws)
    got = run_twice(shape, name, lambda out: dll.xrfthip_detrend_inner(CODE[name], naxes, batch, ny, nx, inner, KINDS[kind], xin.data_ptr(), out, ws.data_ptr(), nws, stream()))
    c = assert_fit(got, ref, xw, fit, name, f"detrend_inner {cid} {name} {kind}")
    # the wrapper takes this case (it returns None where it declines: the caller transposes) and gives the same bits
    w = engine.detrend_inner(torch.from_numpy(x).to(dev()), axis0, naxes, KINDS[kind])
    assert isinstance(w, torch.Tensor), f"engine.detrend_inner declined {cid} {name}"
    assert w.cpu().numpy().tobytes() == got.tobytes()
    return note("detrend_inner", name, c)


def detrend_params(cases, emulated=False):
    """(case, dtype, kind) of every case; emulated: without the cases of EMU_SKIP."""
    return [pytest.param(case, name, kind, id=f"{case[0]}-{name}-{kind}") for case in cases if not (emulated and case[0] in EMU_SKIP) for name in NAMES for kind in KINDS]


def reference_rendering_figures():
    """The worst error of plain_detrend against ref_detrend over every detrend case, per precision, in units of u max |x| per fit: what C_OP is 4x of."""
    worst = {"float32": 0.0, "float64": 0.0}
    todo = [(c[2], tuple(range(1, len(c[2]))), 1000 + len(c[0]) + 7 * c[1]) for c in DETREND]
    todo += [(c[1], (1, 2, 3), 2000 + len(c[0])) for c in DETREND3]
    todo += [(c[1], tuple(range(c[2], c[2] + c[3])), 3000 + len(c[0])) for c in INNER]
    for shape, fit, seed in todo:
        for name in NAMES:
            for kind in KINDS.values():
                x, xw = trend_field(np.random.default_rng(seed), shape, fit, name)
                c = fit_error(plain_detrend(x, fit, kind), ref_detrend(xw, fit, kind), xw, fit, name)
                worst[REAL[name]] = max(worst[REAL[name]], c)
    return worst


# ---------------------------------------------------------------------------------- spectrum_tail, spectrum_tail_axis
TAIL_N = [1, 255, 257]
TAIL_WRAP_N = TAIL_GRID + 257  # the grid-stride loop wraps (complex64 only: 100 MB with b and the result)
SCALE = 0.37 / 1021.0          # (no power of two: the cast of `scale` to float32 rounds)
TAIL_AXIS = [(3, 1, 4), (3, 2, 4), (2, 5, 1), (1, 5, 1), (2, 6, 3), (4, 7, 1)]  # (outer, na, inner); at na = 1, k = 0 is also the last


def ref_tail(aw, bw, f, name):
    """(|a|^2 f or a conj(b) f, the bound's scale per element) in the reference precision; f: `scale`, or the array of real-dim factors times it."""
    rt, ct = hp(name)
    a = aw.astype(ct)
    f = np.asarray(f, dtype=rt)
    if bw is None:
        ref = (a.real * a.real + a.imag * a.imag) * f
        return ref, np.abs(ref)
    b = bw.astype(ct)
    return a * np.conj(b) * f, np.abs(a) * np.abs(b) * np.abs(f)


def assert_tail(got, ref, scale_of, name, cross, what=""):
    c = rel_u(np.abs(got.astype(ref.dtype) - ref), scale_of, name)
    bound = C_CROSS if cross else C_POWER
    assert c <= bound, f"{what}: {c:.2f} u > {bound}"
    return c


def realdim_factor(outer, na, inner, last_is_one, at_zero=1.0, ignore_last=False):
    """[1, 2, ..., 2, (1 if last_is_one)] along the middle axis of (outer, na, inner); at_zero / ignore_last: the faults of check_sensitivity."""
    f = np.full(na, 2.0)
    if last_is_one and not ignore_last:
        f[na - 1] = 1.0
    f[0] = at_zero
    return np.broadcast_to(f.reshape(1, na, 1), (outer, na, inner))


def check_spectrum_tail(n, name, cross):
    dll = L.load()
    if n > TAIL_GRID:
        assert n > 16384 * 256 and n % 256 != 0
    rng = np.random.default_rng(4000 + n % 1000)
    a, aw = samples(rng, (n,), name)
    b, bw = samples(rng, (n,), name) if cross else (None, None)
    ref, sc = ref_tail(aw, bw, SCALE, name)
    da, db = dev_bytes(a), (dev_bytes(b) if cross else None)
    got = run_twice((n,), name if cross else REAL[name],
                    lambda out: dll.xrfthip_spectrum_tail(CODE[name], n, da.data_ptr(), db.data_ptr() if cross else None, out, SCALE, stream()))
    return note("cross" if cross else "power", name, assert_tail(got, ref, sc, name, cross, f"spectrum_tail n={n} {name}"))


def check_spectrum_tail_axis(shape, last_is_one, name, cross):
    dll = L.load()
    outer, na, inner = shape
    rng = np.random.default_rng(4100 + 100 * outer + 10 * na + inner)
    a, aw = samples(rng, shape, name)
    b, bw = samples(rng, shape, name) if cross else (None, None)
    ref, sc = ref_tail(aw, bw, realdim_factor(outer, na, inner, last_is_one) * SCALE, name)
    da, db = dev_bytes(a), (dev_bytes(b) if cross else None)
    got = run_twice(shape, name if cross else REAL[name],
                    lambda out: dll.xrfthip_spectrum_tail_axis(CODE[name], outer, na, inner, int(last_is_one), da.data_ptr(), db.data_ptr() if cross else None, out, SCALE, stream()))
    return note("cross" if cross else "power", name, assert_tail(got, ref, sc, name, cross, f"spectrum_tail_axis {shape} last_is_one={last_is_one} {name}"))


# ---------------------------------------------------------------------------------- gather_axis
GATHER_SHAPES = [((3, 7, 1), 1), ((3, 7, 5), 1), ((7,), 0), ((2, 1, 3), 1), ((300, 5), 0)]  # (shape, axis)
ROLLS = [0, 1, -1, 3, -10, 23]  # (beyond the axis, and negative)


def gather_indices(n):
    """An index longer than the axis, one of length 1, one with repeated entries."""
    return [(np.arange(n + 4)[::-1] * 3) % n, np.array([n - 1]), np.array([0, 0, n - 1, 0, n // 2, n // 2])]


def check_gather_axis(shape, axis, esz):
    dll = L.load()
    rng = np.random.default_rng(5000 + esz + len(shape))
    n_in = shape[axis]
    outer, inner = int(np.prod(shape[:axis])), int(np.prod(shape[axis + 1:]))
    x = rng.integers(0, 256, size=tuple(shape) + (esz,), dtype=np.uint8)  # any bit pattern: elements are copied by size, not read as numbers
    xv = x.view(np.dtype((np.void, esz))).reshape(shape)
    dx = dev_bytes(x)
    for roll in ROLLS:
        got = run_twice(shape, xv.dtype, lambda out: dll.xrfthip_gather_axis(esz, outer, n_in, inner, n_in, None, roll, dx.data_ptr(), out, stream()))
        assert got.tobytes() == np.roll(xv, roll, axis=axis).tobytes(), f"gather_axis {shape} axis {axis} roll {roll}, {esz}-byte elements"
    for index in gather_indices(n_in):
        didx = dev_bytes(index.astype(np.int64))
        oshape = list(shape)
        oshape[axis] = index.size
        got = run_twice(oshape, xv.dtype, lambda out: dll.xrfthip_gather_axis(esz, outer, index.size, inner, n_in, didx.data_ptr(), 0, dx.data_ptr(), out, stream()))
        assert got.tobytes() == np.take(xv, index, axis=axis).tobytes(), f"gather_axis {shape} axis {axis} index {index}, {esz}-byte elements"


# ---------------------------------------------------------------------------------- table_mul
TABLE_MUL = [(1, 1, 1), (3, 5, 8), (3, 8, 5), (2, 300, 257), (2, 257, 600)]  # (batch, n_in, n_out)


def ref_table_mul(xw, tw, n_out, name, table_shift=0):
    """(x[j] table[j] for j < min(n_in, n_out), the bound's scale |x| |table|); table_shift: the fault of check_sensitivity."""
    _rt, ct = hp(name)
    m = min(xw.shape[-1], n_out)
    t = np.roll(tw, table_shift)[:m].astype(ct)
    xs = xw[..., :m].astype(ct)
    return xs * t, np.abs(xs) * np.abs(t)


def assert_table_mul(got, ref, sc, name, what=""):
    c = rel_u(np.abs(got.astype(ref.dtype) - ref), sc, name)
    assert c <= C_TABLE_MUL, f"{what}: {c:.2f} u |x| |table| > {C_TABLE_MUL}"
    return c


def check_table_mul(case, name):
    dll = L.load()
    batch, n_in, n_out = case
    rng = np.random.default_rng(6000 + n_in + n_out)
    x, xw = samples(rng, (batch, n_in), name)
    t, tw = samples(rng, (min(n_in, n_out),), CPLX[name])
    dx, dt = dev_bytes(x), dev_bytes(t)
    got = run_twice((batch, n_out), CPLX[name], lambda out: dll.xrfthip_table_mul(CODE[name], batch, n_in, n_out, dx.data_ptr(), dt.data_ptr(), out, stream()))
    m = min(n_in, n_out)
    pad = got[:, m:].view(REAL[name])
    assert not pad.any() and not np.signbit(pad).any(), f"table_mul {case} {name}: the padded part is not +0"
    ref, sc = ref_table_mul(xw, tw, n_out, name)
    return note("table_mul", name, assert_table_mul(got[:, :m], ref, sc, name, f"table_mul {case} {name}"))


# ---------------------------------------------------------------------------------- angle
ANGLE_N = 5000
# (re, im)
ANGLE_SPECIALS = [(-1.0, 0.0), (-1.0, -0.0), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (np.nan, 1.0), (np.inf, np.inf), (-np.inf, -0.0)]


def angle_inputs(name):
    return samples(np.random.default_rng(7000), (ANGLE_N,), name)


def angle_ulp_error(got, aw, name):
    """max |got - arctan2 in long double| in ulp of the result's precision."""
    ref = np.arctan2(aw.imag.astype(np.longdouble), aw.real.astype(np.longdouble))
    ulp = np.spacing(np.abs(ref).astype(REAL[name])).astype(np.longdouble)
    return float((np.abs(got.astype(np.longdouble) - ref) / ulp).max())


def check_angle(name):
    dll = L.load()
    a, aw = angle_inputs(name)
    da = dev_bytes(a)
    got = run_twice((ANGLE_N,), REAL[name], lambda out: dll.xrfthip_angle(CODE[name], ANGLE_N, da.data_ptr(), out, stream()))
    c = angle_ulp_error(got, aw, name)
    bound = 1.0 if name == "complex64" else C_ANGLE_F64
    assert c <= bound, f"angle {name}: {c:.3f} ulp > {bound}"
    return note("angle", name, c)


def check_angle_specials(name):
    dll = L.load()
    s = np.array([complex(re, im) for re, im in ANGLE_SPECIALS]).astype(name)
    assert np.array_equal(np.signbit(s.real), [np.signbit(re) for re, _ in ANGLE_SPECIALS])  # (the signs of zero reached the array)
    ds = dev_bytes(s)
    got = run_twice(s.shape, REAL[name], lambda out: dll.xrfthip_angle(CODE[name], s.size, ds.data_ptr(), out, stream()))
    want = np.angle(s.astype(np.complex128)).astype(REAL[name])
    for (re, im), g, w in zip(ANGLE_SPECIALS, got, want):
        assert np.isnan(g) == np.isnan(w) and (np.isnan(w) or (g == w and np.signbit(g) == np.signbit(w))), f"angle({re}, {im}) {name}: {g!r}, numpy.angle {w!r}"


# ---------------------------------------------------------------------------------- convert (float32 <-> float64, complex64 <-> complex128)
# (float16 / bfloat16 -> float32 from a source one sample in -- 2-byte but not 4-byte aligned, the `pairs = 0` branch of widen16_kernel, with an odd count -- is not
# repeated here: test_half_input_emulated.py::test_convert_is_exact_on_every_bit_pattern and its GPU twin convert x[1:] of all 65 536 patterns, 65 535 samples.)
CONVERT_WRAP_N = CONVERT_GRID + 3
CONVERT_N = [1, 7, 1001, CONVERT_WRAP_N]
_F32_SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 1.0, 1.0000001]
# to float32: a tie (1 + 2^-24 -> 1, to even; 1 + 3 2^-24 -> 1 + 2^-22, to even the other way), results that are denormal in float32, FLT_MAX, the first value
# that rounds to inf (FLT_MAX + half an ulp: a tie, to even = inf) and 3.5e38, the largest value that still rounds to FLT_MAX, underflow to 0
_F64_SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * 1.0000001,
                 1e-320, 3.4028234663852886e38, 3.4028235677973366e38, np.nextafter(3.4028235677973366e38, 0.0), 3.5e38, -3.5e38, 1e300]


def check_convert(n, src):
    """n elements of `src` to the other precision: the bits of astype (NaN: NaN)."""
    dll = L.load()
    if n > 1001:
        assert n * (2 if src.startswith("complex") else 1) > CONVERT_GRID and n % 2 == 1
    wider = {"float32": "float64", "complex64": "complex128"}
    dst = wider.get(src) or {v: k for k, v in wider.items()}[src]
    rng = np.random.default_rng(8000 + n % 100)
    sp = np.array(_F32_SPECIALS if REAL[src] == "float32" else _F64_SPECIALS, dtype=REAL[src])
    v = (rng.standard_normal(2 * n) * 10.0 ** rng.integers(-3, 4, 2 * n)).astype(REAL[src])
    k = min(sp.size, 2 * n)
    v[:k] = sp[:k]
    if n > sp.size:
        v[-sp.size:] = sp[::-1]  # ... and at the far end (behind the wrap of the long case)
    if src.startswith("complex"):
        x = np.empty(n, dtype=src)  # (component by component: 1j * inf would put a NaN into the real part)
        x.real, x.imag = v[:n], v[n:]
    else:
        x = v[:n].copy()
    dx = dev_bytes(x)
    got = run_twice((n,), dst, lambda out: dll.xrfthip_convert(CODE[src], CODE[dst], n, dx.data_ptr(), out, stream()))
    with np.errstate(over="ignore"):
        want = x.astype(dst)
    g, w = got.view(REAL[dst]), want.view(REAL[dst])
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan) and g[~nan].tobytes() == w[~nan].tobytes(), f"convert {src} -> {dst}, n = {n}: differs from astype at {np.flatnonzero((g != w) & ~nan)[:8]}"


# ---------------------------------------------------------------------------------- the bounds reject what they are there to reject (numpy only: no kernel)
def check_sensitivity():
    """Each fault is applied to the REFERENCE; the correct reference, rounded to the output's precision, passes the bound, and the faulty one fails it."""
    rng = np.random.default_rng(9000)
    lin = L.DETREND_LINEAR
    for name in NAMES:
        # the centre of a 3-row fit off by a half; n^2 for n^2 - 1 at n = 2 and 5
        for shape, fault in (((2, 3, 4), dict(centre_off=0.5)), ((2, 2, 7), dict(square_denominator=True)), ((2, 5, 5), dict(square_denominator=True))):
            x, xw = trend_field(rng, shape, (1, 2), name)
            ref = ref_detrend(xw, (1, 2), lin)
            assert_fit(ref.astype(name), ref, xw, (1, 2), name)
            with pytest.raises(AssertionError):
                assert_fit(ref_detrend(xw, (1, 2), lin, **fault).astype(name), ref, xw, (1, 2), name)
    # (at n = 20000 the same perturbation of the denominator is below u in float32: why the small shapes are in the case lists)
    x, xw = trend_field(rng, (1, 20000), (1,), "float32")
    ref = ref_detrend(xw, (1,), lin)
    assert fit_error(ref_detrend(xw, (1,), lin, square_denominator=True).astype("float32"), ref, xw, (1,), "float32") <= C_OP["float32"]
    for name in CNAMES:
        shape = (2, 6, 3)
        a, aw = samples(rng, shape, name)
        b, bw = samples(rng, shape, name)
        for cross in (False, True):
            good = realdim_factor(*shape, 1) * SCALE
            ref, sc = ref_tail(aw, bw if cross else None, good, name)
            assert_tail(ref.astype(name if cross else REAL[name]), ref, sc, name, cross)
            # the real-dim factor 2 at k = 0; last_is_one ignored
            for bad in (realdim_factor(*shape, 1, at_zero=2.0), realdim_factor(*shape, 1, ignore_last=True)):
                wrong, _ = ref_tail(aw, bw if cross else None, bad * SCALE, name)
                with pytest.raises(AssertionError):
                    assert_tail(wrong.astype(name if cross else REAL[name]), ref, sc, name, cross)
    # a roll by -r in place of r
    xv = rng.integers(0, 256, size=(3, 7, 4), dtype=np.uint8)
    assert np.roll(xv, 3, axis=1).tobytes() != np.roll(xv, -3, axis=1).tobytes()
    # a table index off by one
    for name in NAMES:
        x, xw = samples(rng, (3, 8), name)
        _t, tw = samples(rng, (8,), CPLX[name])
        ref, sc = ref_table_mul(xw, tw, 8, name)
        assert_table_mul(ref.astype(CPLX[name]), ref, sc, name)
        with pytest.raises(AssertionError):
            assert_table_mul(ref_table_mul(xw, tw, 8, name, table_shift=1)[0].astype(CPLX[name]), ref, sc, name)


# ---------------------------------------------------------------------------------- status codes
WORKSPACE_TOO_SMALL = -3


def check_status_codes():
    """Every documented refusal answers before anything is launched (the pointers that are not null point at 4 KB buffers, the sizes are tiny), and every
    zero-size call answers OK with its sentinel-filled output untouched."""
    dll = L.load()
    assert "workspace" in dll.xrfthip_strerror(WORKSPACE_TOO_SMALL).decode().lower()
    big = 4 << 20
    a, b, ws = scratch(4096), scratch(4096), scratch(big)
    A, B, W, st = a.data_ptr(), b.data_ptr(), ws.data_ptr(), stream()
    lin = L.DETREND_LINEAR
    nws = int(dll.xrfthip_detrend_workspace_bytes(2))
    nwi = int(dll.xrfthip_detrend_inner_workspace_bytes(L.F32, 2, 3))
    assert 0 < nws <= big and 0 < nwi <= big
    assert dll.xrfthip_detrend_inner_workspace_bytes(9, 2, 3) == 0 and dll.xrfthip_detrend_inner_workspace_bytes(L.F32, 2, 0) == 0
    bad = {
        "detrend: null in": lambda: dll.xrfthip_detrend(L.F32, 2, 2, 2, 3, lin, None, B, W, big, st),
        "detrend: null out": lambda: dll.xrfthip_detrend(L.F32, 2, 2, 2, 3, lin, A, None, W, big, st),
        "detrend: dtype": lambda: dll.xrfthip_detrend(L.F16, 2, 2, 2, 3, lin, A, B, W, big, st),
        "detrend: dtype < 0": lambda: dll.xrfthip_detrend(-1, 2, 2, 2, 3, lin, A, B, W, big, st),
        "detrend: ndim 1 with ny 2": lambda: dll.xrfthip_detrend(L.F32, 1, 2, 2, 3, lin, A, B, W, big, st),
        "detrend: ndim 3": lambda: dll.xrfthip_detrend(L.F32, 3, 2, 2, 3, lin, A, B, W, big, st),
        "detrend: kind none": lambda: dll.xrfthip_detrend(L.F32, 2, 2, 2, 3, L.DETREND_NONE, A, B, W, big, st),
        "detrend: kind 3": lambda: dll.xrfthip_detrend(L.F32, 2, 2, 2, 3, 3, A, B, W, big, st),
        "detrend: nx 0": lambda: dll.xrfthip_detrend(L.F32, 2, 2, 2, 0, lin, A, B, W, big, st),
        "detrend: batch < 0": lambda: dll.xrfthip_detrend(L.F32, 2, -1, 2, 3, lin, A, B, W, big, st),
        "detrend3: null in": lambda: dll.xrfthip_detrend3(L.F32, 2, 2, 2, 3, lin, None, B, W, big, st),
        "detrend3: dtype": lambda: dll.xrfthip_detrend3(7, 2, 2, 2, 3, lin, A, B, W, big, st),
        "detrend3: kind": lambda: dll.xrfthip_detrend3(L.F32, 2, 2, 2, 3, 0, A, B, W, big, st),
        "detrend3: n1 0": lambda: dll.xrfthip_detrend3(L.F32, 2, 2, 0, 3, lin, A, B, W, big, st),
        "detrend_inner: null out": lambda: dll.xrfthip_detrend_inner(L.F32, 2, 2, 2, 3, 3, lin, A, None, W, big, st),
        "detrend_inner: dtype": lambda: dll.xrfthip_detrend_inner(L.BF16, 2, 2, 2, 3, 3, lin, A, B, W, big, st),
        "detrend_inner: ndim 1 with ny 2": lambda: dll.xrfthip_detrend_inner(L.F32, 1, 2, 2, 3, 3, lin, A, B, W, big, st),
        "detrend_inner: kind": lambda: dll.xrfthip_detrend_inner(L.F32, 2, 2, 2, 3, 3, 5, A, B, W, big, st),
        "detrend_inner: inner 0": lambda: dll.xrfthip_detrend_inner(L.F32, 2, 2, 2, 3, 0, lin, A, B, W, big, st),
        "detrend_inner: inner > 2^30": lambda: dll.xrfthip_detrend_inner(L.F32, 2, 2, 2, 3, (1 << 30) + 1, lin, A, B, W, big, st),
        "spectrum_tail: null a": lambda: dll.xrfthip_spectrum_tail(L.C64, 4, None, None, B, 1.0, st),
        "spectrum_tail: null out": lambda: dll.xrfthip_spectrum_tail(L.C64, 4, A, None, None, 1.0, st),
        "spectrum_tail: real dtype": lambda: dll.xrfthip_spectrum_tail(L.F32, 4, A, None, B, 1.0, st),
        "spectrum_tail: n < 0": lambda: dll.xrfthip_spectrum_tail(L.C64, -1, A, None, B, 1.0, st),
        "spectrum_tail_axis: null a": lambda: dll.xrfthip_spectrum_tail_axis(L.C64, 2, 2, 2, 1, None, None, B, 1.0, st),
        "spectrum_tail_axis: real dtype": lambda: dll.xrfthip_spectrum_tail_axis(L.F64, 2, 2, 2, 1, A, None, B, 1.0, st),
        "spectrum_tail_axis: na 0": lambda: dll.xrfthip_spectrum_tail_axis(L.C64, 2, 0, 2, 1, A, None, B, 1.0, st),
        "spectrum_tail_axis: inner 0": lambda: dll.xrfthip_spectrum_tail_axis(L.C64, 2, 2, 0, 1, A, None, B, 1.0, st),
        "angle: null a": lambda: dll.xrfthip_angle(L.C64, 4, None, B, st),
        "angle: null out": lambda: dll.xrfthip_angle(L.C64, 4, A, None, st),
        "angle: real dtype": lambda: dll.xrfthip_angle(L.F32, 4, A, B, st),
        "gather_axis: null in": lambda: dll.xrfthip_gather_axis(4, 2, 2, 2, 2, None, 1, None, B, st),
        "gather_axis: in place": lambda: dll.xrfthip_gather_axis(4, 2, 2, 2, 2, None, 1, A, A, st),
        "gather_axis: element size 3": lambda: dll.xrfthip_gather_axis(3, 2, 2, 2, 2, None, 1, A, B, st),
        "gather_axis: element size 2": lambda: dll.xrfthip_gather_axis(2, 2, 2, 2, 2, None, 1, A, B, st),
        "gather_axis: n_in 0": lambda: dll.xrfthip_gather_axis(4, 2, 2, 2, 0, None, 1, A, B, st),
        "table_mul: null table": lambda: dll.xrfthip_table_mul(L.F32, 2, 2, 2, A, None, B, st),
        "table_mul: null in": lambda: dll.xrfthip_table_mul(L.F32, 2, 2, 2, None, W, B, st),
        "table_mul: dtype": lambda: dll.xrfthip_table_mul(L.F16, 2, 2, 2, A, W, B, st),
        "table_mul: n_out 0": lambda: dll.xrfthip_table_mul(L.F32, 2, 2, 0, A, W, B, st),
        "convert: null in": lambda: dll.xrfthip_convert(L.F32, L.F64, 4, None, B, st),
        "convert: same dtype": lambda: dll.xrfthip_convert(L.F32, L.F32, 4, A, B, st),
        "convert: real to complex": lambda: dll.xrfthip_convert(L.F32, L.C128, 4, A, B, st),
        "convert: to half": lambda: dll.xrfthip_convert(L.F32, L.F16, 4, A, B, st),
        "convert: n < 0": lambda: dll.xrfthip_convert(L.F32, L.F64, -1, A, B, st),
        "convert: half input at an odd address": lambda: dll.xrfthip_convert(L.F16, L.F32, 4, A + 1, B, st),
        "convert: half input to an output off 4 bytes": lambda: dll.xrfthip_convert(L.BF16, L.F32, 4, A, B + 2, st),
        "reduce_axis: null out": lambda: dll.xrfthip_reduce_axis(L.F32, 2, 2, 2, A, None, 1.0, st),
        "reduce_axis: dtype": lambda: dll.xrfthip_reduce_axis(L.F16, 2, 2, 2, A, B, 1.0, st),
        "reduce_axis: n 0": lambda: dll.xrfthip_reduce_axis(L.F32, 2, 0, 2, A, B, 1.0, st),
    }
    for what, call in bad.items():
        assert call() == L.BAD_ARG, what
    small = {
        "detrend: one byte under": lambda: dll.xrfthip_detrend(L.F32, 2, 2, 2, 3, lin, A, B, W, nws - 1, st),
        "detrend: null workspace": lambda: dll.xrfthip_detrend(L.F32, 2, 2, 2, 3, lin, A, B, None, nws, st),
        "detrend3: one byte under": lambda: dll.xrfthip_detrend3(L.F32, 2, 2, 2, 3, lin, A, B, W, nws - 1, st),
        "detrend_inner: one byte under": lambda: dll.xrfthip_detrend_inner(L.F32, 2, 2, 2, 3, 3, lin, A, B, W, nwi - 1, st),
        "detrend_inner: null workspace": lambda: dll.xrfthip_detrend_inner(L.F32, 2, 2, 2, 3, 3, lin, A, B, None, nwi, st),
    }
    for what, call in small.items():
        assert call() == WORKSPACE_TOO_SMALL, what
    # at the queried size the same calls run (2 slabs of 2 x 3 (x 3) float32: 144 bytes of the 4 KB buffers)
    assert dll.xrfthip_detrend(L.F32, 2, 2, 2, 3, lin, A, B, W, nws, st) == 0
    assert dll.xrfthip_detrend_inner(L.F32, 2, 2, 2, 3, 3, lin, A, B, W, nwi, st) == 0
    empty = {
        "detrend: batch 0": lambda out: dll.xrfthip_detrend(L.F32, 2, 0, 2, 3, lin, A, out, W, big, st),
        "detrend3: batch 0": lambda out: dll.xrfthip_detrend3(L.F32, 0, 2, 2, 3, lin, A, out, W, big, st),
        "detrend_inner: batch 0": lambda out: dll.xrfthip_detrend_inner(L.F32, 2, 0, 2, 3, 3, lin, A, out, W, big, st),
        "spectrum_tail: n 0": lambda out: dll.xrfthip_spectrum_tail(L.C64, 0, A, None, out, 1.0, st),
        "spectrum_tail_axis: outer 0": lambda out: dll.xrfthip_spectrum_tail_axis(L.C64, 0, 2, 2, 1, A, None, out, 1.0, st),
        "angle: n 0": lambda out: dll.xrfthip_angle(L.C64, 0, A, out, st),
        "gather_axis: outer 0": lambda out: dll.xrfthip_gather_axis(4, 0, 2, 2, 2, None, 1, A, out, st),
        "gather_axis: n_out 0": lambda out: dll.xrfthip_gather_axis(4, 2, 0, 2, 2, W, 0, A, out, st),
        "gather_axis: inner 0": lambda out: dll.xrfthip_gather_axis(4, 2, 2, 0, 2, None, 1, A, out, st),
        "table_mul: batch 0": lambda out: dll.xrfthip_table_mul(L.F32, 0, 2, 2, A, W, out, st),
        "convert: n 0": lambda out: dll.xrfthip_convert(L.F32, L.F64, 0, A, out, st),
        "convert: n 0, half": lambda out: dll.xrfthip_convert(L.F16, L.F32, 0, A, out, st),
        "reduce_axis: outer 0": lambda out: dll.xrfthip_reduce_axis(L.F32, 0, 2, 2, A, out, 1.0, st),
        "reduce_axis: inner 0": lambda out: dll.xrfthip_reduce_axis(L.F32, 2, 2, 0, A, out, 1.0, st),
    }
    for what, call in empty.items():
        g = Guarded((32,), np.float32)  # (no element belongs to the call: all of it must stay the sentinel)
        assert call(g.ptr) == 0, what
        assert (g.buf.cpu().numpy() == SENT).all(), what


def check_wrapper_errors():
    """The ValueError / TypeError paths of the engine.* wrappers: refused in Python, before the library is called."""
    d = dev()
    f = torch.zeros((4, 6), dtype=torch.float32, device=d)
    c = torch.zeros((4, 6), dtype=torch.complex64, device=d)
    i = torch.zeros((4, 6), dtype=torch.int32, device=d)
    for call in (lambda: engine.detrend(f.t(), 2, L.DETREND_LINEAR), lambda: engine.detrend(i, 2, L.DETREND_LINEAR), lambda: engine.detrend(f.t(), 3, L.DETREND_LINEAR),
                 lambda: engine.detrend_inner(f.t(), 0, 1, L.DETREND_LINEAR), lambda: engine.detrend_inner(i, 0, 1, L.DETREND_LINEAR),
                 lambda: engine.convert(f, torch.float64, out=torch.zeros((4, 6), dtype=torch.float32, device=d)),
                 lambda: engine.convert(f, torch.float64, out=torch.zeros((4, 5), dtype=torch.float64, device=d)),
                 lambda: engine.convert(f, torch.float64, out=torch.zeros((6, 4), dtype=torch.float64, device=d).t()),
                 lambda: engine.spectrum_tail(f, None, 1.0), lambda: engine.spectrum_tail(c.t(), None, 1.0), lambda: engine.spectrum_tail(c, c.to(torch.complex128), 1.0),
                 lambda: engine.spectrum_tail(c, c[:2], 1.0), lambda: engine.spectrum_tail(c, c.t().contiguous().t(), 1.0),
                 lambda: engine.spectrum_tail_axis(f, None, 1.0, 0, True), lambda: engine.spectrum_tail_axis(c, c[:, :3], 1.0, 0, True), lambda: engine.spectrum_tail_axis(c.t(), None, 1.0, 0, True),
                 lambda: engine.angle(f),
                 lambda: engine.table_mul(f, torch.zeros(6, dtype=torch.complex128, device=d), 8), lambda: engine.table_mul(f, torch.zeros(5, dtype=torch.complex64, device=d), 8),
                 lambda: engine.table_mul(f, torch.zeros(12, dtype=torch.complex64, device=d)[::2], 8)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: engine.convert(f, torch.float32), lambda: engine.convert(f, torch.complex128), lambda: engine.convert(i, torch.float32),
                 lambda: engine.convert(f.to(torch.float16), torch.float64), lambda: engine.reduce_axis(i, 0)):
        with pytest.raises(TypeError):
            call()
