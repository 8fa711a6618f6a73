"""Rounding-level accuracy bounds, shared by the accuracy ladder and the layout x parity matrix (CPU: tests/test_accuracy_emulated.py,
tests/test_layout_matrix_emulated.py; GPU: tests/test_gpu_accuracy.py).  Not a conftest: imported by the tests that use it.

The contract: against the plain float64 transform of the SAME samples (the float32 / complex64 input cast exactly to
float64 / complex128), a result holds

    rms error     || got - ref ||_2 / || ref ||_2               <=  C_RMS * u * log2 N  (+ C_DETREND[dtype] * u * kappa with a detrend)
    max error     max |got - ref| / rms(ref)                    <=  C_MAX * u * log2 N  (+ the same detrend term), flat-spectrum inputs

u = 2^-24 (float32) or 2^-53 (float64), N = the points of ONE transform, kappa = max |x| / rms(x - fit) of a detrended input.  The
norm-wise bound holds for any input (an FFT's error is norm-wise); the max-norm bound only means something on a flat spectrum (seeded
noise), where rms(ref) is the size of a typical bin.  These bounds are 150-1000 times tighter than the float32 bar of tests/cases.py
(3e-4 of the largest bin): a normalisation off by 1/N, a twiddle off by 1e-4 or a phase factor wrong at one position fails them
(test_accuracy_emulated.py::test_the_bound_is_sensitive).
"""
import math

import numpy as np
import pytest
import torch

from xrft_amd import _lib as L
from xrft_amd import engine

import cases

F32, F64, C64, C128 = torch.float32, torch.float64, torch.complex64, torch.complex128

U = {"float32": 2.0 ** -24, "complex64": 2.0 ** -24, "float64": 2.0 ** -53, "complex128": 2.0 ** -53}
C_RMS = 2.0  # fixed: the contract.  Measured worst per family and dtype: DESIGN.md section 2
# max |err| / rms(ref) of seeded noise through OUT_COMPLEX, in units of u log2 N.  Measured worst: 3.24 (complex64 fastr complex rows,
# inverse, 2^14 points; emulator; 2.99 on the MI355X); set at 2.5x
C_MAX = 8.0
# the detrend's conditioning term, per dtype, in units of u * kappa: x - fit is rounded at the magnitude of x, in the product and in the
# oracle alike.  Measured worst excess over C_RMS u log2 N, per unit of u kappa: float64 3.56 (linear + Hann over a 16 x 9 pair of
# non-trailing axes, kappa 8.5, against the oracle's normal-equation plane fit), set at 2.2x.  float32: no case measured an excess
# (<= 0), so there is no value to take 2-4x of; 0.1 is a chosen margin, NOT a multiple of a measurement.  The float32 case it serves:
# a last-sample impulse through the 64 x 128 fasts row with a linear detrend, kappa 91, measured C = 2.00 on the emulator (0.43 on the
# MI355X) -- at C_RMS with no room; the term widens that case's bound by about 35 %.
C_DETREND = {"float32": 0.1, "complex64": 0.1, "float64": 8.0, "complex128": 8.0}


def dtype_name(dtype):
    return str(dtype).replace("torch.", "") if isinstance(dtype, torch.dtype) else np.dtype(dtype).name


def log2n(n):
    return max(math.log2(n), 1.0)


def errors(got, ref):
    """(|| got - ref ||_2 / || ref ||_2, max |got - ref| / rms(ref)) in float64."""
    g = np.asarray(got, dtype=np.complex128 if np.iscomplexobj(got) or np.iscomplexobj(ref) else np.float64)
    r = np.asarray(ref, dtype=g.dtype)
    assert g.shape == r.shape, (g.shape, r.shape)
    d = np.abs(g - r)
    nr = float(np.sqrt(np.mean(np.abs(r) ** 2)))
    if nr == 0.0:
        return float(np.sqrt(np.mean(d ** 2))), float(d.max(initial=0.0))
    return float(np.sqrt(np.mean(d ** 2))) / nr, float(d.max(initial=0.0)) / nr


def bound(dtype, n, kappa=0.0, c=C_RMS):
    """The rms bound of a result of precision `dtype` whose transforms have `n` points each."""
    dt = dtype_name(dtype)
    return c * U[dt] * log2n(n) + C_DETREND[dt] * U[dt] * kappa


def kappa(x, resid):
    """max |x| / rms(x - fit): the conditioning of a detrend (resid = x - fit)."""
    x = np.asarray(x)
    r = float(np.sqrt(np.mean(np.abs(np.asarray(resid)) ** 2)))
    return float(np.abs(x).max()) / r if r > 0 else 0.0


def assert_accurate(got, ref, dtype, n, kap=0.0, flat=False, what=""):
    """The contract: rms error (and, on a flat spectrum, the max error) within the bound.  Returns the rms error in units of u log2 N."""
    rms, mx = errors(got, ref)
    dt = dtype_name(dtype)
    b = bound(dt, n, kap)
    assert rms <= b, f"{what}: rms error {rms:.3e} > {b:.3e} (C = {rms / (U[dt] * log2n(n)):.2f}, N = {n}, kappa = {kap:.1f})"
    if flat:
        bm = bound(dt, n, kap, C_MAX)
        assert mx <= bm, f"{what}: max error / rms(ref) {mx:.3e} > {bm:.3e} ({mx / (U[dt] * log2n(n)):.2f} u log2 N, N = {n})"
    return rms / (U[dt] * log2n(n))


# ---------------------------------------------------------------------------------- the routing table (one row per family, per demotion)
def make(ndim=2, batch=2, ny=1, nx=1, dtype=F32, out_mode=L.OUT_POWER, detrend=L.DETREND_NONE, flags=0, **kw):
    if ndim == 1:
        ny = 1
    return engine.SpectralPlan(ndim=ndim, batch=batch, ny=ny, nx=nx, dtype=dtype, out_mode=out_mode, detrend=detrend, flags=flags, scale=1.0, **kw)


def radial_map(ny, nx):
    ky = np.minimum(np.arange(ny), ny - np.arange(ny))[:, None]
    kx = np.minimum(np.arange(nx), nx - np.arange(nx))[None, :]
    nb = min(ny, nx) // 2 + 1
    return np.minimum(np.floor(np.hypot(ky, kx)).astype(np.int32), nb - 1), nb


def herm_kw(shape, cdtype, mode, flags=0, batch=2):
    """make() arguments of the last pass of a three-axis spectrum (herm_ny / herm_nx): the transform along t of the half spectrum of a (nt, ny, nx) grid."""
    nt, ny, nx = shape
    return dict(batch=batch, ny=nt, nx=ny * (nx // 2 + 1), dtype=cdtype, out_mode=mode, flags=L.AXIS_Y | flags, herm_ny=ny, herm_nx=nx)


def herm_full(v, hny, hnx, conj):
    """[batch][nt][hny (hnx/2 + 1)] values on the stored half of a real grid's spectrum -> the full [batch][nt][hny][hnx] result of a herm_ny / herm_nx plan: the
    columns kx > hnx/2 from the twin (-kt, -ky, -kx), conjugated for a cross spectrum."""
    b, nt = v.shape[:2]
    nxh = hnx // 2 + 1
    h = v.reshape(b, nt, hny, nxh)
    full = np.empty((b, nt, hny, hnx), dtype=h.dtype)
    full[..., :nxh] = h
    tw = h[:, (-np.arange(nt)) % nt][:, :, (-np.arange(hny)) % hny][..., hnx - np.arange(nxh, hnx)]
    full[..., nxh:] = np.conj(tw) if conj else tw
    return full


def family(p):
    """(kernel kind, the first family tag describe prints)"""
    line = p.describe().splitlines()[1]
    return p.kernel_info()[0], line[line.index("[") + 1:line.index("]")]


# (id, make() arguments, environment, expected kind, expected tag)
ROWS = [
    ("fasty", dict(ny=4096, nx=4096), {}, L.K_FASTY, "fasty"),
    ("fasty-cross", dict(ny=1024, nx=1024, out_mode=L.OUT_CROSS), {}, L.K_FASTY, "fasty"),
    ("fasts-over-fasty", dict(ny=256, nx=256), {}, L.K_FASTS, "fasts"),
    ("fasts", dict(ny=64, nx=128, detrend=L.DETREND_LINEAR), {}, L.K_FASTS, "fasts"),
    ("fasts-off-fastg", dict(ny=128, nx=128), {"XRFTHIP_FASTS": "0"}, L.K_FASTG, "fastg"),
    ("fasts-off-fasty", dict(ny=256, nx=256), {"XRFTHIP_FASTS": "0"}, L.K_FASTY, "fasty"),
    ("fastm", dict(ny=720, nx=1440, dtype=F64), {}, L.K_FASTM, "fastm"),
    ("fastm-f32", dict(ny=360, nx=720, detrend=L.DETREND_LINEAR), {}, L.K_FASTM, "fastm"),
    ("fastn", dict(ny=3000, nx=3000, dtype=F64), {}, L.K_FASTN, "fastn"),
    ("fastn-tables-off", dict(ny=720, nx=1440, dtype=F64), {"XRFTHIP_FASTN_TABLES": "0"}, L.K_FASTN, "fastn"),
    ("fastg", dict(ny=50, nx=50, dtype=F64), {}, L.K_FASTG, "fastg"),
    ("fastg-complex", dict(ny=96, nx=128, dtype=C64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTG, "fastg"),
    ("fastg-off", dict(ny=50, nx=50, dtype=F64), {"XRFTHIP_FASTG": "0"}, L.K_FASTN, "fastn"),
    ("fastyc", dict(ny=1024, nx=1024, dtype=C64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTY, "fasty complex"),
    ("fastyc-off", dict(ny=1024, nx=1024, dtype=C64, out_mode=L.OUT_COMPLEX), {"XRFTHIP_FASTYC": "0"}, L.K_GENERIC, "main"),
    ("fastyc-four-step", dict(ndim=1, nx=1 << 20, dtype=C64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTY, "fasty complex rows, four-step"),
    ("fastr", dict(ndim=1, nx=65536), {}, L.K_FASTR, "fastr"),
    ("fastr-off-fast1d", dict(ndim=1, nx=65536), {"XRFTHIP_FASTR": "0"}, L.K_FASTY, "fasty four-step"),
    ("fast1d", dict(ndim=1, nx=1 << 20, detrend=L.DETREND_LINEAR), {}, L.K_FASTY, "fasty four-step"),
    ("fastr-complex", dict(ndim=1, nx=16384, dtype=C64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTR, "fastr complex rows"),
    ("fastr-rows-over-complex", dict(ndim=1, nx=2048, dtype=C64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTR, "fasty complex rows"),
    ("crows-off", dict(ndim=1, nx=2048, dtype=C64, out_mode=L.OUT_COMPLEX), {"XRFTHIP_CROWS": "0"}, L.K_FASTR, "fastr complex rows"),
    ("fastmx", dict(ndim=1, nx=1000, dtype=F64), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-off", dict(ndim=1, nx=1000, dtype=F64), {"XRFTHIP_FASTM": "0"}, L.K_FASTG_ROWS, "fastg rows"),
    ("fastg-rows", dict(ndim=1, nx=50, dtype=F64), {}, L.K_FASTG_ROWS, "fastg rows"),
    ("fastgy-rows", dict(ndim=1, nx=365, dtype=F64), {}, L.K_FASTG_ROWS, "fastg rows Rader"),
    ("fastmy", dict(ny=100, nx=200, dtype=F64, flags=L.AXIS_Y), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastgy", dict(ny=103, nx=206, dtype=F64, flags=L.AXIS_Y), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fastmy-off", dict(ny=100, nx=200, dtype=F64, flags=L.AXIS_Y), {"XRFTHIP_FASTM": "0"}, L.K_FASTG_Y, "fastg y-only"),
    ("fusedi", dict(ny=128, nx=256, inner=4), {}, L.K_FASTN, "inner layout"),
    ("composite", dict(ny=128, nx=256, dtype=C64, out_mode=L.OUT_COMPLEX, mid=4), {}, L.K_COMPOSITE, "inner layout"),
    ("no-fast", dict(ny=4096, nx=4096), {"XRFTHIP_NO_FAST": "1"}, L.K_GENERIC, "main"),
    ("no-fast-rows", dict(ndim=1, nx=65536), {"XRFTHIP_NO_FAST": "1"}, L.K_GENERIC, "main"),
    ("generic-prime", dict(ndim=1, nx=1031, dtype=F64), {}, L.K_GENERIC, "main"),
    # the segment families (seg_hop) at hop = nx: the segments are the rows of the (batch, nx) input, so the model below is theirs as it stands -- the mean over every
    # mean_batch rows (segment_mean), or every row's own spectrum.  Overlap, odd counts, runs and the column layout: tests/welch.py, welch_cols.py, spectrogram.py
    ("fastw", dict(ndim=1, nx=256, mean_batch=2, seg_hop=256, detrend=L.DETREND_LINEAR), {}, L.K_FASTW, "fastw"),
    ("fastw-cross", dict(ndim=1, nx=1024, mean_batch=2, seg_hop=1024, out_mode=L.OUT_CROSS), {}, L.K_FASTW, "fastw"),
    ("fastk", dict(ndim=1, nx=256, mean_batch=1, seg_hop=256, seg_keep=1, out_mode=L.OUT_COMPLEX), {}, L.K_FASTW, "fastw segments kept"),
    ("fastk-power", dict(ndim=1, nx=1024, mean_batch=1, seg_hop=1024, seg_keep=1, detrend=L.DETREND_LINEAR), {}, L.K_FASTW, "fastw segments kept"),
]


# ---------------------------------------------------------------------------------- engine-level reference
def _axes(kw):
    """(numpy shape of one call's input, the transform axes, the axis real_dim halves or None) of a make() descriptor."""
    ndim, batch, ny, nx = kw.get("ndim", 2), kw.get("batch", 2), kw.get("ny", 1), kw.get("nx", 1)
    flags, inner, mid = kw.get("flags", 0), kw.get("inner", 1), kw.get("mid", 1)
    if ndim == 1:
        return (batch, nx), (1,), (1 if flags & L.HALF_X else None)
    if mid > 1:
        return (batch, ny, mid, nx, inner), (1, 3), (3 if flags & L.HALF_X else 1 if flags & L.HALF_Y else None)
    if inner > 1:
        return (batch, ny, nx, inner), (1, 2), (2 if flags & L.HALF_X else 1 if flags & L.HALF_Y else None)
    if flags & L.AXIS_Y:
        return (batch, ny, nx), (1,), (1 if flags & L.HALF_X else None)
    return (batch, ny, nx), (1, 2), (2 if flags & L.HALF_X else None)


def points(kw):
    shape, axes, _ = _axes(kw)
    return int(np.prod([shape[a] for a in axes]))


def detrended(a, axes, kind):
    """x - fit over `axes` in float64: the mean, or the least-squares line / plane (centred, orthogonal coordinates: exact for a full grid)."""
    if kind == L.DETREND_NONE:
        return a
    out = a - a.mean(axis=axes, keepdims=True)
    if kind == L.DETREND_LINEAR:
        m = int(np.prod([a.shape[k] for k in axes]))
        for ax in axes:
            n = a.shape[ax]
            shp = [1] * a.ndim
            shp[ax] = n
            c = (np.arange(n, dtype=np.float64) - 0.5 * (n - 1)).reshape(shp)
            out = out - c * ((a * c).sum(axis=axes, keepdims=True) / ((c * c).sum() * (m // n)))
    return out


def reference(kw, x0, x1=None, binmap=None, nbins=0, phase_x=None):
    """What a make(**kw) plan computes (scale 1), in float64 / complex128 from the float64 image of its input(s).  Returns (out, iso).
    A herm descriptor (herm_ny / herm_nx): the transform along t of the complex half-spectrum input, |F|^2 or F0 conj(F1), expanded to the
    full grid by herm_full, with the plan's rotations (the other descriptors of the ladder carry none)."""
    shape, axes, half = _axes(kw)
    flags, mode, det = kw.get("flags", 0), kw.get("out_mode", L.OUT_POWER), kw.get("detrend", L.DETREND_NONE)
    herm = kw.get("herm_ny", 0) > 0
    if flags & L.C2R_X:  # irfftn: the half spectrum [.., nx/2 + 1] in, nx real samples out, unnormalised (the caller folds 1/N into scale)
        s = [shape[k] for k in axes]
        a = np.asarray(x0, dtype=np.complex128).reshape(shape[:-1] + (shape[-1] // 2 + 1,))
        return np.fft.irfftn(a, s=s, axes=axes) * np.prod(s), None

    def fwd(x):
        a = np.asarray(x).reshape(shape)
        a = a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)
        if herm and flags & L.ISHIFT_Y:
            a = np.fft.ifftshift(a, axes=1)
        a = detrended(a, axes, det)
        if flags & L.PHASE_IN:
            a = a * np.asarray(phase_x, dtype=np.complex128)
        if flags & L.INVERSE:
            f = np.fft.ifftn(a, axes=axes) * np.prod([shape[k] for k in axes])
        else:
            f = np.fft.fftn(a, axes=axes)
        if half is not None:
            n = shape[half]
            f = np.take(f, np.arange(n // 2 + 1), axis=half)
            if flags & L.REALDIM_X2:  # (the kept half of a real axis counts twice in a power or cross spectrum: 0 < k, k != n / 2)
                k = np.arange(n // 2 + 1)
                w = np.where((k > 0) & (2 * k != n), 2.0, 1.0).reshape([-1 if i == half else 1 for i in range(f.ndim)])
                f = f * np.sqrt(w) if mode == L.OUT_POWER else f
                return f, w
        return f, None

    f0, w = fwd(x0)
    if mode == L.OUT_COMPLEX:
        out = f0
    elif mode == L.OUT_POWER:
        out = np.abs(f0) ** 2
    else:
        c = f0 * np.conj(fwd(x1)[0])
        if w is not None:
            c = c * w
        out = c if mode == L.OUT_CROSS else np.angle(c)
    if herm:
        out = herm_full(out, kw["herm_ny"], kw["herm_nx"], mode == L.OUT_CROSS)
        if flags & L.SHIFT_Y:
            out = np.fft.fftshift(out, axes=1)
        if flags & L.SHIFT_X:  # (of a herm plan: the two Hermitian axes)
            out = np.fft.fftshift(out, axes=(2, 3))
    iso = None
    if flags & L.ISO:
        bm = np.asarray(binmap).ravel()

        def bsum(w):  # (accumulated in long double: a bin of 10^5 terms summed in float64 order would carry the reference's own error)
            acc = np.zeros(nbins, dtype=np.longdouble)
            np.add.at(acc, bm, w.astype(np.longdouble))
            return acc.astype(np.float64)

        iso = np.stack([bsum(o.ravel().real) + (1j * bsum(o.ravel().imag) if np.iscomplexobj(o) else 0) for o in out])
    return out, iso


def segment_rows(kw, t):
    """The (batch, nx) samples of a seg_hop descriptor with hop = nx as its plan reads them: (series, mean_batch nx), every row of `t` a segment."""
    return t.reshape(-1, max(kw.get("mean_batch", 0), 1) * kw["nx"]) if t is not None and kw.get("seg_hop") else t


def segment_mean(kw, out):
    """A mean plan's result from the model's per-row one: the mean over every mean_batch consecutive rows (not of a seg_keep plan: there mean_batch only counts)."""
    m = kw.get("mean_batch", 0)
    return out.reshape((-1, m) + out.shape[1:]).mean(axis=1) if m > 1 and not kw.get("seg_keep") else out


def tensor(a, dtype):
    """The samples `a` (float64 / complex128) rounded to the plan's dtype, as a CPU tensor, and their exact float64 image."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    wide = torch.complex128 if t.is_complex() else torch.float64
    return t, t.to(wide).numpy()


# ---------------------------------------------------------------------------------- the ladder: modes per family, beyond the routing table
# (id, make() arguments, environment, expected kind, expected tag); "iso": a radial bin map of the plan's output shape
MODES = [
    ("fasty-complex", dict(ny=1024, nx=1024, out_mode=L.OUT_COMPLEX), {}, L.K_FASTY, "fasty"),
    ("fasty-half", dict(ny=1024, nx=1024, flags=L.HALF_X), {}, L.K_FASTY, "fasty"),
    ("fasty-iso", dict(ny=1024, nx=1024, flags=L.ISO, iso=True), {}, L.K_FASTY, "fasty"),
    ("fasty-phase", dict(ny=1024, nx=1024, out_mode=L.OUT_PHASE), {}, L.K_FASTY, "fasty"),
    ("fasts-complex", dict(ny=64, nx=128, out_mode=L.OUT_COMPLEX), {}, L.K_FASTS, "fasts"),
    ("fasts-iso", dict(ny=256, nx=256, flags=L.ISO, iso=True), {}, L.K_FASTS, "fasts"),
    ("fasts-cross", dict(ny=256, nx=256, out_mode=L.OUT_CROSS), {}, L.K_FASTY, "fasty"),
    ("fastm-complex", dict(ny=720, nx=1440, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM, "fastm"),
    ("fastm-half", dict(ny=360, nx=720, flags=L.HALF_X), {}, L.K_FASTM, "fastm"),
    ("fastm-cross", dict(ny=360, nx=720, dtype=F64, out_mode=L.OUT_CROSS), {}, L.K_FASTM, "fastm"),
    ("fastm-iso", dict(ny=360, nx=720, dtype=F64, flags=L.ISO, iso=True), {}, L.K_FASTM, "fastm"),
    ("fastm-phase", dict(ny=360, nx=720, dtype=F64, out_mode=L.OUT_PHASE), {}, L.K_FASTM, "fastm"),
    ("fastn-complex-f32", dict(ny=1215, nx=700, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "fastn"),
    ("fastg-complex-f64", dict(ny=50, nx=50, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTG, "fastg"),
    ("fastg-half", dict(ny=50, nx=50, dtype=F64, flags=L.HALF_X), {}, L.K_FASTG, "fastg"),
    ("fastg-iso", dict(ny=50, nx=50, dtype=F64, flags=L.ISO, iso=True), {}, L.K_FASTG, "fastg"),
    ("fastg-f32", dict(ny=50, nx=50), {}, L.K_FASTG, "fastg"),
    ("fastyc-inverse", dict(ny=1024, nx=1024, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.INVERSE), {}, L.K_FASTY, "fasty complex"),
    ("generic-c128", dict(ny=1024, nx=1024, dtype=C128, out_mode=L.OUT_COMPLEX), {}, L.K_GENERIC, "main"),
    ("fastr-complex-inverse", dict(ndim=1, nx=16384, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.INVERSE), {}, L.K_FASTR, "fastr complex rows"),
    ("fastr-half", dict(ndim=1, nx=65536, flags=L.HALF_X), {}, L.K_FASTR, "fastr"),
    ("fastr-complex-out", dict(ndim=1, nx=65536, out_mode=L.OUT_COMPLEX), {}, L.K_FASTR, "fastr"),
    ("generic-rows-f64", dict(ndim=1, nx=65536, dtype=F64), {}, L.K_GENERIC, "main"),
    ("fast1d-complex", dict(ndim=1, nx=1 << 20, out_mode=L.OUT_COMPLEX), {}, L.K_FASTY, "fasty four-step"),
    ("fastyc-four-step-inverse", dict(ndim=1, nx=1 << 20, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.INVERSE), {}, L.K_FASTY, "fasty complex rows, four-step"),
    ("fastmx-complex", dict(ndim=1, nx=1000, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmx-f32-half", dict(ndim=1, nx=1000, flags=L.HALF_X), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastmy-half", dict(ny=100, nx=200, dtype=F64, flags=L.AXIS_Y | L.HALF_X), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastmy-complex-f32", dict(ny=100, nx=200, flags=L.AXIS_Y, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastmy-inverse", dict(ny=100, nx=200, dtype=C128, flags=L.AXIS_Y | L.INVERSE, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastgy-complex-f32", dict(ny=103, nx=206, flags=L.AXIS_Y, out_mode=L.OUT_COMPLEX), {}, L.K_FASTG_Y, "fastg y-only"),
    ("fusedi-complex-f64", dict(ny=128, nx=256, inner=4, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-x", dict(ny=128, nx=256, inner=4, flags=L.HALF_X), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-y", dict(ny=128, nx=256, inner=4, flags=L.HALF_Y), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-y-odd", dict(ny=33, nx=32, inner=4, dtype=F64, flags=L.HALF_Y, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-y-odd-f32", dict(ny=33, nx=32, inner=4, flags=L.HALF_Y), {}, L.K_FASTN, "inner layout"),
    ("fusedi-cross", dict(ny=128, nx=256, inner=4, dtype=F64, out_mode=L.OUT_CROSS), {}, L.K_FASTN, "inner layout"),
    ("fusedm-complex", dict(ny=64, nx=96, mid=3, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "inner layout"),
    ("composite-f64", dict(ny=128, nx=256, dtype=C128, out_mode=L.OUT_COMPLEX, mid=4), {}, L.K_COMPOSITE, "inner layout"),
    ("generic-complex", dict(ny=1024, nx=1024, out_mode=L.OUT_COMPLEX), {"XRFTHIP_NO_FAST": "1"}, L.K_GENERIC, "main"),
    ("fusedi-half-y-odd-power-x2", dict(ny=33, nx=32, inner=4, flags=L.HALF_Y | L.REALDIM_X2), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-y-odd-cross-x2", dict(ny=33, nx=32, inner=4, dtype=F64, out_mode=L.OUT_CROSS, flags=L.HALF_Y | L.REALDIM_X2), {}, L.K_FASTN, "inner layout"),
    ("fusedi-half-y-power-x2", dict(ny=32, nx=48, inner=4, dtype=F64, flags=L.HALF_Y | L.REALDIM_X2), {}, L.K_FASTN, "inner layout"),
    # inverse transforms, and irfftn from a half spectrum (INVERSE | C2R_X: nx/2 + 1 complex values in, nx real samples out)
    ("fastg-inverse", dict(ny=50, nx=50, dtype=C128, out_mode=L.OUT_COMPLEX, flags=L.INVERSE), {}, L.K_FASTG, "fastg"),
    ("fastmx-inverse", dict(ndim=1, nx=1000, dtype=C128, out_mode=L.OUT_COMPLEX, flags=L.INVERSE), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastg-c2r", dict(ny=50, nx=50, dtype=C128, out_mode=L.OUT_COMPLEX, flags=L.INVERSE | L.C2R_X), {}, L.K_FASTG, "fastg"),
    ("fastg-c2r-c64", dict(ny=48, nx=64, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.INVERSE | L.C2R_X), {}, L.K_FASTG, "fastg"),
    ("fastg-rows-c2r", dict(ndim=1, nx=50, dtype=C128, out_mode=L.OUT_COMPLEX, flags=L.INVERSE | L.C2R_X), {}, L.K_FASTG_ROWS, "fastg rows"),
    ("fastmx-c2r", dict(ndim=1, nx=1000, dtype=C128, out_mode=L.OUT_COMPLEX, flags=L.INVERSE | L.C2R_X), {}, L.K_FASTM_X, "fastm x-only"),
    ("fastr-rows-c2r", dict(ndim=1, nx=2048, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.INVERSE | L.C2R_X), {}, L.K_FASTR, "fasty complex rows"),
    ("fastyc-c2r", dict(ny=1024, nx=1024, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.INVERSE | L.C2R_X), {}, L.K_FASTY, "fasty complex"),
    ("generic-c2r", dict(ny=64, nx=128, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.INVERSE | L.C2R_X), {"XRFTHIP_NO_FAST": "1"}, L.K_GENERIC, "main"),
    # the two-pass families at slabs / rows small enough for every signal (batch strides and tails, tones, impulse, Nyquist)
    ("fastm-small", dict(ny=180, nx=360, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTM, "fastm"),
    ("fastm-small-f32", dict(ny=180, nx=360, detrend=L.DETREND_LINEAR), {}, L.K_FASTM, "fastm"),
    ("fastn-small", dict(ny=125, nx=250, dtype=F64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTN, "fastn"),
    ("fastn-small-f32", dict(ny=243, nx=270), {}, L.K_FASTN, "fastn"),
    ("fastyc-small", dict(ny=256, nx=256, dtype=C64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTY, "fasty complex"),
    ("fastyc-four-step-small", dict(ndim=1, nx=65536, dtype=C64, out_mode=L.OUT_COMPLEX), {}, L.K_FASTY, "fasty complex rows, four-step"),
    ("fast1d-small", dict(ndim=1, nx=65536, detrend=L.DETREND_LINEAR), {"XRFTHIP_FASTR": "0"}, L.K_FASTY, "fasty four-step"),
    ("fasty-small", dict(ny=256, nx=512), {}, L.K_FASTY, "fasty"),
    # the last pass of a three-axis spectrum on the half spectrum of a (nt, ny, nx) grid: the smallest shapes at which the twin indexing (kx = 0, the Nyquist
    # column, an odd ny) and the 128-byte runs with a ragged last block can go wrong; the tone / impulse / Nyquist signals lie along t (the one transform axis)
    ("fasth-power-f32", herm_kw((8, 6, 10), C64, L.OUT_POWER, L.SHIFT_Y | L.SHIFT_X), {}, L.K_FASTH, "fasth"),
    ("fasth-cross-f64", herm_kw((12, 4, 6), C128, L.OUT_CROSS), {}, L.K_FASTH, "fasth"),
    ("fasth-power-odd", herm_kw((15, 5, 7), C64, L.OUT_POWER), {}, L.K_FASTH, "fasth"),  # (odd Hermitian axes, no Nyquist column; 15 = 5 x 3: two radices)
    # the per-column line fit of AXIS_Y plans with a detrend (column_fit_kernel, csrc/aux_kernels.h): both y-only families, and 3 rows x 65 columns (64 columns x 4 row
    # parts per workgroup: the fourth row part has no row, the second column block one column)
    ("fastmy-linear", dict(ny=100, nx=200, dtype=F64, flags=L.AXIS_Y, detrend=L.DETREND_LINEAR), {}, L.K_FASTM_Y, "fastm y-only"),
    ("fastgy-linear", dict(ny=103, nx=206, dtype=F64, flags=L.AXIS_Y, detrend=L.DETREND_LINEAR), {}, L.K_FASTG_Y, "fastg y-only"),
    ("column-fit-3x65", dict(ny=3, nx=65, dtype=F64, flags=L.AXIS_Y, detrend=L.DETREND_LINEAR), {}, L.K_GENERIC, "main"),  # (three rows: the generic passes; the fit is the same kernel)
]

# xrfthip Family (csrc/plan.h) -> the (kernel kind, describe tag) forms it shows; every Family has a ladder case (test_every_family_is_executed)
FAMILY_FORMS = {
    "Generic": {(L.K_GENERIC, "main")},
    "Composite": {(L.K_COMPOSITE, "inner layout")},
    "FusedInner": {(L.K_FASTN, "inner layout")},
    "FastS": {(L.K_FASTS, "fasts")},
    "FastG": {(L.K_FASTG, "fastg"), (L.K_FASTG_ROWS, "fastg rows")},
    "FastGY": {(L.K_FASTG_Y, "fastg y-only"), (L.K_FASTG_ROWS, "fastg rows Rader")},
    "FastMX": {(L.K_FASTM_X, "fastm x-only")},
    "FastMY": {(L.K_FASTM_Y, "fastm y-only")},
    "FastR": {(L.K_FASTR, "fastr")},
    "FastRComplex": {(L.K_FASTR, "fastr complex rows")},
    "FastRRows": {(L.K_FASTR, "fasty complex rows")},
    "FastW": {(L.K_FASTW, "fastw")},
    "FastK": {(L.K_FASTW, "fastw segments kept")},
    "FastYC": {(L.K_FASTY, "fasty complex")},
    "FastYCFourStep": {(L.K_FASTY, "fasty complex rows, four-step")},
    "FastY": {(L.K_FASTY, "fasty")},
    "FastY1D": {(L.K_FASTY, "fasty four-step")},
    "FastM": {(L.K_FASTM, "fastm")},
    "FastN": {(L.K_FASTN, "fastn")},
    "FastH": {(L.K_FASTH, "fasth")},
}


# ---------------------------------------------------------------------------------- the four-step input phase (a table off the separable form)
def four_step_phase(n):
    ph = np.exp(0.001j * np.arange(n))
    ph[1000] *= np.exp(0.3j)  # one entry off the separable form (1000 is not a multiple of 97: a sampled check missed it)
    return ph


def run_four_step_phase(n, ph, dev, seed=3):
    """fft(x * ph) of one complex64 row of n points through a PHASE_IN plan, held to the contract; returns the plan."""
    kw = dict(ndim=1, nx=n, dtype=C64, out_mode=L.OUT_COMPLEX, flags=L.PHASE_IN, batch=1)
    p = make(**kw, phase_x=ph)
    rng = np.random.default_rng(seed)
    x, x64 = tensor(rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n)), C64)
    out, _ = p.execute(x.to(dev))
    ref, _ = reference(kw, x64, phase_x=ph)
    assert_accurate(out.cpu().numpy().reshape(ref.shape), ref, C64, n, what=f"four-step PHASE_IN {family(p)}")
    return p

# every signal on descriptors of at most SMALL points per transform; seeded noise alone above
SIGNALS = ["noise", "tone1", "tone-mid", "tone-last", "impulse", "nyquist", "batch1", "batch3", "batch17"]
SMALL = 1 << 17


def ladder_params(rows, every_signal_to=SMALL):
    """(id, kw, env, kind, tag, signal) for every row and every signal it takes: every signal up to `every_signal_to` points per
    transform (batches of 17 up to SMALL), seeded noise alone above."""
    out = []
    for rid, kw, env, kind, tag in rows:
        n = points(dict(kw))
        sigs = [s for s in SIGNALS if s != "batch17" or n <= SMALL] if n <= every_signal_to else ["noise"]
        for s in sigs:
            out.append((f"{rid}-{s}", kw, env, kind, tag, s))
    return out


def signal(kw, sig, rng):
    """Samples (float64 / complex128) of one call's input: the plan's batch may be replaced by the signal's (batchB)."""
    shape, axes, _ = _axes(kw)
    cplx = kw.get("dtype", F32) in (C64, C128)
    if sig == "noise" or sig.startswith("batch"):
        v = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0.0)
        if sig.startswith("batch"):
            v = v * (np.arange(shape[0]) + 1.0).reshape((-1,) + (1,) * (len(shape) - 1))
        return v
    ax = axes[-1]
    n = shape[ax]
    idx = np.arange(n, dtype=np.float64)
    shp = [1] * len(shape)
    shp[ax] = n
    if sig.startswith("tone"):
        k = {"tone1": 1, "tone-mid": n // 2 - 1, "tone-last": n - 1}[sig]
        ph = 2.0 * np.pi * ((k * np.arange(n)) % n) / n  # (exact phase argument: the reference's own rounding stays at u)
        t = np.exp(1j * ph) if cplx else np.cos(ph)
        return np.broadcast_to(t.reshape(shp), shape).copy()
    if sig == "nyquist":
        v = np.ones(shape)
        for a in axes:
            s2 = [1] * len(shape)
            s2[a] = shape[a]
            v = v * ((-1.0) ** np.arange(shape[a])).reshape(s2)
        return v.astype(np.complex128) if cplx else v
    if sig == "impulse":
        v = np.zeros(shape, dtype=np.complex128 if cplx else np.float64)
        sl = [slice(None)] * len(shape)
        for a in axes:
            sl[a] = shape[a] - 1
        v[tuple(sl)] = 1.0 + (1j if cplx else 0.0)
        return v
    raise ValueError(sig)


def run_ladder(kw, sig, dev, seed=0):
    """Execute one ladder case on `dev` ("cpu": the emulated library, "cuda": the real one) and hold it to the contract.
    Returns the measured rms error in units of u log2 N."""
    kw = dict(kw)
    iso = kw.pop("iso", False)
    if sig.startswith("batch"):
        kw["batch"] = int(sig[5:])
    else:
        kw["batch"] = 1 if points(kw) > SMALL else 2
    if kw.get("mean_batch", 0) > 1:  # (a mean plan: that many outputs, mean_batch rows each)
        kw["batch"] *= kw["mean_batch"]
    rng = np.random.default_rng(seed)
    extra = {}
    if iso:
        _, nb = radial_map(kw["ny"], kw["nx"])
        bm = radial_map(kw["ny"], kw["nx"])[0][:, :kw["nx"] // 2 + 1] if kw.get("flags", 0) & L.HALF_X else radial_map(kw["ny"], kw["nx"])[0]
        extra = dict(binmap=bm, nbins=nb)
    p = make(**kw, **extra)
    dt = kw.get("dtype", F32)
    shape, axes, _ = _axes(kw)
    if kw.get("flags", 0) & L.C2R_X:  # the half spectrum of a real signal (Hermitian where irfftn assumes it)
        x, x64 = tensor(np.fft.rfftn(signal(dict(kw, dtype=F64), sig, rng), axes=axes), dt)
    else:
        x, x64 = tensor(signal(kw, sig, rng), dt)
    mode = kw.get("out_mode", L.OUT_POWER)
    x1 = x164 = None
    if mode in (L.OUT_CROSS, L.OUT_PHASE):
        x1, x164 = tensor(signal(kw, "noise", np.random.default_rng(seed + 1)), dt)
        x1 = x1.to(dev)
    out, isoo = p.execute(segment_rows(kw, x.to(dev)), segment_rows(kw, x1))
    n = points(kw)
    det = kw.get("detrend", L.DETREND_NONE)
    kap = kappa(x64.reshape(shape), detrended(x64.reshape(shape), axes, det)) if det else 0.0
    if mode == L.OUT_PHASE:  # angles, weighted by |F0 conj(F1)|: a phase is only defined as well as the cross spectrum it comes from
        cref, _ = reference(dict(kw, out_mode=L.OUT_CROSS), x64, x164)
        got = np.abs(cref) * np.exp(1j * out.cpu().numpy().astype(np.float64).reshape(cref.shape))
        c = assert_accurate(got, cref, dt, n, kap, what=f"{sig} phase")
    else:
        ref, iref = reference(kw, x64, x164, extra.get("binmap"), extra.get("nbins", 0))
        ref = segment_mean(kw, ref)  # (a segment row's mean over its segments: the model above is per row and stays as it is)
        c = assert_accurate(out.cpu().numpy().reshape(ref.shape), ref, dt, n, kap, flat=(sig == "noise" and mode == L.OUT_COMPLEX), what=sig)
        if iref is not None:
            c = max(c, assert_accurate(isoo.cpu().numpy().reshape(iref.shape), iref, dt, n, kap, what=f"{sig} iso"))
    return p, c


# ---------------------------------------------------------------------------------- the layout x parity matrix (product API against the oracle)
ORDERS = [("t", "y", "x"), ("t", "x", "y"), ("y", "t", "x"), ("y", "x", "t"), ("x", "t", "y"), ("x", "y", "t")]
SIZES = [(16, 12), (15, 12), (16, 9), (15, 9), (8, 33)]
DIMS = [["y", "x"], ["x", "y"], ["y"], ["x"]]
OPS = ["fft", "fft_linear_hann", "power_spectrum", "cross_spectrum", "cross_phase", "ifft_fft"]


def matrix_params():
    out = []
    for order in ORDERS:
        for ny, nx in SIZES:
            for dim in DIMS:
                for rd in [None] + dim:
                    out.append(("".join(order) + f"-{ny}x{nx}-{''.join(dim)}-real{rd or ''}", order, ny, nx, dim, rd))
    return out


def _matrix_call(mod, op, a, b, dim, rd):
    if op == "fft":
        return mod.fft(a, dim=dim, real_dim=rd)
    if op == "fft_linear_hann":
        return mod.fft(a, dim=dim, real_dim=rd, detrend="linear", window="hann")
    if op == "power_spectrum":
        return mod.power_spectrum(a, dim=dim, real_dim=rd)
    if op == "cross_spectrum":
        return mod.cross_spectrum(a, b, dim=dim, real_dim=rd)
    if op == "cross_phase":
        return mod.cross_phase(a, b, dim=dim, real_dim=rd)
    f = mod.fft(a, dim=dim, real_dim=rd)
    return mod.ifft(f, dim=["freq_" + d for d in dim], real_dim=None if rd is None else "freq_" + rd)


def run_matrix_cell(order, ny, nx, dim, rd, dtype, seed=0):
    """Every operation of OPS on a (t = 3, y, x) field held in `order`: the product's result meets the contract against the oracle fed
    the same samples as float64, or both raise the same exception.  Returns the worst rms error in units of u log2 N."""
    import xrft_amd as xa
    from oracle import xrft_oracle as o

    ext = {"t": 3, "y": ny, "x": nx}
    shape = tuple(ext[d] for d in order)
    coords = {"t": np.arange(3.0), "y": np.arange(ny) * 0.5 + 1.0, "x": np.arange(nx) * 2.0 - 3.0}
    rng = np.random.default_rng(seed)
    ii = {d: np.arange(ext[d]).reshape([-1 if e == d else 1 for e in order]) for d in order}
    v0 = rng.standard_normal(shape) + 0.3 * ii["y"] - 0.2 * ii["x"] + 2.0  # (a plane under the noise: the detrend has work to do)
    v1 = rng.standard_normal(shape)
    n = int(np.prod([ext[d] for d in dim]))
    worst = 0.0
    for op in OPS:
        a, oa = cases.pair(v0.astype(dtype), order, coords)
        b, ob = cases.pair(v1.astype(dtype), order, coords)
        try:
            ref = _matrix_call(o, op, oa, ob, dim, rd)
        except Exception as e:  # the oracle refuses: the product must refuse the same way
            with pytest.raises(type(e)):
                _matrix_call(xa, op, a, b, dim, rd)
            continue
        got = _matrix_call(xa, op, a, b, dim, rd)
        what = f"{op} {order} {ny}x{nx} dim={dim} real_dim={rd} {dtype}"
        assert tuple(got.dims) == tuple(ref.dims), (what, got.dims, ref.dims)
        g = np.asarray(got.values)
        kap = 0.0
        if op == "fft_linear_hann":
            kap = kappa(oa.values, o.detrend(oa, dim, "linear").transpose(*order).values)
        if op == "cross_phase":  # angles modulo 2 pi, weighted by |cross spectrum|: a phase is only as defined as the product it comes from
            cs = _matrix_call(o, "cross_spectrum", oa, ob, dim, rd).values
            worst = max(worst, assert_accurate(np.abs(cs) * np.exp(1j * g.astype(np.float64)), cs, dtype, n, kap, what=what))
        else:
            worst = max(worst, assert_accurate(g, ref.values, dtype, n, kap, what=what))
    return worst


def run_odd_real_axis_first(order, dtype, op):
    """real_dim along the first of two non-trailing transform axes, odd length, long enough for the fused passes (XRFTHIP_HALF_Y; with
    REALDIM_X2 in a power or cross spectrum: every ky > 0 counts twice).  The plan that ran is asserted to be the fused one."""
    import xrft_amd as xa
    from xrft_amd import api
    from oracle import xrft_oracle as o

    ext = {"y": 33, "x": 32, "t": 4}
    rng = np.random.default_rng(7)
    shape = tuple(ext[d] for d in order)
    c = {"y": np.arange(33.0), "x": np.arange(32) * 0.5, "t": np.arange(4.0)}
    da, od = cases.pair(rng.standard_normal(shape).astype(dtype), order, c)
    db, ob = cases.pair(rng.standard_normal(shape).astype(dtype), order, c)
    api._plan_cache.clear()
    if op == "fft":
        got, ref = xa.fft(da, dim=["x", "y"], real_dim="y"), o.fft(od, dim=["x", "y"], real_dim="y")
    elif op == "power_spectrum":
        got, ref = xa.power_spectrum(da, dim=["x", "y"], real_dim="y"), o.power_spectrum(od, dim=["x", "y"], real_dim="y")
    else:
        got, ref = xa.cross_spectrum(da, db, dim=["x", "y"], real_dim="y"), o.cross_spectrum(od, ob, dim=["x", "y"], real_dim="y")
    assert tuple(got.dims) == tuple(ref.dims)
    assert_accurate(got.values, ref.values, dtype, 33 * 32, what=op)
    cases.check(got, ref, cases.TOL[dtype])
    plans = list(api._plan_cache.values())
    assert plans and all(family(p) == (L.K_FASTN, "inner layout") and p.flags & L.HALF_Y for p in plans), [family(p) for p in plans]
