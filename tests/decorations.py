"""The decoration ladder: windows, shifts, flips, phase tables, a constant detrend and `scale`, per kernel family, held to the rounding-level contract of
tests/accuracy.py (CPU: tests/test_decorations_emulated.py; GPU: tests/test_gpu_decorations.py).  Not a conftest: imported by the tests that use it.

tests/accuracy.py runs every family on the bare transform.  Each family applies the decorations in load and store code of its own, and API parity (3e-4 of the
largest bin, a nearly symmetric Hann window, one bundle of flags) cannot tell a window applied in source order from one applied behind a flip or a rotation.
Here every decoration runs alone and all of them together, per family, at the smallest shape at which the family still routes, with inputs that discriminate:
windows 0.5 + U(0, 1) (positive, asymmetric, another one per axis), phase tables exp(2 pi i U(0, 1)), scale 0.37, batches of unequal size.

reference() is a plain float64 / complex128 numpy model of include/xrft_hip.h, per field and in this order:
  1 detrend   2 x window_y (x) window_x, source order   3 PHASE_IN: x the phase tables, source position   4 np.flip (CROSS / PHASE: FLIP0_* field 0, FLIP_* field 1)
  5 np.fft.ifftshift (ISHIFT_*)   6 fftn, or ifftn x prod(N) (INVERSE)   7 0 .. n/2 of the half axis   8 F | |F|^2 | F0 conj(F1)
  9 without PHASE_IN, COMPLEX and CROSS: x the phase tables by unshifted frequency   10 np.fft.fftshift (SHIFT_*)   11 x scale
The radial sums of an ISO plan are taken of the unshifted result (the bin map is indexed by unshifted frequency), scale included.

Every case also asserts the (kind, tag) that ran, as recorded on the emulated library; where a family declines a decoration, the family it is demoted to
(DEMOTED) -- a routing change fails the case instead of quietly testing the generic passes.  A case the library refuses asserts the documented status."""
import numpy as np
import pytest

from xrft_amd import _lib as L
from xrft_amd import engine

import accuracy as A

F32, F64, C64, C128 = A.F32, A.F64, A.C64, A.C128
SCALE = 0.37
BATCH = 3
OFFSET = 1.5  # under a constant detrend: the mean has work to do

TOKENS = ("win", "shift", "ishift", "flip", "flip0", "phase", "phasein", "scale", "const")
# mutations of the reference that the bound must notice (test_the_reference_is_sensitive)
MUTATIONS = ("window-after-flip", "window-by-destination", "fftshift-for-ifftshift", "phase-by-shifted-index", "flips-swapped", "scale-omitted")


def yx_axes(kw):
    """{"y": numpy axis or None, "x": numpy axis or None} of a make() descriptor: an AXIS_Y plan has only y, a 1-D plan only x."""
    _, axes, _ = A._axes(kw)
    if kw.get("ndim", 2) == 1:
        return {"y": None, "x": axes[0]}
    if len(axes) == 1:
        return {"y": axes[0], "x": None}
    return {"y": axes[0], "x": axes[1]}


def two_fields(kw):
    return kw.get("out_mode", L.OUT_POWER) in (L.OUT_CROSS, L.OUT_PHASE)


def decorate(kw, tokens, seed=0):
    """(make() arguments with the flags / detrend of `tokens`, the tables: window_y, window_x, phase_y, phase_x, scale) of a base descriptor."""
    tokens = set(tokens)
    assert tokens <= set(TOKENS), tokens
    kw = dict(kw, batch=BATCH)
    yx = yx_axes(kw)
    shape, _, _ = A._axes(kw)
    c2r = bool(kw.get("flags", 0) & L.C2R_X)
    rng = np.random.default_rng(1000 + seed)
    flags = kw.get("flags", 0)
    tab = dict(window_y=None, window_x=None, phase_y=None, phase_x=None, scale=SCALE if "scale" in tokens else 1.0)
    for name, sh, ish, fl in (("y", L.SHIFT_Y, L.ISHIFT_Y, L.FLIP_Y), ("x", L.SHIFT_X, L.ISHIFT_X, L.FLIP_X)):
        if yx[name] is None:
            continue
        n = shape[yx[name]]
        w, ph = 0.5 + rng.random(n), np.exp(2j * np.pi * rng.random(n))  # (drawn whether used or not: a case's tables do not depend on its other tokens)
        if "win" in tokens:
            tab["window_" + name] = w
        if "phase" in tokens or "phasein" in tokens:
            tab["phase_" + name] = ph[:n // 2 + 1] if (c2r and name == "x") else ph
        if "shift" in tokens:
            flags |= sh
        if "ishift" in tokens and not (c2r and name == "x"):
            flags |= ish
        if "flip" in tokens:
            flags |= fl
    if "shift" in tokens and kw.get("herm_ny", 0):  # (a herm plan: SHIFT_X is the fftshift of the two Hermitian axes of the result)
        flags |= L.SHIFT_X
    if "flip0" in tokens and two_fields(kw):  # x alone: with both axes of both fields flipped, FLIP0 and FLIP swapped would compute the same
        flags |= L.FLIP0_X if yx["x"] is not None else L.FLIP0_Y
    if "phasein" in tokens:
        flags |= L.PHASE_IN
    if "const" in tokens:
        kw["detrend"] = L.DETREND_CONSTANT
    kw["flags"] = flags
    return kw, tab


def inputs(kw, seed=0):
    """The fields (float64 / complex128 samples) of a decorated descriptor: seeded noise, batch b scaled by b + 1, + OFFSET under a detrend; a C2R_X plan
    takes the half spectrum of such a real field (Hermitian where irfftn assumes it)."""
    shape, axes, _ = A._axes(kw)
    cplx = kw.get("dtype", F32) in (C64, C128)
    out = []
    for f in range(2 if two_fields(kw) else 1):
        rng = np.random.default_rng(seed + f)
        amp = (np.arange(shape[0]) + 1.0).reshape((-1,) + (1,) * (len(shape) - 1))
        if kw.get("flags", 0) & L.C2R_X:
            v = np.fft.rfftn(rng.standard_normal(shape) * amp, axes=axes)
        else:
            v = (rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0.0)) * amp
        if kw.get("detrend", L.DETREND_NONE):
            v = v + OFFSET
        out.append(v)
    return out


def _along(v, a, ax):
    shp = [1] * a.ndim
    shp[ax] = -1
    return np.asarray(v).reshape(shp)


def reference(kw, tab, x0, x1=None, binmap=None, nbins=0, mutate=None):
    """What the plan of a decorated descriptor computes, in float64 / complex128 from the float64 image of its input(s).  Returns (out, iso).
    `mutate`: one of MUTATIONS -- the same model with that one mistake in it."""
    assert mutate is None or mutate in MUTATIONS
    shape, axes, half = A._axes(kw)
    flags, mode, det = kw.get("flags", 0), kw.get("out_mode", L.OUT_POWER), kw.get("detrend", L.DETREND_NONE)
    yx = yx_axes(kw)
    names = [n for n in ("y", "x") if yx[n] is not None]
    c2r = bool(flags & L.C2R_X)
    bit = {"y": dict(shift=L.SHIFT_Y, ishift=L.ISHIFT_Y, flip=L.FLIP_Y, flip0=L.FLIP0_Y), "x": dict(shift=L.SHIFT_X, ishift=L.ISHIFT_X, flip=L.FLIP_X, flip0=L.FLIP0_X)}
    sizes = [shape[k] for k in axes]

    def windowed(a):
        for n in names:
            if tab["window_" + n] is not None:
                a = a * _along(tab["window_" + n], a, yx[n])
        return a

    def phased(a):
        for n in names:
            if tab["phase_" + n] is not None:
                a = a * _along(np.asarray(tab["phase_" + n])[:a.shape[yx[n]]], a, yx[n])
        return a

    def fwd(x, field):
        a = np.asarray(x).reshape(shape[:-1] + (shape[-1] // 2 + 1,) if c2r else shape)
        a = a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)
        a = A.detrended(a, axes, det)  # 1
        if mutate not in ("window-after-flip", "window-by-destination"):
            a = windowed(a)  # 2
        if flags & L.PHASE_IN:
            a = phased(a)  # 3
        own = "flip0" if (two_fields(kw) and field == 0) else "flip"
        if mutate == "flips-swapped" and two_fields(kw):
            own = "flip" if own == "flip0" else "flip0"
        fl = [yx[n] for n in names if flags & bit[n][own]]
        if fl:
            a = np.flip(a, axis=tuple(fl))  # 4
        if mutate == "window-after-flip":
            a = windowed(a)
        ish = [yx[n] for n in names if flags & bit[n]["ishift"]]
        if ish:
            a = (np.fft.fftshift if mutate == "fftshift-for-ifftshift" else np.fft.ifftshift)(a, axes=ish)  # 5
        if mutate == "window-by-destination":
            a = windowed(a)
        if c2r:
            return np.fft.irfftn(a, s=sizes, axes=axes) * np.prod(sizes)
        f = np.fft.ifftn(a, axes=axes) * np.prod(sizes) if flags & L.INVERSE else np.fft.fftn(a, axes=axes)  # 6
        if half is not None:
            f = np.take(f, np.arange(shape[half] // 2 + 1), axis=half)  # 7
        return f

    f0 = fwd(x0, 0)
    if mode == L.OUT_COMPLEX:  # 8
        out = f0
    elif mode == L.OUT_POWER:
        out = np.abs(f0) ** 2
    else:
        out = f0 * np.conj(fwd(x1, 1))
    sh = [yx[n] for n in names if flags & bit[n]["shift"]]
    if kw.get("herm_ny", 0):  # the last pass of a three-axis spectrum: the full (nt, herm_ny, herm_nx) result from the half spectrum's twins
        out = A.herm_full(out, kw["herm_ny"], kw["herm_nx"], mode == L.OUT_CROSS)
        sh += [2, 3] if flags & L.SHIFT_X else []
    out_phase = not (flags & L.PHASE_IN) and mode in (L.OUT_COMPLEX, L.OUT_CROSS)
    if out_phase and mutate != "phase-by-shifted-index":
        out = phased(out)  # 9
    scale = 1.0 if mutate == "scale-omitted" else tab["scale"]
    iso = None
    if flags & L.ISO:
        bm = np.asarray(binmap).ravel()

        def bsum(w):  # (accumulated in long double, as accuracy.reference does)
            acc = np.zeros(nbins, dtype=np.longdouble)
            np.add.at(acc, bm, w.astype(np.longdouble))
            return acc.astype(np.float64)

        iso = np.stack([bsum(o.ravel().real) + (1j * bsum(o.ravel().imag) if np.iscomplexobj(o) else 0) for o in out * scale])
    if sh:
        out = np.fft.fftshift(out, axes=sh)  # 10
    if out_phase and mutate == "phase-by-shifted-index":
        out = phased(out)
    return out * scale, iso  # 11


# ---------------------------------------------------------------------------------- the cases
# a decoration is named by its tokens joined with "+", the combined ones by a word
NAMED = {
    "all": "win+shift+ishift+flip+flip0+phase+scale+const",  # (every FLIP_* goes to the generic passes: this one tests THEM under everything at once ...
    "noflip": "win+shift+ishift+phase+scale+const",          # ... and this one the family's own load and store code)
    "all-nodetrend": "win+shift+ishift+flip+phase+scale",          # (a detrend on an inverse plan is BAD_ARG: EXTRA_REFUSED)
    "noflip-nodetrend": "win+shift+ishift+phase+scale",
    "all-nodetrend-phasein": "win+shift+ishift+flip+phasein+scale",
    "noflip-nodetrend-phasein": "win+shift+ishift+phasein+scale",
}
FWD = ["win", "shift", "ishift", "flip", "phase", "const+scale", "all", "noflip", "noflip-nodetrend"]  # (a detrend sends complex input to the generic passes)
HALF = ["win+ishift+phase"]  # (SHIFT_* with HALF_X is BAD_ARG)
INV = ["win", "shift", "ishift", "flip", "phase", "scale", "win+ishift", "ishift+shift", "all-nodetrend", "noflip-nodetrend", "phasein", "win+ishift+phasein", "all-nodetrend-phasein", "noflip-nodetrend-phasein"]
C2R = ["ishift", "shift", "phasein"]  # (ISHIFT_Y; SHIFT_Y | SHIFT_X; PHASE_IN on y and x)
ISO = ["win+shift"]
SEG = ["win", "shift", "ishift", "const+scale", "win+shift+ishift+scale+const"]  # (the segment families take no flip; the phase table only a two-field mean, held by tests/welch.py)
SEG_X = ["win", "shift", "const+scale", "win+shift+scale+const"]                 # (... and a kept complex spectrum no input rotation)
HERM = ["win", "shift", "ishift", "scale", "win+shift+ishift+scale"]  # (herm_ny / herm_nx: a window along t, the rotations, scale; no phase table, no detrend, no flip)

CX, PW, CR = L.OUT_COMPLEX, L.OUT_POWER, L.OUT_CROSS
IV = L.INVERSE

# (id, make() arguments, environment, kind, tag of the family the row is written for, its decorations)
BASE = [
    ("fasty-power", dict(ny=256, nx=512), {}, L.K_FASTY, "fasty", FWD),
    ("fasty-cross", dict(ny=256, nx=512, out_mode=CR), {}, L.K_FASTY, "fasty", FWD),
    ("fasty-complex", dict(ny=256, nx=512, out_mode=CX), {}, L.K_FASTY, "fasty", FWD),
    ("fasty-half", dict(ny=256, nx=512, out_mode=CX, flags=L.HALF_X), {}, L.K_FASTY, "fasty", HALF),
    ("fasts", dict(ny=64, nx=128, out_mode=CX), {}, L.K_FASTS, "fasts", FWD),
    ("fastm", dict(ny=180, nx=360, dtype=F64, out_mode=CX), {}, L.K_FASTM, "fastm", FWD),
    ("fastm-cross-f32", dict(ny=180, nx=360, out_mode=CR), {}, L.K_FASTM, "fastm", FWD),
    ("fastm-half", dict(ny=180, nx=360, dtype=F64, out_mode=CX, flags=L.HALF_X), {}, L.K_FASTM, "fastm", HALF),
    ("fastn", dict(ny=125, nx=250, dtype=F64, out_mode=CX), {}, L.K_FASTN, "fastn", FWD),
    ("fastn-f32", dict(ny=243, nx=270), {}, L.K_FASTN, "fastn", FWD),
    ("fastg", dict(ny=50, nx=50, dtype=F64, out_mode=CX), {}, L.K_FASTG, "fastg", FWD),
    ("fastg-odd", dict(ny=45, nx=49, dtype=F64, out_mode=CX), {}, L.K_FASTG, "fastg", FWD),
    ("fastg-c64", dict(ny=96, nx=128, dtype=C64, out_mode=CX), {}, L.K_FASTG, "fastg", FWD),
    ("fastg-odd-half", dict(ny=45, nx=49, dtype=F64, out_mode=CX, flags=L.HALF_X), {}, L.K_FASTG, "fastg", HALF),
    ("fastyc", dict(ny=256, nx=256, dtype=C64, out_mode=CX), {}, L.K_FASTY, "fasty complex", FWD),
    ("fastr", dict(ndim=1, nx=65536, out_mode=CX), {}, L.K_FASTR, "fastr", FWD),
    ("fastr-half", dict(ndim=1, nx=65536, out_mode=CX, flags=L.HALF_X), {}, L.K_FASTR, "fastr", HALF),
    ("fastr-complex", dict(ndim=1, nx=16384, dtype=C64, out_mode=CX), {}, L.K_FASTR, "fastr complex rows", FWD),
    ("fastr-rows", dict(ndim=1, nx=2048, dtype=C64, out_mode=CX), {}, L.K_FASTR, "fasty complex rows", FWD),
    ("fast1d", dict(ndim=1, nx=65536, out_mode=CX), {"XRFTHIP_FASTR": "0"}, L.K_FASTY, "fasty four-step", FWD),
    ("fastyc-four-step", dict(ndim=1, nx=65536, dtype=C64, out_mode=CX), {}, L.K_FASTY, "fasty complex rows, four-step", FWD),
    ("fastmx", dict(ndim=1, nx=1000, dtype=F64, out_mode=CX), {}, L.K_FASTM_X, "fastm x-only", FWD),
    ("fastg-rows", dict(ndim=1, nx=50, dtype=F64, out_mode=CX), {}, L.K_FASTG_ROWS, "fastg rows", FWD),
    ("rader-rows", dict(ndim=1, nx=365, dtype=F64, out_mode=CX), {}, L.K_FASTG_ROWS, "fastg rows Rader", FWD),
    ("fastmy", dict(ny=100, nx=200, dtype=F64, out_mode=CX, flags=L.AXIS_Y), {}, L.K_FASTM_Y, "fastm y-only", FWD),
    ("fastgy", dict(ny=103, nx=206, dtype=F64, out_mode=CX, flags=L.AXIS_Y), {}, L.K_FASTG_Y, "fastg y-only", FWD),
    ("fastgy-odd", dict(ny=105, nx=200, dtype=F64, out_mode=CX, flags=L.AXIS_Y), {}, L.K_FASTG_Y, "fastg y-only", FWD),
    ("fusedi", dict(ny=128, nx=256, inner=4, out_mode=CX), {}, L.K_FASTN, "inner layout", FWD),
    ("fusedi-odd", dict(ny=33, nx=45, inner=4, dtype=F64, out_mode=CX), {}, L.K_FASTN, "inner layout", FWD),
    ("fusedm", dict(ny=64, nx=96, mid=3, out_mode=CX), {}, L.K_FASTN, "inner layout", FWD),
    ("composite", dict(ny=128, nx=256, mid=4, dtype=C64, out_mode=CX), {}, L.K_COMPOSITE, "inner layout", FWD),
    ("generic-prime", dict(ndim=1, nx=1031, dtype=F64, out_mode=CX), {}, L.K_GENERIC, "main", FWD),
    # the segment families at hop = nx (accuracy.ROWS): BATCH = mean_batch rows are the three segments of one series
    ("fastw", dict(ndim=1, nx=256, mean_batch=BATCH, seg_hop=256), {}, L.K_FASTW, "fastw", SEG),
    ("fastk-power", dict(ndim=1, nx=256, mean_batch=1, seg_hop=256, seg_keep=1), {}, L.K_FASTW, "fastw segments kept", SEG),
    ("fastk", dict(ndim=1, nx=256, mean_batch=1, seg_hop=256, seg_keep=1, out_mode=CX), {}, L.K_FASTW, "fastw segments kept", SEG_X),
    # inverse transforms (complex input, complex output)
    ("fastyc-inverse", dict(ny=256, nx=256, dtype=C64, out_mode=CX, flags=IV), {}, L.K_FASTY, "fasty complex", INV),
    ("fastr-complex-inverse", dict(ndim=1, nx=16384, dtype=C64, out_mode=CX, flags=IV), {}, L.K_FASTR, "fastr complex rows", INV),
    ("fastr-rows-inverse", dict(ndim=1, nx=2048, dtype=C64, out_mode=CX, flags=IV), {}, L.K_FASTR, "fasty complex rows", INV),
    ("fastmy-inverse", dict(ny=100, nx=200, dtype=C128, out_mode=CX, flags=L.AXIS_Y | IV), {}, L.K_FASTM_Y, "fastm y-only", INV),
    ("fastgy-inverse", dict(ny=103, nx=206, dtype=C128, out_mode=CX, flags=L.AXIS_Y | IV), {}, L.K_FASTG_Y, "fastg y-only", INV),
    ("fastg-odd-inverse", dict(ny=45, nx=49, dtype=C128, out_mode=CX, flags=IV), {}, L.K_FASTG, "fastg", INV),
    ("fastmx-inverse", dict(ndim=1, nx=1000, dtype=C128, out_mode=CX, flags=IV), {}, L.K_FASTM_X, "fastm x-only", INV),
    ("fastyc-four-step-inverse", dict(ndim=1, nx=65536, dtype=C64, out_mode=CX, flags=IV), {}, L.K_FASTY, "fasty complex rows, four-step", INV),
    ("generic-prime-inverse", dict(ndim=1, nx=1031, dtype=C128, out_mode=CX, flags=IV), {}, L.K_GENERIC, "main", INV),
    # irfftn from a half spectrum
    ("fastg-c2r", dict(ny=48, nx=64, dtype=C64, out_mode=CX, flags=IV | L.C2R_X), {}, L.K_FASTG, "fastg", C2R),
    ("fastyc-c2r", dict(ny=256, nx=256, dtype=C64, out_mode=CX, flags=IV | L.C2R_X), {}, L.K_FASTY, "fasty complex", C2R),
    ("fastyc-c2r-512", dict(ny=256, nx=512, dtype=C64, out_mode=CX, flags=IV | L.C2R_X), {}, L.K_FASTY, "fasty complex", C2R),  # (the row transforms have nx/2 points: from 512 up)
    ("generic-c2r", dict(ny=64, nx=128, dtype=C64, out_mode=CX, flags=IV | L.C2R_X), {"XRFTHIP_NO_FAST": "1"}, L.K_GENERIC, "main", C2R),
    # the last pass of a three-axis spectrum on the half spectrum of a (nt, ny, nx) grid (accuracy.MODES: the shapes at which the twin indexing can go wrong)
    ("fasth-power", A.herm_kw((8, 6, 10), C64, PW), {}, L.K_FASTH, "fasth", HERM),
    ("fasth-cross-f64", A.herm_kw((12, 4, 6), C128, CR), {}, L.K_FASTH, "fasth", HERM),
    ("fasth-power-odd", A.herm_kw((15, 5, 7), C64, PW), {}, L.K_FASTH, "fasth", HERM),
    # radial sums: the bin map stays indexed by unshifted frequency under SHIFT_*
    ("fasty-iso", dict(ny=256, nx=512, flags=L.ISO), {}, L.K_FASTY, "fasty", ISO),
    ("fasts-iso", dict(ny=64, nx=128, flags=L.ISO), {}, L.K_FASTS, "fasts", ISO),
    ("fastm-iso", dict(ny=180, nx=360, dtype=F64, flags=L.ISO), {}, L.K_FASTM, "fastm", ISO),
    ("fastg-odd-iso", dict(ny=45, nx=49, dtype=F64, flags=L.ISO), {}, L.K_FASTG, "fastg", ISO),
]

def _ids(table):
    return {f"{rid}-{d}" for rid, decos in table.items() for d in decos.split()}


# The (kind, tag) a family that declines a decoration is demoted to, as RECORDED on the emulated library (the MI355X must agree): row -> its demoted decorations.
# Every FLIP_* goes to the generic passes (the composite of one-axis plans under inner / mid); ISHIFT_* on float32 POWER fasty / fastn (the sign (-1)^k rides on
# the phase tables, which a power spectrum does not read); a detrend on complex input; a window or an input phase off the separable form on the four-step rows;
# irfftn of 256 x 256 (the row transforms of the two-pass complex family have nx/2 points, 256 at least: fastyc-c2r-512 stays).
# ... and a window on the rotated input of an inverse plan in the one-axis families (FastRComplex, FastRRows, FastMX, FastMY, FastGY: their kernels, the forward
# transforms' too, read the window by the transform's own sample index, so one_axis_tables -- csrc/host_fasty.cpp -- hands window + ISHIFT of an inverse plan to
# the generic passes, which index by the source position; with PHASE_IN an AXIS_Y plan has no generic form and is refused: REFUSED).
_WIN_ROTATED = "win+ishift win+ishift+phasein noflip-nodetrend noflip-nodetrend-phasein"
_TO_GENERIC = {
    "fasty-power": "ishift flip all noflip noflip-nodetrend", "fasty-complex": "flip all", "fasts": "flip all", "fastm": "flip all", "fastn": "flip all",
    "fastn-f32": "ishift flip all noflip noflip-nodetrend", "fastg": "flip all", "fastg-odd": "flip all", "fastg-c64": "flip const+scale all noflip",
    "fastyc": "flip const+scale all noflip", "fastr": "flip all", "fastr-complex": "flip const+scale all noflip", "fastr-rows": "flip all", "fast1d": "flip all",
    "fastyc-four-step": "win flip const+scale all noflip noflip-nodetrend", "fastmx": "flip all", "fastg-rows": "flip all", "rader-rows": "flip all",
    "fastmy": "flip all", "fastgy": "flip all", "fastgy-odd": "flip all",
    "fastyc-inverse": "flip all-nodetrend all-nodetrend-phasein", "fastr-complex-inverse": "flip all-nodetrend all-nodetrend-phasein " + _WIN_ROTATED,
    "fastr-rows-inverse": "flip all-nodetrend all-nodetrend-phasein " + _WIN_ROTATED, "fastmy-inverse": "flip all-nodetrend win+ishift noflip-nodetrend", "fastgy-inverse": "flip all-nodetrend win+ishift noflip-nodetrend",
    "fastg-odd-inverse": "flip all-nodetrend all-nodetrend-phasein", "fastmx-inverse": "flip all-nodetrend all-nodetrend-phasein " + _WIN_ROTATED,
    "fastyc-four-step-inverse": "win flip win+ishift all-nodetrend noflip-nodetrend phasein win+ishift+phasein all-nodetrend-phasein noflip-nodetrend-phasein",
    "fastyc-c2r": "ishift shift phasein",
}
_TO_GENERIC_F0 = {"fasty-cross": "flip all", "fastm-cross-f32": "flip all"}  # (a cross plan's generic passes: field 0 first)
_TO_FASTM_X = {"fastr-rows": "const+scale noflip"}  # (a detrend on 2048 complex points: the table-length rows)
_TO_COMPOSITE = {"fusedi": "flip all", "fusedi-odd": "flip all", "fusedm": "flip all"}
DEMOTED = {}
for _table, _fam in ((_TO_GENERIC, (L.K_GENERIC, "main")), (_TO_GENERIC_F0, (L.K_GENERIC, "f0")), (_TO_FASTM_X, (L.K_FASTM_X, "fastm x-only")),
                     (_TO_COMPOSITE, (L.K_COMPOSITE, "inner layout"))):
    DEMOTED.update({cid: _fam for cid in _ids(_table)})

# case id -> the status of xrfthip_plan_create / xrfthip_plan_set_*.  An AXIS_Y inverse plan takes PHASE_IN only where a one-pass kernel takes the plan
# (include/xrft_hip.h, XRFTHIP_AXIS_Y): with a flip, or with a window on the rotated input, it is the generic passes' and XRFTHIP_BAD_ARG
_PHASE_IN_Y = "all-nodetrend-phasein win+ishift+phasein noflip-nodetrend-phasein"
REFUSED = {cid: L.BAD_ARG for cid in _ids({"fastmy-inverse": _PHASE_IN_Y, "fastgy-inverse": _PHASE_IN_Y})}

# (id, make() arguments, environment, tokens): refusals outside the rows' decoration lists
EXTRA_REFUSED = [
    ("fastyc-inverse-const", dict(ny=256, nx=256, dtype=C64, out_mode=CX, flags=IV), {}, "const", L.BAD_ARG),  # (INVERSE with a detrend)
    ("fasty-half-shift", dict(ny=256, nx=512, out_mode=CX, flags=L.HALF_X), {}, "shift", L.BAD_ARG),  # (HALF_X with SHIFT_*)
]


def cases():
    """[(id, make() arguments, environment, tokens, (kind, tag) | status)]"""
    out = []
    for rid, kw, env, kind, tag, decos in BASE:
        for d in decos:
            cid = f"{rid}-{d}"
            out.append((cid, kw, env, tuple(NAMED.get(d, d).split("+")), REFUSED.get(cid, DEMOTED.get(cid, (kind, tag)))))
    for cid, kw, env, d, status in EXTRA_REFUSED:
        out.append((cid, kw, env, tuple(d.split("+")), status))
    return out


def plan_of(kw, tab, extra):
    kw = dict(kw)
    if kw.get("ndim", 2) == 1:
        kw.pop("ny", None)
    return engine.SpectralPlan(ndim=kw.pop("ndim", 2), batch=kw.pop("batch"), ny=kw.pop("ny", 1), nx=kw.pop("nx"), dtype=kw.pop("dtype", F32), out_mode=kw.pop("out_mode", L.OUT_POWER), **tab, **extra, **kw)


def run(kw, tokens, expect, dev, seed=0):
    """Execute one case on `dev` ("cpu": the emulated library, "cuda": the real one): the family that ran is the recorded one and the result meets the contract,
    or the library refuses with the documented status.  Returns (plan, rms error in units of u log2 N) or (None, None)."""
    kw, tab = decorate(kw, tokens, seed)
    extra = {}
    if kw.get("flags", 0) & L.ISO:
        bm, nb = A.radial_map(kw["ny"], kw["nx"])
        extra = dict(binmap=bm, nbins=nb)
    if isinstance(expect, int):
        with pytest.raises(L.XrftHipError) as e:
            plan_of(kw, tab, extra)
        assert e.value.status == expect, (e.value.status, expect)
        return None, None
    p = plan_of(kw, tab, extra)
    assert A.family(p) == expect, (A.family(p), expect)
    dt = kw.get("dtype", F32)
    shape, axes, _ = A._axes(kw)
    xs = [A.tensor(v, dt) for v in inputs(kw, seed)]
    x1, x164 = (xs[1][0].to(dev), xs[1][1]) if len(xs) == 2 else (None, None)
    out, isoo = p.execute(A.segment_rows(kw, xs[0][0].to(dev)), A.segment_rows(kw, x1))
    x64 = xs[0][1]
    det = kw.get("detrend", L.DETREND_NONE)
    kap = A.kappa(x64.reshape(shape), A.detrended(x64.reshape(shape), axes, det)) if det else 0.0
    ref, iref = reference(kw, tab, x64, x164, extra.get("binmap"), extra.get("nbins", 0))
    ref = A.segment_mean(kw, ref)  # (a segment row's mean over its segments: the model above is per row and stays as it is)
    n = A.points(kw)
    what = "+".join(tokens)
    # the max-norm bound is for a flat spectrum: noise through OUT_COMPLEX.  Noise + OFFSET under a detrend is not one -- the offset is a zero-frequency term of
    # N OFFSET that cancels in ONE bin, where a mean off by c u moves the result by c u sqrt(N) OFFSET / sigma of rms(ref) (177 c u at 180 x 360: 11 c u log2 N), for
    # any summation order; the norm-wise bound with its kappa term is what a detrended case is held to, as in accuracy.run_ladder's detrended rows (all OUT_POWER)
    flat = kw.get("out_mode", L.OUT_POWER) == L.OUT_COMPLEX and not det
    c = A.assert_accurate(out.cpu().numpy().reshape(ref.shape), ref, dt, n, kap, flat=flat, what=what)
    if iref is not None:
        c = max(c, A.assert_accurate(isoo.cpu().numpy().reshape(iref.shape), iref, dt, n, kap, what=what + " iso"))
    return p, c
