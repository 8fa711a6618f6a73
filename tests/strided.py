"""Shared by tests/test_strided_emulated.py (CPU, the emulated library) and tests/test_gpu_strided.py (GPU): boxes inside buffers of NaN, the families that
read strided input and the modes they serve, and the plan-level property -- a strided plan on the view is bit-identical to the dense plan of the same shape
on ``view.contiguous()``.  Not a conftest: imported by the tests that use it."""
import numpy as np
import pytest
import torch

from xrft_amd import _lib as L

import accuracy as A


# rows beyond the table of tests/accuracy.py, one per strided code path the table's rows do not reach: the shorter FastR rows (fastr2_kernel), the rows of a
# fastg tile / the columns of fastn that are not packed in pairs (an odd nx), pass 1 of fastm with four sequences per workgroup (float32, 2000 rows), the other
# shapes of FastS, float32 row groups of FastG
EXTRA = [
    ("fastr-4096", dict(ndim=1, nx=4096), {}, L.K_FASTR, "fastr"),
    ("fastr-8192", dict(ndim=1, nx=8192), {}, L.K_FASTR, "fastr"),
    ("fastr-16384", dict(ndim=1, nx=16384), {}, L.K_FASTR, "fastr"),
    ("fastr-32768", dict(ndim=1, nx=32768), {}, L.K_FASTR, "fastr"),
    ("fastg-odd", dict(ny=50, nx=45, dtype=A.F64), {}, L.K_FASTG, "fastg"),
    ("fastg-odd-f32", dict(ny=50, nx=45), {}, L.K_FASTG, "fastg"),
    ("fastg-rows-f32", dict(ndim=1, nx=50), {}, L.K_FASTG_ROWS, "fastg rows"),
    ("fastg-rows-odd", dict(ndim=1, nx=45, dtype=A.F64), {}, L.K_FASTG_ROWS, "fastg rows"),
    ("fastn-odd", dict(ny=125, nx=243, dtype=A.F64), {}, L.K_FASTN, "fastn"),
    ("fastn-odd-f32", dict(ny=250, nx=243), {}, L.K_FASTN, "fastn"),
    # the forms of fastn's column kernel beyond the plain radix passes (FASTN_FORM): columns with a prime factor as a chirp convolution (262 = 2 x 131), as the
    # prime-factor form with Rader's convolution along the prime (146 = 2 x 73), and float32 columns with a radix above 16 (400 = 20 x 20: the 20-register form)
    ("fastn-chirp-f32", dict(ny=262, nx=270), {}, L.K_FASTN, "fastn"),
    ("fastn-chirp", dict(ny=262, nx=250, dtype=A.F64), {}, L.K_FASTN, "fastn"),
    ("fastn-rader-f32", dict(ny=146, nx=270), {}, L.K_FASTN, "fastn"),
    ("fastn-rader", dict(ny=146, nx=250, dtype=A.F64), {}, L.K_FASTN, "fastn"),
    ("fastn-r20-f32", dict(ny=400, nx=270), {}, L.K_FASTN, "fastn"),
    ("fastm-wide", dict(ny=2000, nx=2000), {}, L.K_FASTM, "fastm"),
] + [(f"fasts-{ny}x{nx}", dict(ny=ny, nx=nx), {}, L.K_FASTS, "fasts") for ny in (64, 128, 256) for nx in (64, 128, 256)]


def table_row(rid):
    """(make() arguments, kind, tag) of a row of the routing table / the ladder of tests/accuracy.py, or of EXTRA"""
    for r, kw, env, kind, tag in A.ROWS + A.MODES + EXTRA:
        if r == rid:
            assert not env
            return dict(kw), kind, tag
    raise KeyError(rid)


# family -> rows of the table of tests/accuracy.py that route to it (both precisions where the family has them)
FAMILIES = {
    "FastY": ["fasty-small"],
    "FastM": ["fastm-small-f32", "fastm-small"],
    "FastN": ["fastn-small-f32", "fastn-small", "fastn-odd", "fastn-odd-f32", "fastn-chirp-f32", "fastn-chirp", "fastn-rader-f32", "fastn-rader", "fastn-r20-f32"],
    "FastS": ["fasts", "fasts-128x64", "fasts-128x128", "fasts-over-fasty"],
    "FastG": ["fastg-f32", "fastg", "fastg-odd", "fastg-odd-f32"],
    "FastG-rows": ["fastg-rows", "fastg-rows-f32", "fastg-rows-odd"],
    "FastR": ["fastr", "fastr-16384", "fastr-4096"],
}
# the modes of the issue; a family is run in those it serves (FastS: no cross spectrum -- a 64 x 128 cross spectrum is FastG's; 1-D plans: no radial sums,
# FastR: no cross spectrum)
MODES = {
    "power-linear-windows": dict(out_mode=L.OUT_POWER, detrend=L.DETREND_LINEAR, windows=True),
    "complex-shifts": dict(out_mode=L.OUT_COMPLEX, flags=L.SHIFT_Y | L.SHIFT_X),
    "cross": dict(out_mode=L.OUT_CROSS, detrend=L.DETREND_CONSTANT),
    "iso-sums-only": dict(out_mode=L.OUT_POWER, flags=L.ISO | L.NO_SPECTRUM_OUT, iso=True),
}
SERVES = {
    "FastY": list(MODES), "FastM": list(MODES), "FastN": list(MODES), "FastG": list(MODES),
    "FastS": ["power-linear-windows", "complex-shifts", "iso-sums-only"],
    "FastG-rows": ["power-linear-windows", "complex-shifts", "cross"],
    "FastR": ["power-linear-windows", "complex-shifts"],
}


# the form of fastn's column kernel that every FastN row here launches, as describe() tells it (fastn_form): each strided instantiation of that kernel -- plain
# radix passes with radices up to 16 and up to 20, the chirp convolution, the Rader columns, in the precisions they exist in -- is launched by a row
FASTN_FORM = {
    "fastn-small-f32": "radix-16", "fastn-small": "radix-16", "fastn-odd": "radix-16", "fastn-odd-f32": "radix-16",
    "fastn-chirp-f32": "chirp", "fastn-chirp": "chirp", "fastn-rader-f32": "rader", "fastn-rader": "rader", "fastn-r20-f32": "radix-20",
    "fastn": "radix-16", "fastn-complex-f32": "radix-16",  # (rows of the table that the GPU tests run)
}


def fastn_form(text):
    """Which column kernel a FastN plan launches, from the "cols:" part of its describe() line: "table" (fastm's kernel), or fastn's with plain radix passes
    ("radix-16" / "radix-20": the largest radix decides the register form), as a chirp convolution ("chirp") or with Rader's convolution ("rader")."""
    line = next(l for l in text.splitlines() if l.lstrip().startswith("[fastn]"))
    cols = line[line.index("cols:"):line.index("-> W2")]
    if "table kernel" in cols:
        return "table"
    if "chirp convolution" in cols:
        return "chirp"
    if "Rader" in cols:
        return "rader"
    radices = cols[cols.index(" r", cols.index("(FFT")) + 2:].split(" ")[0]
    return "radix-20" if max(int(r) for r in radices.split("x")) > 16 else "radix-16"


def plan_params():
    out = []
    for fam, rows in FAMILIES.items():
        for rid in rows:
            for mode in SERVES[fam]:
                out.append(pytest.param(rid, mode, id=f"{fam}-{rid}-{mode}"))
    out.append(pytest.param("fastm-wide", "power-linear-windows", id="FastM-fastm-wide-power-linear-windows"))  # (2000 x 2000: one mode on the CPU, all four on the GPU)
    return out


def box_in_nan(kw, rng, place, dtype, pad_x=8, scale=1.0, dev="cpu"):
    """A (batch, ny, nx) -- 1-D: (batch, nx) -- view of seeded noise on a plane inside a larger buffer of NaN: origin on a 16-byte boundary, pitch > nx,
    batch stride > ny * pitch.  place = "end": the box's last sample is the buffer's last element.  Returns (view, in_stride_y, in_stride_batch)."""
    ndim, batch, nx = kw.get("ndim", 2), kw.get("batch", 2), kw["nx"]
    ny = kw["ny"] if ndim == 2 else 1
    q = 16 // torch.empty((), dtype=dtype).element_size()  # elements per 16 bytes
    pitch = (nx + pad_x + q - 1) // q * q
    sb = ny * pitch + 2 * q
    off = 2 * q + (0 if place == "end" else 3 * pitch)
    last = off + (batch - 1) * sb + (ny - 1) * pitch + nx  # one past the box's last sample
    buf = torch.full((last + (0 if place == "end" else 5 * q + 1),), float("nan"), dtype=dtype)
    v = rng.standard_normal((batch, ny, nx)) * scale + 0.01 * np.arange(ny).reshape(1, ny, 1) - 0.02 * np.arange(nx).reshape(1, 1, nx) + 0.5
    view = torch.as_strided(buf, (batch, ny, nx), (sb, pitch, 1), off)
    view.copy_(torch.from_numpy(v).to(dtype))
    if dev != "cpu":
        buf = buf.to(dev)
        view = torch.as_strided(buf, (batch, ny, nx), (sb, pitch, 1), off)
    assert view.data_ptr() % 16 == 0 and int(torch.isnan(buf).sum()) == buf.numel() - batch * ny * nx
    if ndim == 1:
        return torch.as_strided(buf, (batch, nx), (sb, 1), off), 0, sb
    return view, pitch, sb


def windows(kw):
    ndim, nx = kw.get("ndim", 2), kw["nx"]
    w = dict(window_x=0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nx) / nx))
    if ndim == 2:
        ny = kw["ny"]
        w["window_y"] = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(ny) / ny)
    return w


def finite(t):
    return bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all())


def run_plan_case(kw, kind, tag, mode, dev="cpu", batch=3, pad_x=8, form=None):
    """One family x mode: the strided plan on a box in NaN against the dense plan on its contiguous copy, bit for bit; both route to (kind, tag) -- and, a
    FastN row, to the form of the column kernel that FASTN_FORM names."""
    kw = dict(kw)
    m = dict(MODES[mode])
    kw.update(out_mode=m["out_mode"], detrend=m.get("detrend", L.DETREND_NONE), flags=m.get("flags", 0), batch=batch)
    if kw.get("ndim", 2) == 1:
        kw["flags"] &= ~L.SHIFT_Y
    kw.pop("iso", None)
    dtype = kw.get("dtype", A.F32)
    extra = {}
    if m.get("windows"):
        extra.update(windows(kw))
    if m.get("iso"):
        bm, nb = A.radial_map(kw["ny"], kw["nx"])
        extra.update(binmap=bm, nbins=nb)
    rng = np.random.default_rng(5)
    place = "end" if mode == "power-linear-windows" else "middle"
    x, sy, sb = box_in_nan(kw, rng, place, dtype, pad_x=pad_x, dev=dev)
    x1 = None
    if m["out_mode"] == L.OUT_CROSS:
        x1, sy1, sb1 = box_in_nan(kw, rng, "middle", dtype, pad_x=pad_x, dev=dev)  # the second field: a box of its own buffer, the same strides
        assert (sy1, sb1) == (sy, sb)
    dense = A.make(**kw, **extra)
    strided = A.make(**kw, **extra, in_stride_y=sy, in_stride_batch=sb)
    assert A.family(dense) == (kind, tag), (A.family(dense), kind, tag)
    assert A.family(strided) == (kind, tag) and strided.kernel_info() == dense.kernel_info()
    line = next(t for t in strided.describe().splitlines() if t.lstrip().startswith(f"[{tag}]"))  # (the line of the pass that reads the input)
    assert f"in pitch {sy or kw['nx']} / slab {sb}" in line and "in pitch" not in dense.describe()
    if tag == "fastn":
        assert form is not None and fastn_form(strided.describe()) == fastn_form(dense.describe()) == form, (fastn_form(strided.describe()), form)
    assert not x.is_contiguous()
    out_s, iso_s = strided.execute(x, x1)
    out_d, iso_d = dense.execute(x.contiguous(), None if x1 is None else x1.contiguous())
    if m.get("iso"):
        assert out_s is None and out_d is None
        assert torch.equal(iso_s, iso_d) and finite(iso_s)
    else:
        assert torch.equal(out_s, out_d) and finite(out_s)
    with pytest.raises(ValueError):  # a tensor with other strides than the plan's is refused before the device sees its pointer
        strided.execute(x.contiguous(), None if x1 is None else x1.contiguous())
    return strided
