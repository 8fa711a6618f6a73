"""Shared cases of the half-precision input tests (CPU: tests/test_half_input_emulated.py, GPU: tests/test_gpu_half_input.py).  Not a conftest: imported.

The sharp property needs no tolerance: widening float16 / bfloat16 to float32 is exact, and a half plan is the float32 plan behind its loads, so

    half_plan(x16)  ==  f32_plan(x16.float())        bit for bit

for every family that reads 2-byte samples (FastY and its four-step form, FastS, FastR, FastG slabs and row groups) -- and at the API level for every call,
whether its plan reads the field where it lies or the field is widened once (xrfthip_convert) for a family that declines."""
import itertools

import numpy as np
import scipy.signal as sps
import torch

from xrft_amd import _lib as L
from xrft_amd import engine

import accuracy as A

HALVES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
NOTE = {"float16": "float16 input read where it lies", "bfloat16": "bfloat16 input read where it lies"}

# (id, make() arguments without dtype / batch, environment at plan creation, kernel kind, describe tag): the smallest row of each family that takes half input in
# the routing ladder of tests/accuracy.py (a 256 x 256 slab is FastS's: the two-pass kernels take it with FastS off; 256 x 512 is theirs anyway)
ROWS = [
    ("fasts-64x64", dict(ny=64, nx=64), {}, L.K_FASTS, "fasts"),
    ("fasty-256x256", dict(ny=256, nx=256), {"XRFTHIP_FASTS": "0"}, L.K_FASTY, "fasty"),
    ("fasty-256x512", dict(ny=256, nx=512), {}, L.K_FASTY, "fasty"),
    ("fastr-4096", dict(ndim=1, nx=4096), {}, L.K_FASTR, "fastr"),
    ("fastg-50x50", dict(ny=50, nx=50), {}, L.K_FASTG, "fastg"),
    ("fastg-6x10", dict(ny=6, nx=10), {}, L.K_FASTG, "fastg"),
    ("fastg-15x9", dict(ny=15, nx=9), {}, L.K_FASTG, "fastg"),       # odd x odd: the rows as complex sequences, one sample per load
    ("fastg-rows-50", dict(ndim=1, nx=50), {}, L.K_FASTG_ROWS, "fastg rows"),
]
ROW_IDS = [r[0] for r in ROWS]
MODES = ("power", "complex", "cross", "phase", "iso", "half_x")
HALF_KINDS = (L.K_FASTY, L.K_FASTS, L.K_FASTR, L.K_FASTG, L.K_FASTG_ROWS)
HALF_TAGS = ("fasty", "fasty four-step", "fasts", "fastr", "fastg", "fastg rows")

# (detrend, Hann window, shifts, batch): the whole product for power spectra, a covering set for the other modes
FULL = list(itertools.product((L.DETREND_NONE, L.DETREND_CONSTANT, L.DETREND_LINEAR), (False, True), (False, True), (1, 3)))
COVER = [(L.DETREND_NONE, False, False, 1), (L.DETREND_CONSTANT, True, True, 3), (L.DETREND_LINEAR, True, False, 3), (L.DETREND_LINEAR, False, True, 1)]


def row(rid):
    r = ROWS[ROW_IDS.index(rid)]
    return dict(r[1]), dict(r[2]), r[3], r[4]


def field(shape, dtype, seed, dev="cpu"):
    """Seeded noise on a plane in half precision: (the 2-byte tensor, its exact float32 image)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float32)
    x = x + 0.01 * torch.arange(shape[-1], dtype=torch.float32) + 1.5
    if len(shape) > 2:
        x = x - 0.02 * torch.arange(shape[-2], dtype=torch.float32).reshape(-1, 1)
    h = x.to(dtype).to(dev)
    return h, h.float()


def mode_kw(kw, mode, detrend, window, shift, batch):
    """make() arguments of one case, or None where the descriptor does not exist (radial sums of a 1-D transform)."""
    ndim, ny, nx = kw.get("ndim", 2), kw.get("ny", 1), kw["nx"]
    if mode == "iso" and ndim == 1:
        return None
    out = dict(kw, batch=batch, detrend=detrend)
    flags = 0
    if shift and mode != "half_x":  # (real_dim output is unshifted)
        flags |= L.SHIFT_X | (L.SHIFT_Y if ndim == 2 else 0)
    out["out_mode"] = {"power": L.OUT_POWER, "complex": L.OUT_COMPLEX, "cross": L.OUT_CROSS, "phase": L.OUT_PHASE, "iso": L.OUT_POWER, "half_x": L.OUT_POWER}[mode]
    if mode == "half_x":
        flags |= L.HALF_X | L.REALDIM_X2
    if mode == "iso":
        bm, nb = A.radial_map(ny, nx)
        flags |= L.ISO
        out.update(binmap=bm, nbins=nb)
    if window:
        out["window_x"] = sps.windows.hann(nx, sym=False)
        if ndim == 2:
            out["window_y"] = sps.windows.hann(ny, sym=False)
    out["flags"] = flags
    return out


def try_make(**kw):
    """The plan, or None where the library answers XRFTHIP_UNSUPPORTED_LENGTH (the documented "caller falls back")."""
    try:
        return A.make(**kw)
    except L.XrftHipError as e:
        if e.status != L.UNSUPPORTED_LENGTH:
            raise
        return None


def run_plan_case(kw, hname, seed, dev="cpu"):
    """One descriptor with half input against the float32 plan on the widened samples.  Returns "taken" or "declined" (the float32 plan's family has no 2-byte
    loader); a family that has one must take the plan, say so in describe(), and give the float32 plan's bits."""
    hdt = HALVES[hname]
    two = kw["out_mode"] in (L.OUT_CROSS, L.OUT_PHASE)
    shape = (kw["batch"], kw.get("ny", 1), kw["nx"]) if kw.get("ndim", 2) == 2 else (kw["batch"], kw["nx"])
    x16, x32 = field(shape, hdt, seed, dev)
    y16, y32 = field(shape, hdt, seed + 1000, dev) if two else (None, None)
    pf = A.make(**kw, dtype=torch.float32)
    kind, tag = A.family(pf)
    ph = try_make(**kw, dtype=hdt)
    taught = kind in HALF_KINDS and tag in HALF_TAGS
    if ph is None:
        assert not taught, f"a {tag} plan declined {hname} input: {kw}"
        return "declined"
    assert taught and A.family(ph) == (kind, tag), (A.family(ph), kind, tag)
    assert NOTE[hname] in ph.describe() and "input read where it lies" not in pf.describe(), ph.describe()
    assert ph.workspace_bytes == pf.workspace_bytes and ph.out_dtype() == pf.out_dtype()
    oh, ih = ph.execute(x16, y16)
    of, if_ = pf.execute(x32, y32)
    for a, b in ((oh, of), (ih, if_)):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), f"{hname} {tag}: {int((a != b).sum())} of {a.numel()} values differ from the float32 plan's ({kw})"
            assert bool(torch.isfinite(torch.view_as_real(a) if a.is_complex() else a).all())
    oh2, ih2 = ph.execute(x16, y16)  # repeated calls: the same bits
    assert (oh2 is None or torch.equal(oh2, oh)) and (ih2 is None or torch.equal(ih2, ih))
    return "taken"


def all_patterns(hname, dev="cpu"):
    """All 65 536 bit patterns of the format, as a tensor of that dtype."""
    bits = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy())
    return bits.view(HALVES[hname]).to(dev)


def bits32(t):
    return t.contiguous().view(torch.int32)
