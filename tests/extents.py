"""The extent ladder, shared by tests/test_gpu_extents.py (the MI355X) and tests/test_extents_emulated.py (the emulated library: the guards, the checker's own
tests, a few cases through the whole harness at a batch of 96).  Not a conftest: imported by the tests that use it.

Every other test of the suite runs batches of 1 to 17 and buffers of a few MB.  Here a slab, row or series COUNT exceeds one grid dimension (rung A), an element
offset exceeds 2^31 and a byte offset 2^32 and 2^33 (rung B: dense; rung C: through the descriptor's strides), and the host guards that the kernels' 32-bit
in-slab arithmetic rests on are pinned at the limit and one step past it (rung D).

Data.  One PERIOD of 48 distinct slabs (rows, series, columns) per case: seeded standard normal noise on a small plane (line), slab j scaled by 1 + j / 48, rounded
to the plan's dtype; its exact float64 image feeds the reference (accuracy.tensor).  The device input is the period repeated batch / 48 times.  48 is a multiple of
16 -- a kernel that packs 2, 4, 8 or 16 consecutive sequences into one transform gives every copy of a slab the same partners in the same roles -- and divides no
power of two: a read or write displaced by 2^31 or 2^32 elements, or 2^32 or 2^33 bytes, lands on ANOTHER member of the period or off the slab grid altogether
(boundaries() asserts it per case).  The second field of a two-field case is the period rolled by 5 slabs plus seeded noise: the pairing depends on the position.

Reference and bound.  accuracy.reference (decorations.reference, the same model with windows and rotations, where a case has them) on the float64 image of the 48
slabs -- one small CPU computation per case --, welch.reference / batch_mean.reference / coherence's quotient for the averaged forms; accuracy.bound,
batch_mean.bound, welch.bound, coherence.bound.  No tolerance of its own.

check() is the one checker: the windows (whole periods: the first, the last, every period that holds a boundary slab) slab by slab against float64; EVERY slab on
the device against its member of the first period, || out[k] - out[k % 48] || <= 2 bound || out[k % 48] || and finite -- bit for bit where EXACT says so --; the
guard bands around output, radial sums and workspace unchanged.  run_banded() executes through xrfthip_exec with its own pointers: output, sums and workspace carved
from one device buffer, 1 MiB of 0xA5 in front of and behind each, the workspace exactly xrfthip_workspace_bytes, the output 0xFF (NaN) before the call."""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from xrft_amd import _lib as L
from xrft_amd import api, engine

import accuracy as A
import batch_mean as B
import coherence as CO
import decorations as D
import strided as S
import welch as W
import welch_cols as WC

PERIOD = 48
BAND = 1 << 20
PATTERN = 0xA5
COUNT = PERIOD * 1460  # 70 080: more than one grid dimension holds
F16 = torch.float16

# Families whose results are held to torch.equal across the batch: a slab's arithmetic does not know the slab's position.  Decided from the code (xrft_amd/csrc, the
# lines that map workgroups to slabs), then observed on the MI355X (every case prints "bit-identical across the batch: True | False" whether it asserts it or not):
EXACT = {
    "fasty": "host_fasty.cpp:307, 341: gc x (column blocks | row units) workgroups, each inside ONE slab; :327-328 the plane fit, one workgroup per slab; groups only "
             "bound the intermediate (the older FastY test relies on it)",
    "fasty complex": "host_fasty.cpp:640, 644: the same two passes on complex slabs, gc x units of one slab each",
    "fasts": "fasts.h:224: a workgroup walks whole slabs one at a time (registers + LDS); sums in wave order inside it",
    "fastm": "host_fastm.cpp:494, 508: units = gc x column blocks of a slab (pairs of columns packed INSIDE a slab); :548 rows of one slab; :529-533 the fit, one "
             "workgroup per slab; radial sums per slab in a fixed order",
    "fastn": "host_fastm.cpp:429, 454: the same units with run-time lengths",
    "fastr": "fastr.h:212, 382: a workgroup walks whole rows one at a time (row += gridDim.x), fastr_kernel and fastr2_kernel alike",
    "fastg": "fastg.h:288: a workgroup walks whole slabs one at a time (slab += gridDim.x), the slab in LDS",
    "fasth": "fasth.h:105-107: unit = (slab, block of G columns of ITS half spectrum); no sums",
    "fastg y-only": "fastg.h:695-697: unit = (slab, block of columns of that slab); the columns packed in pairs are neighbours inside the slab",
    "fastm y-only": "host_fastm.cpp:717: units = batch x column blocks of a slab, likewise",
}
# Held to the 2 x bound form only -- a sequence shares a transform or a tile with sequences of OTHER slabs, so its bits may depend on who they are or where it lies:
#   "fastm x-only", "fastg rows Rader"   two real ROWS packed into one complex transform (fastm.h:266, host_fastm.cpp:784-785: 2 g rows per workgroup; fastg.h:699-700):
#                                        a row's rounding depends on its partner, the row before or behind it
#   "fastg rows"                         g_rows rows share one tile (host_fastg.cpp:75, fastg.h:44, :288 with slab = a group of rows); a row's place in the tile decides
#                                        which lanes hold and reduce it -- not followed further
#   "fasty complex rows"                 R.rk rows per workgroup of fastyc_rows_kernel (host_rows.cpp:217)
#   "main" (the generic passes), "inner layout" (the composite runs them)   tiles of T consecutive sequences across slab borders (tile_fft.h:556-561); T need not divide 48
#   the mean forms                       a run adds its slabs in an order that depends on how the outputs fall on the groups (host_fasty.cpp:372-375: the outputs a
#                                        group reaches; fastw: host_welch.inc:47-48, pairs of segments per round)
# Observed (profiles/r23_extents.txt): every case of rungs A and B, these included, returned the same bits for every copy of a slab -- with a period of 48 the partners
# and the orders repeat at these group and tile sizes; a change of either may break that without breaking the contract, so they are not held to it.


@contextlib.contextmanager
def library_env(env):
    """The library's environment variables (read when a plan is created) while the block runs: every XRFTHIP_* removed, then `env`; put back afterwards."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("XRFTHIP_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def precision(dtype):
    """The dtype whose unit roundoff bounds a plan's result: a half-precision plan is the float32 plan reading 2-byte samples."""
    return A.F32 if dtype in engine._HALF else dtype


def esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


# ---------------------------------------------------------------------------------- the period
def period_field(shape, axes, cplx, seed, period=PERIOD):
    """[period, *shape] float64 / complex128: seeded noise on a small plane over `axes` (of the slab), slab j scaled by 1 + j / period; a complex field has
    independent real and imaginary parts."""
    rng = np.random.default_rng(seed)
    full = (period,) + tuple(shape)

    def part(sign):
        v = rng.standard_normal(full) + 0.5
        for a in axes:
            shp = [1] * len(full)
            shp[a + 1] = shape[a]
            v = v + sign * 0.01 * (a + 1) * np.arange(shape[a]).reshape(shp)
        return v

    v = part(1.0) + (1j * part(-1.0) if cplx else 0.0)
    return v * (1.0 + np.arange(period) / period).reshape((-1,) + (1,) * len(shape))


def second_period(v, seed):
    """The period rolled by 5 slabs plus a tenth of seeded noise (welch.second_series along the batch): slab j is paired with slab j - 5."""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(v.shape) + (1j * rng.standard_normal(v.shape) if np.iscomplexobj(v) else 0.0)
    return np.roll(v, 5, axis=0) + 0.1 * n


# ---------------------------------------------------------------------------------- boundaries
LIMITS = (("2^31 elements", 1 << 31, False), ("2^32 bytes", 1 << 32, True), ("2^33 bytes", 1 << 33, True))


def boundaries(n, in_elems, in_esz, out_elems, out_esz, period=PERIOD):
    """{name: the first of `n` slabs whose input / output element offset is at or above 2^31, whose byte offset is at or above 2^32 / 2^33} -- those the case reaches.
    in_elems / out_elems: elements per slab (per output of the period's index); a wrap distance that is a whole number of slabs is no multiple of the period."""
    out = {}
    for side, per, esz in (("input", in_elems, in_esz), ("output", out_elems, out_esz)):
        if not per:
            continue
        for wrap, step in ((1 << 31, per), (1 << 32, per), (1 << 32, per * esz), (1 << 33, per * esz)):  # 2^31, 2^32 elements; 2^32, 2^33 bytes
            assert wrap % step != 0 or (wrap // step) % period != 0, (side, wrap, step)
        for name, lim, in_bytes in LIMITS:
            step = per * esz if in_bytes else per
            k = -(-lim // step)
            if k < n:
                out[f"{side} {name}"] = k
    return out


def batch_beyond(in_elems, out_elems, period=PERIOD, limit=1 << 31):
    """The smallest multiple of the period for which one whole period lies beyond element offset `limit` in input and output."""
    k = -(-limit // min(e for e in (in_elems, out_elems) if e))
    return (-(-k // period) + 1) * period


# ---------------------------------------------------------------------------------- the checker
def _real2d(t):
    t = t.reshape(t.shape[0], -1)
    return torch.view_as_real(t).reshape(t.shape[0], -1) if t.is_complex() else t


def plain_accurate(dtype, n, kap):
    """The window check of a plain plan: accuracy.assert_accurate per slab."""
    def f(got, ref, j, what):
        A.assert_accurate(got.reshape(ref.shape), ref, dtype, n, kap, what=what)
    return f


def mean_accurate(bnd, mag=None):
    """The window check of an averaged form: batch_mean.rel_error within bnd[j] (a cross spectrum's against the mean of the terms' magnitudes)."""
    def f(got, ref, j, what):
        err = B.rel_error(got.reshape(ref.shape), ref, None if mag is None else mag[j])
        assert np.isfinite(got).all() and err <= bnd[j], f"{what}: error {err:.3e} > {bnd[j]:.3e}"
    return f


def absolute_accurate(bnd):
    """... of a coherence (values in [0, 1]): rms(got - ref) within bnd[j], as coherence.assert_outputs."""
    def f(got, ref, j, what):
        err = float(np.sqrt(np.mean((got.reshape(ref.shape).astype(np.float64) - ref) ** 2)))
        assert np.isfinite(got).all() and err <= bnd[j], f"{what}: rms error {err:.3e} > {bnd[j]:.3e}"
    return f


def check(out, ref, bnd, bounds, accurate, exact=False, bands=(), period=PERIOD, what="", chunk_bytes=256 << 20, absolute=False):
    """out: [n, ...] tensor on any device, n a multiple of `period`; ref: [period, ...] float64 / complex128; bnd: the bound (a number, or one per member of the
    period); bounds: {name: slab index} from boundaries(); accurate(got, ref_j, j, what): the window check; bands: uint8 tensors that must still hold PATTERN.
    absolute: the all-slab form is || out[k] - out[k % period] || <= 2 bound sqrt(elements) (a coherence).  Returns whether every slab equalled its member bit for bit."""
    n = out.shape[0]
    assert n % period == 0 and n >= period and ref.shape[0] == period, (n, period, ref.shape)
    o2 = _real2d(out)
    # 2. windows against the float64 reference, slab by slab
    wins = {0: "first", n // period - 1: "last"}
    for name, k in bounds.items():
        assert 0 <= k < n, (name, k, n)
        wins.setdefault(k // period, name)
    for q, name in sorted(wins.items()):
        host = out[q * period:(q + 1) * period].cpu().numpy()
        for j in range(period):
            accurate(host[j], ref[j], j, f"{what} slab {q * period + j} (period {q}: {name})")
    # 3. every slab against its member of the first period, on the device
    base = o2[:period]
    assert bool(torch.isfinite(base).all()), f"{what}: a value of the first period is not finite"
    b2 = torch.as_tensor(np.broadcast_to(np.asarray(bnd, dtype=np.float64), (period,)).copy(), device=out.device)
    lim = (2.0 * b2) ** 2 * (float(o2.shape[1]) if absolute else base.double().pow(2).sum(1))
    per_chunk = max(1, chunk_bytes // max(1, period * o2.shape[1] * o2.element_size()))
    same = True
    for q0 in range(0, n // period, per_chunk):
        q1 = min(n // period, q0 + per_chunk)
        c = o2[q0 * period:q1 * period].reshape(q1 - q0, period, -1)
        fin = torch.isfinite(c).reshape(q1 - q0, period, -1).all(2)
        if not bool(fin.all()):
            q, j = [int(v[0]) for v in torch.nonzero(~fin, as_tuple=True)]
            raise AssertionError(f"{what}: slab {(q0 + q) * period + j} holds a value that is not finite")
        d = (c - base).double().pow(2).sum(2)
        bad = d > lim
        if bool(bad.any()):
            q, j = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
            raise AssertionError(f"{what}: slab {(q0 + q) * period + j} is {float(d[q, j]) ** 0.5:.3e} from slab {j} of the first period, more than {float(lim[j]) ** 0.5:.3e}")
        same = same and bool((c == base).all())
    print(f"{what}: {n} slabs, windows {sorted(set(wins.values()))}, bit-identical across the batch: {same}")
    if exact:
        assert same, f"{what}: a slab differs in its bits from its member of the first period"
    # 4. guard bands
    for i, band in enumerate(bands):
        assert bool((band == PATTERN).all()), f"{what}: guard band {i} was written"
    return same


# ---------------------------------------------------------------------------------- execution with the case's own pointers
class Banded:
    """One uint8 device buffer: [band | region | band | region | ... | band], every region on a 256-byte boundary, at least BAND bytes of PATTERN between."""

    def __init__(self, dev, regions, band=BAND):
        self.offs, at = {}, band
        for name, nbytes in regions:
            self.offs[name] = (at, int(nbytes))
            at = (at + int(nbytes) + band + 255) & ~255
        self.total = at
        self.buf = torch.empty(self.total + 256, dtype=torch.uint8, device=dev)
        self.start = (-self.buf.data_ptr()) % 256
        prev = 0
        self.bands = []
        for name, (off, nbytes) in self.offs.items():
            self.bands.append(self.buf[self.start + prev:self.start + off])
            prev = off + nbytes
        self.bands.append(self.buf[self.start + prev:self.start + self.total])
        for b in self.bands:
            b.fill_(PATTERN)

    def bytes_of(self, name):
        off, nbytes = self.offs[name]
        return self.buf[self.start + off:self.start + off + nbytes]

    def ptr(self, name):
        return C.c_void_p(self.buf.data_ptr() + self.start + self.offs[name][0])


def out_shape(plan):
    """(outputs, elements per output) of a plan's result."""
    if plan.herm_ny:
        return plan.batch, plan.ny * plan.herm_ny * plan.herm_nx
    if plan.seg_hop and plan.seg_stride > 1:
        return plan.batch_out * plan.inner, plan.nx_out
    return plan.batch_out, plan.ny_out * plan.nx_out * plan.inner * plan.mid


def device_bytes(plan, in_bytes, nfields=1):
    """What a case needs on the device: input(s), output, radial sums, workspace and bands, and the checker's chunk temporaries."""
    n, e = out_shape(plan)
    want_out = not (plan.flags & L.NO_SPECTRUM_OUT)
    iso = n * plan.nbins * (16 if plan.out_mode == L.OUT_CROSS else 8) if plan.flags & L.ISO else 0
    return in_bytes * nfields + (n * e * esize(plan.out_dtype()) if want_out else 0) + iso + plan.workspace_bytes + 4 * BAND + (2 << 30)


def run_banded(plan, x0, x1=None):
    """xrfthip_exec on the null stream with output, radial sums and workspace carved from one buffer between guard bands; the workspace is exactly
    xrfthip_workspace_bytes, the output and the sums hold NaN (0xFF) before the call.  Returns (out [outputs, elements] | None, iso | None, the bands)."""
    dev = x0.device
    n, e = out_shape(plan)
    odt = plan.out_dtype()
    want_out = not (plan.flags & L.NO_SPECTRUM_OUT)
    idt = torch.complex128 if plan.out_mode == L.OUT_CROSS else torch.float64
    iso_on = bool(plan.flags & L.ISO)
    need = plan.workspace_bytes
    regions = [("out", n * e * esize(odt) if want_out else 0), ("iso", n * plan.nbins * esize(idt) if iso_on else 0), ("ws", need)]
    m = Banded(dev, regions)
    m.bytes_of("out").fill_(0xFF)
    m.bytes_of("iso").fill_(0xFF)
    null = C.c_void_p(0)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    rc = plan._dll.xrfthip_exec(plan._h, C.c_void_p(x0.data_ptr()), null if x1 is None else C.c_void_p(x1.data_ptr()), m.ptr("out") if want_out else null,
                                m.ptr("iso") if iso_on else null, m.ptr("ws"), need, null)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    L.check(rc)
    out = m.bytes_of("out").view(odt).reshape(n, e) if want_out else None
    iso = m.bytes_of("iso").view(idt).reshape(n, plan.nbins) if iso_on else None
    return out, iso, m.bands


def enough_memory(need, dev):
    """(enough?, the sentence for a skip): torch.cuda.mem_get_info() against what the case states; the emulated device is the host."""
    if torch.device(dev).type != "cuda":
        return True, ""
    free = torch.cuda.mem_get_info()[0]
    return free >= need, f"needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB are free"


def release(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class NeedsMemory(Exception):
    """A case states more device memory than is free: the GPU test skips (and the issue's "none skipped" then fails the run)."""


# ---------------------------------------------------------------------------------- the plain plans (rungs A and B)
def row(rid, **over):
    """(make() arguments, environment, kind, tag) of a row of the tables of tests/accuracy.py / tests/strided.py, with arguments replaced."""
    for r, kw, env, kind, tag in A.ROWS + A.MODES + S.EXTRA:
        if r == rid:
            return dict(kw, **over), dict(env), kind, tag
    raise KeyError(rid)


def _narrow(rid, nx):
    kw, env, kind, tag = row(rid)
    return dict(kw, nx=nx), env, kind, tag


# the narrowest nx at which family() still reports the y-only families at a batch of COUNT: fastm y-only (100 rows of float64) from 8 columns -- below it the plan
# is fastg y-only's or the generic passes' --, fastg y-only (103 rows) from 2; test_extents_emulated.py::test_the_y_only_rows_are_the_narrowest pins both
FASTMY_NX, FASTGY_NX = 8, 2

# id -> (make() arguments, environment at plan creation, kind, tag); "windows": Hann x Hamming tables (strided.windows), "iso": a radial bin map
RUNG_A = {
    "fasts-linear-windows-shifts": (dict(ny=64, nx=64, detrend=L.DETREND_LINEAR, flags=L.SHIFT_Y | L.SHIFT_X, windows=True), {}, L.K_FASTS, "fasts"),
    "fasts-iso": (dict(ny=64, nx=64, flags=L.ISO, iso=True), {}, L.K_FASTS, "fasts"),
    "fastg": row("fastg"),
    "fastg-rows": row("fastg-rows"),
    "fastgy-rows-rader": row("fastgy-rows"),
    "fastmx-complex": row("fastmx-complex"),
    "fastr-4096-complex": row("fastr-4096", out_mode=L.OUT_COMPLEX),
    "fastr-rows-2048-c64": row("fastr-rows-over-complex"),
    "fusedi-33x32-half-y": row("fusedi-half-y-odd-f32"),
    "fasth-shifts": row("fasth-power-f32"),
    "fastmy-linear": _narrow("fastmy-linear", FASTMY_NX),
    "fastgy-linear": _narrow("fastgy-linear", FASTGY_NX),
    "generic-16x16": (dict(ny=16, nx=16), {"XRFTHIP_NO_FAST": "1"}, L.K_GENERIC, "main"),
}
RUNG_B = {
    "fasts-256x256": row("fasts-over-fasty"),
    "fasts-256x256-float16": row("fasts-over-fasty", dtype=F16),
    "fastr-65536": row("fastr"),
    "fastr-4096": row("fastr-4096"),
    "fastg-f64": row("fastg"),
    "fastg-f32": row("fastg-f32"),
    "fastm-180x360-linear": row("fastm-small-f32"),
    "fastn-243x270": row("fastn-small-f32"),
    "fastn-125x250-f64-complex": row("fastn-small"),
    "fasty-256x512": row("fasty-small"),
    "fastyc-256x256": row("fastyc-small"),
    "fusedi-128x256": row("fusedi"),
    "composite-128x256": row("composite"),
    "fasth": row("fasth-power-f32"),
    "fastmx-1000-f64": row("fastmx"),
    "fastmy-100x200-f64": row("fastmy"),
    "generic-256x256": (dict(ny=256, nx=256), {"XRFTHIP_NO_FAST": "1"}, L.K_GENERIC, "main"),
}


def plain_setup(kw, env, batch):
    """(plan, the period's tensors [x0, x1 | None], reference out [48, ...], reference iso | None, bound, window check) of a plain plan at `batch` slabs."""
    kw = dict(kw)
    extra, tab = {}, dict(window_y=None, window_x=None, phase_y=None, phase_x=None, scale=1.0)
    if kw.pop("iso", False):
        bm, nb = A.radial_map(kw["ny"], kw["nx"])
        extra.update(binmap=bm, nbins=nb)
    if kw.pop("windows", False):
        tab.update(S.windows(kw))
        extra.update(S.windows(kw))
    dt = kw.get("dtype", A.F32)
    prec = precision(dt)
    rkw = dict(kw, batch=PERIOD, dtype=prec)
    shape, axes, _ = A._axes(rkw)
    v = period_field(shape[1:], [a - 1 for a in axes], prec in (A.C64, A.C128), seed=7)
    x0, x064 = A.tensor(v, dt)
    two = kw.get("out_mode", L.OUT_POWER) in (L.OUT_CROSS, L.OUT_PHASE)
    x1, x164 = A.tensor(second_period(v, seed=8), dt) if two else (None, None)
    decorated = tab["window_x"] is not None or (not kw.get("herm_ny") and kw.get("flags", 0) & (L.SHIFT_Y | L.SHIFT_X))
    if decorated:
        ref, iref = D.reference(rkw, tab, x064, x164, extra.get("binmap"), extra.get("nbins", 0))
    else:
        ref, iref = A.reference(rkw, x064, x164, extra.get("binmap"), extra.get("nbins", 0))
    det = kw.get("detrend", L.DETREND_NONE)
    kap = A.kappa(x064.reshape(shape), A.detrended(x064.reshape(shape), axes, det)) if det else 0.0
    n = A.points(rkw)
    with library_env(env):
        plan = A.make(**dict(kw, batch=batch), **extra)
    return plan, [x0, x1], ref.reshape(PERIOD, -1), iref, A.bound(prec, n, kap), plain_accurate(prec, n, kap)


def dense_batch(kw, env):
    """The batch of a rung B case: the smallest multiple of the period with one whole period beyond element offset 2^31 in input and output."""
    kw = {k: v for k, v in kw.items() if k not in ("iso", "windows")}
    with library_env(env):
        plan = A.make(**dict(kw, batch=PERIOD))
    shape, _, _ = A._axes(dict(kw, batch=PERIOD, dtype=precision(kw.get("dtype", A.F32))))
    return batch_beyond(int(np.prod(shape[1:])), out_shape(plan)[1])


def tiled(x, batch, dev):
    """The period repeated to `batch` slabs on the device."""
    x = x.to(dev)
    return x.repeat((batch // x.shape[0],) + (1,) * (x.dim() - 1))


def run_plain(cid, kw, env, kind, tag, batch, dev, exact=None):
    """One plain case at `batch` slabs: family, windows against float64, every slab against the period, guard bands; the same for the radial sums."""
    assert batch % PERIOD == 0
    plan, xs, ref, iref, bnd, accurate = plain_setup(kw, env, batch)
    assert A.family(plan) == (kind, tag), (A.family(plan), kind, tag)
    in_elems = xs[0][0].numel()
    n, e = out_shape(plan)
    assert n == batch
    need = device_bytes(plan, batch * in_elems * esize(xs[0].dtype), 2 if xs[1] is not None else 1)
    print(f"{cid}: batch {batch}, {need / 2 ** 30:.2f} GiB of device memory (workspace {plan.workspace_bytes / 2 ** 20:.1f} MiB)")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    bounds = boundaries(batch, in_elems, esize(xs[0].dtype), e, esize(plan.out_dtype()))
    try:
        x0 = tiled(xs[0], batch, dev)
        x1 = None if xs[1] is None else tiled(xs[1], batch, dev)
        out, iso, bands = run_banded(plan, x0, x1)
        del x0, x1
        ex = (tag in EXACT) if exact is None else exact
        if out is not None:
            check(out, ref, bnd, bounds, accurate, exact=ex, bands=bands, what=cid)
        if iso is not None:
            check(iso, iref.reshape(PERIOD, -1), bnd, {}, accurate, exact=ex, bands=bands, what=cid + " radial sums")
        return plan, bounds
    finally:
        out = iso = bands = None
        release(dev)


# ---------------------------------------------------------------------------------- the averaged forms
def run_mean(cid, ny, nx, m, batch, env, kind, dev, coherence=False):
    """mean_batch = m over `batch` slabs of a PERIOD of 48 (48 / m distinct outputs): batch_mean's reference and bound (coherence's for the coherence)."""
    assert batch % PERIOD == 0 and PERIOD % m == 0
    case = (ny, nx, batch, m, 0)
    pcase = (ny, nx, PERIOD, m, 0)
    po = PERIOD // m
    v = period_field((ny, nx), (0, 1), False, seed=9)
    x0, x064 = A.tensor(v, A.F32)
    form = "linear-hann-shift"
    if coherence:
        x1, x164 = A.tensor(second_period(v, seed=10) + 0.5 * np.random.default_rng(11).standard_normal(v.shape), A.F32)
        cs, _ = B.reference(pcase, form, x064, x164, CO.LAG)
        p0, _ = B.reference(pcase, form, x064)
        p1, _ = B.reference(pcase, form, x164)
        ref = np.abs(cs) ** 2 / (p0 * p1)
        kaps = [max(a, c) for a, c in zip(B.kappa(pcase, form, x064), B.kappa(pcase, form, x164))]
        bnd = [CO.bound(ny, nx, k) for k in kaps]
        accurate = absolute_accurate(bnd)
        with library_env(env):
            plan = CO.make_plan(case, form)
        assert CO.is_coherence_plan(plan), plan.describe()
    else:
        x1 = None
        ref, _ = B.reference(pcase, form, x064)
        bnd = [B.bound(ny, nx, k) for k in B.kappa(pcase, form, x064)]
        accurate = mean_accurate(bnd)
        with library_env(env):
            plan = B.make_plan(case, form)
    assert plan.kernel_info()[0] == kind and "[mean over the batch]" in plan.describe(), plan.describe()
    n, e = out_shape(plan)
    assert n == batch // m
    need = device_bytes(plan, batch * ny * nx * 4, 2 if coherence else 1)
    print(f"{cid}: batch {batch}, {n} outputs, {need / 2 ** 30:.2f} GiB of device memory (workspace {plan.workspace_bytes / 2 ** 20:.1f} MiB)")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    bounds = boundaries(n, m * ny * nx, 4, e, 4, period=po)
    try:
        t0 = tiled(x0, batch, dev)
        t1 = None if x1 is None else tiled(x1, batch, dev)
        out, _, bands = run_banded(plan, t0, t1)
        del t0, t1
        check(out, ref.reshape(po, -1), bnd, bounds, accurate, bands=bands, period=po, what=cid, absolute=coherence)
        return plan, bounds
    finally:
        out = bands = None
        release(dev)


def run_welch_rows(cid, l, h, m, p, dev):
    """Welch rows: p dense series of a PERIOD of 48, welch.reference and welch.bound."""
    assert p % PERIOD == 0
    form = "linear-hann-shift"
    pcase = (l, h, m, PERIOD, 0, None)
    sp = W.span(pcase)
    v = period_field((sp,), (0,), False, seed=13)
    x0, x064 = A.tensor(v, A.F32)
    ref, _ = W.reference(pcase, form, x064)
    bnd = [W.bound(l, k) for k in W.kappa(pcase, form, x064)]
    plan = W.make_plan((l, h, m, p, 0, None), form)
    assert plan.kernel_info()[0] == L.K_FASTW and "[fastw]" in plan.describe() and "[fastw columns]" not in plan.describe(), plan.describe()
    need = device_bytes(plan, p * sp * 4)
    print(f"{cid}: {p} series of {sp} samples, {need / 2 ** 30:.2f} GiB of device memory (workspace {plan.workspace_bytes / 2 ** 20:.1f} MiB)")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    bounds = boundaries(p, sp, 4, l, 4)
    try:
        t0 = tiled(x0, p, dev)
        out, _, bands = run_banded(plan, t0)
        del t0
        check(out, ref, bnd, bounds, mean_accurate(bnd), bands=bands, what=cid)
        return plan, bounds
    finally:
        out = bands = None
        release(dev)


def run_welch_cols(cid, l, h, m, blocks, inner, dev):
    """Welch columns: `blocks` dense blocks of `inner` adjacent columns (seg_stride = inner) of a PERIOD of 48 columns; block b carries a further factor 2^b, which
    scales its spectra by 4^b exactly and is taken out again before the check: a segment read from the wrong block misses the bound."""
    assert inner % PERIOD == 0
    form = "linear-hann-shift"
    pcase = (l, h, m, PERIOD, 0, None)
    sp = W.span(pcase)
    v = period_field((sp,), (0,), False, seed=14)          # [48][span]: the columns as series
    x0, x064 = A.tensor(v, A.F32)
    ref, _ = W.reference(pcase, form, x064)
    bnd = [W.bound(l, k) for k in W.kappa(pcase, form, x064)]
    c = (l, h, m, blocks, inner, inner, 0, None, 0)
    plan = WC.make_plan(c, form)
    assert plan.kernel_info()[0] == L.K_FASTW and "[fastw columns]" in plan.describe(), plan.describe()
    need = device_bytes(plan, blocks * sp * inner * 4)
    print(f"{cid}: {blocks} blocks of {inner} columns, {need / 2 ** 30:.2f} GiB of device memory (workspace {plan.workspace_bytes / 2 ** 20:.1f} MiB)")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    bounds = boundaries(blocks * inner, 1, 4, l, 4)  # (a column's first sample: one element further per column)
    try:
        cols = x0.to(dev).t().contiguous()                                                   # [span][48]
        t0 = cols.repeat(1, inner // PERIOD).unsqueeze(0).repeat(blocks, 1, 1)               # [blocks][span][inner]
        t0 = (t0 * (2.0 ** torch.arange(blocks, device=dev, dtype=torch.float32)).reshape(-1, 1, 1)).contiguous()
        assert plan._layout_ok(t0)
        out, _, bands = run_banded(plan, t0)
        del t0
        scaled = out.reshape(blocks, inner * l) * (0.25 ** torch.arange(blocks, device=dev, dtype=torch.float32)).reshape(-1, 1)  # (a power of two: exact)
        check(scaled.reshape(blocks * inner, l), ref, bnd, bounds, mean_accurate(bnd), bands=bands, what=cid)
        return plan, bounds
    finally:
        out = scaled = bands = None
        release(dev)


# ---------------------------------------------------------------------------------- rung C: offsets through the descriptor's strides
HUGE_STRIDE = (1 << 30) + 16  # elements between the slabs: slab 2 starts beyond element 2^31 (float32: byte 2^33)
# one row of strided.FAMILIES each, float32 (a float64 row needs 17 GB for the same element offsets and crosses no further boundary)
RUNG_C_BATCH_STRIDE = {"FastY": "fasty-small", "FastM": "fastm-small-f32", "FastN": "fastn-small-f32", "FastS": "fasts", "FastG": "fastg-f32", "FastG-rows": "fastg-rows-f32",
                       "FastR": "fastr-4096"}
RUNG_C_PITCH = {"FastS": "fasts", "FastG": "fastg-f32", "FastM": "fastm-small-f32", "FastN": "fastn-small-f32", "FastY": "fasty-small"}


ROWS_BATCH = 300  # FastG rows: more rows than one workgroup takes


def largest_rows_stride(rid, batch, esz=4):
    """FastG rows address the rows of ONE workgroup with 32-bit offsets from its first row: (rows per workgroup) x in_stride_batch <= 2^31 - 1 elements, or the
    caller copies.  The largest stride (a multiple of 16 bytes) the plan accepts at `batch` rows: 2^30 + 16 is refused, and the offsets pass 2^31 between workgroups."""
    kw, _, _ = S.table_row(rid)
    rows = A.make(**dict(kw, batch=batch)).kernel_info()[1]
    return ((1 << 31) - 1) // rows // (16 // esz) * (16 // esz)


def largest_pitch(ny, esz):
    """The largest in_stride_y (elements, a multiple of 16 bytes) whose slab ny * pitch * esz stays within 2^32 - 1 bytes."""
    return ((1 << 32) - 1) // ny // 16 * 16 // esz


def run_strided(cid, rid, batch, pitch, slab, dev, beyond=0):
    """A (batch, ny, nx) box with rows `pitch` and slabs `slab` elements apart (0: dense rows) inside a buffer that is allocated and never filled: only the box is
    written.  The strided plan is bit-identical to the dense plan on view.contiguous() (the property of tests/strided.py), the dense result within the bound."""
    kw, kind, tag = S.table_row(rid)
    kw.pop("iso", None)
    dt = kw.get("dtype", A.F32)
    ndim, nx = kw.get("ndim", 2), kw["nx"]
    ny = kw["ny"] if ndim == 2 else 1
    py = pitch or nx
    rkw = dict(kw, batch=batch)
    shape, axes, _ = A._axes(rkw)
    v = period_field(shape[1:], [a - 1 for a in axes], False, seed=15, period=batch)
    x, x64 = A.tensor(v, dt)
    dense = A.make(**rkw)
    plan = A.make(**rkw, in_stride_y=pitch, in_stride_batch=slab)
    assert A.family(dense) == A.family(plan) == (kind, tag), (A.family(plan), kind, tag)
    assert f"in pitch {py} / slab {slab}" in plan.describe(), plan.describe()
    total = (batch - 1) * slab + (ny - 1) * py + nx
    assert (batch - 1) * slab >= beyond, (batch, slab, beyond)  # (the last slab starts at or beyond this element offset)
    need = total * esize(dt) + 3 * batch * ny * nx * 16 + plan.workspace_bytes + (1 << 30)
    print(f"{cid}: pitch {py}, slab stride {slab}: the last sample at element {total - 1} (byte {(total - 1) * esize(dt)}), {need / 2 ** 30:.2f} GiB of device memory")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    try:
        buf = torch.empty(total, dtype=dt, device=dev)
        view = torch.as_strided(buf, (batch, ny, nx), (slab, py, 1))
        view.copy_(x.reshape(batch, ny, nx).to(dev))
        arg = torch.as_strided(buf, (batch, nx), (slab, 1)) if ndim == 1 else view
        out_s, _ = plan.execute(arg)
        out_d, _ = dense.execute(arg.contiguous())
        assert S.finite(out_s) and torch.equal(out_s, out_d), f"{cid}: the strided plan differs from the dense plan on the contiguous copy"
        det = kw.get("detrend", L.DETREND_NONE)
        kap = A.kappa(x64.reshape(shape), A.detrended(x64.reshape(shape), axes, det)) if det else 0.0
        ref, _ = A.reference(rkw, x64)
        got = out_d.cpu().numpy().reshape(ref.shape)
        for j in range(batch):
            A.assert_accurate(got[j], ref[j], dt, A.points(rkw), kap, what=f"{cid} slab {j}")
        return plan
    finally:
        buf = view = arg = out_s = out_d = None
        release(dev)


def run_welch_rows_pitched(cid, dev, pitch=(1 << 30) + 5, case=(64, 32, 3, 3, 0, None)):
    """Welch rows whose series start `pitch` samples apart (odd: 4-byte boundaries only) in a buffer that is never filled: against welch.reference, and the bits of
    the dense plan."""
    form = "linear-hann-shift"
    l, h, m, p = case[:4]
    sp = W.span(case)
    x = W.series(case)
    plan = W.make_plan(case, form, pitch=pitch)
    total = (p - 1) * pitch + sp
    need = total * 4 + plan.workspace_bytes + (1 << 30)
    print(f"{cid}: series pitch {pitch}: the last sample at element {total - 1}, {need / 2 ** 30:.2f} GiB of device memory")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    try:
        buf = torch.empty(total, dtype=torch.float32, device=dev)
        view = torch.as_strided(buf, (p, sp), (pitch, 1))
        view.copy_(torch.from_numpy(x).to(dev))
        out, _ = plan.execute(view)
        got = out.cpu().numpy().reshape(p, -1)
        ref, _ = W.reference(case, form, x)
        W.assert_outputs(case, got, ref, None, W.kappa(case, form, x), cid)
        assert np.array_equal(got, W.run(W.make_plan(case, form), x)), f"{cid}: the pitched plan differs from the dense plan"
        return plan
    finally:
        buf = view = out = None
        release(dev)


def run_welch_cols_strided(cid, dev, s=1 << 20, c=(64, 32, 69, 2, 40), beyond=1 << 31):
    """Welch columns whose samples lie `s` elements apart: sample (seg H + j) of column e at ((seg H + j) s + e), past 2^31 elements inside ONE block; the second
    block a dense pitch (span x s) further.  Against welch's reference, and the bits of the plan on the arranged (dense) copy."""
    form = "linear-hann-shift"
    l, h, m, p, inner = c
    case = (l, h, m, p, inner, s, 0, None, 0)
    sp = WC.span(case)
    pitch = sp * s
    assert (sp - 1) * s + inner > beyond
    x = WC.cube(case)
    plan = WC.make_plan(case, form, in_stride_batch=pitch)
    WC.assert_column_plan(plan, case)
    total = (p - 1) * pitch + (sp - 1) * s + inner
    need = total * 4 + plan.workspace_bytes + (1 << 30)
    print(f"{cid}: sample stride {s}, block pitch {pitch}: the last sample at element {total - 1}, {need / 2 ** 30:.2f} GiB of device memory")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    try:
        buf = torch.empty(total, dtype=torch.float32, device=dev)
        view = torch.as_strided(buf, (p, sp, inner), (pitch, s, 1))
        view.copy_(torch.from_numpy(x).to(dev))
        out, _ = plan.execute(view)
        got = out.cpu().numpy().reshape(p * inner, -1)
        rc = WC.rows_case(case)
        rows = WC.as_rows(x)
        ref, _ = W.reference(rc, form, rows)
        W.assert_outputs(rc, got, ref, None, W.kappa(rc, form, rows), cid)
        dense = case[:5] + (inner, 0, None, 0)
        assert np.array_equal(got, WC.run(WC.make_plan(dense, form), dense, x)), f"{cid}: the strided plan differs from the plan on the arranged copy"
        return plan
    finally:
        buf = view = out = None
        release(dev)


# ---------------------------------------------------------------------------------- rung D: the guards (plan creation only)
def status(**kw):
    """The status of xrfthip_plan_create for make() arguments (0: the plan exists)."""
    try:
        A.make(**kw)
    except L.XrftHipError as e:
        return e.status
    return 0


WELCH_OUTPUTS = ((1 << 31) - 1) // 1024  # a Welch plan's outputs (series, or columns of every block): one launch of outputs x runs workgroups
WELCH_KW = dict(ndim=1, nx=64, dtype=A.F32, out_mode=L.OUT_POWER, mean_batch=3, seg_hop=32, batch=3)


def check_guards():
    """The status at the limit and one step past it, for each host guard that the kernels' 32-bit arithmetic rests on.  Already pinned elsewhere and not repeated:
    ny * in_stride_y beyond 2^31 - 1 elements (test_strided_emulated.py::test_refused_descriptors), herm lengths that no kernel takes
    (test_three_axes_emulated.py), inner beyond 2^30 of the stand-alone detrend (test_emulated_api.py)."""
    bad, unsup = L.BAD_ARG, L.UNSUPPORTED_LENGTH
    # nx * ny <= 2^31 - 1 (a prime: no slab has exactly that many points; the largest products of two lengths on either side of it)
    assert status(ny=32768, nx=65535, batch=1) == 0 and status(ny=32768, nx=65536, batch=1) == bad
    assert status(ny=46340, nx=46341, batch=1) == 0 and status(ny=46341, nx=46341, batch=1) == bad
    assert status(ndim=1, nx=1 << 30, batch=1) != bad and status(ndim=1, nx=(1 << 30) + 1, batch=1) == bad
    # the strided slab: ny * pitch * esz <= 2^32 - 1 bytes, one 16-byte step more is "the caller copies"
    for rid, dt in (("fasts", A.F32), ("fastg-f32", A.F32), ("fastm-small-f32", A.F32), ("fastn-small-f32", A.F32), ("fasty-small", A.F32), ("fastg", A.F64), ("fastn-small", A.F64)):
        kw, kind, tag = S.table_row(rid)
        assert kw.get("dtype", A.F32) == dt
        esz = esize(dt)
        p = largest_pitch(kw["ny"], esz)
        assert kw["ny"] * p * esz <= (1 << 32) - 1 < kw["ny"] * (p + 16 // esz) * esz
        kw = dict(kw, batch=2)
        assert status(**kw, in_stride_y=p, in_stride_batch=kw["ny"] * p) == 0, rid
        assert status(**kw, in_stride_y=p + 16 // esz, in_stride_batch=kw["ny"] * (p + 16 // esz)) == unsup, rid
    # (complex input reads no strides -- test_strided_emulated.py --, 2-byte input is read dense: refused on either side of the limit, never routed to 32-bit offsets)
    for dt in (A.C64, A.C128):
        esz = esize(dt)
        p = largest_pitch(64, esz)
        for q in (p, p + 16 // esz):
            assert status(ny=64, nx=128, dtype=dt, out_mode=L.OUT_COMPLEX, batch=2, in_stride_y=q, in_stride_batch=64 * q) == unsup, (dt, q)
    for dt in (torch.float16, torch.bfloat16):
        for q in (largest_pitch(64, 4), largest_pitch(64, 2), largest_pitch(64, 2) + 8):
            assert status(ny=64, nx=128, dtype=dt, batch=2, in_stride_y=q, in_stride_batch=64 * q) == unsup, (dt, q)
    # FastG rows: the rows of one workgroup times the stride between them within 2^31 - 1 elements
    st = largest_rows_stride("fastg-rows-f32", ROWS_BATCH)
    rk = dict(S.table_row("fastg-rows-f32")[0], batch=ROWS_BATCH)
    assert status(**rk, in_stride_batch=st) == 0 and status(**rk, in_stride_batch=st + 4) == unsup and status(**rk, in_stride_batch=HUGE_STRIDE) == unsup
    # Welch plans: seg_stride, inner, span and mean_batch at 2^31 - 1 against 2^31; (2^31 - 1) / 1024 outputs in one launch
    big = (1 << 31) - 1
    assert status(**dict(WELCH_KW, batch=3 * WELCH_OUTPUTS)) == 0 and status(**dict(WELCH_KW, batch=3 * (WELCH_OUTPUTS + 1))) == unsup
    wk = dict(WELCH_KW)
    assert status(**wk, inner=4, seg_stride=big) == 0 and status(**wk, inner=4, seg_stride=big + 1) == bad
    # (inner: NOT pinned by itself -- a descriptor needs seg_stride >= inner, so one step past the limit of inner is refused by the guard of seg_stride above as well)
    assert status(**wk, inner=big, seg_stride=big) == unsup and status(**dict(wk, inner=big + 1, seg_stride=big + 1)) == bad  # (that many columns: no kernel, but no bad descriptor)
    m = (big - 64) // 32 + 1  # (M - 1) 32 + 64 <= 2^31 - 1
    assert (m - 1) * 32 + 64 <= big < m * 32 + 64
    assert status(**dict(wk, mean_batch=m, batch=m), inner=4, seg_stride=4) == 0 and status(**dict(wk, mean_batch=m + 1, batch=m + 1), inner=4, seg_stride=4) == bad
    assert status(**dict(wk, mean_batch=big, batch=big, seg_hop=1)) == 0 and status(**dict(wk, mean_batch=big + 1, batch=big + 1, seg_hop=1)) == bad
    # a mean plan: (batch / M) x ny output rows within 2^31 - 1 (one workgroup of mean_finish_kernel each), refused when the plan is created -- "the caller composes"
    # (2^31 - 1 is prime: the largest output counts on either side of it, for the FastY form and, with XRFTHIP_MEAN_ALL, the FastS form)
    for ny, nx, env in ((256, 256, {}), (256, 512, {}), (128, 128, {}), (64, 64, {"XRFTHIP_MEAN_ALL": "1"})):
        nout = big // ny
        assert nout * ny <= big < (nout + 1) * ny
        with library_env(env):
            for mode in (L.OUT_POWER, L.OUT_CROSS) if ny == 256 else (L.OUT_POWER,):
                mk = dict(ny=ny, nx=nx, out_mode=mode, mean_batch=2)
                assert status(**mk, batch=2 * nout) == 0, (ny, nx, mode)
                assert status(**mk, batch=2 * (nout + 1)) == unsup, (ny, nx, mode)
    with library_env({}):
        assert status(ny=256, nx=256, out_mode=L.OUT_COHERENCE, mean_batch=2, batch=2 * (big // 256)) == 0
        assert status(ny=256, nx=256, out_mode=L.OUT_COHERENCE, mean_batch=2, batch=2 * (big // 256 + 1)) == unsup
    # herm_ny / herm_nx <= 2^30
    hk = dict(dtype=A.C64, out_mode=L.OUT_POWER, flags=L.AXIS_Y, batch=1)
    assert status(**hk, ny=2, nx=(1 << 29) + 1, herm_ny=1, herm_nx=1 << 30) == 0 and status(**hk, ny=2, nx=(1 << 29) + 1, herm_ny=1, herm_nx=(1 << 30) + 1) == bad
    # (herm_ny: NOT pinned by itself -- nx = herm_ny (herm_nx / 2 + 1) >= herm_ny, so one step past it the guard of nx refuses first; herm_nx is pinned above)
    assert status(**hk, ny=1, nx=1 << 30, herm_ny=1 << 30, herm_nx=1) != bad and status(**hk, ny=1, nx=(1 << 30) + 1, herm_ny=(1 << 30) + 1, herm_nx=1) == bad


def group_of(plan):
    return int(plan.describe().split("group=")[1].split()[0])


def check_iso_group_limit():
    """slabs_per_group above 65 535 on an ISO FastY / FastM plan: iso_reduce_kernel takes the group's slabs on grid.y, so the host runs such a group as several
    (the group is held to 65 535 slabs when the plan is laid out); without radial sums the group is the caller's."""
    bm, nb = A.radial_map(256, 512)
    p = A.make(ny=256, nx=512, batch=COUNT, flags=L.ISO, binmap=bm, nbins=nb, slabs_per_group=COUNT)
    assert A.family(p) == (L.K_FASTY, "fasty") and group_of(p) == 65535, p.describe()
    assert group_of(A.make(ny=256, nx=512, batch=COUNT, flags=L.ISO, binmap=bm, nbins=nb, slabs_per_group=65535)) == 65535
    assert group_of(A.make(ny=256, nx=512, batch=COUNT, flags=L.ISO, binmap=bm, nbins=nb, slabs_per_group=4096)) == 4096
    assert group_of(A.make(ny=256, nx=512, batch=COUNT, slabs_per_group=COUNT)) == COUNT
    bm, nb = A.radial_map(180, 360)
    p = A.make(ny=180, nx=360, batch=COUNT, dtype=A.F64, flags=L.ISO, binmap=bm, nbins=nb, slabs_per_group=COUNT)
    assert A.family(p) == (L.K_FASTM, "fastm") and group_of(p) == 65535, p.describe()


def run_iso_in_groups(dev, batch=2 * PERIOD, spg=PERIOD + 5):
    """The radial sums of a FastY and a FastM plan whose batch runs as several groups (the path a group above 65 535 slabs now takes), the last one short."""
    for cid, kw, kind, tag in (("fasty-iso-groups", dict(ny=256, nx=512, flags=L.ISO, iso=True, slabs_per_group=spg), L.K_FASTY, "fasty"),
                               ("fastm-iso-groups", dict(ny=180, nx=360, dtype=A.F64, flags=L.ISO, iso=True, slabs_per_group=spg), L.K_FASTM, "fastm")):
        plan, _ = run_plain(cid, kw, {}, kind, tag, batch, dev)
        assert group_of(plan) == spg


def teardown(dev):
    """The plan cache and the engine's grow-only scratch: the rest of the suite sees the memory it saw before."""
    api.clear_plan_cache()
    engine.clear_workspaces()
    release(dev)
