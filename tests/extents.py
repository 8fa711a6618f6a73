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
from one device buffer, 1 MiB of 0xA5 in front of and behind each, the workspace exactly xrfthip_workspace_bytes, the output 0xFF (NaN) before the call.

The segment kernels (spectrogram fastk.h, istft fasto.h, fir_filter fastf.h: the three non-Welch forms of Family::FastK) have cases of their own on every rung,
because their offsets grow INSIDE a series: (s0 + sl) hop + j, s0 (n + 1), first / idx < N / o0, obase + r.  Beside the batch-direction cases (48 series or columns,
tiled) the period lies ALONG one series (run_along, check(along=Along(...))): a pattern of 48 H (48 V) samples, or 48 half spectra, repeated; N a whole number of
periods.  The reference is spectrogram.reference / istft.model / fir_filter.model on a SHORT series of four periods, whose first, second and last periods are exactly
the first, every interior and the last period of the long one, and whose K - 1 / L - H samples behind the last whole period are its tail.  The first and last periods
(the zeros outside a filtered series, the segments an overlap-add lacks at its ends) are held to float64 only, every interior period to the bits of the first interior
one (SEGMENT_EXACT).  Rung A: 70 080 series or columns, several workgroups each, the last one short.  Rung B: one series of 2^26 segments per kernel (sample offsets
beyond 2^31 inside the series: 17 to 26 GiB), dense batches of short series, and the column layout's output beyond 2^31 elements inside one block.  Rung C: a series
pitch of 2^30 + 5, a sample stride of 2^20.  Rung D: check_segment_guards().
Not covered: API-level calls at these sizes (xrft_amd.istft on a span past 2^31 - 1, where the fused plan declines and the composed route runs), 2^32 complex
elements of istft input, L = 4096 variants of the one-series cases (the same code path with other constants)."""
import contextlib
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

from xrft_amd import _lib as L
from xrft_amd import api, engine

import accuracy as A
import batch_mean as B
import coherence as CO
import decorations as D
import fir_filter as FF
import istft as IS
import spectrogram as SP
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


MORE_LIMITS = LIMITS + (("2^34 bytes", 1 << 34, True),)  # (the synthesis reads 8-byte elements: 2^31 of them)


def boundaries(n, in_elems, in_esz, out_elems, out_esz, period=PERIOD, limits=LIMITS):
    """{name: the first of `n` slabs whose input / output element offset is at or above 2^31, whose byte offset is at or above 2^32 / 2^33} -- those the case reaches.
    in_elems / out_elems: elements per slab (per output of the period's index); a wrap distance that is a whole number of slabs is no multiple of the period."""
    out = {}
    for side, per, esz in (("input", in_elems, in_esz), ("output", out_elems, out_esz)):
        if not per:
            continue
        for wrap, step in ((1 << 31, per), (1 << 32, per), (1 << 32, per * esz), (1 << 33, per * esz)) + (((1 << 34, per * esz),) if limits is MORE_LIMITS else ()):
            assert wrap % step != 0 or (wrap // step) % period != 0, (side, wrap, step)  # 2^31, 2^32 elements; 2^32, 2^33 (2^34) bytes
        for name, lim, in_bytes in limits:
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


class Along:
    """The period lies ALONG a series (the segment kernels): the slabs are the series' segments (blocks of kept samples), and its two ends are not copies of its
    middle -- the zeros outside a filtered series, the segments an overlap-add lacks at its ends.
    member: the period of `out` every interior period is compared with, and the period of `ref` it is checked against (the first interior one);
    edges: {period of out: period of ref} -- held to float64 only, each a window; ref: [periods of the SHORT series x period, ...], computed on four periods;
    tail: (got, check(got, what)) -- the K - 1 / L - H samples behind the last whole period, held to float64 and finite;
    whole: accurate(got [period, e], ref [period, e], period of ref, what) takes a whole period (a norm-wise bound over its 48 segments), bnd is then one ABSOLUTE
    bound per period of ref and the all-period form || out[q] - out[member] ||_2 <= 2 bnd[member]."""

    def __init__(self, member=1, edges=None, tail=None, whole=False):
        self.member, self.edges, self.tail, self.whole = member, dict(edges or {}), tail, whole


def _check_along(out, ref, bnd, bounds, accurate, exact, bands, period, what, chunk_bytes, along):
    n = out.shape[0]
    nq = n // period
    mb = along.member
    assert n % period == 0 and ref.shape[0] % period == 0 and 0 <= mb < min(nq, ref.shape[0] // period) and mb not in along.edges, (n, period, ref.shape, mb)
    assert all(0 <= q < nq and 0 <= rp < ref.shape[0] // period for q, rp in along.edges.items()), (along.edges, nq)
    o2 = _real2d(out)
    # 2. windows against the float64 reference: the edges, the first and the last period, every one that holds a boundary
    wins = {0: "first", nq - 1: "last"}
    for name, k in bounds.items():
        assert 0 <= k < n, (name, k, n)
        wins.setdefault(k // period, name)
    for q in along.edges:
        wins.setdefault(q, "edge")
    for q, name in sorted(wins.items()):
        rp = along.edges.get(q, mb)
        host = out[q * period:(q + 1) * period].cpu().numpy()
        if along.whole:
            accurate(host, ref[rp * period:(rp + 1) * period], rp, f"{what} period {q} ({name})")
        else:
            for j in range(period):
                accurate(host[j], ref[rp * period + j], rp * period + j, f"{what} slab {q * period + j} (period {q}: {name})")
    if along.tail is not None:
        got, tail_ok = along.tail
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), f"{what}: the tail behind the last whole period holds a value that is not finite"
        tail_ok(got, f"{what} tail")
    # 3. every interior period against the member period, on the device
    base = o2[mb * period:(mb + 1) * period]
    assert bool(torch.isfinite(base).all()), f"{what}: a value of the member period is not finite"
    if along.whole:
        lim = torch.full((1, 1), (2.0 * float(np.asarray(bnd, dtype=np.float64).reshape(-1)[mb])) ** 2, dtype=torch.float64, device=out.device)
    else:
        b2 = torch.as_tensor(np.broadcast_to(np.asarray(bnd, dtype=np.float64), (ref.shape[0],))[mb * period:(mb + 1) * period].copy(), device=out.device)
        lim = ((2.0 * b2) ** 2 * base.double().pow(2).sum(1)).reshape(1, period)
    interior = torch.ones(nq, dtype=torch.bool, device=out.device)
    for q in along.edges:
        interior[q] = False
    per_chunk = max(1, chunk_bytes // max(1, period * o2.shape[1] * o2.element_size()))
    same = True
    for q0 in range(0, nq, per_chunk):
        q1 = min(nq, q0 + per_chunk)
        c = o2[q0 * period:q1 * period].reshape(q1 - q0, period, -1)
        fin = torch.isfinite(c).all(2)
        if not bool(fin.all()):
            q, j = [int(v[0]) for v in torch.nonzero(~fin, as_tuple=True)]
            raise AssertionError(f"{what}: slab {(q0 + q) * period + j} holds a value that is not finite")
        ins = interior[q0:q1].reshape(-1, 1)
        d = (c - base).double().pow(2).sum(2)
        if along.whole:
            d = d.sum(1, keepdim=True)
        bad = (d > lim) & ins
        if bool(bad.any()):
            q, j = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
            unit = f"period {q0 + q}" if along.whole else f"slab {(q0 + q) * period + j}"
            raise AssertionError(f"{what}: {unit} is {float(d[q, j]) ** 0.5:.3e} from its member of period {mb}, more than {float(lim.reshape(-1)[j if not along.whole else 0]) ** 0.5:.3e}")
        same = same and bool(((c == base).all(2) | ~ins).all())
    print(f"{what}: {n} slabs along the series, windows {sorted(set(wins.values()))}, bit-identical across the batch: {same}")
    if exact:
        assert same, f"{what}: an interior period differs in its bits from period {mb}"
    for i, band in enumerate(bands):
        assert bool((band == PATTERN).all()), f"{what}: guard band {i} was written"
    return same


def check(out, ref, bnd, bounds, accurate, exact=False, bands=(), period=PERIOD, what="", chunk_bytes=256 << 20, absolute=False, along=None):
    """out: [n, ...] tensor on any device, n a multiple of `period`; ref: [period, ...] float64 / complex128; bnd: the bound (a number, or one per member of the
    period); bounds: {name: slab index} from boundaries(); accurate(got, ref_j, j, what): the window check; bands: uint8 tensors that must still hold PATTERN.
    absolute: the all-slab form is || out[k] - out[k % period] || <= 2 bound sqrt(elements) (a coherence).  along: an Along -- the period lies along a series, whose
    first and last periods are edges (class Along); left out, nothing changes.  Returns whether every slab equalled its member bit for bit."""
    if along is not None:
        assert not absolute
        return _check_along(out, ref, bnd, bounds, accurate, exact, bands, period, what, chunk_bytes, along)
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
    if getattr(plan, "seg_synth", 0):  # (the series)
        return plan.batch_out, (plan.mean_batch - 1) * plan.seg_hop + plan.nx
    if getattr(plan, "seg_filter", 0):  # (the filtered series)
        return plan.batch_out, plan.seg_out_len
    if getattr(plan, "seg_keep", 0):  # (every segment's spectrum; the column layout: [block][segment][frequency][column])
        return plan.batch_out, plan.mean_batch * plan.nx_out * (plan.inner if plan.seg_stride > 1 else 1)
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


# ---------------------------------------------------------------------------------- the segment kernels: spectrogram, istft, fir_filter
# The three non-Welch forms of Family::FastK (fastk.h, fasto.h, fastf.h; launched from host_welch.inc).  Their workload is ONE very long series, so their offsets grow
# inside a series: the period of 48 lies ALONG it (run_along) -- a pattern of 48 H (48 V) samples, 48 half spectra, repeated -- as well as across the batch
# (run_batch, run_keep_cols: 48 series or columns, tiled, the scheme of the Welch runners above).
# Reference: spectrogram.reference, istft.model, fir_filter.model (scipy's direct float64 convolution) on a SHORT series of four periods: with N a whole number of
# periods, its first, second and last periods are exactly the first, every interior and the last period of the long series, and the K - 1 / L - H samples behind
# its last whole period are the long series' tail.  Bound: what those files' check_plan functions apply -- accuracy.bound per segment; istft.the_bound and
# fir_filter.the_bound with A over ONE period's 48 segments (the batch runners: over one series' segments).  No tolerance of the ladder's own.
#
# All three are held to bit identity, across the batch and along the series (an interior period has the bits of the first interior period), from the code:
SEGMENT_EXACT = {
    "spectrogram": "fastk.h:44-50: a workgroup is one round of ONE series (one group of columns); :61-75 every output element from its own segment's sequence, a "
                   "segment packed with itself, computed and stored by one thread; seg_tile.h:86-110 the detrend's sums per segment over a fixed tree",
    "istft": "fasto.h:42-48: a workgroup is NS consecutive segments of ONE series; :79-91 every sample gathered by one thread over its own covering segments in "
             "ascending order, the place in the tile (m, sl) enters the addresses only",
    "fir_filter": "fastf.h:45-59: a workgroup is NS consecutive segments of ONE series, each packed with itself, the guard idx < N per sample; :104-112 every kept "
                  "sample written once from its own segment",
}
FORM = "linear-hann-shift"


class Worst:
    """The largest figure / bound a case met (printed once per case, before the checker's verdict on the bits)."""

    def __init__(self):
        self.ratio = 0.0

    def within(self, fig, bnd, what):
        fig = np.asarray(fig, dtype=np.float64)
        ok = np.isfinite(fig).all() and bool((fig <= bnd).all())
        with np.errstate(divide="ignore", invalid="ignore"):
            self.ratio = max(self.ratio, float(np.max(np.where(np.asarray(bnd) > 0, fig / bnd, np.where(fig > 0, np.inf, 0.0)))))
        assert ok, f"{what}: {float(np.max(fig)):.3e} against the bound {float(np.max(bnd)):.3e}"


def _rows_rms(got, ref):
    """accuracy.errors' first figure, || got - ref ||_2 / || ref ||_2, for every row at once."""
    wide = np.complex128 if np.iscomplexobj(ref) else np.float64
    d = np.abs(np.asarray(got).astype(wide) - ref) ** 2
    return np.sqrt(d.mean(-1) / (np.abs(ref) ** 2).mean(-1))


def _keep_dt(mode):
    return "float32" if mode == L.OUT_POWER else "complex64"


def _amp(v):
    return float(np.sqrt(np.sum(np.abs(v) ** 2)))


def _rows_plan(l, h, m, p, mode):
    plan = SP.make_plan((l, h, m, p), FORM, mode)
    SP.assert_keep_plan(plan)
    assert "[fastw columns]" not in plan.describe(), plan.describe()
    return plan


# ---- the period along the series: .plan(q) for q periods, .pattern (one period of input elements), elements per member in and out, the tails, .reference(qs)
def keep_along(l, h, mode=L.OUT_POWER):
    """A spectrogram of ONE series: a pattern of 48 H samples (stretch j of H samples scaled by 1 + j / 48) repeated, L - H samples more; slab = a segment's spectrum."""
    x, x64 = A.tensor(period_field((h,), (0,), False, seed=31), A.F32)
    dt = _keep_dt(mode)

    def reference(qs):
        xs = np.concatenate([np.tile(x64.reshape(-1), qs), x64.reshape(-1)[:l - h]])[None]
        case = (l, h, qs * PERIOD, 1)
        ref, kaps = SP.reference(case, FORM, xs, mode)[0], SP.kappas(case, FORM, xs)[0]
        bnd = np.array([A.bound(dt, l, k) for k in kaps])
        worst = Worst()

        def accurate(got, r, j, what):
            worst.within(A.errors(got.reshape(r.shape), r)[0], bnd[j], what)
        return SimpleNamespace(ref=ref, bnd=bnd, accurate=accurate, tail=None, whole=False, worst=worst)

    return SimpleNamespace(plan=lambda q: _rows_plan(l, h, q * PERIOD, 1, mode), reference=reference, pattern=x.reshape(-1), in_step=h, in_tail=l - h, out_step=l,
                           out_periods=lambda q: q, out_tail=0, limits=LIMITS)


def synth_spectra(l, h, m, p, wname):
    """[p][m][L / 2 + 1] complex64 and its complex128 image: istft.spectra (the stft of spectrogram.series), segment j (p = 1) or series j further scaled by 1 + j / 48."""
    z = IS.spectra((l, h, m, p), wname).astype(np.complex128)
    z *= (1.0 + np.arange(PERIOD) / PERIOD).reshape((1, -1, 1) if p == 1 else (-1, 1, 1))
    return A.tensor(z, torch.complex64)


def _synth_plan(l, h, m, p, wname):
    plan = IS.make_plan((l, h, m, p), wname)
    IS.assert_synth_plan(plan)
    return plan


def synth_along(l, h, wname="hann"):
    """An istft of ONE series: 48 distinct half spectra, repeated; slab = H samples, the L - H samples behind the last segment's start + H the tail.  The samples of
    a period are those of its 48 segments' hops: A over 48 segments bounds the first period (segments 0 .. 47 alone cover it) and an interior or last one (it holds
    the tails of the R - 1 segments before it and lacks the tails of its own last R - 1: the same 48 segments' errors, once each)."""
    spec, spec128 = synth_spectra(l, h, PERIOD, 1, wname)
    w, r = IS.window(wname, l), IS.ceil_div(l, h)

    def reference(qs):
        m = qs * PERIOD
        zs = np.tile(spec128[0], (qs, 1))[None]
        ref, dp, _ = IS.model(zs, l, h, w, 1.0 / l)
        segs = IS.inverse_segments(zs, l, 1.0 / l)[0]
        body = m * h
        bnd = np.array([IS.the_bound(l, h, _amp(segs[rp * PERIOD:(rp + 1) * PERIOD])) for rp in range(qs)])
        dpp = dp[:body].reshape(qs, -1)
        worst = Worst()

        def accurate(got, rr, rp, what):
            worst.within(IS.figure(got.reshape(-1), rr.reshape(-1), dpp[rp]), bnd[rp], what)

        def tail(got, what):  # (covered by the last R - 1 segments)
            worst.within(IS.figure(got, ref[0, body:], dp[body:]), IS.the_bound(l, h, _amp(segs[m - (r - 1):])), what)
        return SimpleNamespace(ref=ref[0, :body].reshape(m, h), bnd=bnd, accurate=accurate, tail=tail, whole=True, worst=worst)

    return SimpleNamespace(plan=lambda q: _synth_plan(l, h, q * PERIOD, 1, wname), reference=reference, pattern=spec.reshape(-1), in_step=l // 2 + 1, in_tail=0,
                           out_step=h, out_periods=lambda q: q, out_tail=l - h, limits=MORE_LIMITS)


def _filter_plan(l, k, n, p, mode, taps):
    plan = FF.make_plan((l, k, n, p), mode, taps)
    FF.assert_filter_plan(plan)
    return plan


def _filter_unit(x64, taps, l, a, n_out, segs):
    """(2 b + 4 u) Hmax of fir_filter.the_bound: the bound per unit of A."""
    return FF.the_bound(x64, taps, l, a, n_out) / _amp(segs)


def filter_along(l, k, mode="same", kind="normal"):
    """A fir_filter of ONE series: a pattern of 48 V samples (stretch j of V samples scaled by 1 + j / 48) repeated, N a whole number of periods; slab = the V
    samples kept of a segment; the tail: K - 1 samples ("full"), none ("same"), a period less K - 1 samples behind one period fewer ("valid")."""
    v = l - k + 1
    x, x64 = A.tensor(period_field((v,), (0,), False, seed=33), A.F32)
    taps = FF.taps_of(kind, k)
    per = PERIOD * v

    def sizes(q):
        a, n_out = FF.offsets(mode, q * per, k)
        return q * per, a, n_out

    def reference(qs):
        n, a, n_out = sizes(qs)
        xs = np.tile(x64.reshape(-1), qs)[None]
        ref = FF.model(xs, taps, mode)[0]
        segs = FF.segment_inputs(xs, l, k, a, n_out)[0]
        unit = _filter_unit(xs, taps, l, a, n_out, segs)
        nq = n_out // per
        bnd = np.array([unit * _amp(segs[rp * PERIOD:(rp + 1) * PERIOD]) for rp in range(nq)])
        worst = Worst()

        def accurate(got, rr, rp, what):
            worst.within(FF.figure(got.reshape(-1), rr.reshape(-1)), bnd[rp], what)

        def tail(got, what):
            worst.within(FF.figure(got, ref[nq * per:]), unit * _amp(segs[nq * PERIOD:]), what)
        return SimpleNamespace(ref=ref[:nq * per].reshape(nq * PERIOD, v), bnd=bnd, accurate=accurate, tail=tail, whole=True, worst=worst)

    return SimpleNamespace(plan=lambda q: _filter_plan(l, k, q * per, 1, mode, taps), reference=reference, pattern=x.reshape(-1), in_step=v, in_tail=0, out_step=v,
                           out_periods=lambda q: sizes(q)[2] // per, out_tail=sizes(4)[2] % per, limits=LIMITS)


def along_input(pattern, q, tail, dev):
    """The pattern q times and `tail` elements of it more, built in place on the device."""
    pat = pattern.to(dev)
    body = q * pat.numel()
    buf = torch.empty(body + tail, dtype=pat.dtype, device=dev)
    buf[:body].view(q, -1).copy_(pat.reshape(1, -1).expand(q, -1))
    buf[body:].copy_(pat[:tail])
    return buf


def run_along(cid, c, q, dev, qs=4):
    """One series of q periods: the first and the last period (edges) and every period that holds a boundary against the short series' float64 reference, every
    interior period bit for bit against the first interior one, the tail, the guard bands.  Returns (plan, the boundaries reached, whether the bits repeated)."""
    assert q >= 3 and qs >= 4
    plan = c.plan(q)
    nqo, nqs = c.out_periods(q), c.out_periods(qs)
    n_in, body = q * PERIOD * c.in_step + c.in_tail, nqo * PERIOD * c.out_step
    series, e = out_shape(plan)
    assert series == 1 and e == body + c.out_tail and plan.workspace_bytes == 0, (series, e, body, c.out_tail)
    isz, osz = esize(c.pattern.dtype), esize(plan.out_dtype())
    need = device_bytes(plan, n_in * isz)
    print(f"{cid}: one series of {q} periods of {PERIOD} segments, {n_in} elements in and {e} out, {need / 2 ** 30:.2f} GiB of device memory (workspace {plan.workspace_bytes} bytes)")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    bounds = boundaries(nqo * PERIOD, c.in_step, isz, c.out_step, osz, limits=c.limits)
    try:
        x = along_input(c.pattern, q, c.in_tail, dev)
        out, _, bands = run_banded(plan, x)
        del x
        flat = out.reshape(-1)
        r = c.reference(qs)
        along = Along(1, {0: 0, nqo - 1: nqs - 1}, (flat[body:], r.tail) if c.out_tail else None, r.whole)
        same = check(flat[:body].reshape(nqo * PERIOD, c.out_step), r.ref, r.bnd, bounds, r.accurate, exact=True, bands=bands, what=cid, along=along)
        print(f"{cid}: boundaries {bounds}; worst figure / bound {r.worst.ratio:.3f}")
        return plan, bounds, same
    finally:
        out = flat = bands = along = None
        release(dev)


# ---- the period across the batch: 48 series, tiled
def keep_batch(l, h, m, mode=L.OUT_POWER):
    sp = (m - 1) * h + l
    x, x64 = A.tensor(period_field((sp,), (0,), False, seed=35), A.F32)
    dt = _keep_dt(mode)

    def reference():
        case = (l, h, m, PERIOD)
        ref, kaps = SP.reference(case, FORM, x64, mode), SP.kappas(case, FORM, x64)
        bnd = np.array([[A.bound(dt, l, k) for k in ks] for ks in kaps])
        worst = Worst()

        def accurate(got, r, j, what):  # (every segment within the bound of one transform, as spectrogram.assert_segments)
            worst.within(_rows_rms(got.reshape(r.shape), r), bnd[j], what)
        return SimpleNamespace(ref=ref, bnd=bnd.max(1), accurate=accurate, worst=worst)

    return SimpleNamespace(plan=lambda p: _rows_plan(l, h, m, p, mode), reference=reference, data=x, limits=LIMITS)


def synth_batch(l, h, m, wname="hann"):
    spec, spec128 = synth_spectra(l, h, m, PERIOD, wname)
    w = IS.window(wname, l)

    def reference():
        ref, dp, _ = IS.model(spec128, l, h, w, 1.0 / l)
        segs = IS.inverse_segments(spec128, l, 1.0 / l)
        bnd = np.array([IS.the_bound(l, h, _amp(s)) for s in segs])
        worst = Worst()

        def accurate(got, r, j, what):
            worst.within(IS.figure(got, r, dp), bnd[j], what)
        # (the all-slab pass holds these kernels to bit identity; the relative figure it takes only words the message of a slab that differs)
        return SimpleNamespace(ref=ref, bnd=bnd / np.sqrt((ref ** 2).sum(1)), accurate=accurate, worst=worst)

    return SimpleNamespace(plan=lambda p: _synth_plan(l, h, m, p, wname), reference=reference, data=spec.reshape(PERIOD, -1), limits=MORE_LIMITS)


def filter_batch(l, k, n, mode="same", kind="normal"):
    x, x64 = A.tensor(period_field((n,), (0,), False, seed=37), A.F32)
    taps = FF.taps_of(kind, k)
    a, n_out = FF.offsets(mode, n, k)

    def reference():
        ref = FF.model(x64, taps, mode)
        segs = FF.segment_inputs(x64, l, k, a, n_out)
        unit = _filter_unit(x64, taps, l, a, n_out, segs)
        bnd = np.array([unit * _amp(s) for s in segs])
        worst = Worst()

        def accurate(got, r, j, what):
            worst.within(FF.figure(got, r), bnd[j], what)
        return SimpleNamespace(ref=ref, bnd=bnd / np.sqrt((ref ** 2).sum(1)), accurate=accurate, worst=worst)

    return SimpleNamespace(plan=lambda p: _filter_plan(l, k, n, p, mode, taps), reference=reference, data=x, limits=LIMITS)


def run_batch(cid, c, p, dev):
    """p dense series of a PERIOD of 48: the windows series by series against float64, every series bit for bit against its member of the first period, the bands."""
    assert p % PERIOD == 0
    plan = c.plan(p)
    n, e = out_shape(plan)
    in_elems = c.data[0].numel()
    isz, osz = esize(c.data.dtype), esize(plan.out_dtype())
    assert n == p and plan.workspace_bytes == 0
    need = device_bytes(plan, p * in_elems * isz)
    print(f"{cid}: {p} series, {in_elems} elements in and {e} out each, {need / 2 ** 30:.2f} GiB of device memory (workspace {plan.workspace_bytes} bytes)")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    bounds = boundaries(p, in_elems, isz, e, osz, limits=c.limits)
    try:
        x = tiled(c.data, p, dev)
        out, _, bands = run_banded(plan, x)
        del x
        r = c.reference()
        same = check(out, r.ref, r.bnd, bounds, r.accurate, exact=True, bands=bands, what=cid)
        print(f"{cid}: boundaries {bounds}; worst figure / bound {r.worst.ratio:.3f}")
        return plan, bounds, same
    finally:
        out = bands = None
        release(dev)


def run_keep_cols(cid, l, h, m, blocks, inner, dev):
    """Spectrogram columns (POWER): `blocks` dense blocks of `inner` adjacent columns (seg_stride = inner) of a PERIOD of 48 columns; block b carries a further factor
    2^b, which scales its spectra by 4^b exactly and is taken out again before the check (run_welch_cols).  The result [block][segment][frequency][column] is checked
    with the columns first.  Returns (plan, the boundaries the output rows [segment][frequency] reach, bits)."""
    assert inner % PERIOD == 0
    c = (l, h, m, blocks, inner, inner, 0, None, 0)
    kb = keep_batch(l, h, m, L.OUT_POWER)
    sp = kb.data.shape[1]
    plan = SP.make_col_plan(c, FORM, L.OUT_POWER)
    SP.assert_keep_plan(plan, c)
    n, e = out_shape(plan)
    assert (n, e) == (blocks, m * l * inner)
    need = device_bytes(plan, blocks * sp * inner * 4) + n * e * 4  # (... and the copy with the columns first)
    print(f"{cid}: {blocks} blocks of {inner} columns, {m} segments, {need / 2 ** 30:.2f} GiB of device memory (workspace {plan.workspace_bytes} bytes)")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    bounds = boundaries(blocks * inner, 1, 4, 1, 4)  # (a column's first sample and first output: one element further per column)
    reached = boundaries(blocks * m * l, 0, 4, inner, 4)  # (an output row [block][segment][frequency]: `inner` elements further per row)
    try:
        cols = kb.data.to(dev).t().contiguous()                                              # [span][48]
        t0 = cols.repeat(1, inner // PERIOD).unsqueeze(0).repeat(blocks, 1, 1)               # [blocks][span][inner]
        if blocks > 1:
            t0 = (t0 * (2.0 ** torch.arange(blocks, device=dev, dtype=torch.float32)).reshape(-1, 1, 1)).contiguous()
        assert plan._layout_ok(t0)
        out, _, bands = run_banded(plan, t0)
        del t0, cols
        if blocks > 1:
            out.reshape(blocks, -1).mul_((0.25 ** torch.arange(blocks, device=dev, dtype=torch.float32)).reshape(-1, 1))  # (a power of two: exact)
        first = out.reshape(blocks, m * l, inner).transpose(1, 2).reshape(blocks * inner, m * l)
        r = kb.reference()
        same = check(first, r.ref, r.bnd, bounds, r.accurate, exact=True, bands=bands, what=cid)
        print(f"{cid}: boundaries of the output rows {reached}; worst figure / bound {r.worst.ratio:.3f}")
        return plan, reached, same
    finally:
        out = first = bands = None
        release(dev)


# ---- rung C: through the pitch.  The buffer is allocated and never filled; only the series are written
def _pitched(cid, dev, total, dtype, shape, strides, x, plan, extra=0):
    need = total * esize(dtype) + extra + (1 << 30)
    print(f"{cid}: strides {strides}: the last element at {total - 1} (byte {(total - 1) * esize(dtype)}), {need / 2 ** 30:.2f} GiB of device memory")
    ok, why = enough_memory(need, dev)
    if not ok:
        raise NeedsMemory(why)
    buf = torch.empty(total, dtype=dtype, device=dev)
    view = torch.as_strided(buf, shape, strides)
    view.copy_(torch.from_numpy(x).to(dev))
    out, _ = plan.execute(view)
    return out.cpu().numpy()


def run_keep_rows_pitched(cid, dev, pitch=(1 << 30) + 5, case=(64, 32, 3, 3), mode=L.OUT_POWER):
    l, h, m, p = case
    sp = W.span(case)
    x = SP.series(case)
    plan = SP.make_plan(case, FORM, mode, pitch=pitch)
    SP.assert_keep_plan(plan)
    try:
        got = _pitched(cid, dev, (p - 1) * pitch + sp, torch.float32, (p, sp), (pitch, 1), x, plan)
        SP.assert_segments(case, got, SP.reference(case, FORM, x, mode), SP.kappas(case, FORM, x), mode, cid)
        assert np.array_equal(got, SP.run(SP.make_plan(case, FORM, mode), x)), f"{cid}: the pitched plan differs from the dense plan"
        return plan
    finally:
        release(dev)


def run_keep_cols_strided(cid, dev, s=1 << 20, c=(64, 32, 69, 2, 40), beyond=1 << 31, mode=L.OUT_POWER):
    """Spectrogram columns whose samples lie `s` elements apart (run_welch_cols_strided): past 2^31 elements inside ONE block."""
    l, h, m, p, inner = c
    case = (l, h, m, p, inner, s, 0, None, 0)
    sp = WC.span(case)
    pitch = sp * s
    assert (sp - 1) * s + inner > beyond
    x = SP.cube(case)
    plan = SP.make_col_plan(case, FORM, mode, in_stride_batch=pitch)
    SP.assert_keep_plan(plan, case)
    try:
        out = _pitched(cid, dev, (p - 1) * pitch + (sp - 1) * s + inner, torch.float32, (p, sp, inner), (pitch, s, 1), x, plan)
        assert out.shape == (p, m, plan.nx_out, inner), out.shape
        got = np.ascontiguousarray(np.transpose(out, (0, 3, 1, 2))).reshape(p * inner, m, plan.nx_out)
        rc, rows = (l, h, m, p * inner), WC.as_rows(x)
        SP.assert_segments(rc, got, SP.reference(rc, FORM, rows, mode), SP.kappas(rc, FORM, rows), mode, cid)
        dense = case[:5] + (inner, 0, None, 0)
        assert np.array_equal(got, SP.run_cols(SP.make_col_plan(dense, FORM, mode), dense, x)), f"{cid}: the strided plan differs from the plan on the arranged copy"
        return plan
    finally:
        release(dev)


def run_synth_pitched(cid, dev, pitch=(1 << 30) + 5, case=(64, 32, 3, 3), wname="hann"):
    l, h, m, p = case
    nb = l // 2 + 1
    spec = IS.spectra(case, wname)
    plan = IS.make_plan(case, wname, pitch=pitch)
    IS.assert_synth_plan(plan)
    try:
        got = _pitched(cid, dev, (p - 1) * pitch + m * nb, torch.complex64, (p, m, nb), (pitch, nb, 1), spec, plan)
        ref, dp, a = IS.model(spec, l, h, IS.window(wname, l), 1.0 / l)
        IS.assert_within(cid, got, ref, dp, l, h, a)
        assert np.array_equal(got, IS.run(IS.make_plan(case, wname), spec)), f"{cid}: the pitched plan differs from the dense plan"
        return plan
    finally:
        release(dev)


def run_filter_pitched(cid, dev, pitch=(1 << 30) + 5, case=(256, 65, 700, 3), mode="same", kind="normal"):
    l, k, n, p = case
    a, n_out = FF.offsets(mode, n, k)
    x, taps = FF.series(case), FF.taps_of(kind, k)
    plan = FF.make_plan(case, mode, taps, pitch=pitch)
    FF.assert_filter_plan(plan)
    try:
        got = _pitched(cid, dev, (p - 1) * pitch + n, torch.float32, (p, n), (pitch, 1), x, plan)
        FF.assert_within(cid, got, FF.model(x, taps, mode), FF.the_bound(x, taps, l, a, n_out))
        assert np.array_equal(got, FF.run(FF.make_plan(case, mode, taps), x)), f"{cid}: the pitched plan differs from the dense plan"
        return plan
    finally:
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
    check_segment_guards()


def check_segment_guards():
    """The spectrogram, istft and fir_filter plans (host_welch.inc): the four "one launch; declined, never truncated" guards with 1000 workgroups per series, the
    istft span, the segments of a series, seg_in_len.  Pinned elsewhere and not repeated: one workgroup per series at 2^31 - 1 / 2^31 series and an istft span of
    2^31 from hop = L (istft.check_status_codes, fir_filter.check_status_codes); seg_in_len, seg_out_len and seg_lead at and below 0 (fir_filter.check_status_codes)."""
    bad, unsup, big = L.BAD_ARG, L.UNSUPPORTED_LENGTH, (1 << 31) - 1
    # istft: span = (M - 1) H + L <= 2^31 - 1 (fasto.h:74-77 keeps lo, hi in 64 bits and m0, count as ints inside the span)
    m = (1 << 31) - 64
    assert (m - 1) + 64 == big
    assert IS._status(nx=64, seg_hop=1, mean_batch=m, batch=m) == 0 and IS._status(nx=64, seg_hop=1, mean_batch=m + 1, batch=m + 1) == unsup
    # one launch of series x workgroups <= 2^31 - 1: istft (R = 2, F = 127: 1000 workgroups serve 127 001 segments), spectrogram (128 segments a round), fir (V = 57)
    p = big // 1000
    assert IS._status(nx=64, seg_hop=32, mean_batch=127001, batch=127001 * p) == 0 and IS._status(nx=64, seg_hop=32, mean_batch=127001, batch=127001 * (p + 1)) == unsup
    assert SP._status(nx=64, seg_hop=32, mean_batch=128000, batch=128000 * p) == 0 and SP._status(nx=64, seg_hop=32, mean_batch=128000, batch=128000 * (p + 1)) == unsup
    for pp, want in ((p, 0), (p + 1, unsup)):
        assert FF._status(**FF.plan_kw((64, 8, 57 * 128 * 1000, pp), "same")) == want, pp
    # the segments of a series: mean_batch <= 2^31 - 1 (SegTile.M is an int)
    assert SP._status(nx=64, seg_hop=1, mean_batch=big, batch=big) == 0 and SP._status(nx=64, seg_hop=1, mean_batch=big + 1, batch=big + 1) == bad
    for n, want in ((32 * big - 16, 0), (32 * big + 40, bad)):
        kw = FF.plan_kw((64, 33, n, 1), "same")
        assert kw["mean_batch"] == (big if want == 0 else big + 2)
        assert FF._status(**kw) == want, n
    # fir_filter's seg_in_len: 2^60 (a small seg_out_len: the segments follow the output)
    fk = FF.plan_kw((64, 8, 100, 1), "same")
    assert FF._status(**dict(fk, seg_in_len=1 << 60)) == 0 and FF._status(**dict(fk, seg_in_len=(1 << 60) + 1)) == bad
    # the column-layout spectrogram: a span of 2^31 - 1 samples (the seg_keep = 1 twin of the Welch line above)
    assert SP._status(nx=64, seg_hop=1, mean_batch=m, batch=m, inner=4, seg_stride=4) == 0
    assert SP._status(nx=64, seg_hop=1, mean_batch=m + 1, batch=m + 1, inner=4, seg_stride=4) == bad


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
