"""Reuse of a field's column pass across spectral products (engine.reuse_column_pass; include/xrft_hip.h: xrfthip_exec_ex).  The scenarios, shared by

  tests/test_column_reuse_emulated.py   CPU: the product's host code and kernels compiled for the emulator
  tests/test_gpu_column_reuse.py        GPU: the real libxrft_hip.so  (-m gpu)

Every result with reuse on is compared with the same call with reuse off by torch.equal / np.array_equal: bit for bit, not merely close.  What a call launched
is read from the profiling records of the plans (SpectralPlan.read_profile): a field whose pass-1 block was read records no "fasty_cols" launch.

Shapes: batch 3 of 256 x 256 and of 512 x 256 float32, the smallest of the two-pass float32 family.  (A 256 x 256 POWER plan is served by the one-pass small-slab
kernel: its calls hand no block over and launch no column pass at all; the 512 x 256 plans are all two-pass plans.)"""
import ctypes as C

import numpy as np
import torch

import xrft_amd as xa
from xrft_amd import _lib, api, engine

SHAPES = [(3, 256, 256), (3, 512, 256)]
DIMS = ("time", "y", "x")
HANN = dict(dim=["y", "x"], window="hann")
LIN = dict(dim=["y", "x"], detrend="linear", window="hann")


def fields(shape, seed=0):
    """Two correlated float32 fields with a plane on top (so that the linear detrend has work), as device tensors, and their coordinates."""
    nt, ny, nx = shape
    rng = np.random.default_rng(1000 + seed)
    ii, jj = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    a = (rng.standard_normal(shape) + 0.01 * ii - 0.02 * jj + 3.0).astype(np.float32)
    b = (0.5 * a + rng.standard_normal(shape)).astype(np.float32)
    coords = {"time": np.arange(nt), "y": np.arange(ny) * 0.5, "x": np.arange(nx) * 2.0}
    dev = _lib.device()
    return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), coords


def arr(t, coords):
    return xa.DataArray(t, DIMS, coords)


def values(res):
    d = res.data
    return d if isinstance(d, torch.Tensor) else torch.from_numpy(np.asarray(d))


def same(x, y):
    return torch.equal(values(x).cpu(), values(y).cpu())


def launches(call):
    """(result, {label: launches}) of one API call: the profiling records of every cached plan, fresh for this call (the call's plan must exist: run it once before)."""
    plans = list(api._plan_cache.values())
    for p in plans:
        p.set_profiling(True)
    try:
        res = call()
        got = {}
        for p in plans:
            for label, (n, _ms) in p.read_profile().items():
                got[label] = got.get(label, 0) + n
    finally:
        for p in plans:
            p.set_profiling(False)
    return res, got


def fresh(call):
    """The call with reuse off and nothing kept: what every variant must equal bit for bit."""
    was = engine.reuse_column_pass()
    engine.reuse_column_pass(False)
    try:
        return call()
    finally:
        engine.reuse_column_pass(was)


def start():
    api.clear_plan_cache()
    engine.reuse_column_pass(True)


# ---- the sequences of the issue
def cross_then_isotropic(shape, check=None):
    """cross_spectrum(a, b), isotropic_power_spectrum(a), (b), all with Hann: the cross call launches the column pass twice, the isotropic calls not at all."""
    start()
    ta, tb, coords = fields(shape)
    da, db = arr(ta, coords), arr(tb, coords)
    calls = [lambda: xa.cross_spectrum(da, db, **HANN), lambda: xa.isotropic_power_spectrum(da, **HANN), lambda: xa.isotropic_power_spectrum(db, **HANN)]
    ref = [fresh(c) for c in calls]  # (also builds the plans)
    got = [launches(c) for c in calls]
    for (res, _n), r in zip(got, ref):
        assert same(res, r)
    assert got[0][1].get("fasty_cols", 0) == 2, got[0][1]
    assert got[1][1].get("fasty_cols", 0) == 0 and got[2][1].get("fasty_cols", 0) == 0, (got[1][1], got[2][1])
    if shape[1] > 256:  # (two-pass plans throughout: the isotropic calls ran their row pass on the blocks the cross call left)
        assert got[1][1].get("fasty_rows", 0) == 1 and got[2][1].get("fasty_rows", 0) == 1, (got[1][1], got[2][1])
    # a second round: the cross call computes both fields again (its own blocks are never its input), the isotropic calls read them again
    again = [launches(c) for c in calls]
    assert again[0][1].get("fasty_cols", 0) == 2 and again[1][1].get("fasty_cols", 0) == 0 and again[2][1].get("fasty_cols", 0) == 0
    for (res, _n), r in zip(again, ref):
        assert same(res, r)
    if check is not None:
        check(ta, tb, coords, [g[0] for g in got])


def power_then_isotropic_detrended(shape):
    """power_spectrum(a, linear, hann) then isotropic_power_spectrum(a, linear, hann): the second call reads the block -- sums, lines and corrections with it."""
    start()
    ta, _tb, coords = fields(shape, seed=1)
    da = arr(ta, coords)
    calls = [lambda: xa.power_spectrum(da, **LIN), lambda: xa.isotropic_power_spectrum(da, **LIN)]
    ref = [fresh(c) for c in calls]
    got = [launches(c) for c in calls]
    assert same(got[0][0], ref[0]) and same(got[1][0], ref[1])
    assert got[1][1].get("fasty_cols", 0) == 0 and got[1][1].get("fasty_fit", 0) == 0, got[1][1]
    if shape[1] > 256:
        assert got[0][1].get("fasty_cols", 0) == 1 and got[0][1].get("fasty_fit", 0) == 1 and got[1][1].get("fasty_rows", 0) == 1, (got[0][1], got[1][1])


def _two_pass_shape(shape):
    return shape[1] > 256


def no_reuse_cases(shape):
    """Where nothing may be reused -- and the results equal a fresh computation."""
    ta, tb, coords = fields(shape, seed=2)
    da, db = arr(ta, coords), arr(tb, coords)
    iso_a = lambda: xa.isotropic_power_spectrum(da, **HANN)  # noqa: E731
    cross = lambda: xa.cross_spectrum(da, db, **HANN)  # noqa: E731
    cols = 1 if _two_pass_shape(shape) else 0  # column passes of a one-field call that computes everything

    # the same call twice: both launch the column pass
    start()
    ref = fresh(iso_a)
    first, second = launches(iso_a), launches(iso_a)
    assert first[1].get("fasty_cols", 0) == cols and second[1].get("fasty_cols", 0) == cols, (first[1], second[1])
    assert same(first[0], ref) and same(second[0], ref)

    # after a.add_(1): the tensor's version moved
    start()
    cross(), iso_a()  # (the plans)
    launches(cross)
    ta.add_(1)
    res, n = launches(iso_a)
    assert n.get("fasty_cols", 0) == cols, n
    assert same(res, fresh(iso_a))
    ta.sub_(1)

    # after a call with another window or detrend: another signature
    for other in (dict(dim=["y", "x"], window="hamming"), dict(dim=["y", "x"], window="hann", detrend="constant")):
        start()
        ref = fresh(iso_a)
        xa.cross_spectrum(da, db, **other)
        res, n = launches(iso_a)
        assert n.get("fasty_cols", 0) == cols, (other, n)
        assert same(res, ref)

    # on a view with the same data_ptr but other strides: the left half of the columns of a field twice as wide
    start()
    nt, ny, nx = shape
    wide = torch.cat([ta, tb], dim=2).contiguous()
    wa = arr(wide[:, :, :nx], coords)  # (same data_ptr as `dense` below would have if it were this memory: the tag carries the strides)
    assert wa.data.data_ptr() == wide.data_ptr() and not wa.data.is_contiguous()
    dense = xa.DataArray(wide.reshape(-1)[:nt * ny * nx].reshape(shape), DIMS, coords)  # the same first byte, dense strides, other samples
    assert dense.data.data_ptr() == wide.data_ptr()
    iso_view = lambda: xa.isotropic_power_spectrum(wa, **HANN)  # noqa: E731
    iso_dense = lambda: xa.isotropic_power_spectrum(dense, **HANN)  # noqa: E731
    ref_v, ref_d = fresh(iso_view), fresh(iso_dense)
    xa.cross_spectrum(wa, wa, **HANN)
    res, n = launches(iso_dense)
    assert n.get("fasty_cols", 0) == cols, n
    assert same(res, ref_d)
    assert same(iso_view(), ref_v) and same(ref_v, fresh(iso_a))

    # after a larger call regrew the scratch
    start()
    iso_a(), cross()
    size = engine._WS[next(iter(engine._WS))].numel()
    big = torch.cat([ta, ta, ta, ta], dim=0)
    cbig = dict(coords, time=np.arange(big.shape[0]))
    xa.cross_spectrum(arr(big, cbig), arr(big, cbig), **HANN)
    assert engine._WS[next(iter(engine._WS))].numel() > size
    res, n = launches(iso_a)
    assert n.get("fasty_cols", 0) == cols, n
    assert same(res, fresh(iso_a))

    # with reuse_column_pass(False)
    start()
    ref = fresh(iso_a)
    engine.reuse_column_pass(False)
    try:
        cross()
        res, n = launches(iso_a)
    finally:
        engine.reuse_column_pass(True)
    assert n.get("fasty_cols", 0) == cols, n
    assert same(res, ref)

    # inputs that are not device tensors never take part (numpy data: a fresh device copy per call)
    start()
    na, nb_ = xa.DataArray(ta.cpu().numpy(), DIMS, coords), xa.DataArray(tb.cpu().numpy(), DIMS, coords)
    xa.cross_spectrum(na, nb_, **HANN)
    xa.isotropic_power_spectrum(na, **HANN)
    xa.cross_spectrum(na, nb_, **HANN)
    res, n = launches(lambda: xa.isotropic_power_spectrum(na, **HANN))
    assert n.get("fasty_cols", 0) == cols, n
    assert same(res, fresh(iso_a))


def other_stream(shape):
    """A block written on one stream is not read on another (GPU only: the emulated device has one stream)."""
    start()
    ta, tb, coords = fields(shape, seed=3)
    da, db = arr(ta, coords), arr(tb, coords)
    iso_a = lambda: xa.isotropic_power_spectrum(da, **HANN)  # noqa: E731
    ref = fresh(iso_a)
    xa.cross_spectrum(da, db, **HANN)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        iso_a()  # (plan and scratch of that stream)
        res, n = launches(iso_a)
    s.synchronize()
    assert n.get("fasty_cols", 0) == (1 if _two_pass_shape(shape) else 0), n
    assert same(res, ref)


# ---- the C ABI
def _plan(batch, ny, nx, dtype=torch.float32, out_mode=_lib.OUT_POWER, **kw):
    return engine.SpectralPlan(2, batch, ny, nx, dtype, out_mode=out_mode, **kw)


def c_abi_errors():
    dll = _lib.load()
    dev = _lib.device()
    # no block: a fastm plan, a batch in more than one group of slabs, the four-step 1-D form
    assert _plan(2, 360, 360, torch.float64).pass1() == (0, ())
    assert _plan(4, 512, 256, slabs_per_group=2).pass1() == (0, ())
    assert engine.SpectralPlan(1, 2, 1, 65536, torch.float32, out_mode=_lib.OUT_POWER).pass1() == (0, ())
    p = _plan(3, 512, 256)
    q = _plan(3, 512, 256, out_mode=_lib.OUT_CROSS)
    nb, sigs = p.pass1()
    assert nb > 0 and nb % 256 == 0 and q.pass1()[0] == nb
    # one signature for the same column pass, whatever the plan does behind it; another for another window or detrend
    assert q.pass1()[1] == (sigs[0], sigs[0])
    assert _plan(3, 512, 256, flags=_lib.SHIFT_Y | _lib.SHIFT_X, scale=2.0).pass1()[1] == sigs
    assert _plan(3, 512, 256, detrend=_lib.DETREND_LINEAR).pass1()[1] != sigs
    assert _plan(3, 512, 256, window_y=np.hanning(512)).pass1()[1] != sigs
    assert _plan(3, 512, 256, window_x=np.hanning(256)).pass1()[1] != sigs
    assert _plan(3, 256, 512).pass1()[1] != sigs and _plan(2, 512, 256).pass1()[1] != sigs
    sig = C.c_uint64(0)
    assert dll.xrfthip_plan_pass1_signature(p._h, 1, C.byref(sig)) == _lib.BAD_ARG  # (a one-field plan has no field 1)
    assert dll.xrfthip_plan_pass1_signature(_plan(2, 360, 360, torch.float64)._h, 0, C.byref(sig)) == _lib.BAD_ARG

    x = torch.randn((3, 512, 256), dtype=torch.float32, generator=torch.Generator().manual_seed(5)).to(dev)
    out = torch.empty((3, 512, 256), dtype=torch.float32, device=dev)
    wsb = p.workspace_bytes
    buf = torch.empty(wsb + nb + 1024, dtype=torch.uint8, device=dev)
    base = (buf.data_ptr() + 255) & ~255

    def run(plan, mode, block, ws=None, ws_bytes=None, field=0, inp=x):
        a = _lib.ExecArgs()
        a.struct_size = C.sizeof(_lib.ExecArgs)
        a.d_in0, a.d_out = inp.data_ptr(), out.data_ptr()
        a.d_workspace, a.ws_bytes = (base + nb if ws is None else ws), (wsb if ws_bytes is None else ws_bytes)
        a.field[field].pass1_block, a.field[field].pass1_mode = block, mode
        return dll.xrfthip_exec_ex(plan._h, C.byref(a))

    assert run(p, 3, base) == _lib.BAD_ARG                                   # no such mode
    assert run(p, _lib.PASS1_PRODUCE, None) == _lib.BAD_ARG                  # no block
    assert run(p, _lib.PASS1_PRODUCE, base + 64) == _lib.BAD_ARG             # not 256-byte aligned
    assert run(p, _lib.PASS1_PRODUCE, base + 256) == _lib.BAD_ARG            # reaches into the workspace
    assert run(p, _lib.PASS1_CONSUME, base + nb, ws=base) == _lib.BAD_ARG    # the workspace reaches into the block
    assert run(p, _lib.PASS1_PRODUCE, base, field=1) == _lib.BAD_ARG         # field 1 of a one-field plan
    g = _plan(2, 360, 360, torch.float64)
    x64 = torch.zeros((2, 360, 360), dtype=torch.float64, device=dev)
    assert run(g, _lib.PASS1_PRODUCE, base, inp=x64) == _lib.BAD_ARG         # a plan that hands no block over
    assert run(p, _lib.PASS1_PRODUCE, base, ws_bytes=wsb - nb - 256) == -3   # XRFTHIP_WORKSPACE_TOO_SMALL
    # ... and the good calls: produce with the smaller workspace, then consume, then everything private -- one result
    assert run(p, _lib.PASS1_PRODUCE, base, ws_bytes=wsb - nb) == 0
    first = out.clone()
    assert run(p, _lib.PASS1_CONSUME, base, ws_bytes=wsb - nb) == 0
    assert torch.equal(out, first)
    assert run(p, _lib.PASS1_PRIVATE, None) == 0
    assert torch.equal(out, first)
