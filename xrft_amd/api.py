"""The xrft call surface (same names, argument meaning and error behaviour as the reference's
``xrft/xrft.py`` and ``xrft/detrend.py``), executed by the MI355X engine in libxrft_hip.so.

Host side (this file): argument normalisation, coordinate validation, spacing / lag / frequency vectors,
window vectors, the radial bin map -- all tiny float64 numpy work that must match the reference bit for bit.
Device side (one fused plan per call): detrend, window, flip/ifftshift, FFT, fftshift, phase, scaling,
|F|^2 / F conj(G), Hermitian mirror, radial bin-sum.

Deviations from the reference, all documented in DESIGN.md:
  * float32 input is computed and returned in float32/complex64 (the reference promotes to float64 as soon as a
    float64 window or ``prod(dx)`` touches the data); isotropic results are returned in float64/complex128;
  * float16 / bfloat16 input (numpy float16 arrays, torch float16 / bfloat16 tensors) is computed in float32 and returned as
    float32/complex64, exactly what the call on ``x.float()`` returns: where a float32 kernel family reads 2-byte samples the
    field is read where it lies (no widened copy), everywhere else it is widened once, exactly, on the device.  (torch half
    tensors used to be widened to float64 and returned as float64/complex128.)
  * at most two transform dimensions (the reference also offers 3-D linear detrend / N-D fftn);
  * ``chunks_to_segments`` takes its segment length from ``DataArray.chunk({dim: n})`` metadata (no dask here).
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import torch

from . import _lib, engine
from ._bluestein import _BLUE_TABLES, _bluestein_1d, _narrow, _wide
from ._hostside import (_TORCH_HALF, _analyze, _diff_coord, _dim_list, _direct_lag_attrs, _flags_tables, _freq_name, _label_guard, _label_output,  # noqa: F401
                        _lag_coord, _nd_scale, _real_dim_last, _real_flag_warning, _spectrum_scale, _swap_xy, _to_device, _widen_half, _window_vector)
from ._inverse import idft, ifft
from ._plans import (_HALF_REFUSED, _MEAN_REFUSED, _STRIDED_REFUSED, _TWO_STAGE, _akey, _get_plan, _memoised, _plan_cache, _plan_key, _plan_lock, _ro,  # noqa: F401
                     _rung)
from ._radial import _finish_iso, _radial_bins, _radial_bins_uncached, isotropize  # noqa: F401
from .labeled import Coordinate, DataArray, from_any, to_like

__all__ = ["clear_plan_cache", "fft", "ifft", "dft", "idft", "detrend", "power_spectrum", "cross_spectrum", "cross_phase", "isotropize",
           "isotropic_power_spectrum", "isotropic_cross_spectrum", "fit_loglog", "mean_power_spectrum", "mean_cross_spectrum", "welch_power_spectrum", "welch_cross_spectrum",
           "welch_coherence", "spectrogram", "stft", "istft", "fir_filter", "multitaper_power_spectrum", "multitaper_cross_spectrum", "multitaper_coherence"]


def clear_plan_cache():
    """Drop every cached plan (device tables) and the shared scratch buffers."""
    with _plan_lock:
        _plan_cache.clear()
        _STRIDED_REFUSED.clear()
        _HALF_REFUSED.clear()
        _MEAN_REFUSED.clear()
        _BLUE_TABLES.clear()
        _TWO_STAGE.clear()
    engine.clear_workspaces()


def _view_strides(t, ndim):
    """(in_stride_y, in_stride_batch) if the library can read the view ``t`` (*other, [ny,] nx) where it lies -- xrfthip_desc.in_stride_y / in_stride_batch: unit
    stride along x, the leading dims collapsing to one batch stride, both strides and the first element on 16-byte boundaries, the rows of one slab within 32-bit
    offsets -- else None (the view is copied, as every view was before the descriptor had strides)."""
    if t.is_contiguous() or t.numel() == 0:
        return None
    sy, sb = engine.strides_of(t, ndim)
    if sy is None:
        return None
    esz = t.element_size()
    ny = t.shape[-2] if ndim == 2 else 1
    if (sy * esz) % 16 or (sb * esz) % 16 or t.data_ptr() % 16 or ny * sy > (1 << 31) - 1 or ny * sy * esz > (1 << 32) - 1:
        return None
    return (sy if ndim == 2 else 0), sb


def _arrange_view(c, da, view_ok=True, keep_half=False):
    """The device tensor with the transform axes last, (*other, [ny,] nx); it leaves a box cut out of a larger array (``da.isel(y=slice(..), x=slice(..))``) where it lies when the transform dims are already the last
    ones, in order, and the library can address the view (_view_strides): returns (tensor, other_dims, strides or None).  Everything else is made contiguous.
    ``keep_half``: a float16 / bfloat16 field stays in its 2-byte samples; a view of one is copied contiguous in half precision (half plans read dense input)."""
    t = _to_device(da.data, keep_half)
    tdims = ([c.ydim] if c.ydim is not None else []) + [c.xdim]
    other = [d for d in da.dims if d not in tdims]
    order = other + tdims
    if tuple(order) != tuple(da.dims):
        t = t.permute([da.get_axis_num(d) for d in order])
    elif view_ok and t.dtype not in _TORCH_HALF:
        st = _view_strides(t, len(tdims))
        if st is not None:
            return t, other, st
    return t.contiguous(), other, None


def _inplace_axis(c, da, iso):
    """Axis number k if the call is a single-axis transform along a middle or first axis that the engine can do where the
    axis lies (XRFTHIP_AXIS_Y: the array is (batch, n, inner) with no transposed copy, like the reference, xrft.py:395-409)."""
    if len(c.dim) != 1 or iso is not None:  # (real_dim along the axis: the half output of the one-pass kernels, ABI 0.1.4)
        return None
    k = da.get_axis_num(c.xdim)
    return k if k != len(da.dims) - 1 else None


def _execute_axis_y(c, da, mode, scale, k, da2=None, c2=None, extra_flags=0):
    """Single transform axis k < last: (batch, ny, nx) = (prod(shape[:k]), shape[k], prod(shape[k+1:])), y transformed in
    place.  Returns the output tensor in the ORIGINAL dim order, or None if the plan cannot be built (column too long
    for one LDS tile): the caller then takes the transposing path."""
    t = _to_device(da.data).contiguous()  # C-contiguous input: no copy
    shape = list(t.shape)
    ny = shape[k]
    nx = int(np.prod(shape[k + 1:], dtype=np.int64))
    batch = int(np.prod(shape[:k], dtype=np.int64))
    flags, win, ph = _flags_tables(c, da, None if c2 is None else c2.lag_x, None if c2 is None else c2.reversed)
    if mode == _lib.OUT_POWER:
        ph = {"y": None, "x": None}
    yflags = _lib.AXIS_Y | (flags & _lib.HALF_X) | extra_flags  # (HALF_X / REALDIM_X2 with AXIS_Y: along the transformed axis)
    if (yflags & _lib.HALF_X) and (t.is_complex() or (flags & (_lib.FLIP_X | _lib.FLIP0_X))):
        return None  # (the half output exists for real input in coordinate order only: the transposing path)
    for fx, fy in ((_lib.SHIFT_X, _lib.SHIFT_Y), (_lib.ISHIFT_X, _lib.ISHIFT_Y), (_lib.FLIP_X, _lib.FLIP_Y), (_lib.FLIP0_X, _lib.FLIP0_Y)):
        if flags & fx:
            yflags |= fy
    t2 = None
    if da2 is not None:
        t2 = _to_device(da2.data).contiguous()
        if tuple(da2.dims) != tuple(da.dims) or t2.shape != t.shape:
            raise ValueError("The two datasets have different dimensions")
        if t2.dtype != t.dtype:
            dt = torch.promote_types(t.dtype, t2.dtype)
            t, t2 = t.to(dt), t2.to(dt)
    kw = dict(ndim=2, batch=batch, ny=ny, nx=nx, dtype=t.dtype, out_mode=mode, detrend=c.detrend, flags=yflags,
              scale=float(scale), window_y=win["x"], window_x=None, phase_y=ph["x"], phase_x=None)
    if ny * nx > (1 << 31) - 1 or nx > (1 << 30) or ny > (1 << 30):
        return None  # the engine indexes a slab with 32 bits: a cube this large along a first / middle axis takes the transposing path
    try:
        plan = _get_plan(**kw)
    except _lib.XrftHipError as e:
        if e.status == _lib.UNSUPPORTED_LENGTH:
            return None
        raise
    out, _ = plan.execute(t.reshape(batch, ny, nx), None if t2 is None else t2.reshape(batch, ny, nx))
    shape[k] = plan.ny_out
    return out.reshape(shape)


def _execute_inner(c, da, mode, scale, extra_flags=0, da2=None, c2=None, iso=None):
    """Two transform axes that are not the trailing pair, wherever they lie -- dim = ["y", "x"] of a (y, x, time) array, dim = ["t", "x"] of a (t, y, x) array:
    the engine's layout [batch][n0][mid][n1][inner] (xrfthip_desc.inner, .mid: the products of the extents in front of, between and behind the two axes)
    transforms them where they lie, as the reference does (xrft.py:395-409) -- no transposed copy of the input or of the result.  Returns the result in
    the input's dim order, or None when the call is not of this kind (the caller then takes the transposing path).
    ``iso`` (bin map on the (ydim, xdim) grid, nbins, key; ``extra_flags`` then carry ISO | NO_SPECTRUM_OUT): returns the radial sums instead, one row of nbins per
    element in the input's order of the other dims -- the reference's ``other dims + [freq_r]`` (xrft.py:1076-1095)."""
    if len(c.dim) != 2 or mode not in (_lib.OUT_COMPLEX, _lib.OUT_POWER, _lib.OUT_CROSS):
        return None
    p, q = da.get_axis_num(c.ydim), da.get_axis_num(c.xdim)
    first, second = min(p, q), max(p, q)
    if second == first + 1 and second == len(da.dims) - 1:
        return None  # (the trailing pair: the fused two-axis plans)
    t = _to_device(da.data).contiguous()  # C-contiguous input: no copy
    shape = list(t.shape)
    inner = int(np.prod(shape[second + 1:], dtype=np.int64))
    mid = int(np.prod(shape[first + 1:second], dtype=np.int64))
    batch = int(np.prod(shape[:first], dtype=np.int64))
    # the extents the composite plan carries in 32 bits (create_inner_plan; the one-axis stages): known limits are checked HERE,
    # so that a BAD_ARG from the library means a bug in the descriptor and is raised, not hidden behind the transposing path
    if (inner < 2 and mid < 2) or mid * inner * shape[second] > (1 << 30) or shape[first] * shape[second] * inner * mid > (1 << 31) - 1:
        return None
    t2 = None
    if mode == _lib.OUT_CROSS:  # (round 6: the cross spectrum of two real fields on the fused passes -- both fields where they lie)
        if da2 is None or tuple(da2.dims) != tuple(da.dims):
            return None
        t2 = _to_device(da2.data).contiguous()
        if t2.shape != t.shape or t2.dtype != t.dtype or t.is_complex():
            return None
    flags, win, ph = _flags_tables(c, da, None if c2 is None else c2.lag_x, None if c2 is None else c2.reversed)
    flags |= extra_flags  # (REALDIM_X2: the kept half of the real axis counts twice in a power spectrum)
    if mode == _lib.OUT_POWER:
        ph = {"y": None, "x": None}
    if p > q:  # the array holds (x, y): the plan's first axis is the one that comes first in memory
        flags, win, ph = _swap_xy(flags), {"y": win["x"], "x": win["y"]}, {"y": ph["x"], "x": ph["y"]}
    kw = dict(ndim=2, batch=batch, ny=shape[first], nx=shape[second], inner=inner, mid=mid, dtype=t.dtype, out_mode=mode, detrend=c.detrend, flags=flags,
              scale=float(scale), window_y=win["y"], window_x=win["x"], phase_y=ph["y"], phase_x=ph["x"])
    bkey = None
    if iso is not None:
        if flags & (_lib.HALF_X | _lib.HALF_Y):
            return None  # (real_dim: the radial sums of a half spectrum are not taken where the axes lie)
        bm, bkey = iso["binmap"], iso.get("binmap_key")
        if p > q:  # (the map is laid out (ydim, xdim): the plan's first axis is xdim)
            bm, bkey = np.ascontiguousarray(bm.T), (bkey, "T")
        kw.update(binmap=bm, nbins=iso["nbins"])
    try:
        plan = _get_plan(binmap_key=bkey, **kw)
    except _lib.XrftHipError as e:
        if e.status == _lib.UNSUPPORTED_LENGTH:  # a length the one-axis plans do not take: the transposing path
            return None
        raise
    out, iso_out = plan.execute(t, t2)
    if iso is not None:
        return iso_out
    shape[first], shape[second] = plan.ny_out, plan.nx_out  # (real_dim: n / 2 + 1 samples along that axis -- the second of the pair in memory, or the first: XRFTHIP_HALF_Y)
    return out.reshape(shape)


def _own_tensor(da, t):
    """The caller's own device tensor behind ``t`` -- ``da.data`` when ``t`` is its memory, not a copy made for the call -- else None.  Only such a field takes part
    in the reuse of the column pass (engine.reuse_column_pass): its identity and ``_version`` say whether it is unchanged since an earlier call."""
    d = da.data
    if isinstance(d, torch.Tensor) and d.device.type == _lib.device() and d.dtype == t.dtype and d.untyped_storage().data_ptr() == t.untyped_storage().data_ptr():
        return d
    return None


def _run(plan, da, t, da2, t2, other):
    """(out, iso, other) of the plan on the arranged fields; ``sources``: per field the caller's own tensor, or None (_own_tensor)."""
    return plan.execute(t, t2, sources=(_own_tensor(da, t),) if t2 is None else (_own_tensor(da, t), _own_tensor(da2, t2))) + (other,)


class _MeanDeclined(Exception):
    """No plan takes this call with mean_batch (xrfthip_desc.mean_batch: XRFTHIP_UNSUPPORTED_LENGTH): the caller composes the plain call and .mean()."""


def _execute(c, da, mode, scale, da2=None, c2=None, iso=None, extra_flags=0, mean_batch=0):
    if mean_batch:  # the mean over every ``mean_batch`` consecutive slabs of the arranged (batch, ny, nx) array inside the last pass, or _MeanDeclined
        return _execute_trailing(c, da, mode, scale, da2, c2, iso, extra_flags, mean_batch)
    k = _inplace_axis(c, da, iso) if (extra_flags & ~_lib.REALDIM_X2) == 0 else None
    if k is not None:
        out = _execute_axis_y(c, da, mode, scale, k, da2, c2, extra_flags)
        if out is not None:
            return out, None, None  # other = None: the output has the input's dim order
    if (extra_flags & ~_lib.REALDIM_X2) == 0 and iso is None and (da2 is None or mode == _lib.OUT_CROSS):
        out = _execute_inner(c, da, mode, scale, extra_flags, da2, c2)
        if out is not None:
            return out, None, None
    if iso is not None and (extra_flags & ~_lib.REALDIM_X2) == (_lib.ISO | _lib.NO_SPECTRUM_OUT) and (da2 is None or mode == _lib.OUT_CROSS):
        # isotropic spectra on non-trailing axes: the radial sums of every element from the fused passes where the axes lie -- no transposed copy
        iso_out = _execute_inner(c, da, mode, scale, extra_flags, da2, c2, iso)
        if iso_out is not None:
            tdims = (c.ydim, c.xdim)
            return None, iso_out, [d for d in da.dims if d not in tdims]
    if extra_flags == 0 and iso is None and da2 is not None and mode == _lib.OUT_PHASE:
        # the cross phase of two fields on non-trailing axes: the fused cross spectrum where the axes lie, then its angle (xrft.py:871-874) -- no transposed copy
        out = _execute_inner(c, da, _lib.OUT_CROSS, scale, 0, da2, c2)
        if out is not None:
            return engine.angle(out), None, None
    return _execute_trailing(c, da, mode, scale, da2, c2, iso, extra_flags, 0)


def _execute_trailing(c, da, mode, scale, da2, c2, iso, extra_flags, mean_batch):
    """The plan over the trailing axes of the arranged array (*other, [ny,] nx)."""
    t, other, strides = _arrange_view(c, da, keep_half=True)  # (a qualifying view of a larger array stays where it lies: no contiguous copy)
    if mean_batch and t.dtype not in (torch.float32,) + _TORCH_HALF:
        raise _MeanDeclined()
    ndim = len(c.dim)
    nx = da.sizes[c.xdim]
    ny = da.sizes[c.ydim] if c.ydim is not None else 1
    batch = t.numel() // max(ny * nx, 1)
    flags, win, ph = _flags_tables(c, da, None if c2 is None else c2.lag_x, None if c2 is None else c2.reversed)
    if mode == _lib.OUT_POWER:
        ph = {"y": None, "x": None}
    flags |= extra_flags
    t2 = None
    if da2 is not None:
        t2, other2, strides2 = _arrange_view(c2, da2, keep_half=True)
        if t2.shape != t.shape or other2 != other:
            raise ValueError("The two datasets have different dimensions")
        if t2.dtype != t.dtype and (t.dtype in _TORCH_HALF or t2.dtype in _TORCH_HALF):  # half with anything else: widened first, then promoted as ever
            t, t2 = _widen_half(t), _widen_half(t2)
        if strides2 != strides or t2.dtype != t.dtype:  # one set of strides serves both fields: anything else is copied
            t, t2, strides = t.contiguous(), t2.contiguous(), None
        if t2.dtype != t.dtype:
            dt = torch.promote_types(t.dtype, t2.dtype)
            t, t2 = t.to(dt), t2.to(dt)
    kw = dict(ndim=ndim, batch=batch, ny=ny, nx=nx, dtype=t.dtype, out_mode=mode, detrend=c.detrend, flags=flags,
              scale=float(scale), window_y=win["y"], window_x=win["x"], phase_y=ph["y"], phase_x=ph["x"])
    bkey = None
    if iso is not None:
        kw.update(binmap=iso["binmap"], nbins=iso["nbins"])
        bkey = iso.get("binmap_key")
    mkey = None
    if mean_batch:
        kw["mean_batch"] = int(mean_batch)
        mkey = _plan_key(bkey, dict(kw, dtype=torch.float32))  # (the float32 key: a half mean call the library declined before is not widened again)
        if mkey in _MEAN_REFUSED:
            raise _MeanDeclined()

    if t.dtype in _TORCH_HALF:
        # the plan that reads the 2-byte samples where they lie: the float32 plan of this call with a half loader, or UNSUPPORTED_LENGTH (a family without one, a
        # field that is not 16-byte aligned): then the field is widened once and the float32 plan runs -- the same bits either way
        if t.data_ptr() % 16 == 0 and (t2 is None or t2.data_ptr() % 16 == 0):
            done = _rung(_HALF_REFUSED, bkey, kw, lambda plan: _run(plan, da, t, da2, t2, other))  # (run inside _rung's try: the execution of a half plan can decline, too)
            if done is not None:
                return done
        t = _widen_half(t)
        t2 = None if t2 is None else _widen_half(t2)
        kw["dtype"] = t.dtype
    if strides is not None:
        # the plan that reads the view: the family of the dense plan of this shape, or UNSUPPORTED_LENGTH (then: the copy and the dense plan, exactly as before)
        done = _rung(_STRIDED_REFUSED, bkey, dict(kw, in_stride_y=strides[0], in_stride_batch=strides[1]), lambda plan: _run(plan, da, t, da2, t2, other))
        if done is not None:
            return done
        t = t.contiguous()
        t2 = None if t2 is None else t2.contiguous()
    if mean_batch:
        plan = _rung(_MEAN_REFUSED, bkey, kw, key=mkey if kw["dtype"] == torch.float32 else None)  # (float32: the key looked up above)
        if plan is None:
            raise _MeanDeclined()
        return _run(plan, da, t, da2, t2, other)
    try:
        plan = _get_plan(binmap_key=bkey, **kw)
    except _lib.XrftHipError as e:
        if e.status != _lib.UNSUPPORTED_LENGTH:
            raise
        # numpy.fft takes any length; here a prime factor above 128 goes through Bluestein inside one LDS tile, which bounds
        # the length (2 n - 1 rounded up to 2^a 3^b 5^c complex samples must fit 160 KB)
        if ndim == 1 and iso is None and t2 is None and mode in (_lib.OUT_COMPLEX, _lib.OUT_POWER) and not (flags & (_lib.INVERSE | _lib.C2R_X | _lib.PHASE_IN)):
            return _bluestein_1d(t, nx, mode, c.detrend, flags, scale, win["x"], ph["x"]), None, other
        lens = {d: da.sizes[d] for d in c.dim}
        lim = 8800 if t.dtype in (torch.float32, torch.complex64) else 4400
        raise _UnsupportedLength(f"transform length(s) {lens} not supported on the device: a length with a prime factor above 128 must be "
                         f"<= ~{lim} samples for {str(t.dtype).replace('torch.', '')} data (Bluestein inside one LDS tile) unless it is the only "
                         f"transform axis; transform the axes one at a time, or pad / crop the axis (e.g. xrft_amd.pad) to a smooth length") from e
    return _run(plan, da, t, da2, t2, other)


class _UnsupportedLength(ValueError):
    """A two-axis plan could not be built for these lengths: the callers transform the axes one at a time instead."""


# ------------------------------------------------------------------------------------------------------
# more than two transform axes: numpy's fftn is separable, so the reference's N-D transform
# (xrft.py:439-447) is the fused two-axis plan over the last two listed dims followed by one- or two-axis plans over
# the remaining ones; detrending needs the whole block and runs first as its own device pass; windows, shifts, phase
# factors and the dx amplitude factor are per-axis and travel with the stage that transforms the axis.
# ------------------------------------------------------------------------------------------------------
def _nd_dims(da, dim, real_dim, real):
    """The normalised dim list if it has more than two entries, else None."""
    dims = _dim_list(da, dim)
    if len(dims) <= 2:
        return None
    rd = real if real is not None else real_dim
    if rd is not None:
        dims = _real_dim_last(da, dims, rd)
    for d in dims:
        da.get_axis_num(d)
    return dims


def _two_dims(da, dim, real_dim, real):
    """The normalised list of two transform dims (the real one last), for the one-axis-at-a-time fallback (after _analyze: the real dim exists)."""
    dims = _dim_list(da, dim)
    rd = real if real is not None else real_dim
    return _real_dim_last(da, dims, rd) if rd is not None else dims


def _fft_nd(da, dims, spacing_tol, real_dim, shift, detrend_, window, true_phase, true_amplitude, chunks_to_segments,
            prefix, one_at_a_time=False):
    if chunks_to_segments:
        raise NotImplementedError("chunks_to_segments is implemented for one or two transform dimensions.")
    if detrend_ not in (None, "constant", "linear"):
        raise NotImplementedError("%s is not a valid detrending option. Valid options are: 'constant','linear', "
                                  "or None." % detrend_)
    cur = da
    if detrend_ is not None:
        cur = from_any(detrend(cur, dims, detrend_))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        g = 1 if one_at_a_time else 2  # (one axis per stage: a length no two-axis plan takes goes through the one-axis paths, which take any)
        cur = fft(cur, spacing_tol=spacing_tol, dim=dims[-g:], real_dim=real_dim, shift=shift, detrend=None,
                  window=window, true_phase=true_phase, true_amplitude=true_amplitude, prefix=prefix)
        rest = dims[:-g]
        sh = False if real_dim is not None else shift  # xrft.py:403: a real transform switches every shift off
        while rest:
            grp, rest = rest[-g:], rest[:-g]
            cur = fft(cur, spacing_tol=spacing_tol, dim=grp, shift=sh, detrend=None, window=window,
                      true_phase=true_phase, true_amplitude=true_amplitude, prefix=prefix)
    return cur


# power_spectrum / cross_spectrum and fft / dft over the trailing THREE axes of real data take the fused routes (_spectrum_3d_fused, _fft_3d_fused); False: the
# composition of _fft_nd stages (and the elementwise tail), as before round 9 -- the tests and scripts/bench_three_axes.py compare the two on one build
_FUSE_THREE_AXES = True


def _real_dtype(data):
    """float32 / float64 as it lies (anything else -- integers, float16, complex -- keeps the composition and its conversions)."""
    dt = data.dtype if isinstance(data, torch.Tensor) else {"float32": torch.float32, "float64": torch.float64}.get(np.asarray(data).dtype.name)
    return dt if dt in (torch.float32, torch.float64) else None


def _three_axis_info(a, dims, spacing_tol, shift, window, true_phase, prefix):
    """Per transform dim of a three-axis call what the composition's two stages derive (the last two listed dims, then the first): spacing, lag, a descending
    coordinate, the window vector, the output coordinate and its name."""
    ca = _analyze(a, spacing_tol, dims[-2:], None, shift, None, window, true_phase, False, prefix, None)
    cb = _analyze(a, spacing_tol, [dims[0]], None, shift, None, window, true_phase, False, prefix, None)
    info = {}
    for c in (ca, cb):
        for i, d in enumerate(c.dim):
            info[d] = dict(dx=c.delta_x[i], lag=c.lag_x[i], rev=c.reversed[i], win=None if c.windows is None else c.windows[i],
                           name=c.swap[d], coord=c.new_coords[c.swap[d]])
    return info


def _three_axis_labels(da, dims, order, info, true_phase, out):
    """The composition's labels on the fused result: dims, the stages' coordinates in their order, spacing and (true_phase) direct_lag."""
    final = [info[d]["name"] if d in info else d for d in da.dims]
    coords = {k: v._clone(k) for k, v in da.coords.items() if k not in dims}
    for d in order:
        cv = info[d]["coord"]
        attrs = dict(cv.attrs)
        if true_phase:
            attrs["direct_lag"] = info[d]["lag"]  # xrft.py:469 (not _direct_lag_attrs: the lags of two contexts, in the stages' order)
        coords[info[d]["name"]] = Coordinate(cv.dims, cv.values, attrs, info[d]["name"])
    return DataArray(out.reshape(tuple(da.shape)), final, coords, None, None)


def _three_axis_front(da, da2, dims, spacing_tol, shift, detrend_, window, true_phase, chunks_to_segments, prefix):
    """What the fused three-axis routes ask before their plans: the per-dim info (_three_axis_info) of real float32 / float64 data whose three transform dims are the
    trailing three axes (any order in ``dim``) -- or None where the routes do not apply (the caller composes as before): other dims, chunks_to_segments, extents
    beyond the 32-bit indices of a slab, two fields that differ in dims, shape or dtype, a descending coordinate (FLIP)."""
    if len(dims) != 3 or len(da.dims) < 3 or set(dims) != set(da.dims[-3:]) or chunks_to_segments or detrend_ not in (None, "constant", "linear"):
        return None
    if da2 is not None and (tuple(da2.dims) != tuple(da.dims) or tuple(da2.shape) != tuple(da.shape)):
        return None
    nt, ny, nx = (da.sizes[d] for d in da.dims[-3:])
    nxh = nx // 2 + 1
    if min(nt, ny, nx) < 2 or ny * nx > (1 << 31) - 1 or nt * ny * nxh > (1 << 31) - 1 or ny * nxh > (1 << 30):
        return None
    if _real_dtype(da.data) is None or (da2 is not None and _real_dtype(da2.data) != _real_dtype(da.data)):
        return None
    info = _three_axis_info(da, dims, spacing_tol, shift, window, true_phase, prefix)
    if any(v["rev"] for v in info.values()):
        return None
    return info


def _three_axis_run(da, da2, dims, info, detrend_, shift, true_phase, kw2):
    """The two plans of a fused three-axis route: detrend as before, the two-axis plan over the last two axes in memory with the HALF spectrum as its complex output
    (XRFTHIP_HALF_X: 4 bytes per point written instead of 8), then ONE plan (xrfthip_desc.herm_ny / herm_nx, csrc/fasth.h) that transforms along the first of the
    three and writes the full shifted result, the redundant half from the Hermitian twin.  ``kw2``: what the second plan's descriptor has of its caller -- out_mode,
    scale, output-phase tables, flags beyond axis, shifts and ifftshift.  Returns the labelled result, or None: a length either stage does not take."""
    pt, py, px = da.dims[-3:]
    nt, ny, nx = (da.sizes[d] for d in (pt, py, px))
    nxh = nx // 2 + 1
    cur, cur2 = da, da2
    if detrend_ is not None:
        cur = from_any(detrend(da, dims, detrend_))
        cur2 = None if da2 is None else from_any(detrend(da2, dims, detrend_))
    t = _to_device(cur.data).contiguous()
    t2 = None if cur2 is None else _to_device(cur2.data).contiguous()
    batch = t.numel() // (nt * ny * nx)
    ish = (_lib.ISHIFT_Y | _lib.ISHIFT_X) if true_phase else 0  # (the reference ifftshifts the windowed input, xrft.py:436-441)
    kw1 = dict(ndim=2, batch=batch * nt, ny=ny, nx=nx, dtype=t.dtype, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=_lib.HALF_X | ish, scale=1.0,
               window_y=info[py]["win"], window_x=info[px]["win"], phase_y=None, phase_x=None)
    kw2 = dict(kw2, ndim=2, batch=batch, ny=nt, nx=ny * nxh, dtype=engine._CPLX_OF[t.dtype], detrend=_lib.DETREND_NONE,
               flags=kw2.get("flags", 0) | _lib.AXIS_Y | ((_lib.SHIFT_Y | _lib.SHIFT_X) if shift else 0) | (_lib.ISHIFT_Y if true_phase else 0),
               window_y=info[pt]["win"], window_x=None, herm_ny=ny, herm_nx=nx)
    try:
        plan1 = _get_plan(**kw1)
        plan2 = _get_plan(**kw2)  # (the newest plan of the call: describe() shows [fasth])
    except _lib.XrftHipError as e:
        if e.status != _lib.UNSUPPORTED_LENGTH:
            raise
        return None
    h, _ = plan1.execute(t)
    h2 = None if t2 is None else plan1.execute(t2)[0]
    del t, t2, cur, cur2  # (a detrended copy is not alive beside the result)
    out, _ = plan2.execute(h.reshape(batch, nt, ny * nxh), None if h2 is None else h2.reshape(batch, nt, ny * nxh))
    del h, h2
    return _three_axis_labels(da, dims, [dims[-2], dims[-1], dims[0]], info, true_phase, out)  # (the stages of the composition: their labels, in their order)


def _fft_3d_fused(da, dims, spacing_tol, shift, detrend_, window, true_phase, true_amplitude, chunks_to_segments, prefix):
    """The frequency-wavenumber transform -- ``fft(da, dim=["time", "y", "x"])`` -- on the fused route (_three_axis_front, _three_axis_run): the last plan is the
    field form (XRFTHIP_HERM_FIELD), the complex transform itself; it writes the redundant half as the conjugate of the Hermitian twin, each element times the
    true-phase factors of its OWN indices (the twin of a sample at a Nyquist index does not carry the conjugate factor).  20 bytes per point behind the detrend
    instead of the composition's 28, half its peak intermediate memory.  None where the route does not apply."""
    info = _three_axis_front(da, None, dims, spacing_tol, shift, detrend_, window, true_phase, chunks_to_segments, prefix)
    if info is None:
        return None
    pt, py, px = da.dims[-3:]
    scale = math.prod([info[d]["dx"] for d in (dims[-2], dims[-1], dims[0])]) if true_amplitude else 1.0  # xrft.py:471-472, in the order of the composition's stages
    ph = {d: None for d in dims}
    if true_phase:  # xrft.py:462-469 -- indexed by unshifted frequency, as _flags_tables builds them
        for d in dims:  # (memoised: the same table object on every call of a shape, identified by its key where the plan is looked up)
            n, dx, lag = da.sizes[d], info[d]["dx"], info[d]["lag"]
            ph[d] = _memoised(("phase3", int(n), float(dx), float(lag)), lambda: _ro(np.exp(-1j * 2.0 * np.pi * np.fft.fftfreq(n, dx) * lag)))
    return _three_axis_run(da, None, dims, info, detrend_, shift, true_phase,
                           dict(out_mode=_lib.OUT_COMPLEX, flags=_lib.HERM_FIELD, scale=float(scale), phase_y=ph[pt], phase_x=ph[py], phase_hx=ph[px]))


def _spectrum_3d_fused(da, da2, dims, scaling, window_correction, true_phase, kw):
    """Frequency-wavenumber spectra -- ``power_spectrum(da, dim=["time", "y", "x"])``, ``cross_spectrum`` of two such fields -- on the fused route (_three_axis_front,
    _three_axis_run): the last plan takes |F|^2 or F1 conj(F2); the lags' phase factors cancel in the product.  The composition moved ~48 bytes per point behind the
    first stage's intermediate and held two full complex arrays; this moves ~12 and holds the half spectrum.  None where the route does not apply, and for two fields
    that differ in spacing or lag (a true-phase factor: the twin of a Nyquist sample does not carry its conjugate)."""
    args = (dims, kw["spacing_tol"], kw["shift"], kw["detrend"], kw["window"], true_phase, kw["chunks_to_segments"], kw["prefix"])
    info = _three_axis_front(da, da2, *args)
    if info is None or any("spacing" not in v["coord"].attrs for v in info.values()):
        return None
    amp = math.prod([info[d]["dx"] for d in (dims[-2], dims[-1], dims[0])]) ** 2
    if da2 is not None:
        info2 = _three_axis_front(da2, None, *args)
        if info2 is None or any(info[d]["dx"] != info2[d]["dx"] or info[d]["lag"] != info2[d]["lag"] for d in dims):
            return None
    scale = amp * _nd_scale(da, dims, kw["window"], scaling, window_correction, [float(info[d]["coord"].attrs["spacing"]) for d in dims])
    return _three_axis_run(da, da2, dims, info, kw["detrend"], kw["shift"], true_phase,
                           dict(out_mode=_lib.OUT_POWER if da2 is None else _lib.OUT_CROSS, scale=float(scale), phase_y=None, phase_x=None))


def _spectrum_nd(da, da2, dims, real_dim, scaling, window_correction, true_phase, kwargs, one_at_a_time=False):
    """power_spectrum / cross_spectrum over more than two axes: N-D transform(s), then the elementwise tail."""
    kw, scaling, real_dim = _spectrum_keywords(kwargs, scaling, real_dim, warn=False)
    if _FUSE_THREE_AXES and real_dim is None and not one_at_a_time:
        fused = _spectrum_3d_fused(da, da2, dims, scaling, window_correction, true_phase, kw)
        if fused is not None:
            return fused
    f1 = _fft_nd(da, dims, kw["spacing_tol"], real_dim, kw["shift"], kw["detrend"], kw["window"], true_phase, True,
                 kw["chunks_to_segments"], kw["prefix"], one_at_a_time)
    f2 = None
    if da2 is not None:
        f2 = _fft_nd(da2, dims, kw["spacing_tol"], real_dim, kw["shift"], kw["detrend"], kw["window"], true_phase, True,
                     kw["chunks_to_segments"], kw["prefix"], one_at_a_time)
        if tuple(f1.dims) != tuple(f2.dims):
            raise ValueError("The two datasets have different dimensions")
    new = [_freq_name(d, kw["prefix"]) for d in dims]
    scale = _nd_scale(da, dims, kw["window"], scaling, window_correction, [float(f1[n].attrs["spacing"]) for n in new])
    a = _to_device(f1.data).contiguous()
    b = None
    if f2 is not None:
        b = _to_device(f2.data).contiguous()
        if b.dtype != a.dtype:
            dt = torch.promote_types(a.dtype, b.dtype)
            a, b = a.to(dt), b.to(dt)
    if real_dim is not None:  # xrft.py:673-682: the kept half of the real axis counts twice, except k = 0 and Nyquist
        out = engine.spectrum_tail_axis(a, b, scale, f1.get_axis_num(new[-1]), da.sizes[real_dim] % 2 == 0)
    else:
        out = engine.spectrum_tail(a, b, scale)
    return DataArray(out, f1.dims, f1.coords, None, None)


# ------------------------------------------------------------------------------------------------------
# public API
# ------------------------------------------------------------------------------------------------------
def _refuse_nonfinite(c):
    """A least-squares line along ONE axis is scipy.signal.detrend in the reference (detrend.py:64-71), which refuses input that is not finite: the same refusal
    here.  The price is one pass over the input and a device-to-host synchronisation per call with THIS detrend (not timed yet: profiles/r13_nonfinite.txt); the other
    detrends and every transform let a NaN through, into its own transform alone.  Called before a plan is looked for, so the fallbacks of an unsupported length
    are covered; transforms over more than two dims never take a one-axis line."""
    if c.detrend == _lib.DETREND_LINEAR and len(c.dim) == 1:
        t = c.da.data
        if not (bool(np.isfinite(t).all()) if isinstance(t, np.ndarray) else bool(torch.isfinite(t).all())):
            raise ValueError("array must not contain infs or NaNs")


def fft(da, spacing_tol=1e-3, dim=None, real_dim=None, shift=True, detrend=None, window=None, true_phase=True,
        true_amplitude=True, chunks_to_segments=False, prefix="freq_", real=None):
    """Discrete Fourier transform of ``da`` along ``dim`` (reference: xrft/xrft.py:307-476; same arguments)."""
    src = da
    da = from_any(da)
    nd = _nd_dims(da, dim, real_dim, real)
    if nd is not None:
        if _FUSE_THREE_AXES and real_dim is None and real is None:
            fused = _fft_3d_fused(da, nd, spacing_tol, shift, detrend, window, true_phase, true_amplitude, chunks_to_segments, prefix)
            if fused is not None:
                return to_like(fused, src)
        return to_like(_fft_nd(da, nd, spacing_tol, real_dim if real is None else real, shift, detrend, window,
                               true_phase, true_amplitude, chunks_to_segments, prefix), src)
    c = _analyze(da, spacing_tol, dim, real_dim, shift, detrend, window, true_phase, chunks_to_segments, prefix, real)
    _refuse_nonfinite(c)
    scale = math.prod(c.delta_x) if true_amplitude else 1.0  # xrft.py:471-472 (math.prod: the same left-to-right product as np.prod of a short list, a tenth of its call time)
    try:
        out, _, other = _execute(c, c.da, _lib.OUT_COMPLEX, scale)
    except _UnsupportedLength:
        if chunks_to_segments:
            raise
        daw, wide = _wide(da)
        return to_like(_narrow(_fft_nd(daw, _two_dims(da, dim, real_dim, real), spacing_tol, real_dim if real is None else real, shift, detrend, window,
                                       true_phase, true_amplitude, False, prefix, one_at_a_time=True), wide), src)
    return to_like(_label_output(c, c.da, out, other, _direct_lag_attrs(c) if c.true_phase else None), src)  # xrft.py:469


def dft(da, dim=None, true_phase=False, true_amplitude=False, **kwargs):
    """Deprecated alias of ``fft`` with numpy-like defaults (xrft/xrft.py:237-250)."""
    warnings.warn("This function has been renamed and will disappear in the future. Please use `fft` instead",
                  FutureWarning)
    return fft(da, dim=dim, true_phase=true_phase, true_amplitude=true_amplitude, **kwargs)


def detrend(da, dim, detrend_type="constant"):
    """Remove the mean or the least-squares line / plane over ``dim`` (xrft/detrend.py:11-97)."""
    src = da
    da = from_any(da)
    dim = _dim_list(da, dim)
    if detrend_type not in ["constant", "linear", None]:
        raise NotImplementedError("%s is not a valid detrending option. Valid options are: 'constant','linear', "
                                  "or None." % detrend_type)
    if detrend_type is None:
        return src
    if detrend_type == "linear" and len(dim) > 3:
        raise NotImplementedError("Only 1D, 2D, and 3D detrending are implemented so far.")
    axes = [da.get_axis_num(d) for d in dim]
    t = _to_device(da.data)
    if detrend_type == "linear" and len(dim) == 1 and not bool(torch.isfinite(t).all()):  # (scipy.signal.detrend's refusal, detrend.py:64-71; _refuse_nonfinite)
        raise ValueError("array must not contain infs or NaNs")
    dim = [d for _, d in sorted(zip(axes, dim))]  # memory order: the fit does not depend on the order of the axes
    other = [d for d in da.dims if d not in dim]
    order = other + dim
    kind = _lib.DETREND_CONSTANT if detrend_type == "constant" else _lib.DETREND_LINEAR
    ax_sorted = sorted(axes)
    if (len(dim) <= 2 and ax_sorted[-1] != len(da.dims) - 1 and ax_sorted == list(range(ax_sorted[0], ax_sorted[0] + len(dim)))
            and int(np.prod(t.shape[ax_sorted[-1] + 1:], dtype=np.int64)) > 1):
        # one or two adjacent axes that are not the trailing ones: detrended where they lie (xrfthip_detrend_inner), no transposed copies
        # -- unless the extents exceed what the library carries in 32 bits, or its scratch would outgrow the array (None: transposing path)
        out = engine.detrend_inner(t.contiguous(), ax_sorted[0], len(dim), kind)
        if out is not None:
            return to_like(DataArray(out, da.dims, da.coords, da.name, da.attrs), src)
    if tuple(order) != tuple(da.dims):
        t = t.permute([da.get_axis_num(d) for d in order])
    t = t.contiguous()
    if len(dim) > 3 or (len(dim) == 3 and detrend_type == "constant"):
        # the mean over any number of trailing axes is the mean of the flattened block
        nblk = int(np.prod([da.sizes[d] for d in dim]))
        out = engine.detrend(t.reshape(-1, nblk), 1, kind).reshape(t.shape)
    else:
        out = engine.detrend(t, len(dim), kind)
    if tuple(order) != tuple(da.dims):
        out = out.permute([order.index(d) for d in da.dims])
    return to_like(DataArray(out, da.dims, da.coords, da.name, da.attrs), src)


def _spectrum_keywords(kwargs, scaling, real_dim, warn):
    """(the keywords that reach ``fft`` with their defaults, scaling, real_dim) of a spectrum call (xrft.py:718-734); an unknown keyword is refused as fft refuses
    it.  ``warn``: the one- and two-axis calls warn on ``real`` and ``density`` and let a ``real`` that is given override ``real_dim`` even as None; the calls over
    more axes do neither (a ``real`` of None is no flag there)."""
    if ("real" in kwargs) if warn else (kwargs.get("real") is not None):  # xrft.py:728-730 (`real` stays in kwargs and reaches fft as well)
        real_dim = kwargs.get("real")
        if warn:
            warnings.warn(_real_flag_warning, FutureWarning)
    if "density" in kwargs:  # xrft.py:718-726
        density = kwargs.pop("density")
        if warn:
            warnings.warn("density flag will be deprecated in future version of xrft and replaced by scaling flag. "
                          'density=True should be replaced by scaling="density" and density=False will not be '
                          "maintained.\nscaling flag is ignored !", FutureWarning)
        scaling = "density" if density else "false_density"
    kw = dict(spacing_tol=1e-3, shift=True, detrend=None, window=None, chunks_to_segments=False, prefix="freq_", real=None)
    for k in ("true_amplitude", "true_phase"):
        kwargs.pop(k, None)  # overridden by the reference (xrft.py:732-734, 814)
    unknown = set(kwargs) - set(kw)
    if unknown:
        raise TypeError(f"fft() got an unexpected keyword argument {sorted(unknown)[0]!r}")
    kw.update(kwargs)
    return kw, scaling, real_dim


def _spectrum(da, da2, dim, real_dim, scaling, window_correction, true_phase, kwargs, iso=None):
    kw, scaling, real_dim = _spectrum_keywords(kwargs, scaling, real_dim, warn=True)
    c = _analyze(da, kw["spacing_tol"], dim, real_dim, kw["shift"], kw["detrend"], kw["window"], true_phase,
                 kw["chunks_to_segments"], kw["prefix"], kw["real"])
    _refuse_nonfinite(c)
    c2 = None
    amp = math.prod(c.delta_x) ** 2
    if da2 is not None:
        c2 = _analyze(da2, kw["spacing_tol"], dim, real_dim, kw["shift"], kw["detrend"], kw["window"], true_phase,
                      kw["chunks_to_segments"], kw["prefix"], kw["real"])
        _refuse_nonfinite(c2)
        if [c.swap.get(d, d) for d in c.rawdims] != [c2.swap.get(d, d) for d in c2.rawdims]:  # xrft.py:819-820
            raise ValueError("The two datasets have different dimensions")
        if c.N != c2.N or not np.allclose(c.delta_x, c2.delta_x, rtol=1e-12):
            raise ValueError("The two datasets have different frequency coordinates (size or spacing)")
        amp = math.prod(c.delta_x) * math.prod(c2.delta_x)
    scale = _spectrum_scale(c, amp, scaling, window_correction, kw["window"])
    flags = _lib.REALDIM_X2 if c.real_dim is not None else 0  # xrft.py:742-743
    mode = _lib.OUT_POWER if da2 is None else _lib.OUT_CROSS
    return c, c2, mode, scale, flags


def power_spectrum(da, dim=None, real_dim=None, scaling="density", window_correction=False, **kwargs):
    """Power spectrum |F(da')|^2 with density / spectrum scaling (xrft/xrft.py:685-750)."""
    src = da
    da = from_any(da)
    nd = _nd_dims(da, dim, real_dim, kwargs.get("real"))
    if nd is not None:
        return to_like(_spectrum_nd(da, None, nd, real_dim, scaling, window_correction, False, dict(kwargs)), src)
    c, _, mode, scale, flags = _spectrum(da, None, dim, real_dim, scaling, window_correction, False, dict(kwargs))
    try:
        out, _, other = _execute(c, c.da, mode, scale, extra_flags=flags)
    except _UnsupportedLength:
        daw, wide = _wide(da)
        return to_like(_narrow(_spectrum_nd(daw, None, _two_dims(da, dim, real_dim, kwargs.get("real")), real_dim, scaling, window_correction, False,
                                            dict(kwargs), one_at_a_time=True), wide), src)
    return to_like(_label_output(c, c.da, out, other), src)


def cross_spectrum(da1, da2, dim=None, real_dim=None, scaling="density", window_correction=False, true_phase=True,
                   **kwargs):
    """Cross spectrum F(da1') conj(F(da2')) (xrft/xrft.py:753-835)."""
    src = da1
    da1, da2 = from_any(da1), from_any(da2)
    nd = _nd_dims(da1, dim, real_dim, kwargs.get("real"))
    if nd is not None:
        return to_like(_spectrum_nd(da1, da2, nd, real_dim, scaling, window_correction, true_phase, dict(kwargs)), src)
    c, c2, mode, scale, flags = _spectrum(da1, da2, dim, real_dim, scaling, window_correction, true_phase, dict(kwargs))
    try:
        return to_like(_cross_result(c, c2, mode, scale, flags), src)
    except _UnsupportedLength:
        d1w, wide1 = _wide(da1)
        d2w, wide2 = _wide(da2)  # (narrowed back only when BOTH were widened: float32 x float64 stays the promoted complex128, whatever the order)
        return to_like(_narrow(_spectrum_nd(d1w, d2w, _two_dims(da1, dim, real_dim, kwargs.get("real")), real_dim, scaling, window_correction, true_phase,
                                            dict(kwargs), one_at_a_time=True), wide1 and wide2), src)


# ------------------------------------------------------------------------------------------------------
# Averaged spectra: power_spectrum(...).mean(mean_dim) / cross_spectrum(...).mean(mean_dim) with the mean taken inside the last pass of the plan
# (xrfthip_desc.mean_batch): what the reference's users do with a batch of spectra (its Parseval, chunk and MITgcm notebooks end every spectral example with a
# .mean over time steps or over the <dim>_segment dims of chunks_to_segments=True) without the spectra of the single slabs ever reaching memory.
# ------------------------------------------------------------------------------------------------------
def _check_mean_dims(names, dims):
    for d in names:
        if d not in dims:
            raise ValueError(f"mean_dim {d!r} is not a non-transform dimension of the result (those are {list(dims)})")


def _mean_fused(c, c2, mode, scale, flags, names, other):
    """The labelled mean from ONE plan with mean_batch, or None where the call composes: the plan declines it (another kernel family, float64), real_dim, one
    transform axis, mean dims that are not the innermost batch dims of the arranged (batch, ny, nx) array, a kept coordinate that spans a transform dim (the
    composition's validating constructor answers that)."""
    cda = c.da
    k = len(set(names))
    m = math.prod(cda.sizes[d] for d in set(names))
    if len(c.dim) != 2 or flags or c.real_dim is not None or set(other[len(other) - k:]) != set(names) or m <= 1 or math.prod(cda.shape) == 0:
        return None
    if any(d in c.dim for n, v in cda.coords.items() if n not in c.dim for d in v.dims):
        return None
    try:
        out, _, _ = _execute(c, cda, mode, scale, da2=None if c2 is None else c2.da, c2=c2, mean_batch=m)
    except _MeanDeclined:
        return None
    # without the averaged dims and the coordinates that span them (DataArray.mean drops those); direct_lag as _cross_result
    return _label_output(c, cda, out, other, _direct_lag_attrs(c) if c2 is not None and c.true_phase else None, dropped=names)


def _mean_spectrum(da, da2, names, dim, real_dim, scaling, window_correction, true_phase, kwargs):
    """The labelled mean of a one- or two-axis spectrum from ONE host analysis of the call -- fused where a plan takes it, else the plain call's execution and
    .mean() -- or None: more than two transform axes, the deprecated ``real`` flag, lengths only the one-axis-at-a-time composition serves (the caller goes through
    the public function)."""
    if "real" in kwargs or _nd_dims(da, dim, real_dim, None) is not None:
        return None
    c, c2, mode, scale, flags = _spectrum(da, da2, dim, real_dim, scaling, window_correction, true_phase, dict(kwargs))
    other = [d for d in c.da.dims if d not in c.dim]
    _check_mean_dims(names, other)
    fused = _mean_fused(c, c2, mode, scale, flags, names, other)
    if fused is not None:
        return fused
    try:
        if c2 is None:
            out, _, oth = _execute(c, c.da, mode, scale, extra_flags=flags)
            full = _label_output(c, c.da, out, oth)
        else:
            full = _cross_result(c, c2, mode, scale, flags)
    except _UnsupportedLength:
        return None
    return full.mean(names)


def mean_power_spectrum(da, mean_dim, dim=None, real_dim=None, scaling="density", window_correction=False, **kwargs):
    """``power_spectrum(da, dim, ...).mean(mean_dim)`` -- same dims, coordinates, attrs and name -- with the mean taken inside the last pass where a plan does that
    (float32 / float16 / bfloat16 fields, two transform axes; ``mean_dim`` all the other dims or the innermost of them; the shape classes whose mean form measured
    faster than the composition, docs/TUNING.md XRFTHIP_MEAN_ALL): the result, and what the call allocates, shrink by the number of spectra averaged.  ``mean_dim``: a
    name or a list of names of non-transform dims of the result, the ``<dim>_segment`` dims of ``chunks_to_segments=True`` included.  Every other call runs the plain
    plan and ``.mean``."""
    src = da
    da = from_any(da)
    names = [mean_dim] if isinstance(mean_dim, str) else list(mean_dim)
    res = _mean_spectrum(da, None, names, dim, real_dim, scaling, window_correction, False, kwargs)
    if res is None:
        ps = power_spectrum(da, dim=dim, real_dim=real_dim, scaling=scaling, window_correction=window_correction, **kwargs)
        _check_mean_dims(names, ps.dims)
        res = ps.mean(names)
    return to_like(res, src)


def mean_cross_spectrum(da1, da2, mean_dim, dim=None, real_dim=None, scaling="density", window_correction=False, true_phase=True, **kwargs):
    """``cross_spectrum(da1, da2, dim, ...).mean(mean_dim)``, the mean taken inside the last pass where a plan does that (see ``mean_power_spectrum``)."""
    src = da1
    da1, da2 = from_any(da1), from_any(da2)
    names = [mean_dim] if isinstance(mean_dim, str) else list(mean_dim)
    res = _mean_spectrum(da1, da2, names, dim, real_dim, scaling, window_correction, true_phase, kwargs)
    if res is None:
        cs = cross_spectrum(da1, da2, dim=dim, real_dim=real_dim, scaling=scaling, window_correction=window_correction, true_phase=true_phase, **kwargs)
        _check_mean_dims(names, cs.dims)
        res = cs.mean(names)
    return to_like(res, src)


def _coherence_name(da1, da2):
    return "{}_{}_coherence".format(da1.name, da2.name) if da1.name and da2.name else None


def _coherence_result(cs, p1, p2, da1, da2):
    """The labelled coherence of a mean cross spectrum and the two mean power spectra: the division is the library's (xrfthip_coherence), in the cross spectrum's
    precision, under its labels."""
    cross = _to_device(cs.data)
    real_dt = torch.float32 if cross.dtype == torch.complex64 else torch.float64
    res = DataArray(engine.coherence(cross.contiguous(), _to_device(p1.data).to(real_dt).contiguous(), _to_device(p2.data).to(real_dt).contiguous()), cs.dims, cs.coords, None, None)
    res.name = _coherence_name(da1, da2)
    return res


def coherence(da1, da2, mean_dim, dim=None, real_dim=None, scaling="density", window_correction=False, true_phase=True, **kwargs):
    """Magnitude-squared coherence ``|<F1 conj F2>|^2 / (<|F1|^2> <|F2|^2>)``, ``<.>`` the mean over ``mean_dim`` (time steps, or the ``<dim>_segment`` dims of
    ``chunks_to_segments=True``): what a batch of cross spectra is averaged for, the other half of the pair ``cross_phase`` begins.  The arguments are those of
    ``mean_cross_spectrum`` and so are dims, coordinates and coordinate attrs of the result; the value does not depend on ``scaling``, ``window_correction`` or
    ``true_phase`` (they cancel), which are accepted so that the call mirrors the cross call.  Real data: float32, or float64 for float64 input; no clamp (a value
    may exceed 1 by rounding).  Where a plan takes the call (the conditions of ``mean_cross_spectrum``'s fused route, two-pass float32 slabs) ONE row pass sums the
    cross spectrum and both powers (XRFTHIP_OUT_COHERENCE) and one real result is written; every other call composes ``mean_cross_spectrum`` and
    ``mean_power_spectrum`` of each field and divides in the library (xrfthip_coherence).  Fewer than two spectra averaged: ValueError (the coherence of one
    spectrum is 1 everywhere)."""
    src = da1
    da1, da2 = from_any(da1), from_any(da2)
    names = [mean_dim] if isinstance(mean_dim, str) else list(mean_dim)
    kw = dict(dim=dim, real_dim=real_dim, scaling=scaling, window_correction=window_correction)

    def count(sizes):
        if math.prod(sizes[d] for d in set(names)) < 2:
            raise ValueError(f"coherence needs at least two spectra to average: mean_dim {names} holds {math.prod(sizes[d] for d in set(names))} (of one spectrum it is 1 everywhere)")

    res = None
    if "real" in kwargs or _nd_dims(da1, dim, real_dim, None) is not None:  # (no one-analysis route: the public functions, as mean_cross_spectrum does there)
        full = from_any(cross_spectrum(da1, da2, true_phase=true_phase, **kw, **kwargs))
        _check_mean_dims(names, full.dims)
        count(full.sizes)
        cs = full.mean(names)
        p1, p2 = (from_any(power_spectrum(d, **kw, **kwargs)).mean(names) for d in (da1, da2))
    else:
        c, c2, _, scale, flags = _spectrum(da1, da2, dim, real_dim, scaling, window_correction, true_phase, dict(kwargs))
        other = [d for d in c.da.dims if d not in c.dim]
        _check_mean_dims(names, other)
        count(c.da.sizes)
        res = _mean_fused(c, c2, _lib.OUT_COHERENCE, scale, flags, names, other)
        if res is None:
            cs = from_any(mean_cross_spectrum(da1, da2, names, true_phase=true_phase, **kw, **kwargs))
            p1, p2 = (from_any(mean_power_spectrum(d, names, **kw, **kwargs)) for d in (da1, da2))
    if res is not None:
        res.name = _coherence_name(da1, da2)
        return to_like(res, src)
    return to_like(_coherence_result(cs, p1, p2, da1, da2), src)


# ------------------------------------------------------------------------------------------------------
# Welch spectra and spectrograms (the spectra of the overlapping segments of a series, averaged or kept): _segments.py, on top of the calls above
# ------------------------------------------------------------------------------------------------------
# The float64 partials of a column plan are twice the float32 result per run (2 GB for a 720 x 1440 grid at nperseg = 256): wider grids run in blocks of columns,
# each a view of the same array (seg_stride > inner), whose plan's workspace stays within this many bytes.  (A starting value: not measured.)  Read here by
# _segments._welch_fused_columns at every call
_WELCH_COLS_WS_CAP = 256 << 20
_WELCH_COLS_ALIGN = 32  # blocks are whole groups of columns (fastw.h, kWCols): every column is summed as in the unblocked call

from ._segments import _welch_segments, fir_filter, istft, multitaper_coherence, multitaper_cross_spectrum, multitaper_power_spectrum, spectrogram, stft, welch_coherence, welch_cross_spectrum, welch_power_spectrum  # noqa: E402,F401


def _cross_result(c, c2, mode, scale, flags):
    out, _, other = _execute(c, c.da, mode, scale, da2=c2.da, c2=c2, extra_flags=flags)
    # the product keeps daft1's coordinates, including their direct_lag attribute (xrft.py:469, 825)
    return _label_output(c, c.da, out, other, _direct_lag_attrs(c) if c.true_phase else None)


def cross_phase(da1, da2, dim=None, true_phase=True, **kwargs):
    """Cross phase arg(F(da1') conj(F(da2'))) in [-pi, pi] (xrft/xrft.py:838-874); the angle is taken in the
    epilogue of the cross-spectrum kernel, the complex cross spectrum is never written."""
    src = da1
    da1, da2 = from_any(da1), from_any(da2)
    kw = dict(kwargs)
    real_dim = kw.pop("real_dim", None)
    scaling = kw.pop("scaling", "density")
    window_correction = kw.pop("window_correction", False)
    c, c2, mode, scale, flags = _spectrum(da1, da2, dim, real_dim, scaling, window_correction, true_phase, kw)
    try:
        cp = _cross_result(c, c2, _lib.OUT_PHASE, abs(scale) if scale != 0 else 1.0, flags & ~_lib.REALDIM_X2)
    except _UnsupportedLength:
        # a length no fused plan takes (numpy.fft takes any): the angle of the cross spectrum, which has its own way round
        # (one axis at a time, Bluestein through global memory) -- what the reference does literally (xrft.py:871-874)
        cs = from_any(cross_spectrum(da1, da2, dim=dim, real_dim=real_dim, scaling=scaling, window_correction=window_correction,
                                     true_phase=true_phase, **kw))
        cp = DataArray(engine.angle(_to_device(cs.data)), cs.dims, cs.coords, None, None)
    if da1.name and da2.name:
        cp.name = "{}_{}_phase".format(da1.name, da2.name)
    return to_like(cp, src)


def _iso_spectrum(da, da2, spacing_tol, dim, shift, detrend_, scaling, window, window_correction, nfactor, truncate,
                  kwargs):
    if "density" in kwargs:  # xrft.py:1072-1074
        density = kwargs.pop("density")
        scaling = "density" if density else "false_density"
    if dim is None:
        dim = da.dims
        if da2 is not None and tuple(dim) != tuple(da2.dims):
            raise ValueError("The two datasets have different dimensions")
    if len(dim) != 2:
        raise ValueError("The Fourier transform should be two dimensional")
    dim = list(dim)
    kw = dict(kwargs, spacing_tol=spacing_tol, shift=shift, detrend=detrend_, window=window)
    true_phase = kw.pop("true_phase", True) if da2 is not None else False
    real_dim = kw.pop("real_dim", None)
    c, c2, mode, scale, flags = _spectrum(da, da2, dim, real_dim, scaling, window_correction, true_phase, kw)
    fftdim = ["freq_" + d for d in dim]  # xrft.py:1093 (hard-coded prefix, as in the reference)
    for f in fftdim:
        if f not in c.new_coords:
            raise KeyError(f)
    # bin map on the engine's (ky, kx) grid in UNSHIFTED index order; radii are order-independent
    ky = c.k_unshifted[c.dim.index(c.ydim)]
    kx = c.k_unshifted[c.dim.index(c.xdim)]
    kk = c.new_coords[fftdim[1]].values
    ll = c.new_coords[fftdim[0]].values
    # reference bins over (fftdim[1], fftdim[0]) of the shifted coordinates: the edges depend only on min/max of the same set
    # of radii; kr (a per-bin mean of the same multiset) is summed in the reference's cell order to match it bit for bit
    codes_yx, kr, nb, bkey = _radial_bins(ky, kx, nfactor, (bool(c.shift), bool(c.shift), fftdim[1] == c.swap[c.xdim]))
    iso_cfg = {"binmap": codes_yx, "nbins": nb, "binmap_key": bkey}
    da_in = da
    da = c.da
    try:
        out, iso, other = _execute(c, da, mode, scale, da2=None if c2 is None else c2.da, c2=c2, iso=iso_cfg,
                                   extra_flags=flags | _lib.ISO | _lib.NO_SPECTRUM_OUT)
    except _UnsupportedLength:
        # no two-axis plan for these lengths: what the reference does literally (xrft.py:1085-1095, 1177-1187) -- the full spectrum
        # (its axes transformed one at a time), then isotropize
        skw = dict(dim=dim, real_dim=real_dim, scaling=scaling, window_correction=window_correction, **kw)
        if da2 is None:
            full = power_spectrum(da_in, **skw)
        else:
            full = cross_spectrum(da_in, da2, true_phase=true_phase, **skw)
        return from_any(isotropize(full, fftdim, nfactor=nfactor, truncate=truncate, complx=da2 is not None))
    vals = iso.reshape([da.sizes[d] for d in other] + [nb])
    if truncate:  # dropna inspects the DATA values (xrft.py:1007-1008): the only case that needs them on the host
        vals = vals.cpu().numpy()
    kr, vals = _finish_iso(kr, kk, ll, truncate, vals)
    coords = {cn: cv for cn, cv in da.coords.items() if not (set(cv.dims) & set(dim))}
    coords["freq_r"] = Coordinate(("freq_r",), kr, None, "freq_r")
    return DataArray(vals, other + ["freq_r"], coords, None, None)


def isotropic_power_spectrum(da, spacing_tol=1e-3, dim=None, shift=True, detrend=None, scaling="density",
                             window=None, window_correction=False, nfactor=4, truncate=False, **kwargs):
    """Isotropic (radially binned) power spectrum (xrft/xrft.py:1013-1095); spectrum and bin-sum are fused on
    the device, the full 2-D spectrum is never written."""
    src = da
    da = from_any(da)
    return to_like(_iso_spectrum(da, None, spacing_tol, dim, shift, detrend, scaling, window, window_correction,
                                 nfactor, truncate, dict(kwargs)), src)


def isotropic_cross_spectrum(da1, da2, spacing_tol=1e-3, dim=None, shift=True, detrend=None, scaling="density",
                             window=None, window_correction=False, nfactor=4, truncate=False, **kwargs):
    """Isotropic cross spectrum (xrft/xrft.py:1098-1187)."""
    src = da1
    da1, da2 = from_any(da1), from_any(da2)
    return to_like(_iso_spectrum(da1, da2, spacing_tol, dim, shift, detrend, scaling, window, window_correction,
                                 nfactor, truncate, dict(kwargs)), src)


def fit_loglog(x, y):
    """Least-squares line in log2-log2 space (xrft/xrft.py:1190-1214)."""
    p = np.polyfit(np.log2(x), np.log2(y), 1)
    y_fit = 2 ** (np.log2(x) * p[0] + p[1])
    return y_fit, p[0], p[1]
