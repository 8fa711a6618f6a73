"""The segment surface of the call API: Welch spectra (welch_power_spectrum, welch_cross_spectrum, welch_coherence) and spectrograms (spectrogram, stft) -- the spectra
of the overlapping segments of a series, averaged or kept -- the synthesis that rebuilds the series from the kept ones (istft), FIR filtering along a dim by overlap-save (fir_filter), and multitaper spectra of a whole record (multitaper_*).  Fused where a segment plan takes the call (xrfthip_desc.seg_hop: csrc/fastw.h, fastk.h), else composed from
the calls of api.py on the unfolded segments.  api.py re-exports the public names.

This module sits ON TOP of api.py and is imported by it, behind the definitions it uses (`_api.` below: resolved at call time; the two tuning constants
`api._WELCH_COLS_WS_CAP` / `_WELCH_COLS_ALIGN` live there too, where the tests patch them).  Import `xrft_amd` or `xrft_amd.api`, never this module first."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib, engine
from . import api as _api  # (the calls the composed paths and the analysis of ONE segment go through; api.py imports this module behind them)
from ._hostside import _analyze, _direct_lag_attrs, _flags_tables, _get_coordinate_spacing, _label_output, _to_device
from ._plans import _MEAN_REFUSED, _digest, _get_plan, _plan_lock, _ro, _rung
from .padding import _pad_coordinate
from .labeled import Coordinate, DataArray, from_any, to_like

# ------------------------------------------------------------------------------------------------------
# Welch spectra: the mean spectrum of the overlapping segments of a long series (scipy.signal.welch / csd / coherence; the reference's
# power_spectrum(da, dim="time", chunks_to_segments=True, window="hann", detrend="linear").mean("time_segment") with an overlap).  Fused where a plan takes the call
# (xrfthip_desc.seg_hop: the segments read where they lie, no segment's spectrum stored), else composed: the segments unfolded, the public call, .mean.
# ------------------------------------------------------------------------------------------------------
def _welch_args(da, dim, nperseg, noverlap, least=1):
    """(hop, number of segments) after the checks; trailing samples that do not fill a segment are dropped (as scipy.signal.welch does)."""
    if not isinstance(dim, str):
        raise ValueError(f"dim must be the name of ONE dimension (the axis the segments are cut from), not {dim!r}")
    n = da.sizes[dim] if dim in da.dims else da.get_axis_num(dim)
    nperseg = int(nperseg)
    if nperseg < 1 or nperseg > n:
        raise ValueError(f"nperseg = {nperseg} is not in 1 .. {n}, the length of {dim!r}")
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if noverlap < 0 or noverlap >= nperseg:
        raise ValueError(f"noverlap = {noverlap} must be in 0 .. nperseg - 1 = {nperseg - 1}")
    hop = nperseg - noverlap
    m = (n - nperseg) // hop + 1
    if m < least:
        raise ValueError(f"{m} segment(s) of {nperseg} samples fit {dim!r} ({n} samples, hop {hop}): at least {least} are needed")
    return nperseg, hop, m


def _welch_segments(da, dim, nperseg, hop):
    """The labelled array of segments, a VIEW of the device data (tensor.unfold): ``dim`` becomes ``<dim>_segment`` where it lay and the samples of a segment are the
    new last dim ``dim``, whose coordinate is the first ``nperseg`` values of the series' (every segment has the same spacing; the lag is the first segment's)."""
    t = _to_device(da.data)
    ax = da.get_axis_num(dim)
    seg = t.unfold(ax, nperseg, hop)
    dims = list(da.dims)
    dims[ax] = dim + "_segment"
    dims.append(dim)
    coords = {}
    for k, v in da.coords.items():
        if k == dim:
            coords[k] = Coordinate((dim,), np.asarray(v.values)[:nperseg], v.attrs, k)
        elif dim not in v.dims:
            coords[k] = v
    return DataArray(seg, dims, coords, da.name, da.attrs)


def _welch_series(t, ax):
    """(series, samples) float32 device tensor with unit stride along the samples and one pitch between the series, and that pitch: the array itself where ``ax`` is
    the trailing, contiguous axis; else arranged first (one transposed copy: what the column layout of the plan, _welch_columns, did not take)."""
    if ax != t.dim() - 1:
        t = t.movedim(ax, -1)
    if not (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        t = t.contiguous().reshape(-1, t.shape[-1])
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _collapse(sizes, strides):
    """(count, stride) of dims that are ONE run of equally spaced elements (size-1 dims skipped; no dims: (1, 0)), or None."""
    n, st = 1, 0
    for k, v in zip(reversed(sizes), reversed(strides)):  # innermost first: each outer stride is (extent x stride) of what lies inside it
        if k == 1:
            continue
        if n > 1 and v != n * st:
            return None
        if n == 1:
            st = v
        n *= k
    return n, st


def _welch_columns(t, ax, span):
    """The (blocks, samples, columns) view of a float32 device tensor that a column plan reads where it lies (xrfthip_desc.seg_stride), with its block pitch and its
    sample stride -- or None: ``ax`` is the trailing axis, the dims behind it are not one unit-stride run, the dims in front not one pitch, or rows would overlap."""
    if ax == t.dim() - 1 or os.environ.get("XRFTHIP_FASTW_COLS", "1") == "0":  # (the knob of the library, honoured before a cached plan could answer)
        return None
    back = _collapse(t.shape[ax + 1:], t.stride()[ax + 1:])
    front = _collapse(t.shape[:ax], t.stride()[:ax])
    if back is None or front is None:
        return None
    inner, s_in = back
    blocks, pitch = front
    ss = t.stride(ax)
    if (inner > 1 and s_in != 1) or ss < inner or (inner == 1 and ss == 1):  # (unit sample stride: the rows layout, no copy either)
        return None
    if blocks > 1 and pitch < (span - 1) * ss + inner:
        return None
    return torch.as_strided(t, (blocks, t.shape[ax], inner), (pitch if blocks > 1 else t.shape[ax] * ss, ss, 1), t.storage_offset()), (pitch if blocks > 1 else 0), ss


def _segment_kw(c, c2, nperseg, hop, m, mode, scale, flags, keep=False):
    """The keywords of a segment plan (xrfthip_desc.seg_hop; seg_keep: every spectrum kept) but for its batch and strides (_segment_view): flags, window and -- a
    two-field mean only -- the net true-phase table are those of ONE segment's spectrum."""
    fl, win, ph = _flags_tables(c, c.da, None if c2 is None else c2.lag_x, None if c2 is None else c2.reversed)
    return dict(ndim=1, ny=1, nx=nperseg, dtype=torch.float32, out_mode=mode, detrend=c.detrend, flags=fl | flags, scale=float(scale), window_x=win["x"],
                phase_x=ph["x"] if mode == _lib.OUT_CROSS else None, mean_batch=m, seg_hop=hop, seg_keep=int(keep))


def _segment_view(t, ax, span, m, columns):
    """(the view of a float32 device tensor that a segment plan executes on, the descriptor's batch and strides) for series along ``ax`` whose segments span ``span``
    samples.  ``columns``: the (blocks, samples, columns) view read where it lies (inner / seg_stride), or None where the array cannot be described by it
    (_welch_columns); else (series, samples) rows, arranged first where they are not rows already (_welch_series)."""
    if columns:
        v = _welch_columns(t, ax, span)
        if v is None:
            return None
        view, pitch, ss = v
        return view, dict(batch=view.shape[0] * m, inner=view.shape[2], seg_stride=ss, in_stride_batch=int(pitch))
    rows, pitch = _welch_series(t, ax)
    return rows, dict(batch=rows.shape[0] * m, in_stride_batch=int(pitch))


def _segment_plan(kw, extras):
    """The plan of the keywords, or None: "the caller arranges or composes" (XRFTHIP_UNSUPPORTED_LENGTH, remembered)."""
    return _rung(_MEAN_REFUSED, None, dict(kw, **extras))


def _welch_fused_columns(kw, t, t2, ax, span, m):
    """The (blocks, columns, nx_out) result of the column plan(s) on the arrays where they lie, or None: a view that does not collapse, two fields with different
    strides, a length the column layout declines.  Wide grids run in blocks of columns (api._WELCH_COLS_WS_CAP): full blocks share one plan, the tail has one more."""
    v = _segment_view(t, ax, span, m, True)
    if v is None:
        return None
    view, extras = v
    view2 = None
    if t2 is not None:
        if t2.shape != t.shape:
            raise ValueError("The two datasets have different dimensions")
        if t2.stride() != t.stride():
            return None
        view2 = _segment_view(t2, ax, span, m, True)[0]
    blocks, _, inner = view.shape
    per_col = blocks * kw["nx"] * 8 * (1 if t2 is None else 2)  # (one run: what a wide grid gets)
    width = max(_api._WELCH_COLS_ALIGN, _api._WELCH_COLS_WS_CAP // per_col // _api._WELCH_COLS_ALIGN * _api._WELCH_COLS_ALIGN)
    out = None
    for c0 in range(0, inner, width):
        w = min(width, inner - c0)
        plan = _segment_plan(kw, dict(extras, inner=w))
        if plan is None:
            return None  # (the first block: the length is the same for all)
        part = [torch.as_strided(x, (blocks, x.shape[1], w), x.stride(), x.storage_offset() + c0) if w != inner else x for x in (view, view2) if x is not None]
        if w == inner:
            return plan.execute(*part)[0]
        if out is None:
            out = torch.empty((blocks, inner, plan.nx_out), dtype=plan.out_dtype(), device=t.device)
        if blocks == 1:
            plan.execute(*part, out=out[0, c0:c0 + w])
        else:
            out[:, c0:c0 + w] = plan.execute(*part)[0]
    return out


def _welch_fused(c, c2, da, da2, dim, nperseg, hop, m, mode, scale, flags):
    """The (series, nx_out) result of ONE plan with seg_hop, or None where the call composes: float64 / complex / half data, fewer than two segments, a length or a
    flag the plan declines (XRFTHIP_UNSUPPORTED_LENGTH: lengths off the power-of-two table, a descending coordinate's flip), an empty array.  A ``dim`` that is not
    the trailing axis is read where it lies by the column layout of the plan (seg_stride) where the array can be described by it; else it is arranged first."""
    if m < 2 or any(d is not None and _to_device(d.data).dtype != torch.float32 for d in (da, da2)) or math.prod(da.shape) == 0:
        return None
    kw = _segment_kw(c, c2, nperseg, hop, m, mode, scale, flags)
    ax, span = da.get_axis_num(dim), (m - 1) * hop + nperseg
    t, t2 = _to_device(da.data), None if da2 is None else _to_device(da2.data)
    out = _welch_fused_columns(kw, t, t2, ax, span, m)
    if out is not None:
        return out
    t, extras = _segment_view(t, ax, span, m, False)
    if t2 is not None:
        t2, extras2 = _segment_view(t2, ax, span, m, False)
        if t2.shape != t.shape:
            raise ValueError("The two datasets have different dimensions")
        if extras2 != extras:  # (two pitches: both arranged)
            t, t2 = t.contiguous(), t2.contiguous()
            extras = dict(extras, in_stride_batch=t.shape[1])
    plan = _segment_plan(kw, extras)
    if plan is None:
        return None
    out, _ = plan.execute(t, t2)
    return out


def _welch_spectrum(da, da2, dim, nperseg, noverlap, real_dim, scaling, window_correction, true_phase, kwargs, least=1):
    da = from_any(da)
    da2 = None if da2 is None else from_any(da2)
    nperseg, hop, m = _welch_args(da, dim, nperseg, noverlap, least)
    if da2 is not None and (tuple(da2.dims) != tuple(da.dims) or da2.shape != da.shape):
        raise ValueError("The two datasets have different dimensions")
    if real_dim is not None and real_dim != dim:
        raise ValueError(f"real_dim must be {dim!r}, the one transform dimension, or None")
    unknown = set(kwargs) - {"detrend", "window", "shift", "spacing_tol"}
    if unknown:
        raise TypeError(f"got an unexpected keyword argument {sorted(unknown)[0]!r}")
    seg = _welch_segments(da, dim, nperseg, hop)
    seg2 = None if da2 is None else _welch_segments(da2, dim, nperseg, hop)
    sname = dim + "_segment"
    # the labels, the scaling and the tables are those of ONE segment's spectrum
    head = seg.isel(**{sname: 0})
    head2 = None if seg2 is None else seg2.isel(**{sname: 0})
    c, c2, mode, scale, flags = _api._spectrum(head, head2, [dim], real_dim, scaling, window_correction, true_phase, dict(kwargs))
    if c.detrend == _lib.DETREND_LINEAR:  # (_refuse_nonfinite has seen the first segment: the refusal of the composed call covers every segment)
        for d in (da, da2):
            if d is not None:
                _refuse_nonfinite_span(d, dim, (m - 1) * hop + nperseg)
    out = _welch_fused(c, c2, da, da2, dim, nperseg, hop, m, mode, scale, flags)
    if out is not None:
        return _label_output(c, head, out, [d for d in head.dims if d != dim], _direct_lag_attrs(c) if c2 is not None and c.true_phase else None)  # (as _cross_result)
    kw = dict(dim=[dim], real_dim=real_dim, scaling=scaling, window_correction=window_correction, **kwargs)
    full = _api.power_spectrum(seg, **kw) if seg2 is None else _api.cross_spectrum(seg, seg2, true_phase=true_phase, **kw)
    return full.mean(sname)


def welch_power_spectrum(da, dim, nperseg, noverlap=None, real_dim=None, scaling="density", window_correction=False, detrend=None, window=None, shift=True,
                         spacing_tol=1e-3):
    """Welch's estimate of the power spectrum along ``dim``: the series is cut into segments of ``nperseg`` samples that overlap by ``noverlap`` (default
    ``nperseg // 2``; trailing samples that do not fill a segment are dropped, as scipy.signal.welch does), and the result is the mean over the segments of
    ``power_spectrum`` of each -- detrend and window per segment.  Dims: the other dims in their order, then ``freq_<dim>``; coordinates and attrs are those of
    ``power_spectrum`` of the first ``nperseg`` samples.  With ``window_correction=True`` and ``window="hann"`` the values are those of
    ``scipy.signal.welch(..., return_onesided=False)`` after an fftshift (``real_dim=dim``: of ``return_onesided=True``).
    float32 series whose ``nperseg`` is a power of two in 64 .. 4096 are read where they lie by ONE pass (xrfthip_desc.seg_hop: neither the copy of the segments nor
    their spectra reach memory).  A ``dim`` that is not the trailing axis -- the time axis of a (time, y, x) cube -- is read where it lies too, for ``nperseg`` up
    to 512, where the dims behind ``dim`` are one unit-stride run and the dims in front one pitch (a contiguous array, a slice of its last dim); longer segments
    and other views are arranged first (one transposed copy).  Every other call unfolds the segments, runs the plain call and ``.mean``."""
    src = da
    kw = dict(detrend=detrend, window=window, shift=shift, spacing_tol=spacing_tol)
    return to_like(_welch_spectrum(da, None, dim, nperseg, noverlap, real_dim, scaling, window_correction, False, kw), src)


def welch_cross_spectrum(da1, da2, dim, nperseg, noverlap=None, real_dim=None, scaling="density", window_correction=False, detrend=None, window=None, shift=True,
                         spacing_tol=1e-3, true_phase=True):
    """Welch's estimate of the cross spectrum: the mean over the overlapping segments of ``cross_spectrum(seg1, seg2)``, ``F1 conj(F2)`` (see
    ``welch_power_spectrum``).  scipy.signal.csd(x, y) forms ``conj(X) Y``: for coordinates that start at 0 (or ``true_phase=False``)
    ``welch_cross_spectrum(x, y, ...)`` with ``window_correction=True`` is ``conj(scipy.signal.csd(x, y, return_onesided=False))`` after an fftshift, which is
    ``csd(y, x)``."""
    src = da1
    kw = dict(detrend=detrend, window=window, shift=shift, spacing_tol=spacing_tol)
    return to_like(_welch_spectrum(da1, da2, dim, nperseg, noverlap, real_dim, scaling, window_correction, true_phase, kw), src)


def welch_coherence(da1, da2, dim, nperseg, noverlap=None, real_dim=None, scaling="density", window_correction=False, detrend=None, window=None, shift=True,
                    spacing_tol=1e-3, true_phase=True):
    """Magnitude-squared coherence ``|<F1 conj F2>|^2 / (<|F1|^2> <|F2|^2>)``, ``<.>`` the mean over the overlapping segments: scipy.signal.coherence.  The three
    means are ``welch_cross_spectrum`` and ``welch_power_spectrum`` of each series; the division is the library's (xrfthip_coherence; no clamp).  Fewer than two
    segments: ValueError (of one spectrum the coherence is 1 everywhere)."""
    src = da1
    da1, da2 = from_any(da1), from_any(da2)
    kw = dict(detrend=detrend, window=window, shift=shift, spacing_tol=spacing_tol)
    cs = from_any(_welch_spectrum(da1, da2, dim, nperseg, noverlap, real_dim, scaling, window_correction, true_phase, kw, least=2))
    p1, p2 = (from_any(_welch_spectrum(d, None, dim, nperseg, noverlap, real_dim, scaling, window_correction, False, kw)) for d in (da1, da2))
    return to_like(_api._coherence_result(cs, p1, p2, da1, da2), src)


# ------------------------------------------------------------------------------------------------------
# Spectrograms: the spectrum of EVERY overlapping segment (scipy.signal.spectrogram / stft; the reference's power_spectrum(da, dim="time",
# chunks_to_segments=True, ...) without .mean("time_segment"), with an overlap).  Fused where a plan takes the call (xrfthip_desc.seg_keep: the segments read where
# they lie, every spectrum written once, no copy of the segments), else composed: the segments unfolded, the public call, the dims moved (a view).
# ------------------------------------------------------------------------------------------------------
def _spectrogram_result(lab, data, da, dim, nperseg, hop, m):
    """The labelled result: ``da.dims`` with ``dim`` replaced, where it lay, by (<dim>_segment, freq_<dim>); the coordinates, attrs and name of ``lab`` (a labelled
    spectrum of the segments, or of the first one: its last dim is freq_<dim>), and the <dim>_segment coordinate -- the middle of each segment's samples,
    c[s hop] + (c[s hop + nperseg - 1] - c[s hop]) / 2 (datetime64 included).  ``data``: the values in that order, or None: those of ``lab``, moved (a view)."""
    sname, fname = dim + "_segment", lab.dims[-1]
    final = [x for d in da.dims for x in ((sname, fname) if d == dim else (d,))]
    if data is None:
        data = lab.transpose(*final).data
    v = np.asarray(da[dim].values)
    lo, hi = v[0:(m - 1) * hop + 1:hop], v[nperseg - 1:(m - 1) * hop + nperseg:hop]
    coords = dict(lab.coords)
    coords[sname] = Coordinate((sname,), lo + (hi - lo) / 2, None, sname)
    return DataArray(data, final, coords, lab.name, lab.attrs)


def _spectrogram_composed(da, dim, nperseg, hop, m, complex_, kw):
    """The definition of the result: the segments unfolded (a view), ``power_spectrum`` / ``fft(true_phase=False)`` along their samples, the dims moved."""
    seg = _welch_segments(da, dim, nperseg, hop)
    full = _api.fft(seg, dim=[dim], true_phase=False, **kw) if complex_ else _api.power_spectrum(seg, dim=[dim], **kw)
    return _spectrogram_result(from_any(full), None, da, dim, nperseg, hop, m)


def _spectrogram_fused(c, da, dim, nperseg, hop, m, mode, scale, flags):
    """The values of ONE plan with seg_keep in the order of the result's dims, or None where the call composes: data that are not float32, an empty array, a length or a
    flag the plan declines (XRFTHIP_UNSUPPORTED_LENGTH, remembered), XRFTHIP_FASTW_KEEP=0.  The trailing axis is read where it lies (a pitch included); a leading or
    middle axis through the column layout (seg_stride, ``nperseg`` <= 512) where the array can be described by it -- the result then lies in its final order."""
    t = _to_device(da.data)
    if t.dtype != torch.float32 or math.prod(t.shape) == 0 or os.environ.get("XRFTHIP_FASTW_KEEP", "1") == "0":  # (the knob of the library, honoured before a cached plan could answer)
        return None
    kw = _segment_kw(c, None, nperseg, hop, m, mode, scale, flags, keep=True)
    ax = da.get_axis_num(dim)
    v = _segment_view(t, ax, (m - 1) * hop + nperseg, m, ax != t.dim() - 1)
    plan = None if v is None else _segment_plan(kw, v[1])
    if plan is None:
        return None
    # (the column layout writes [block][segment][frequency][column]: the final order)
    return plan.execute(v[0])[0].reshape(tuple(t.shape[:ax]) + (m, plan.nx_out) + tuple(t.shape[ax + 1:]))


def _refuse_nonfinite_span(d, dim, n):
    """scipy.signal.detrend's refusal over the first ``n`` samples along ``dim`` (a reduction: no array of flags; a NaN propagates into both ends)."""
    lo, hi = torch.aminmax(_to_device(d.data).narrow(d.get_axis_num(dim), 0, n))
    if not bool(torch.isfinite(lo) & torch.isfinite(hi)):
        raise ValueError("array must not contain infs or NaNs")


def _spectrogram(da, dim, nperseg, noverlap, complex_, analyse, kw):
    da = from_any(da)
    nperseg, hop, m = _welch_args(da, dim, nperseg, noverlap)
    if kw.get("real_dim") is not None and kw["real_dim"] != dim:
        raise ValueError(f"real_dim must be {dim!r}, the one transform dimension, or None")
    # the labels, the scaling and the tables are those of ONE segment's spectrum
    head = _welch_segments(da, dim, nperseg, hop).isel(**{dim + "_segment": 0})
    c, mode, scale, flags = analyse(head)
    if c.detrend == _lib.DETREND_LINEAR and math.prod(da.shape):  # (_refuse_nonfinite has seen the first segment: the refusal of the composed call covers every segment)
        _refuse_nonfinite_span(da, dim, (m - 1) * hop + nperseg)
    out = _spectrogram_fused(c, da, dim, nperseg, hop, m, mode, scale, flags)
    if out is None:
        return _spectrogram_composed(da, dim, nperseg, hop, m, complex_, kw)
    other = [d for d in head.dims if d != dim]
    lab = _label_output(c, head, out.new_empty(()).expand([head.sizes[d] for d in other] + [out.shape[da.get_axis_num(dim) + 1]]), other)
    return _spectrogram_result(lab, out, da, dim, nperseg, hop, m)


def spectrogram(da, dim, nperseg, noverlap=None, real_dim=None, scaling="density", window_correction=False, detrend=None, window=None, shift=True, spacing_tol=1e-3):
    """The power spectrum of every segment of ``da`` along ``dim``: the series is cut into segments of ``nperseg`` samples that overlap by ``noverlap`` (default
    ``nperseg // 2``; trailing samples that do not fill a segment are dropped; one segment is allowed) and the result is ``power_spectrum`` of each -- detrend and
    window per segment -- kept, not averaged: ``welch_power_spectrum`` is its mean over ``<dim>_segment``.  Dims: those of ``da`` with ``dim`` replaced, where it
    lay, by ``(<dim>_segment, freq_<dim>)``; ``freq_<dim>``, attrs and scaling are those of ``power_spectrum`` of the first ``nperseg`` samples; ``<dim>_segment``
    carries the middle of each segment's samples, ``c[s hop] + (c[s hop + nperseg - 1] - c[s hop]) / 2`` (datetime64 too); coordinates that do not depend on
    ``dim`` are kept.  With ``window_correction=True``, ``window="hann"`` and ``real_dim=dim`` the values are ``scipy.signal.spectrogram(..., mode="psd")``'s.
    float32 data whose ``nperseg`` is a power of two in 64 .. 4096 are read where they lie by ONE pass that writes every segment's spectrum once
    (xrfthip_desc.seg_keep): no copy of the segments (twice the series at half overlap) exists.  A ``dim`` that is not the trailing axis -- the time axis of a
    (time, y, x) cube -- is read where it lies too, for ``nperseg`` up to 512, and the result is written in its final order (no transposed copy); every other call
    unfolds the segments, runs ``power_spectrum`` and moves the dims (a view).  A linear detrend refuses non-finite samples inside the used span (ValueError)."""
    src = da
    kw = dict(real_dim=real_dim, scaling=scaling, window_correction=window_correction, detrend=detrend, window=window, shift=shift, spacing_tol=spacing_tol)

    def analyse(head):
        c, _, mode, scale, flags = _api._spectrum(head, None, [dim], real_dim, scaling, window_correction, False, dict(detrend=detrend, window=window, shift=shift, spacing_tol=spacing_tol))
        return c, mode, scale, flags

    return to_like(_spectrogram(da, dim, nperseg, noverlap, False, analyse, kw), src)


def stft(da, dim, nperseg, noverlap=None, real_dim=None, detrend=None, window=None, shift=True, true_amplitude=False, spacing_tol=1e-3):
    """The short-time Fourier transform: ``fft(..., true_phase=False)`` of every segment of ``da`` along ``dim`` (see ``spectrogram`` for the segments, the dims and
    the coordinates); complex.  There is no ``true_phase`` argument: each segment's phase refers to its OWN first sample, not to the origin of the series'
    coordinate (scipy.signal.stft's convention up to its scaling and padding).  ``true_amplitude=True`` multiplies by the spacing of ``dim``, as ``fft`` does.
    Fused and composed as ``spectrogram`` is (XRFTHIP_OUT_COMPLEX)."""
    src = da
    kw = dict(real_dim=real_dim, detrend=detrend, window=window, shift=shift, true_amplitude=true_amplitude, spacing_tol=spacing_tol)

    def analyse(head):
        c = _analyze(head, spacing_tol, [dim], real_dim, shift, detrend, window, False, False, "freq_", None)
        _api._refuse_nonfinite(c)
        return c, _lib.OUT_COMPLEX, (math.prod(c.delta_x) if true_amplitude else 1.0), 0

    return to_like(_spectrogram(da, dim, nperseg, noverlap, True, analyse, kw), src)


# ------------------------------------------------------------------------------------------------------
# Synthesis: the series rebuilt from its short-time transform (scipy.signal.istft) -- the inverse of ``stft``.  Fused where a plan takes the call
# (xrfthip_desc.seg_synth, csrc/fasto.h: inverse transform, window, overlap-add and the division in one pass, no inverse-transformed segment stored), else composed:
# ``ifft`` of every segment, the window, R strided adds, the division.
# ------------------------------------------------------------------------------------------------------
def _istft_args(ds, dim, nperseg, noverlap, real_dim):
    """(axis of <dim>_segment, nperseg, hop, segments) after the checks."""
    if not isinstance(dim, str):
        raise ValueError(f"dim must be the name of ONE dimension (the axis the series is rebuilt along), not {dim!r}")
    sname, fname = dim + "_segment", "freq_" + dim
    if sname not in ds.dims or fname not in ds.dims:
        raise ValueError(f"the short-time transform along {dim!r} has the dimensions {sname!r} and {fname!r}: {tuple(ds.dims)} lacks one of them")
    ax = ds.get_axis_num(sname)
    if ds.get_axis_num(fname) != ax + 1:
        raise ValueError(f"{sname!r} and {fname!r} must be adjacent, in this order (as stft returns them), not {tuple(ds.dims)}")
    if real_dim is not None and real_dim != dim:
        raise ValueError(f"real_dim must be {dim!r}, the one transform dimension, or None")
    nf = ds.sizes[fname]
    implied = 2 * (nf - 1) if real_dim is not None else nf
    nperseg = implied if nperseg is None else int(nperseg)
    if nperseg != implied or nperseg < 1:
        raise ValueError(f"nperseg = {nperseg} disagrees with the length of {fname!r}: {nf} frequencies are those of {implied} samples")
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if noverlap < 0 or noverlap >= nperseg:
        raise ValueError(f"noverlap = {noverlap} must be in 0 .. nperseg - 1 = {nperseg - 1}")
    return ax, nperseg, nperseg - noverlap, ds.sizes[sname]


def _istft_envelope(w, hop, m):
    """D[n] = sum_s w^2[n - s hop] over the span of ``m`` segments, float64, with 1 where D <= 1e-10 (scipy.signal.istft's rule: such samples stay undivided)."""
    nperseg = len(w)
    d = np.zeros((m - 1) * hop + nperseg)
    w2 = np.asarray(w, dtype=np.float64) ** 2
    r = -(-nperseg // hop)
    for q in range(min(r, m)):  # (the segments s = q mod R do not overlap one another)
        np.lib.stride_tricks.as_strided(d[q * hop:], ((m - q + r - 1) // r, nperseg), (r * hop * 8, 8))[...] += w2
    return np.where(d > 1e-10, d, 1.0)


def _istft_composed(ds, ax, fname, nperseg, hop, m, w, real, kw):
    """The definition of the result, values only, the series last: ``ifft`` along freq_<dim> of every segment (true_phase=False; ``shift=True``: of the reference's two
    output shifts the one of true_phase=False and the one of shift cancel, the samples come out in their order, whatever the layout of the frequency axis), times the
    window, overlap-added at s hop -- the segments s = q mod R, R = ceil(nperseg / hop), do not overlap one another: R strided adds in ascending q, no index_add_, no
    atomics -- and divided by the summed squared windows."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = from_any(_api.ifft(ds, dim=[fname], real_dim=fname if real else None, shift=True, true_phase=False, lag=[0.0], **kw))
    v = _to_device(x.data).movedim((ax, ax + 1), (-2, -1))
    rdt = v.real.dtype if v.is_complex() else v.dtype
    if w is not None:
        v = v * torch.tensor(np.asarray(w, dtype=np.float64), dtype=rdt, device=v.device)
    span = (m - 1) * hop + nperseg
    out = torch.zeros(tuple(v.shape[:-2]) + (span,), dtype=v.dtype, device=v.device)
    r = -(-nperseg // hop)
    for q in range(min(r, m)):
        mq = (m - q + r - 1) // r
        dst = torch.as_strided(out, tuple(out.shape[:-1]) + (mq, nperseg), tuple(out.stride()[:-1]) + (r * hop, 1), q * hop)
        dst += v[..., q::r, :]
    out /= torch.from_numpy(_istft_envelope(np.ones(nperseg) if w is None else w, hop, m)).to(rdt).to(v.device)
    return out


def _istft_fused(t, ax, nperseg, hop, m, w, scale):
    """The values of ONE plan with seg_synth, the series last, or None where the call composes: spectra that are not complex64, an empty array, a length or an overlap
    the plan declines (XRFTHIP_UNSUPPORTED_LENGTH, remembered), XRFTHIP_FASTW_SYNTH=0.  The pair (<dim>_segment, freq_<dim>) is read where it lies as the trailing
    axes with one pitch between the series; elsewhere the spectrogram is arranged first (one transposed copy)."""
    if t.dtype != torch.complex64 or math.prod(t.shape) == 0 or os.environ.get("XRFTHIP_FASTW_SYNTH", "1") == "0":  # (the knob of the library, honoured before a cached plan could answer)
        return None
    nb = nperseg // 2 + 1
    v = t if ax == t.dim() - 2 else t.movedim((ax, ax + 1), (-2, -1))
    lead = _collapse(v.shape[:-2], v.stride()[:-2])
    if v.stride(-1) == 1 and (m == 1 or v.stride(-2) == nb) and lead is not None and (lead[0] == 1 or lead[1] >= m * nb):
        rows = torch.as_strided(v, (lead[0], m, nb), (lead[1] if lead[0] > 1 else m * nb, nb, 1), v.storage_offset())
        pitch = lead[1] if lead[0] > 1 else 0
    else:
        rows, pitch = v.contiguous().reshape(-1, m, nb), 0
    kw = dict(ndim=1, ny=1, nx=nperseg, dtype=torch.complex64, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=_lib.INVERSE | _lib.C2R_X, scale=float(scale),
              window_x=w, mean_batch=m, seg_hop=hop, seg_synth=1, batch=rows.shape[0] * m, in_stride_batch=int(pitch))
    plan = _segment_plan(kw, {})
    if plan is None:
        return None
    return plan.execute(rows)[0].reshape(tuple(v.shape[:-2]) + ((m - 1) * hop + nperseg,))


def istft(ds, dim, nperseg=None, noverlap=None, real_dim=None, window=None, shift=True, true_amplitude=False, spacing_tol=1e-3):
    """The inverse short-time Fourier transform: the series along ``dim`` rebuilt from ``ds = stft(da, dim, nperseg, noverlap, real_dim=..., window=..., shift=...,
    true_amplitude=...)``, whose dims are those of ``da`` with ``dim`` replaced by ``(<dim>_segment, freq_<dim>)`` (adjacent, in this order).  Every segment's spectrum
    goes through ``ifft`` along ``freq_<dim>`` (``true_phase=False``: the inverse of what ``stft`` applied per segment), is multiplied by the window
    (``scipy.signal.windows.<window>(nperseg, sym=False)``, the one of the analysis; None: ones), the segments are overlap-added at ``s * hop`` and the sum is divided
    by ``D[n] = sum_s w^2[n - s hop]`` -- where ``D[n] <= 1e-10`` (the first sample under a periodic Hann window) the sum is returned undivided, the rule of
    ``scipy.signal.istft``.  ``nperseg=None``: the length of ``freq_<dim>`` (``2 (len - 1)`` with ``real_dim=dim``); ``noverlap=None``: ``nperseg // 2``, the default
    of ``stft``.  ``shift`` says how ``stft`` laid ``freq_<dim>`` out; the coordinate itself tells the order, and either layout gives the same series.
    The result has ``dim`` back where ``<dim>_segment`` lay, ``(M - 1) hop + nperseg`` samples long (what ``stft`` dropped at the end cannot come back); real with
    ``real_dim=dim``, complex otherwise, as ``ifft``.  Its coordinate is ``t0 + dt arange(span)``, ``dt = 1 / (nperseg df)`` with ``df`` the spacing of ``freq_<dim>``
    (checked with ``spacing_tol``), ``t0 = segment[0] - (nperseg - 1) dt / 2`` where ``<dim>_segment`` carries a numeric coordinate (the middle of the first segment's
    samples), else 0; coordinates that do not depend on the two replaced dims are kept; no name, no attrs, as ``ifft``.
    There is no ``detrend`` argument: a per-segment detrend cannot be undone, and ``istft(stft(..., detrend=...))`` returns the overlap-added DETRENDED segments.
    complex64 half spectra (``real_dim=dim``) whose ``nperseg`` is a power of two in 64 .. 4096 with ``2 (ceil(nperseg / hop) - 1) <= 8192 / nperseg`` are rebuilt by
    ONE pass (xrfthip_desc.seg_synth): no inverse-transformed segment reaches memory.  The pair of dims is read where it lies as the trailing axes; elsewhere the
    spectrogram is arranged first (one transposed copy) and the result moved back as a view.  Every other call -- complex128, a two-sided spectrum, other lengths and
    overlaps, XRFTHIP_FASTW_SYNTH=0 -- composes the definition above."""
    src = ds
    ds = from_any(ds)
    ax, nperseg, hop, m = _istft_args(ds, dim, nperseg, noverlap, real_dim)
    sname, fname = dim + "_segment", "freq_" + dim
    real = real_dim is not None
    fv = np.asarray(ds[fname].values, dtype=np.float64) if fname in ds.coords else None
    if fv is None:
        raise ValueError(f"{fname!r} carries no coordinate: the spacing of {dim!r} comes from it")
    df = float(_get_coordinate_spacing(np.sort(fv), spacing_tol, fname)) if len(fv) > 1 else 1.0
    if real and (np.any(np.diff(fv) < 0) or abs(fv[0]) > spacing_tol):
        raise ValueError(f"with real_dim the coordinate {fname!r} must be ascending from zero frequency (rfftfreq order)")
    dt = 1.0 / (nperseg * df)
    w = None if window is None else _api._window_vector(window, nperseg)
    t = _to_device(ds.data)
    out = None
    if real:
        out = _istft_fused(t if t.is_complex() else t.to(torch.complex64 if t.dtype == torch.float32 else torch.complex128), ax, nperseg, hop, m, w,
                           (1.0 / dt if true_amplitude else 1.0) / nperseg)
    if out is None:
        out = _istft_composed(ds, ax, fname, nperseg, hop, m, w, real, dict(true_amplitude=true_amplitude, spacing_tol=spacing_tol))
    span = (m - 1) * hop + nperseg
    t0 = 0.0
    if sname in ds.coords:
        sv = np.asarray(ds[sname].values)
        if sv.dtype.kind in "fiu" and len(sv):
            t0 = float(sv[0]) - (nperseg - 1) * dt / 2
    dims = [d for d in ds.dims if d != fname]
    dims[ax] = dim
    coords = {k: v for k, v in ds.coords.items() if sname not in v.dims and fname not in v.dims and k != dim}
    coords[dim] = Coordinate((dim,), t0 + dt * np.arange(span), {"spacing": dt}, dim)
    return to_like(DataArray(out.movedim(-1, ax), dims, coords, None, None), src)


# ------------------------------------------------------------------------------------------------------
# FIR filtering along a dim by overlap-save (scipy.signal.convolve along one axis): every L-sample segment transformed, multiplied by the taps' response, transformed
# back, the samples that do not wrap around kept.  Fused where a plan takes the call (xrfthip_desc.seg_filter, csrc/fastf.h: the series read once, the filtered series
# written once, nothing in between), else composed at the same L: a zero-extended copy, the segments unfolded, the real 1-D plan, the product, its inverse, the slice.
# ------------------------------------------------------------------------------------------------------
_FIR_MODES = ("full", "same", "valid")
_FIR_RESPONSES = {}  # (digest of the taps, K, L) -> rfft(taps, L), complex128, read-only: the plan key digests it once


def _fir_response(taps, l):
    key = (_digest(taps), len(taps), l)
    with _plan_lock:
        h = _FIR_RESPONSES.get(key)
    if h is None:
        h = _ro(np.fft.rfft(taps, l))
        with _plan_lock:
            if len(_FIR_RESPONSES) > 64:
                _FIR_RESPONSES.clear()
            _FIR_RESPONSES[key] = h
    return h


_FIR_DEVICE_RESPONSES = {}  # (id of the memoised response, complex dtype, device) -> (the response, its device copy): the composed route uploads a table once


def _fir_device_response(resp, cdt, device):
    key = (id(resp), cdt, str(device))
    with _plan_lock:
        e = _FIR_DEVICE_RESPONSES.get(key)
    if e is None or e[0] is not resp:
        e = (resp, torch.from_numpy(np.array(resp)).to(cdt).to(device))
        with _plan_lock:
            if len(_FIR_DEVICE_RESPONSES) > 64:
                _FIR_DEVICE_RESPONSES.clear()
            _FIR_DEVICE_RESPONSES[key] = e
    return e[1]


def _fir_default_nfft(k, n=None):
    """The smallest power of two >= max(512, 4 (K - 1)), capped at 4096: the sweep of profiles/r27_fir_filter.txt -- the one-pass kernel is fastest at 256 .. 512 for
    K <= 129 (512 is within 4 % of the best everywhere) and at 4 (K - 1) and beyond for longer taps.  A series of ``n`` samples that one shorter segment holds whole
    (N + K - 1 <= L / 2) takes the shorter one, down to max(64, 4 (K - 1)).  K = 2049 fits 4096 exactly (K - 1 = L / 2, the longest taps the one pass takes); longer taps (composed): the
    smallest power of two >= 2 (K - 1)."""
    l = 512
    while l < 4 * (k - 1) and l < 4096:
        l *= 2
    while n is not None and l // 2 >= max(64, 4 * (k - 1), n + k - 1):
        l //= 2
    while l < 2 * (k - 1):
        l *= 2
    return l


def _fir_args(da, dim, taps, mode, nfft):
    """(axis, taps as float64, K, L, a, n_out) after the checks."""
    if not isinstance(dim, str):
        raise ValueError(f"dim must be the name of ONE dimension (the axis the filter runs along), not {dim!r}")
    ax = da.get_axis_num(dim)
    h = np.asarray(taps)
    if h.ndim != 1 or h.size < 1:
        raise ValueError("taps must hold K >= 1 coefficients in one dimension")
    if h.dtype.kind == "c":
        raise ValueError("taps must be real (a complex filter is two real ones)")
    h = np.ascontiguousarray(h, dtype=np.float64)
    if mode not in _FIR_MODES:
        raise ValueError(f"mode must be one of {_FIR_MODES}, not {mode!r}")
    n, k = da.shape[ax], len(h)
    if mode == "valid" and n < k:
        raise ValueError(f"mode 'valid' needs at least K = {k} samples along {dim!r}, which has {n}")
    a, n_out = {"full": (0, n + k - 1), "same": ((k - 1) // 2, n), "valid": (k - 1, n - k + 1)}[mode]
    if nfft is None:
        l = _fir_default_nfft(k, n)
    else:
        l = int(nfft)
        if l < k or l < 2:
            raise ValueError(f"nfft = {l} must be at least K = {k} (and 2): a segment holds the taps")
        l += l & 1  # (the real transforms take even lengths; the result does not depend on L)
    return ax, h, k, l, a, n_out


def _fir_columns(t, ax, k, l, a, n_out, resp, hop, m):
    """The values of ONE plan with seg_filter and seg_filter_cols, contiguous in the dims' own order, or None where the caller arranges: a trailing ``dim``, L beyond
    512, a view the column layout cannot describe (_welch_columns: XRFTHIP_FASTW_COLS=0 included), a refusal of the plan (remembered: a narrow grid -- at most half of the
    column groups live -- is declined by default, profiles/r30_fir_filter_cols.txt), XRFTHIP_FASTW_FILTER_COLS=0."""
    if ax == t.dim() - 1 or l < 64 or l > 512 or l & (l - 1) or os.environ.get("XRFTHIP_FASTW_FILTER_COLS", "1") == "0":  # (the knob of the library, honoured before a cached plan could answer)
        return None
    n = t.shape[ax]
    v = _welch_columns(t, ax, n)
    if v is None:
        return None
    view, pitch, ss = v
    kw = dict(ndim=1, ny=1, nx=l, dtype=torch.float32, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=0, scale=1.0 / l, phase_x=resp, mean_batch=m,
              seg_hop=hop, seg_filter=1, seg_lead=a, seg_in_len=n, seg_out_len=n_out, batch=view.shape[0] * m, in_stride_batch=int(pitch), inner=view.shape[2],
              seg_stride=int(ss), seg_filter_cols=1)
    plan = _segment_plan(kw, {})
    if plan is None:
        return None
    return plan.execute(view)[0].reshape(tuple(t.shape[:ax]) + (n_out,) + tuple(t.shape[ax + 1:]))


def _fir_fused(t, ax, k, l, a, n_out, resp):
    """The values of ONE plan with seg_filter, in the dims' own order, or None where the call composes: data that are not float32, an empty array, L not a power of
    two in 64 .. 4096, K - 1 > L / 2, a class the plan declines (XRFTHIP_UNSUPPORTED_LENGTH, remembered), XRFTHIP_FASTW_FILTER=0.  A trailing ``dim`` is read where it
    lies, with one pitch between the series.  Any other is read where it lies too where the column layout takes it (_fir_columns: L <= 512, the dims behind ``dim``
    one unit-stride run, those in front one pitch) and the result is contiguous; else it is arranged first (one transposed copy) and the result moved back as a view."""
    if t.dtype != torch.float32 or math.prod(t.shape) == 0 or n_out < 1 or os.environ.get("XRFTHIP_FASTW_FILTER", "1") == "0":  # (the knob of the library, honoured before a cached plan could answer)
        return None
    if 2 * (k - 1) > l:  # (the library's XRFTHIP_BAD_ARG: less than half of a transform would be kept; L itself it judges: 64 .. 4096, a power of two)
        return None
    hop = l - k + 1
    m = -(-n_out // hop)
    out = _fir_columns(t, ax, k, l, a, n_out, resp, hop, m)
    if out is not None:
        return out
    v = t if ax == t.dim() - 1 else t.movedim(ax, -1)
    n = v.shape[-1]
    lead = _collapse(v.shape[:-1], v.stride()[:-1])
    if (v.stride(-1) == 1 or n == 1) and lead is not None and (lead[0] == 1 or lead[1] >= n):
        rows = torch.as_strided(v, (lead[0], n), (lead[1] if lead[0] > 1 else n, 1), v.storage_offset())
        pitch = lead[1] if lead[0] > 1 else 0
    else:
        rows, pitch = v.contiguous().reshape(-1, n), 0
    kw = dict(ndim=1, ny=1, nx=l, dtype=torch.float32, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=0, scale=1.0 / l, phase_x=resp, mean_batch=m,
              seg_hop=hop, seg_filter=1, seg_lead=a, seg_in_len=n, seg_out_len=n_out, batch=rows.shape[0] * m, in_stride_batch=int(pitch))
    plan = _segment_plan(kw, {})
    if plan is None:
        return None
    return plan.execute(rows)[0].reshape(tuple(v.shape[:-1]) + (n_out,)).movedim(-1, ax)


def _fir_composed(t, ax, k, l, a, n_out, resp):
    """The definition of the result, values only, in the dims' own order (a view, the series last in memory): overlap-save at the same L out of the library's own pieces -- a zero-extended copy of the series,
    the segments unfolded at hop V = L - K + 1, the real 1-D forward plan, engine.table_mul by the response, the C2R inverse plan, the kept samples sliced out."""
    v = t.movedim(ax, -1)
    n = v.shape[-1]
    cdt = torch.complex64 if t.dtype == torch.float32 else torch.complex128
    hop = l - k + 1
    m = -(-n_out // hop)
    front, span = k - 1 - a, (m - 1) * hop + l
    xe = torch.zeros(tuple(v.shape[:-1]) + (span,), dtype=t.dtype, device=t.device)
    ncopy = min(n, span - front)
    xe[..., front:front + ncopy] = v[..., :ncopy]
    seg = xe.unfold(-1, l, hop).contiguous().reshape(-1, l)
    b, nb = seg.shape[0], l // 2 + 1
    if b == 0:
        return torch.empty(tuple(v.shape[:-1]) + (n_out,), dtype=t.dtype, device=t.device).movedim(-1, ax)
    spec = _get_plan(ndim=1, batch=b, ny=1, nx=l, dtype=t.dtype, out_mode=_lib.OUT_COMPLEX, flags=_lib.HALF_X).execute(seg)[0].reshape(b, nb)
    del seg, xe
    prod = engine.table_mul(spec, _fir_device_response(resp, cdt, t.device), nb)
    del spec
    y = _get_plan(ndim=1, batch=b, ny=1, nx=l, dtype=cdt, out_mode=_lib.OUT_COMPLEX, flags=_lib.INVERSE | _lib.C2R_X, scale=1.0 / l).execute(prod)[0]
    y = y.reshape(tuple(v.shape[:-1]) + (m, l))[..., k - 1:]
    return y.reshape(tuple(v.shape[:-1]) + (m * hop,))[..., :n_out].movedim(-1, ax)


def _fir_coordinate(da, dim, mode, k, n, spacing_tol):
    """The coordinate of ``dim`` in the result, or None where ``da`` carries none: kept ("same"), sliced ("valid"), extended at its spacing ("full")."""
    if dim not in da.coords:
        return None
    c = da.coords[dim]
    v = np.asarray(c.values)
    if mode == "same":
        return c
    if mode == "valid":
        return Coordinate((dim,), v[k // 2:k // 2 + n - k + 1], c.attrs, dim)
    if k == 1:
        return c
    if n < 2:
        raise ValueError(f"the coordinate of {dim!r} has one value: its spacing, by which mode 'full' extends it, is unknown")
    _get_coordinate_spacing(v, spacing_tol, dim)  # (evenly spaced, or ValueError)
    return Coordinate((dim,), _pad_coordinate(v, ((k - 1) // 2, k // 2), (v[-1] - v[0]) / (n - 1)), c.attrs, dim)


def fir_filter(da, dim, taps, mode="same", nfft=None, spacing_tol=1e-3):
    """``da`` filtered along ``dim`` by the K real coefficients ``taps`` (a 1-D array or a sequence): ``scipy.signal.convolve(x, taps, mode)`` of every series --
    ``y_full[m] = sum_k taps[k] x[m - k]`` with x zero outside its N samples, and output sample n' is ``y_full[n' + a]``: ``"full"`` a = 0, N + K - 1 samples;
    ``"same"`` a = (K - 1) // 2, N samples; ``"valid"`` a = K - 1, N - K + 1 samples (ValueError when N < K).  A low-pass, a band-pass or a smoothing kernel designed
    with ``scipy.signal.firwin`` is applied this way; the filter is linear and exact up to rounding: no window, no overlap-add.
    The result keeps the dims, the other coordinates, the name and the attrs of ``da``.  The coordinate of ``dim`` is unchanged ("same"), the slice
    ``[K // 2 : K // 2 + N - K + 1]`` ("valid"), or extended by (K - 1) // 2 points in front and K // 2 behind at its spacing ("full": the coordinate must be evenly
    spaced within ``spacing_tol``, else ValueError); a dim without a coordinate stays without one, and coordinates that span ``dim`` besides others are kept only
    where the length stays.
    The work is overlap-save with segments of ``nfft`` = L samples, of which V = L - K + 1 are kept: by default the smallest power of two >= max(512, 4 (K - 1)),
    capped at 4096 (shorter, down to 64, where one shorter segment holds the whole series; profiles/r27_fir_filter.txt); a given ``nfft`` must be at least K (an odd one is raised by one; the result does not depend on it but for rounding).  float32 data with L a power
    of two in 64 .. 4096 and K - 1 <= L / 2 are filtered by ONE pass (xrfthip_desc.seg_filter): the series is read once and the result written once, no spectrum
    reaches memory.  A trailing ``dim`` is read where it lies (a batch pitch included).  Any other ``dim`` -- ``time`` of a (time, y, x) or (member, time, lat, lon)
    array -- is read where it lies too, by the column layout of the same pass (xrfthip_desc.seg_filter_cols), and the result is contiguous in the dims' own order: no
    transposed copy comes in or goes out.  That holds for L <= 512 (the default for K <= 129; longer taps with ``nfft`` <= 512) where the dims behind ``dim`` are one
    unit-stride run and those in front one pitch, and more than half of the groups of 32 (L = 512: 16) adjacent columns are live (a narrower grid measured slower,
    profiles/r30_fir_filter_cols.txt; XRFTHIP_MEAN_ALL=1 takes it); otherwise, or with XRFTHIP_FASTW_FILTER_COLS=0, the array is arranged first (one transposed copy) and the result moved
    back as a view.  Every other call -- float64, other L, longer taps, XRFTHIP_FASTW_FILTER=0 -- composes the same overlap-save from the library's own real 1-D plans and
    a table product.  float16 / bfloat16 data are widened to float32 first and the result is float32; complex data run as two real calls, the real and the imaginary
    part."""
    src = da
    da = from_any(da)
    ax, h, k, l, a, n_out = _fir_args(da, dim, taps, mode, nfft)
    n = da.shape[ax]
    coord = _fir_coordinate(da, dim, mode, k, n, spacing_tol)
    t = _to_device(da.data)
    if t.dtype in (torch.float16, torch.bfloat16):
        t = engine.convert(t, torch.float32)
    if t.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        t = t.to(torch.float64)
    resp = _fir_response(h, l)

    def one(x):
        if math.prod(x.shape) == 0:  # (nothing to filter: the zeros of an empty sum)
            return x.new_zeros(tuple(n_out if i == ax else s for i, s in enumerate(x.shape)))
        out = _fir_fused(x, ax, k, l, a, n_out, resp)
        return _fir_composed(x, ax, k, l, a, n_out, resp) if out is None else out

    out = torch.complex(one(t.real.contiguous()), one(t.imag.contiguous())) if t.is_complex() else one(t)
    coords = {}
    for name, c in da.coords.items():
        if name == dim:
            if coord is not None:
                coords[name] = coord
        elif dim not in c.dims or n_out == n:
            coords[name] = c
    return to_like(DataArray(out, da.dims, coords, da.name, da.attrs), src)


# ------------------------------------------------------------------------------------------------------
# Multitaper spectra (Thomson): the whole record of N samples under K orthogonal Slepian (DPSS) tapers, zero-extended to L points, transformed K times, the K spectra
# added with weights -- the estimator for short records that cannot be cut into segments.  Fused where a plan takes the call (xrfthip_desc.seg_tapers, csrc/fastt.h:
# neither the K tapered copies nor the K spectra reach memory), else composed: detrend, a taper dim by broadcasting the table, zero-extension, power_spectrum /
# cross_spectrum, the weighted sum.
# ------------------------------------------------------------------------------------------------------
_DPSS = {}  # (N, NW, K, route) -> (tapers [K][N] float64, unit L2 norm, scipy's signs; concentration ratios [K]), read-only


def _dpss_compute(n, nw, k, use_scipy=None):
    """scipy.signal.windows.dpss(n, nw, k, return_ratios=True) without scipy: the K eigenvectors of the largest eigenvalues of the symmetric tridiagonal matrix that
    commutes with the concentration operator (Percival & Walden, 1993, ch. 8), in float64; symmetric tapers with a positive mean, antisymmetric ones beginning with a
    positive lobe; the ratios as scipy computes them, from the tapers' autocorrelation and the sinc kernel.  ``use_scipy``: None = scipy.linalg.eigh_tridiagonal
    where scipy imports, else numpy.linalg.eigh of the dense matrix (seconds at N = 4096: memoised by _dpss)."""
    w = float(nw) / n
    idx = np.arange(n, dtype=np.float64)
    diag = ((n - 1 - 2 * idx) / 2.0) ** 2 * np.cos(2 * np.pi * w)
    off = idx[1:] * (n - idx[1:]) / 2.0
    eigh_tridiagonal = None
    if use_scipy is None or use_scipy:
        try:
            from scipy.linalg import eigh_tridiagonal
        except Exception:
            if use_scipy:
                raise
    if eigh_tridiagonal is not None:
        _, vec = eigh_tridiagonal(diag, off, select="i", select_range=(n - k, n - 1))
    else:
        _, vec = np.linalg.eigh(np.diag(diag) + np.diag(off, 1) + np.diag(off, -1))
        vec = vec[:, n - k:]
    d = np.ascontiguousarray(vec[:, ::-1].T)
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    for j in range(0, k, 2):
        if d[j].sum() < 0:
            d[j] *= -1
    thresh = max(1e-7, 1.0 / n)
    for j in range(1, k, 2):
        if d[j][d[j] * d[j] > thresh][0] < 0:
            d[j] *= -1
    m = 1
    while m < 2 * n - 1:
        m *= 2
    f = np.fft.rfft(d, m)
    rxx = np.fft.irfft(f * np.conj(f), m)[:, :n]
    r = 4 * w * np.sinc(2 * w * idx)
    r[0] = 2 * w
    return _ro(d), _ro(rxx @ r)


def _dpss(n, nw, k, use_scipy=None):
    key = (int(n), float(nw), int(k), use_scipy)
    with _plan_lock:
        hit = _DPSS.get(key)
    if hit is None:
        hit = _dpss_compute(n, nw, k, use_scipy)
        with _plan_lock:
            if len(_DPSS) > 64:
                _DPSS.clear()
            _DPSS[key] = hit
    return hit


_TAPER_TABLES = {}  # (digest of the tapers, digest of the weights, K, N) -> sqrt(w_j) d_j[n] float32, read-only: the plan key digests it once


def _taper_table(d, w):
    key = (_digest(d), _digest(w), d.shape)
    with _plan_lock:
        t = _TAPER_TABLES.get(key)
    if t is None:
        t = _ro((np.sqrt(w).reshape(-1, 1) * d).astype(np.float32))
        with _plan_lock:
            if len(_TAPER_TABLES) > 64:
                _TAPER_TABLES.clear()
            _TAPER_TABLES[key] = t
    return t


def _multitaper_args(da, dim, nw, k, nfft, weights, tapers):
    """(N, L, K, the tapers [K][N] float64 with unit L2 norm, the weights [K] float64, sum 1) after the checks."""
    if not isinstance(dim, str):
        raise ValueError(f"dim must be the name of ONE dimension (the axis the tapers run along), not {dim!r}")
    n = da.shape[da.get_axis_num(dim)]
    if n < 1:
        raise ValueError(f"{dim!r} holds no samples")
    if weights not in ("unity", "eigen"):
        raise ValueError(f"weights must be 'unity' or 'eigen', not {weights!r}")
    if tapers is not None:
        if np.iscomplexobj(tapers):
            raise ValueError("tapers must be real")
        d = np.array(tapers, dtype=np.float64, ndmin=2)
        if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] != n:
            raise ValueError(f"tapers must be a real array (K, {n}): K >= 1 tapers as long as {dim!r}")
        if weights == "eigen":
            raise ValueError("weights='eigen' needs the library's own DPSS tapers: given tapers carry no concentration ratios")
        norm = np.sqrt((d * d).sum(axis=1, keepdims=True))
        if not np.all(np.isfinite(d)) or np.any(norm == 0):
            raise ValueError("every taper must be finite and not identically zero")
        d, k, lam = d / norm, d.shape[0], None
        if k > n:
            raise ValueError(f"K = {k} tapers is not in 1 .. {n}, the length of {dim!r}")
    else:
        nw = float(nw)
        if not nw > 0 or not 2 * nw <= n:
            raise ValueError(f"NW = {nw} must satisfy 0 < 2 NW <= {n}, the length of {dim!r}")
        k = int(2 * nw) - 1 if k is None else int(k)
        if k < 1 or k > n:
            raise ValueError(f"K = {k} tapers is not in 1 .. {n}, the length of {dim!r}")
        d, lam = _dpss(n, nw, k)
    if nfft is None:
        l = 1
        while l < n:
            l *= 2
    else:
        l = int(nfft)
        if l < n:
            raise ValueError(f"nfft = {l} is shorter than {dim!r} ({n} samples): the series is zero-extended, never cut")
    w = np.full(k, 1.0 / k) if weights == "unity" else lam / lam.sum()
    return n, l, k, d, w


def _multitaper_head(da, dim, n, l, spacing_tol):
    """The labels of the series zero-extended to L samples, ``dim`` last, over no data (a 0-stride view): what the analysis of power_spectrum and _label_output read.
    The coordinate of ``dim`` is extended at its spacing (as ``pad`` extends it)."""
    if dim not in da.coords:
        raise ValueError(f"{dim!r} carries no coordinate: the spacing of the spectrum comes from it")
    cv = da.coords[dim]
    v = np.asarray(cv.values)
    if l > n:
        if n < 2:
            raise ValueError(f"the coordinate of {dim!r} has one value: its spacing, by which the zero-extension extends it, is unknown")
        _get_coordinate_spacing(v, spacing_tol, dim)  # (evenly spaced, or ValueError)
        v = _pad_coordinate(v, (0, l - n), (v[-1] - v[0]) / (n - 1))
    other = [d for d in da.dims if d != dim]
    t = _to_device(da.data)
    coords = {name: c for name, c in da.coords.items() if name != dim and dim not in c.dims}
    coords[dim] = Coordinate((dim,), v, cv.attrs, dim)
    return DataArray(t.new_empty(()).expand([da.sizes[d] for d in other] + [l]), other + [dim], coords, da.name, da.attrs), other


def _multitaper_fused(c, c2, ts, ax, n, l, k, table, det, mode, scale, flags):
    """The (series, nx_out) values of ONE plan with seg_tapers, or None where the call composes: data that are not float32, an empty array, L not a power of two in
    64 .. 4096, K > 32, a flag the plan declines (a descending coordinate's flip; XRFTHIP_UNSUPPORTED_LENGTH, remembered), XRFTHIP_FASTW_TAPERS=0.  A trailing ``dim``
    with one pitch between the series is read where it lies; any other is arranged first (one transposed copy)."""
    if any(t.dtype != torch.float32 for t in ts) or math.prod(ts[0].shape) == 0 or os.environ.get("XRFTHIP_FASTW_TAPERS", "1") == "0":  # (the knob of the library, honoured before a cached plan could answer)
        return None
    if l < 64 or l > 4096 or l & (l - 1) or k > 32:  # (what the library would answer XRFTHIP_UNSUPPORTED_LENGTH to, known here)
        return None
    views = []
    for t in ts:
        v = t if ax == t.dim() - 1 else t.movedim(ax, -1)
        lead = _collapse(v.shape[:-1], v.stride()[:-1])
        if (v.stride(-1) == 1 or n == 1) and lead is not None and (lead[0] == 1 or lead[1] >= n):
            views.append((torch.as_strided(v, (lead[0], n), (lead[1] if lead[0] > 1 else n, 1), v.storage_offset()), lead[1] if lead[0] > 1 else 0))
        else:
            views.append((v.contiguous().reshape(-1, n), 0))
    if len(views) == 2 and views[0][1] != views[1][1]:  # (two pitches: both arranged)
        views = [(r.contiguous(), 0) for r, _ in views]
    fl, _, ph = _flags_tables(c, c.da, None if c2 is None else c2.lag_x, None if c2 is None else c2.reversed)
    kw = dict(ndim=1, ny=1, nx=l, dtype=torch.float32, out_mode=mode, detrend=det, flags=fl | flags, scale=float(scale), phase_x=ph["x"] if mode == _lib.OUT_CROSS else None,
              seg_tapers=k, seg_taper_len=n, tapers=table, batch=views[0][0].shape[0], in_stride_batch=int(views[0][1]))
    plan = _segment_plan(kw, {})
    if plan is None:
        return None
    return plan.execute(*[r for r, _ in views])[0]


def _multitaper_composed(das, heads, dim, l, d, w, detrend, real_dim, shift, spacing_tol, true_phase):
    """The definition of the result, values only, ``dim`` last: the library's detrend over the N samples, a leading taper dim by broadcasting the table, zero-extension
    to L, ``power_spectrum`` / ``cross_spectrum`` along ``dim`` (density scaling, no detrend, no window), the weighted sum over the tapers.  The density scaling of an
    L-sample series is dt / L: times L, the tapers having unit norm over their N samples (mean(d^2) = 1 / L of the zero-extended taper)."""
    k, n = d.shape
    tname = "taper"
    while tname in das[0].dims:
        tname += "_"
    stacks = []
    for da, head in zip(das, heads):
        y = from_any(_api.detrend(da, dim, detrend)) if detrend is not None else da
        v = _to_device(y.data).movedim(da.get_axis_num(dim), -1)
        if v.dtype in (torch.float16, torch.bfloat16):
            v = engine.convert(v.contiguous(), torch.float32)
        if v.dtype not in (torch.float32, torch.float64):
            v = v.to(torch.float64)
        tab = torch.from_numpy(np.array(d)).to(v.dtype).to(v.device).reshape((k,) + (1,) * (v.dim() - 1) + (n,))
        ext = torch.zeros((k,) + tuple(v.shape[:-1]) + (l,), dtype=v.dtype, device=v.device)
        ext[..., :n] = v.unsqueeze(0) * tab
        stacks.append(DataArray(ext, (tname,) + tuple(head.dims), {dim: head.coords[dim]}))
    kw = dict(dim=[dim], real_dim=real_dim, scaling="density", detrend=None, window=None, shift=shift, spacing_tol=spacing_tol)
    full = _api.power_spectrum(stacks[0], **kw) if len(stacks) == 1 else _api.cross_spectrum(stacks[0], stacks[1], true_phase=true_phase, **kw)
    f = _to_device(from_any(full).data)
    rdt = f.real.dtype if f.is_complex() else f.dtype
    wt = torch.from_numpy(np.asarray(w, dtype=np.float64) * l).to(rdt).to(f.device).reshape((k,) + (1,) * (f.dim() - 1))
    return (f * wt).sum(dim=0)


def _multitaper(da, da2, dim, nw, k, nfft, weights, tapers, real_dim, detrend, shift, spacing_tol, true_phase, least=1):
    da = from_any(da)
    da2 = None if da2 is None else from_any(da2)
    if da2 is not None and (tuple(da2.dims) != tuple(da.dims) or da2.shape != da.shape):
        raise ValueError("The two datasets have different dimensions")
    n, l, k, d, w = _multitaper_args(da, dim, nw, k, nfft, weights, tapers)
    if k < least:
        raise ValueError(f"K = {k} taper(s): at least {least} are needed (of one spectrum the coherence is 1 everywhere)")
    if real_dim is not None and real_dim != dim:
        raise ValueError(f"real_dim must be {dim!r}, the one transform dimension, or None")
    if detrend not in (None, "constant", "linear"):
        raise NotImplementedError("%s is not a valid detrending option. Valid options are: 'constant','linear', or None." % detrend)
    das = [da] if da2 is None else [da, da2]
    heads = [_multitaper_head(x, dim, n, l, spacing_tol) for x in das]
    other = heads[0][1]
    heads = [h for h, _ in heads]
    # the labels, the scaling and the tables are those of the spectrum of ONE zero-extended series (no detrend there: it is taken over the N samples, below)
    c, c2, mode, scale, flags = _api._spectrum(heads[0], None if da2 is None else heads[1], [dim], real_dim, "density", False, true_phase,
                                               dict(detrend=None, window=None, shift=shift, spacing_tol=spacing_tol))
    det = {None: _lib.DETREND_NONE, "constant": _lib.DETREND_CONSTANT, "linear": _lib.DETREND_LINEAR}[detrend]
    if det == _lib.DETREND_LINEAR and math.prod(da.shape):
        for x in das:
            _refuse_nonfinite_span(x, dim, n)
    ax = da.get_axis_num(dim)
    ts = []
    for x in das:
        t = _to_device(x.data)
        ts.append(engine.convert(t.contiguous(), torch.float32) if t.dtype in (torch.float16, torch.bfloat16) else t)
    out = _multitaper_fused(c, c2, ts, ax, n, l, k, _taper_table(d, w), det, mode, scale * l, flags)
    if out is None:
        out = _multitaper_composed(das, heads, dim, l, d, w, detrend, real_dim, shift, spacing_tol, true_phase)
    res = _label_output(c, heads[0], out, other, _direct_lag_attrs(c) if c2 is not None and c.true_phase else None)  # (as _cross_result)
    res.attrs["tapers"] = k
    return res


def multitaper_power_spectrum(da, dim, NW=4.0, K=None, nfft=None, weights="unity", tapers=None, real_dim=None, detrend=None, shift=True, spacing_tol=1e-3):
    """Thomson's multitaper estimate of the power spectrum along ``dim``: the whole record of N samples is multiplied by K orthogonal Slepian (DPSS) tapers of
    time-bandwidth product ``NW`` (``K`` defaults to ``int(2 NW) - 1``; 1 <= K <= N), zero-extended to ``nfft`` = L samples (default: the smallest power of two
    >= N; a given ``nfft`` < N raises), transformed K times, and the K spectra are added with the weights w_j -- ``weights="unity"``: 1 / K; ``"eigen"``: the
    tapers' concentration ratios over their sum.  With y the series after ``detrend`` (None, "constant", "linear": over its N samples), d_j the tapers (unit L2
    norm) and dt the spacing of ``dim``:
        S[k] = dt sum_j w_j |sum_{n<N} d_j[n] y[n] exp(-2 pi i k n / L)|^2,   k over L frequencies of spacing 1 / (L dt)
    -- a density (sum_k S[k] / (L dt) = sum_j w_j sum_n (d_j y)^2[n]); there is no ``scaling`` argument.  ``real_dim=dim`` gives the half output k <= L / 2 with the
    factor 2 on 0 < k < L / 2.  ``tapers``: a real array (K, N) used as given instead of the DPSS (rows normalised to unit L2 norm; it replaces ``NW`` / ``K``, and
    ``weights="eigen"`` then raises).  The DPSS are computed in the library, in float64, from the symmetric tridiagonal eigenproblem
    (scipy.linalg.eigh_tridiagonal where scipy imports, else numpy.linalg.eigh), with scipy.signal.windows.dpss's signs and ratios, and remembered per (N, NW, K).
    Dims: the other dims in their order, then ``freq_<dim>``; coordinates, name and attrs are those ``power_spectrum`` gives for the same series zero-extended to L
    samples, plus ``attrs["tapers"] = K``.
    float32 data with L a power of two in 64 .. 4096 and K <= 32 are transformed by ONE pass (xrfthip_desc.seg_tapers): the series is read where it lies, neither
    the K tapered copies nor the K spectra reach memory.  A trailing ``dim`` with one pitch between the series is read in place; any other is arranged first (one
    transposed copy); float16 / bfloat16 are widened first.  Every other call -- float64, other L, K > 32, XRFTHIP_FASTW_TAPERS=0 -- composes: ``detrend``, a taper dim by
    broadcasting the table, zero-extension, ``power_spectrum``, the weighted sum.  A linear detrend refuses non-finite samples (ValueError)."""
    src = da
    return to_like(_multitaper(da, None, dim, NW, K, nfft, weights, tapers, real_dim, detrend, shift, spacing_tol, False), src)


def multitaper_cross_spectrum(da1, da2, dim, NW=4.0, K=None, nfft=None, weights="unity", tapers=None, real_dim=None, detrend=None, shift=True, spacing_tol=1e-3,
                              true_phase=True):
    """The multitaper cross spectrum ``dt sum_j w_j X1_j conj(X2_j)`` of two series under the same tapers (see ``multitaper_power_spectrum``), times the net
    true-phase factor of the two coordinates' origins exactly as ``cross_spectrum`` / ``welch_cross_spectrum`` apply it (``true_phase=False``: none).  Complex.  A
    descending coordinate under ``true_phase`` (the reference flips such a field) composes."""
    src = da1
    return to_like(_multitaper(da1, da2, dim, NW, K, nfft, weights, tapers, real_dim, detrend, shift, spacing_tol, true_phase), src)


def multitaper_coherence(da1, da2, dim, NW=4.0, K=None, nfft=None, weights="unity", tapers=None, real_dim=None, detrend=None, shift=True, spacing_tol=1e-3,
                         true_phase=True):
    """Magnitude-squared coherence ``|S12|^2 / (S11 S22)`` of the three multitaper spectra, composed as ``welch_coherence`` is: ``multitaper_cross_spectrum`` and
    ``multitaper_power_spectrum`` of each series, the division the library's (xrfthip_coherence; no clamp).  Fewer than two tapers: ValueError (of one spectrum the
    coherence is 1 everywhere)."""
    src = da1
    da1, da2 = from_any(da1), from_any(da2)
    a = (dim, NW, K, nfft, weights, tapers, real_dim, detrend, shift, spacing_tol)
    cs = _multitaper(da1, da2, *a, true_phase, least=2)
    p1, p2 = (_multitaper(x, None, *a, False) for x in (da1, da2))
    res = _api._coherence_result(cs, p1, p2, da1, da2)
    res.attrs["tapers"] = cs.attrs["tapers"]
    return to_like(res, src)
