"""The radial bins of the isotropic spectra (xrft.py:877-1010) -- host float64, cached -- and ``isotropize`` of an existing spectrum."""
from __future__ import annotations

import warnings
from collections import OrderedDict

import numpy as np
import pandas as pd
import torch

from . import engine
from ._hostside import _to_device
from ._plans import _digest, _plan_lock
from .labeled import Coordinate, DataArray, from_any, to_like

_bins_cache: "OrderedDict[tuple, tuple]" = OrderedDict()


def _radial_bins(k, l, nfactor, ref_order=None):
    """Bin codes and per-bin mean radius for the grid sqrt(k^2 + l^2), dims (k, l)  (xrft.py:975-981, 910-923).

    ``pd.cut`` on the float64 radii, exactly the reference's expression; the per-bin mean replaces
    ``numpy_groupies.aggregate(func="mean", fill_value=0)``.  The result depends only on the two frequency vectors
    and nfactor, and costs seconds of host time at 4096^2, so it is cached (the reference recomputes it per call).
    """
    key = (k.size, l.size, _digest(k), _digest(l), nfactor, ref_order)
    with _plan_lock:
        hit = _bins_cache.get(key)
        if hit is not None:
            _bins_cache.move_to_end(key)
            return hit
    res = _radial_bins_uncached(k, l, nfactor, ref_order) + (key,)
    with _plan_lock:
        _bins_cache[key] = res
        while len(_bins_cache) > 8:
            _bins_cache.popitem(last=False)
    return res


def _radial_bins_uncached(k, l, nfactor, ref_order=None):
    N = [k.size, l.size]
    nbins = int(min(N) / nfactor)
    freq_r = np.sqrt(k[:, None] ** 2 + l[None, :] ** 2)
    binned = pd.cut(np.ravel(freq_r), nbins)
    codes = binned.codes.reshape(freq_r.shape)
    nb = binned.categories.size
    cr, fr = codes, freq_r
    if ref_order is not None:
        # The bin-centre coordinate is a per-bin MEAN: its last bits depend on the order of the sum.  The reference sums
        # over the (fftdim[1], fftdim[0]) grid of the SHIFTED coordinates (xrft.py:980-981); visit the same cells in the
        # same order (the codes and radii themselves are order-independent).
        shift_k, shift_l, transpose = ref_order
        ik = np.fft.fftshift(np.arange(k.size)) if shift_k else np.arange(k.size)
        il = np.fft.fftshift(np.arange(l.size)) if shift_l else np.arange(l.size)
        cr, fr = codes[np.ix_(ik, il)], freq_r[np.ix_(ik, il)]
        if transpose:
            cr, fr = cr.T, fr.T
    valid = cr >= 0
    cnt = np.bincount(cr[valid], minlength=nb)
    s_ = np.bincount(cr[valid], weights=fr[valid], minlength=nb)
    kr = np.where(cnt > 0, s_ / np.maximum(cnt, 1), 0.0)
    return codes.astype(np.int32), kr, nb


def _finish_iso(kr, k, l, truncate, iso_vals):
    """truncate / dropna semantics of xrft.py:983-991, 1007-1010 (dropna only looks at data values)."""
    if truncate:
        kmax = l.max() if k.max() > l.max() else k.max()
        kr = np.where(kr <= kmax, kr, np.nan)
        keep = ~np.isnan(iso_vals).reshape(-1, iso_vals.shape[-1]).any(axis=0)
        if not keep.all():
            iso_vals, kr = iso_vals[..., keep], kr[keep]
    else:
        warnings.warn("Isotropic wavenumber larger than the Nyquist wavenumber may result.", FutureWarning)
    return kr, iso_vals


def isotropize(ps, fftdim, nfactor=4, truncate=True, complx=False):
    """Azimuthal (radial-bin) SUM of an existing 2-D spectrum (xrft/xrft.py:948-1010)."""
    src = ps
    ps = from_any(ps)
    k = np.asarray(ps[fftdim[1]].values, dtype=np.float64)
    l = np.asarray(ps[fftdim[0]].values, dtype=np.float64)
    codes, kr, nb, _ = _radial_bins(k, l, nfactor)  # dims (fftdim[1], fftdim[0])
    other = [d for d in ps.dims if d not in fftdim]
    order = other + [fftdim[1], fftdim[0]]
    t = _to_device(ps.data)
    if tuple(order) != tuple(ps.dims):
        t = t.permute([ps.get_axis_num(d) for d in order])
    t = t.contiguous()
    bm = torch.from_numpy(np.ascontiguousarray(codes)).to(t.device)
    iso = engine.isotropize(t, bm, nb)
    iso = iso.reshape([ps.sizes[d] for d in other] + [nb])
    vals = iso.cpu().numpy() if truncate else iso  # (truncate: dropna inspects the data values, xrft.py:1007-1008)
    kr, vals = _finish_iso(kr, k, l, truncate, vals)
    coords = {c: v for c, v in ps.coords.items() if not (set(v.dims) & set(fftdim))}
    coords["freq_r"] = Coordinate(("freq_r",), kr, None, "freq_r")
    return to_like(DataArray(vals, other + ["freq_r"], coords, ps.name, ps.attrs), src)
