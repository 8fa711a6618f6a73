"""The host side of a call: argument normalisation, coordinate validation, spacing / lag / frequency vectors, window vectors, engine flags and phase tables, the
labels of the result, the scale factors -- tiny float64 numpy work that must match the reference bit for bit -- and the upload of the data."""
from __future__ import annotations

import math
import warnings
from collections import OrderedDict

import numpy as np
import pandas as pd
import scipy.signal as sps
import torch
from pandas.api.types import is_datetime64_any_dtype, is_numeric_dtype

from . import _lib, engine
from ._plans import _akey, _memoised, _ro
from .labeled import Coordinate, DataArray

_WINDOW_NAMES = [  # xrft.py:48-72
    "hann", "hamming", "kaiser", "tukey", "parzen", "taylor", "boxcar", "barthann", "bartlett", "blackman",
    "blackmanharris", "bohman", "chebwin", "cosine", "dpss", "exponential", "flattop", "gaussian",
    "general_cosine", "general_gaussian", "general_hamming", "triang", "nuttall",
]
_real_flag_warning = ("`real` flag will be deprecated in future version of xrft.fft and replaced by `real_dim` flag.")


# ------------------------------------------------------------------------------------------------------
# coordinate helpers (host, float64) -- xrft.py:139-155, 195-234, 269-304
# ------------------------------------------------------------------------------------------------------
def _freq(N, delta_x, real, shift):
    key = ("freq", tuple(int(n) for n in N), tuple(float(d) for d in delta_x), real is not None, bool(shift))
    return list(_memoised(key, lambda: tuple(_ro(k) for k in _freq_uncached(N, delta_x, real, shift))))


def _freq_uncached(N, delta_x, real, shift, real_axis=np.fft.rfftfreq):
    fftfreq = [np.fft.fftfreq] * len(N)
    if real is not None:
        fftfreq[-1] = real_axis
    k = [f(Nx, dx) for (f, Nx, dx) in zip(fftfreq, N, delta_x)]
    if shift:
        k = [np.fft.fftshift(l) for l in k]
    return k


def _ifreq(N, delta_x, real, shift):
    """xrft.py:158-175: the real axis of an inverse transform gets the frequencies of its 2 (n - 1) output samples."""
    return _freq_uncached(N, delta_x, real, shift, lambda Nx, dx: np.fft.fftfreq(2 * (Nx - 1), dx))


def _stack_chunks(da, dim, suffix="_segment"):
    """xrft.py:106-136: reshape every chunked transform dimension d into (d_segment, d) -- a view, no copy."""
    newdims, newshape, newcoords = [], [], {}
    chunks = da._chunks or {}
    for d in da.dims:
        if d in dim:
            ch = chunks.get(d) or (da.sizes[d],)
            if np.diff(ch).sum() != 0:
                raise ValueError("Chunk lengths need to be the same.")
            n = da.sizes[d]
            chunklen = int(ch[0])
            coord_rs = np.asarray(da[d].values).reshape((int(n / chunklen), chunklen))
            newdims += [d + suffix, d]
            newshape += [int(n / chunklen), chunklen]
            newcoords[d + suffix] = np.arange(int(n / chunklen))
            newcoords[d] = coord_rs[0]
        else:
            newdims.append(d)
            newshape.append(da.sizes[d])
            if d in da.coords:
                newcoords[d] = da.coords[d]
    data = da.data
    if isinstance(data, torch.Tensor) and not data.is_contiguous():
        data = data.contiguous()
    return DataArray(data.reshape(newshape), newdims, newcoords, da.name, da.attrs)


def _diff_coord(coord):
    v0 = coord[0]
    if getattr(v0, "calendar", None):
        import cftime  # xrft.py:200-206; only reachable when cftime is installed

        decoded = cftime.date2num(coord, "seconds since 1800-01-01 00:00:00", v0.calendar)
        return np.diff(decoded)
    if pd.api.types.is_datetime64_dtype(v0):
        return np.diff(coord).astype("timedelta64[ns]").astype("f8") / 1e9
    return np.diff(coord)


def _lag_coord(coord):
    v0 = coord[0]
    coord_data = coord if coord[-1] > coord[0] else np.flip(coord, axis=-1)
    lag = coord_data[len(coord) // 2]
    if getattr(v0, "calendar", None):
        import cftime

        return cftime.date2num(lag, "seconds since 1800-01-01 00:00:00", v0.calendar)
    if pd.api.types.is_datetime64_dtype(v0):
        return lag.astype("timedelta64[s]").astype("f8")
    return lag


def _is_valid_fft_coord(coord):
    c0 = coord[0]
    return bool(is_numeric_dtype(coord) or is_datetime64_any_dtype(coord)
                or bool(getattr(c0.item() if hasattr(c0, "item") else c0, "calendar", False)))


def _get_coordinate_spacing(coord, spacing_tol, name):
    diff = _diff_coord(coord)
    delta = np.abs(diff[0])
    if not np.allclose(diff, diff[0], rtol=spacing_tol):
        raise ValueError("Can't take Fourier transform because coodinate %s is not evenly spaced" % name)
    if delta == 0.0:
        raise ValueError("Can't take Fourier transform because spacing in coordinate %s is zero" % name)
    return delta


def _dim_list(da, dim):
    """``dim`` as a list of names: None is every dim of ``da``, a string is one name."""
    if dim is None:
        return list(da.dims)
    return [dim] if isinstance(dim, str) else list(dim)


def _real_dim_last(da, dim, real_dim, what="real FT"):
    """``dim`` with ``real_dim`` moved to its end (xrft.py:380-386; ``what``: "real FT" forward, "real IFT" inverse)."""
    if real_dim not in da.dims:
        raise ValueError(f"The dimension along which {what} is taken must be one of the existing dimensions.")
    return [d for d in dim if d != real_dim] + [real_dim]


def _axis_roles(da, dim, real_dim):
    """(ydim, xdim), the device axis roles of one or two transform dims: x = the last listed dim when real (xrft.py:395-396), else the one stored last in memory."""
    if len(dim) == 1:
        return None, dim[0]
    if real_dim is not None or da.get_axis_num(dim[0]) < da.get_axis_num(dim[1]):
        return dim[0], dim[1]
    return dim[1], dim[0]


def _freq_name(d, prefix):
    """The name of the transformed dim (xrft.py:186): the prefix added, or stripped from a name that carries it."""
    return prefix + d if d[: len(prefix)] != prefix else d[len(prefix):]


def _freq_coords(dim, k, prefix):
    """(swap: dim -> new name, new_coords: new name -> Coordinate with its spacing) of the transformed dims (xrft.py:178-192)."""
    swap, new_coords = OrderedDict(), {}
    for d, kk in zip(dim, k):
        new_name = _freq_name(d, prefix)
        swap[d] = new_name
        new_coords[new_name] = Coordinate((new_name,), kk, {"spacing": kk[1] - kk[0]} if len(kk) > 1 else {}, new_name)
    return swap, new_coords


def _direct_lag_attrs(c):
    """The ``direct_lag`` attribute of every transformed coordinate (xrft.py:469), as _label_output takes it."""
    return {c.swap[d]: {"direct_lag": lag} for d, lag in zip(c.dim, c.lag_x)}


def _window_vector(window_type, n):
    if isinstance(window_type, str) and window_type in _WINDOW_NAMES:
        return _memoised(("window", window_type, int(n)), lambda: _ro(_window_vector_uncached(window_type, n)))
    return _window_vector_uncached(window_type, n)


def _window_vector_uncached(window_type, n):
    if window_type is True:  # xrft.py:42-47
        window_type = "hann"
        warnings.warn("Please provide the name of window adhering to scipy.signal.windows. The boolean option "
                      "will be deprecated in future releases.", FutureWarning)
    elif window_type not in _WINDOW_NAMES:
        raise NotImplementedError(f"Window type {window_type} not supported. Please adhere to "
                                  "scipy.signal.windows for naming convention.")
    return getattr(sps.windows, window_type)(n, sym=False)


# ------------------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------------------
_TORCH_OK = (torch.float32, torch.float64, torch.complex64, torch.complex128)
_TORCH_HALF = (torch.float16, torch.bfloat16)  # real half-precision fields: computed in float32 (the plan reads them where they lie, or engine.convert widens them once)


def _widen_half(t):
    """A float16 / bfloat16 device tensor as float32 (exact; the library's own one-pass kernel); anything else as it is."""
    return engine.convert(t, torch.float32) if t.dtype in _TORCH_HALF else t


def _to_device(data, keep_half=False):
    """``data`` on the device in a dtype the library computes on.  Half-precision fields travel and arrive as 2-byte samples; ``keep_half``: returned as they are (the
    two-trailing-axes route, whose plan may read them where they lie), else widened to float32 on the device."""
    dev = _lib.device()
    if isinstance(data, torch.Tensor):
        # the C library reads raw memory: materialise torch's lazy conjugate / negative views (x.conj(), x.mH)
        t = data.resolve_conj().resolve_neg()
    else:
        a = np.asarray(data)
        if a.dtype == np.float16:
            pass  # uploaded as float16: 2 bytes per sample over the bus
        elif a.dtype.kind in "biu":
            a = a.astype(np.float64)  # numpy.fft promotes integers to float64
        elif a.dtype.kind not in "fc":
            raise TypeError(f"cannot transform data of dtype {a.dtype}")
        elif a.dtype.itemsize > 8 and a.dtype.kind == "f" or a.dtype.itemsize > 16:
            a = a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype in _TORCH_HALF:
        t = t.to(dev)
        return t if keep_half else _widen_half(t)
    if t.dtype not in _TORCH_OK:
        t = t.to(torch.float64 if not t.is_complex() else torch.complex128)
    return t.to(dev)


class _Ctx:
    """Everything ``fft`` derives on the host before touching the device (xrft.py:370-433)."""


def _label_guard(da):
    """What the host analysis of a labelled array depends on: coordinate vectors are owned read-only arrays with a token that is
    issued once per assignment of ``Coordinate.values`` and never reused (labeled.Coordinate), so the same tokens mean the same
    labels.  None: do not remember anything (a coordinate array was made writeable again)."""
    toks = []
    for k, v in da.coords.items():
        vals = v.values
        if vals.flags.writeable:  # (someone re-opened the array for writing: its content is no longer pinned by the token)
            return None
        # ... plus a cheap fingerprint of the content (size, first, second and last sample: origin, spacing, extent): an array re-opened for
        # writing, changed and closed again between two calls keeps its token, and a deep copy shares it while owning another array
        n = vals.size
        fp = (n,) if n == 0 or vals.dtype.kind not in "fiuMm" else (n, vals.flat[0].item(), vals.flat[min(1, n - 1)].item(), vals.flat[n - 1].item())
        toks.append((k, v._token, fp))
    return (da.dims, da.shape, tuple(toks), None if not da._chunks else tuple(sorted(da._chunks.items())))


def _label_memo(da, key, compute):
    """``compute()``, remembered on the labelled array ``da`` under ``key`` for as long as its labels stay what they are (_label_guard); the store starts again
    after more than 16 keys.  ``key`` None, or labels that are not pinned: computed, nothing stored."""
    guard = None if key is None else _label_guard(da)
    if guard is None:
        return compute()
    memo = da._memo
    if memo is not None and memo[0] == guard:
        hit = memo[1].get(key)
        if hit is not None:
            return hit
    val = compute()
    memo = da._memo
    if memo is None or memo[0] != guard or len(memo[1]) > 16:
        memo = da._memo = (guard, {})
    memo[1][key] = val
    return val


def _analyze(da, spacing_tol, dim, real_dim, shift, detrend, window, true_phase, chunks_to_segments, prefix, real):
    """The host side of a call: every check the reference makes, spacings, lags, frequency coordinates.  Remembered on the labelled
    array per argument set (validation, coordinate digests and frequency vectors of a 65536-point axis cost ~0.1 ms a call, more
    than the transform of a small cube): a later call with the same arguments on the same labels starts from the stored context."""
    mkey = None
    if not chunks_to_segments and real is None and isinstance(spacing_tol, (int, float)):
        mkey = (spacing_tol, dim if (dim is None or isinstance(dim, str)) else tuple(dim), real_dim, shift, detrend, window, true_phase, prefix)
        try:
            hash(mkey)
        except TypeError:
            mkey = None
    if mkey is None:
        return _analyze_uncached(da, spacing_tol, dim, real_dim, shift, detrend, window, true_phase, chunks_to_segments, prefix, real)

    def compute():
        stored = _analyze_uncached(da, spacing_tol, dim, real_dim, shift, detrend, window, true_phase, chunks_to_segments, prefix, real)
        stored.da = None  # (kept out of the stored context: no reference cycle through the array and its device memory)
        stored._x = {}    # shared by every copy of this context: what _execute derives from it (flags, phase tables)
        return stored

    c = _Ctx()
    c.__dict__.update(_label_memo(da, mkey, compute).__dict__)
    c.da = da
    return c


def _analyze_uncached(da, spacing_tol, dim, real_dim, shift, detrend, window, true_phase, chunks_to_segments, prefix, real):
    c = _Ctx()
    c._x = None
    dim = _dim_list(da, dim)
    if real is not None:  # xrft.py:376-378
        real_dim = real
        warnings.warn(_real_flag_warning, FutureWarning)
    if real_dim is not None:
        dim = _real_dim_last(da, dim, real_dim)
    for d in dim:
        da.get_axis_num(d)
    if not np.all([_is_valid_fft_coord(da[d].values) for d in dim]):  # xrft.py:277-281
        raise ValueError("All transformed dimensions coordinates must be numerical or datetime.")
    c.corr_N = [da.sizes[d] for d in dim]  # window_correction uses the UNsegmented lengths (xrft.py:747 -> :654)
    if chunks_to_segments:  # xrft.py:390-391
        da = _stack_chunks(da, dim)
    elif da._chunks and any(len(da._chunks.get(d, (0,))) > 1 for d in dim):
        raise ValueError("The transform dimension(s) are split into several chunks; dask.array.fft refuses that "
                         "(use chunks_to_segments=True or rechunk).")
    c.da = da
    if real_dim is not None:
        shift = False  # xrft.py:403
    c.rawdims = da.dims
    c.dim, c.real_dim, c.shift = dim, real_dim, bool(shift)
    c.N = [da.sizes[d] for d in dim]
    for d in dim:  # xrft.py:412-420
        bad = [cn for cn, cv in da.coords.items() if cn != d and d in cv.dims]
        if bad:
            raise ValueError(f"The input array contains coordinate variable(s) ({bad}) whose dims include the "
                             f"transform dimension(s) `{d}`. Please drop these coordinates (`.drop({bad}`) "
                             "before invoking xrft.")
    def _coord_info(d):  # spacing check + lag of one coordinate vector, memoised on its bytes
        cv = np.asarray(da[d].values)
        if cv.dtype.kind not in "fiu" or not isinstance(spacing_tol, (int, float)):  # (a bad spacing_tol must fail in numpy, as in the reference)
            return _get_coordinate_spacing(cv, spacing_tol, d), _lag_coord(cv)
        key = ("coord", cv.dtype.str, cv.size, _akey(cv), float(spacing_tol))
        return _memoised(key, lambda: (_get_coordinate_spacing(cv, spacing_tol, d), _lag_coord(cv)))

    info = [_coord_info(d) for d in dim]
    c.delta_x = [i[0] for i in info]  # xrft.py:422
    c.lag_x = [i[1] for i in info]  # xrft.py:423
    if detrend not in (None, "constant", "linear"):  # detrend.py:46-50
        raise NotImplementedError("%s is not a valid detrending option. Valid options are: 'constant','linear', "
                                  "or None." % detrend)
    if len(dim) > 2 or len(dim) == 0:
        raise NotImplementedError("xrft_amd transforms one or two dimensions per call (the reference's N-D fftn / "
                                  "3-D linear detrend are outside the MI355X hot path, SURVEY.md 8f).")
    c.detrend = {None: _lib.DETREND_NONE, "constant": _lib.DETREND_CONSTANT, "linear": _lib.DETREND_LINEAR}[detrend]
    c.windows = None if window is None else [_window_vector(window, n) for n in c.N]
    c.true_phase = bool(true_phase)
    c.reversed = [bool(da[d].values[-1] < da[d].values[0]) for d in dim] if true_phase else [False] * len(dim)
    c.ydim, c.xdim = _axis_roles(da, dim, real_dim)
    c.k = _freq(c.N, c.delta_x, real_dim, c.shift)  # xrft.py:449
    c.k_unshifted = _freq(c.N, c.delta_x, real_dim, False)
    c.prefix = prefix
    c.swap, c.new_coords = _freq_coords(dim, c.k, prefix)
    return c


def _flags_tables(c, da, other_lag=None, other_reversed=None):
    """Engine flags, window vectors and phase tables per device axis (y, x).  ``other_reversed``: cross spectra -- the
    reference flips each field by its own coordinate (xrft.py:436-441): ``c`` is field 0 (FLIP0_*), the other field 1.
    Remembered on a stored context (the phase factors of a 65536-point axis are 0.8 ms of numpy per call)."""
    x = getattr(c, "_x", None)
    if x is None:
        return _flags_tables_uncached(c, other_lag, other_reversed)
    key = ("ft", None if other_lag is None else tuple(float(v) for v in other_lag), None if other_reversed is None else tuple(other_reversed))
    hit = x.get(key)
    if hit is None:
        flags, win, ph = _flags_tables_uncached(c, other_lag, other_reversed)
        for v in ph.values():
            if v is not None:
                v.setflags(write=False)
        hit = x[key] = (flags, win, ph)
    return hit[0], dict(hit[1]), dict(hit[2])


def _flags_tables_uncached(c, other_lag, other_reversed):
    flags = 0
    win = {"y": None, "x": None}
    ph = {"y": None, "x": None}
    for i, d in enumerate(c.dim):
        ax = "x" if d == c.xdim else "y"
        if c.shift:
            flags |= _lib.SHIFT_X if ax == "x" else _lib.SHIFT_Y
        if c.true_phase:
            flags |= _lib.ISHIFT_X if ax == "x" else _lib.ISHIFT_Y
            if other_reversed is None:
                if c.reversed[i]:
                    flags |= _lib.FLIP_X if ax == "x" else _lib.FLIP_Y
            else:
                if c.reversed[i]:
                    flags |= _lib.FLIP0_X if ax == "x" else _lib.FLIP0_Y
                if other_reversed[i]:
                    flags |= _lib.FLIP_X if ax == "x" else _lib.FLIP_Y
            # xrft.py:462-469 -- indexed by unshifted frequency; the real axis uses rfftfreq on its kept half
            n = c.N[i]
            f = np.fft.fftfreq(n, c.delta_x[i])
            if c.real_dim is not None and d == c.real_dim:
                f[: n // 2 + 1] = np.fft.rfftfreq(n, c.delta_x[i])
            p = np.exp(-1j * 2.0 * np.pi * f * c.lag_x[i])
            if other_lag is not None:  # cross spectrum: F1 phase * conj(F2 phase)
                p = p * np.conj(np.exp(-1j * 2.0 * np.pi * f * other_lag[i]))
            ph[ax] = p
        if c.windows is not None:
            win[ax] = c.windows[i]
    if c.real_dim is not None:
        flags |= _lib.HALF_X
    return flags, win, ph


def _swap_xy(flags):
    """The per-axis flag bits with the roles of x and y exchanged."""
    pairs = ((_lib.SHIFT_X, _lib.SHIFT_Y), (_lib.ISHIFT_X, _lib.ISHIFT_Y), (_lib.FLIP_X, _lib.FLIP_Y), (_lib.HALF_X, _lib.HALF_Y), (_lib.FLIP0_X, _lib.FLIP0_Y))
    out = flags
    for fx, fy in pairs:
        out &= ~(fx | fy)
    for fx, fy in pairs:
        if flags & fx:
            out |= fy
        if flags & fy:
            out |= fx
    return out


def _label_output(c, da, out_t, other, extra_cattrs=None, dropped=(), lags=None, validate=False):
    """Wrap the engine output (other..., ky, kx) as a DataArray in the reference's dim order (xrft.py:451-476).
    ``other is None``: the output already has the input's dim order (in-place axis transform).  ``dropped``: dims the plan averaged over -- they and the
    coordinates that span them leave, as DataArray.mean drops them.  ``lags``: per new coordinate name what its values are shifted by (ifft, xrft.py:634-639;
    keep_attrs: the spacing attribute survives).  ``validate``: the validating constructor whatever the coordinates."""
    tdims = ([c.ydim] if c.ydim is not None else []) + [c.xdim]
    final = [c.swap.get(d, d) for d in c.rawdims]
    keep = da.coords.items()
    if dropped:  # (kept off the path of every other call)
        final = [c.swap.get(d, d) for d in c.rawdims if d not in dropped]
        other = [d for d in other if d not in dropped]
        keep = [(k, v) for k, v in keep if not set(v.dims) & set(dropped)]
    if other is not None:
        cur = other + [c.swap[d] for d in tdims]
        out_t = out_t.reshape([da.sizes[d] for d in other] + list(out_t.shape[-len(tdims):]))
        if cur != final:
            out_t = out_t.permute([cur.index(d) for d in final])
    coords = {k: v._clone(k) for k, v in keep if k not in c.dim}  # (own objects over the input's immutable values)
    for name, cv in c.new_coords.items():
        attrs = dict(cv.attrs)
        if extra_cattrs and name in extra_cattrs:
            attrs.update(extra_cattrs[name])
        coords[name] = Coordinate(cv.dims, cv.values if lags is None else cv.values + lags[name], attrs, name)
    if validate or any(d in c.dim for k, v in da.coords.items() if k not in c.dim for d in v.dims):
        return DataArray(out_t, final, coords, None, None)  # (a kept coordinate that spans a transformed dim: the validating constructor's error, as before)
    return DataArray._trusted(out_t, final, coords)


def _nd_scale(da, dims, window, scaling, window_correction, spacings):
    """What multiplies |F|^2 (or F1 conj F2) of a spectrum over the dims ``dims`` beyond the (prod dx)^2 of the transforms: / window factor, x prod(dk)^(1|2)
    (xrft.py:745-748); ``spacings``: the frequency spacings in the order of ``dims``."""
    scale = 1.0
    if scaling != "false_density":
        if window_correction:
            if window is None:
                raise ValueError("window_correction can only be applied when windowing is turned on.")
            vecs = [_window_vector(window, da.sizes[d]) for d in dims]
            if scaling == "density":
                scale /= float(np.prod([(v ** 2).mean() for v in vecs]))
            elif scaling == "spectrum":
                scale /= float(np.prod([v.mean() for v in vecs])) ** 2
            else:
                raise ValueError("Unknown {} scaling flag".format(scaling))
        fs = float(math.prod(spacings))
        if scaling == "density":
            scale *= fs
        elif scaling == "spectrum":
            scale *= fs ** 2
        else:
            raise ValueError("Unknown {} scaling flag".format(scaling))
    return scale


def _window_correction_factor(c, scaling, window):
    """xrft.py:649-660: mean(w^2) (density) or mean(w)^2 (spectrum) of the outer-product window."""
    if window is None:
        raise ValueError("window_correction can only be applied when windowing is turned on.")
    vecs = [_window_vector(window, n) for n in c.corr_N]
    w = vecs[0]
    for v in vecs[1:]:
        w = np.multiply.outer(w, v)
    if scaling == "density":
        return (w ** 2).mean()
    elif scaling == "spectrum":
        return w.mean() ** 2
    raise ValueError("Unknown {} scaling flag".format(scaling))


def _psd_scaling_factor(c, scaling):
    """xrft.py:663-670."""
    fs = math.prod([float(c.new_coords[c.swap[d]].attrs["spacing"]) for d in c.dim])
    if scaling == "density":
        return fs
    elif scaling == "spectrum":
        return fs ** 2
    raise ValueError("Unknown {} scaling flag".format(scaling))


def _spectrum_scale(c, amp, scaling, window_correction, window):
    """Everything that multiplies |F|^2 (or F1 conj F2): (prod dx)^2, / window factor, x prod(dk)^(1|2)."""
    scale = float(amp)
    if scaling != "false_density":  # xrft.py:745-748
        if window_correction:
            scale = scale / _window_correction_factor(c, scaling, window)
        scale = scale * _psd_scaling_factor(c, scaling)
    return scale
