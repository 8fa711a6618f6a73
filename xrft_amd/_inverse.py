"""The inverse transforms ``ifft`` / ``idft`` (xrft.py:479-646): host side, the plans along trailing, middle and non-adjacent axes, the ways round a long prime length."""
from __future__ import annotations

import math
import warnings

import numpy as np
import torch

from . import _lib, engine
from ._bluestein import _bluestein_1d
from ._hostside import (_Ctx, _axis_roles, _dim_list, _freq_coords, _get_coordinate_spacing, _ifreq, _is_valid_fft_coord, _label_memo, _label_output, _lag_coord,
                        _real_dim_last, _real_flag_warning, _stack_chunks, _swap_xy, _to_device)
from ._plans import _TWO_STAGE, _TWO_STAGE_SIZE, _akey, _get_plan, _plan_lock, _ro
from .labeled import from_any, to_like


def _ifft_host(daft, dim, lag, real_dim, shift, true_phase, spacing_tol, prefix):
    """The host side of an inverse transform (xrft.py:574-576, 598-623): the input phase factors by SOURCE position, the index map that sorting + ifftshift amount to,
    spacing and centring checks, the lag coordinates of the result.  Pure in the labels and the arguments: ifft remembers it per labelled array."""
    phase = {d: (_ro(np.exp(1j * 2.0 * np.pi * np.asarray(daft[d].values, dtype=np.float64) * l)) if true_phase else None)
             for d, l in zip(dim, lag)}
    N = [daft.sizes[d] for d in dim]
    # sortby(dim) + ifftshift (xrft.py:598, 612-614) expressed as an index map of the engine: ascending coordinates ->
    # ISHIFT, descending -> FLIP + ISHIFT, the unshifted layout (fftshift(sort) == identity) -> nothing
    coords_sorted, maps = {}, {}
    for d, n in zip(dim, N):
        cv = np.asarray(daft[d].values)
        order = np.argsort(cv, kind="stable")
        coords_sorted[d] = cv[order]
        if d == real_dim:
            if not np.array_equal(order, np.arange(n)):
                raise ValueError("the real dimension's frequency coordinate must be ascending (rfftfreq order)")
            maps[d] = "none"
            continue
        want = order[(np.arange(n) + n // 2) % n]  # source index feeding unshifted position m
        if np.array_equal(want, np.arange(n)):
            maps[d] = "none"
        elif np.array_equal(order, np.arange(n)):
            maps[d] = "ishift"
        elif np.array_equal(order, np.arange(n)[::-1]):
            maps[d] = "flip_ishift"
        else:
            maps[d] = want  # arbitrary permutation: gather on the device first
    delta_x = [_get_coordinate_spacing(coords_sorted[d], spacing_tol, d) for d in dim]
    for d in dim:  # xrft.py:600-606
        l = _lag_coord(coords_sorted[d]) if d is not real_dim else coords_sorted[d][0]
        if np.abs(l) > spacing_tol:
            raise ValueError("Inverse Fourier Transform can not be computed because coordinate %s is not centered on "
                             "zero frequency" % d)
    swap, new_coords = _freq_coords(dim, _ifreq(N, delta_x, real_dim, shift), prefix)  # xrft.py:623
    return phase, maps, N, swap, new_coords


def _ifft_args(daft, dim, real_dim, real, lag, true_phase):
    """(dim, real_dim, lag) after the reference's checks and warnings (xrft.py:540-566): the real dimension last, one lag per dim."""
    dim = _dim_list(daft, dim)
    if real is not None:
        real_dim = real
        warnings.warn(_real_flag_warning, FutureWarning)
    if real_dim is not None:
        dim = _real_dim_last(daft, dim, real_dim, "real IFT")
    for d in dim:
        daft.get_axis_num(d)
    if not np.all([_is_valid_fft_coord(daft[d].values) for d in dim]):
        raise ValueError("All transformed dimensions coordinates must be numerical or datetime.")
    if lag is None:  # xrft.py:557-560
        lag = [daft[d].attrs.get("direct_lag", 0.0) for d in dim]
        warnings.warn("Default ifft's behaviour (lag=None) changed! Default value of lag was zero (centered output "
                      "coordinates) and is now set to transformed coordinate's attribute: 'direct_lag'.", FutureWarning)
    else:
        if isinstance(lag, float) or isinstance(lag, int):
            lag = [lag]
        if len(dim) != len(lag):
            raise ValueError("dim and lag must have the same length.")
        if not true_phase:
            warnings.warn("Setting lag with true_phase=False does not guarantee accurate ifft.", Warning)
        lag = [daft[d].attrs.get("direct_lag") if l is None else l for d, l in zip(dim, lag)]
    if len(dim) == 0:
        raise NotImplementedError("xrft_amd needs at least one transform dimension")
    return dim, real_dim, lag


def _ifft_staged(daft, groups, real_dim, lag_of, **kw):
    """ifftn / irfftn are separable (xrft.py:612-621): one ``ifft`` per group of dims, in order -- the group that holds the real dimension, whose c2r step must come
    last, at the end.  Each stage has its own plan where its axes lie, or its own way round a long prime length (Bluestein through global memory)."""
    cur = daft
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for grp in groups:
            cur = from_any(ifft(cur, dim=grp, real_dim=real_dim if real_dim in grp else None, lag=[lag_of[d] for d in grp], **kw))
    return cur


def _ifft_axis(m, p, n, true_phase, shift):
    """One inverse transform axis in the terms of the plan's x axis (_swap_xy: of its y axis), from the axis' index map ``m``, input phase table ``p`` and output
    length ``n``: (flags, phase table, index of a device gather or None, roll of the output).  Output: "if not true_phase: ifftshift" then "if shift: fftshift"
    (xrft.py:617-621) -- the two cancel (even n: they are inverses; odd n: roll(-(n//2)) then roll(+n//2)); the engine's output shift is fftshift, so what
    remains is only the fftshift (a flag), or only the ifftshift (a roll afterwards)."""
    flags, index, roll = 0, None, 0
    if isinstance(m, np.ndarray):  # gather to the unshifted layout on the device; the phase follows the data
        index = m
        p = None if p is None else p[m]
    elif m == "ishift":
        flags |= _lib.ISHIFT_X
    elif m == "flip_ishift":
        flags |= _lib.ISHIFT_X | _lib.FLIP_X
    if p is not None:
        flags |= _lib.PHASE_IN
    if true_phase:
        if shift:
            flags |= _lib.SHIFT_X
    elif not shift:
        roll = -(n // 2)
    return flags, p, index, roll


def ifft(daft, spacing_tol=1e-3, dim=None, real_dim=None, shift=True, true_phase=True, true_amplitude=True,
         chunks_to_segments=False, prefix="freq_", lag=None, real=None):
    """Inverse discrete Fourier transform (reference: xrft/xrft.py:479-646; same arguments).  The input phase factor,
    the coordinate sort / ifftshift, the conjugate-FFT-conjugate inverse, the 1/N and 1/prod(dk) factors and (for
    ``real_dim``) the Hermitian extension of the half spectrum are fused into one device plan."""
    src = daft
    daft = from_any(daft)
    dim, real_dim, lag = _ifft_args(daft, dim, real_dim, real, lag, true_phase)
    kw = dict(spacing_tol=spacing_tol, shift=shift, true_phase=true_phase, true_amplitude=true_amplitude, prefix=prefix)
    lag_of = dict(zip(dim, lag))
    if len(dim) > 2:  # complex stages over the leading dims first, two at a time
        if chunks_to_segments:
            raise NotImplementedError("chunks_to_segments is implemented for one or two transform dimensions.")
        return to_like(_ifft_staged(daft, [dim[i:i + 2] for i in range(0, len(dim), 2)], real_dim, lag_of, **kw), src)
    if len(dim) == 2 and real_dim is None and not chunks_to_segments and sorted(daft.get_axis_num(d) for d in dim) != [len(daft.dims) - 2, len(daft.dims) - 1]:
        # two inverse transform axes that are not the trailing pair: each axis has a plan that runs where the axis lies (XRFTHIP_AXIS_Y | XRFTHIP_INVERSE; the
        # contiguous axis: the row kernels) -- one axis at a time, no transposed copy of the spectrum or of the result
        return to_like(_ifft_staged(daft, [[d] for d in sorted(dim, key=daft.get_axis_num)], None, lag_of, **kw), src)
    if chunks_to_segments:  # (not remembered)
        phase = {d: (np.exp(1j * 2.0 * np.pi * np.asarray(daft[d].values, dtype=np.float64) * l) if true_phase else None) for d, l in zip(dim, lag)}  # (before the reshape)
        daft = _stack_chunks(daft, dim)
        _ph, maps, N, swap, new_coords = _ifft_host(daft, dim, lag, real_dim, shift, False, spacing_tol, prefix)
    else:
        # everything the host derives from the labels (phase tables of a 2^20-point axis, sorting, spacing, centring, lag coordinates: ~15 ms of numpy per call)
        # is remembered on the labelled array per argument set, as the forward calls do (_analyze)
        try:
            mkey = ("ifft", tuple(dim), tuple(float(l) for l in lag), real_dim, bool(shift), bool(true_phase), float(spacing_tol), prefix)
            hash(mkey)
        except (TypeError, ValueError):
            mkey = None
        phase, maps, N, swap, new_coords = _label_memo(daft, mkey, lambda: _ifft_host(daft, dim, lag, real_dim, shift, true_phase, spacing_tol, prefix))
    c = _Ctx()  # (what _label_output reads)
    c.dim, c.rawdims, c.swap, c.new_coords = dim, daft.dims, swap, new_coords
    c.ydim, c.xdim = _axis_roles(daft, dim, real_dim)  # device layout: x = real dim if given, else the later axis
    lags = {swap[d]: l for d, l in zip(dim, lag)}
    t = _to_device(daft.data)
    if not t.is_complex():
        t = t.to(torch.complex64 if t.dtype == torch.float32 else torch.complex128)
    n_out = N if real_dim is None else N[:-1] + [2 * (N[-1] - 1)]
    steps = {d: _ifft_axis(maps[d], phase[d], n, true_phase, shift) for d, n in zip(dim, n_out)}
    scale = 1.0 / (float(n_out[-1]) * float(n_out[0] if len(dim) == 2 else 1))  # 1 / (nx ny)
    if true_amplitude:  # xrft.py:641-642
        scale = scale / math.prod([float(new_coords[swap[d]].attrs["spacing"]) for d in dim])
    k = daft.get_axis_num(c.xdim)
    if len(dim) == 1 and real_dim is None and k != len(daft.dims) - 1 and isinstance(maps[c.xdim], str) and maps[c.xdim] in ("none", "ishift"):
        # one inverse transform along a first / middle axis: where the axis lies (XRFTHIP_AXIS_Y), no transposed copies -- as the forward call
        fl, p, _, roll = steps[c.xdim]
        out = _ifft_axis_y(t, k, _swap_xy(fl), p, roll, float(scale))
        if out is not None:
            return to_like(_label_output(c, daft, out, None, lags=lags, validate=True), src)
    try:
        out, other = _ifft_trailing(daft, t, c, steps, real_dim, float(scale))
    except _lib.XrftHipError as e:
        if e.status != _lib.UNSUPPORTED_LENGTH:
            raise
        if len(dim) != 2 or chunks_to_segments:
            raise ValueError(f"transform length(s) {dict(zip(dim, N))} not supported on the device: a length with a prime factor above 128 must "
                             f"be <= ~{8800 if t.dtype == torch.complex64 else 4400} samples (Bluestein inside one LDS tile) unless it is the only transform axis") from e
        # two axes, one of them a length no two-axis plan takes: one axis at a time
        return to_like(_ifft_staged(daft, [[dim[0]], [dim[1]]], real_dim, lag_of, **kw), src)
    return to_like(_label_output(c, daft, out, other, lags=lags, validate=True), src)


def _ifft_trailing(daft, t, c, steps, real_dim, scale):
    """The inverse plan over the trailing axes of the arranged spectrum (*other, [ny,] nx): (result, other dims).  One long prime axis goes through Bluestein in
    global memory; XRFTHIP_UNSUPPORTED_LENGTH is raised where no plan and no such way exists (the caller stages two axes, or refuses)."""
    tdims = ([c.ydim] if c.ydim is not None else []) + [c.xdim]
    other = [d for d in daft.dims if d not in tdims]
    if tuple(other + tdims) != tuple(daft.dims):
        t = t.permute([daft.get_axis_num(d) for d in other + tdims])
    ph, axflags, post_roll = {"y": None, "x": None}, {"y": 0, "x": 0}, []
    for d in c.dim:
        ax = "x" if d == c.xdim else "y"
        fl, ph[ax], index, roll = steps[d]
        if index is not None:
            t = engine.gather_axis(t, t.dim() - 1 if ax == "x" else t.dim() - 2, index=index)
        axflags[ax] = fl if ax == "x" else _swap_xy(fl)
        if roll:
            post_roll.append((ax, roll))
    t = t.contiguous()
    if real_dim is not None:
        axflags["x"] |= _lib.C2R_X
    flags = _lib.INVERSE | axflags["y"] | axflags["x"]
    nx_in = daft.sizes[c.xdim]
    nx = 2 * (nx_in - 1) if real_dim is not None else nx_in
    ny = daft.sizes[c.ydim] if c.ydim is not None else 1
    batch = t.numel() // max(ny * nx_in, 1)
    try:
        out = None
        if len(c.dim) == 2 and not (flags & (_lib.FLIP_X | _lib.FLIP_Y)):
            out = _ifft_two_stages(t, batch, ny, nx, flags, axflags, scale, ph)
        if out is None:
            plan = _get_plan(ndim=len(c.dim), batch=batch, ny=ny, nx=nx, dtype=t.dtype, out_mode=_lib.OUT_COMPLEX,
                             detrend=_lib.DETREND_NONE, flags=flags, scale=scale, window_y=None, window_x=None,
                             phase_y=ph["y"], phase_x=ph["x"])
            out, _ = plan.execute(t)
    except _lib.XrftHipError as e:
        if e.status != _lib.UNSUPPORTED_LENGTH or len(c.dim) != 1 or (real_dim is not None and (flags & (_lib.FLIP_X | _lib.ISHIFT_X))):
            raise
        if real_dim is not None:
            out = _irfft_bluestein(t, nx_in, nx, flags, scale, ph["x"])
        else:
            out = _bluestein_1d(t, nx, _lib.OUT_COMPLEX, _lib.DETREND_NONE, flags & ~_lib.PHASE_IN, scale, None, None, phase_in=ph["x"])
    for ax, sh in post_roll:
        out = engine.gather_axis(out, out.dim() - 1 if ax == "x" else out.dim() - 2, roll=sh)
    return out, other


def _irfft_bluestein(t, nx_in, nx, flags, scale, phx):
    """irfft of a long prime length: x[j] = Re sum_k Y[k] e^(+2 pi i jk / n) with Y = the stored half spectrum, its interior samples doubled, zero beyond n/2 -- the
    zero padding and the factors ride on a table multiply, then the inverse Bluestein pipeline; the real part is a device gather over the (re, im) pairs."""
    two = np.full(nx_in, 2.0)
    two[0] = 1.0
    if nx % 2 == 0:
        two[-1] = 1.0
    fac = two.astype(np.complex128) if phx is None else two * np.asarray(phx, dtype=np.complex128)
    y = engine.table_mul(t.reshape(-1, nx_in), torch.from_numpy(fac).to(t.dtype).to(t.device), nx)
    z = _bluestein_1d(y, nx, _lib.OUT_COMPLEX, _lib.DETREND_NONE, flags & ~(_lib.PHASE_IN | _lib.C2R_X), scale, None, None)
    return engine.gather_axis(torch.view_as_real(z.contiguous()), 2, index=np.array([0])).reshape(list(t.shape[:-1]) + [nx])


def _ifft_two_stages(t, batch, ny, nx, flags, axflags, scale, ph):
    """A two-axis inverse transform of (batch, ny, nx) complex data -- or of (batch, ny, nx / 2 + 1) half spectra with XRFTHIP_C2R_X in ``flags`` -- as two one-axis
    passes: ifftn / irfftn are separable (xrft.py:612-621), y where it lies (XRFTHIP_AXIS_Y) on the stored columns, then x along the rows (the c2r step last).
    ``axflags``: the bits of ``flags`` per axis (_ifft_axis), no flips among them.
    Only when BOTH stages run well on one-pass kernels (csrc/fastg.h) and the two-axis plan would not: the generic two-axis passes take 30-38 GFFT/s, the stages 100
    each.  Returns None otherwise (the caller builds the two-axis plan)."""
    c2r = bool(flags & _lib.C2R_X)
    nxs = nx // 2 + 1 if c2r else nx  # stored columns
    if t.dtype == torch.complex64 and ny in (256, 512, 1024, 2048, 4096) and (nx in (512, 1024, 2048, 4096) if c2r else nx in (256, 512, 1024, 2048, 4096)):
        return None  # (the two-pass pipeline on complex slabs, csrc/fasty_c2c.h: one plan, a tiled intermediate written in whole lines)
    if ny * nx > (1 << 31) - 1 or batch * ny * nx == 0:
        return None
    fy = _lib.AXIS_Y | _lib.INVERSE | axflags["y"]
    fx = _lib.INVERSE | axflags["x"]
    # the decision is taken once per shape / flag / phase-table set and remembered here (not as an attribute hung on a cached plan)
    dkey = (batch, ny, nx, str(t.dtype), int(flags), float(scale), _akey(ph["y"]), _akey(ph["x"]), engine.bluestein_in_float64())
    def stage_plans():
        py_ = _get_plan(ndim=2, batch=batch, ny=ny, nx=nxs, dtype=t.dtype, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=fy, scale=1.0 / float(ny),
                        window_y=None, window_x=None, phase_y=ph["y"], phase_x=None)
        px_ = _get_plan(ndim=1, batch=batch * ny, ny=1, nx=nx, dtype=t.dtype, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=fx, scale=scale * float(ny),
                        window_y=None, window_x=None, phase_y=None, phase_x=ph["x"])
        return py_, px_

    with _plan_lock:
        dec = _TWO_STAGE.get(dkey)
        if dec is not None:
            _TWO_STAGE.move_to_end(dkey)
    if dec is False:
        return None
    if dec is None:
        try:
            py, px = stage_plans()
            # ... and run well: four complex columns or more per workgroup along y (32-byte row segments at least), two rows or more per workgroup along x (one long
            # row per workgroup runs at half the rate: (16, 4096, 4096) 24 GFFT/s in two such stages against 30 on the two-axis plan).  Decided on the kernel
            # kinds the C ABI reports (xrfthip_plan_kernel_info), not on the text of describe()
            (ky, cy), (kx, rx) = py.kernel_info(), px.kernel_info()
            seg = cy * t.element_size()  # bytes of a row one column workgroup reads
            good = ((ky == _lib.K_FASTG_Y and seg >= 32) or (ky == _lib.K_FASTM_Y and seg >= 16)) and ((kx in (_lib.K_FASTG_ROWS, _lib.K_FASTM_X) and rx >= 2) or kx == _lib.K_FASTR)  # (K_FASTR: complex rows in registers, csrc/fastr.h fastc_kernel)
            if good and ny * nxs <= 20000:  # (a slab this small may run in ONE pass over both axes: only then is the two-axis plan built to ask)
                whole = _get_plan(ndim=2, batch=batch, ny=ny, nx=nx, dtype=t.dtype, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=flags, scale=scale,
                                  window_y=None, window_x=None, phase_y=ph["y"], phase_x=ph["x"])
                good = whole.kernel_info()[0] == _lib.K_GENERIC
        except _lib.XrftHipError as e:
            if e.status not in (_lib.UNSUPPORTED_LENGTH, _lib.BAD_ARG):
                raise
            good = False
        dec = bool(good)
        with _plan_lock:
            _TWO_STAGE[dkey] = dec
            while len(_TWO_STAGE) > _TWO_STAGE_SIZE:
                _TWO_STAGE.popitem(last=False)
        if dec is False:
            return None
    py, px = stage_plans()  # (through _plan_cache every call: evicted plans are rebuilt, none is kept alive from here)
    mid, _ = py.execute(t.reshape(batch, ny, nxs))
    out, _ = px.execute(mid.reshape(batch * ny, 1, nxs))
    return out.reshape(list(t.shape[:-1]) + [nx])


def _ifft_axis_y(t, k, flags, phase, roll, scale):
    """ifft along axis k < last of the C-contiguous tensor ``t`` where the axis lies: (batch, n, inner) with XRFTHIP_AXIS_Y | XRFTHIP_INVERSE and the axis' own
    ``flags``, ``phase`` and ``roll`` (_ifft_axis, as y); None when no such plan exists (the caller takes the transposing path)."""
    t = t.contiguous()
    shape = list(t.shape)
    n = shape[k]
    inner = int(np.prod(shape[k + 1:], dtype=np.int64))
    batch = int(np.prod(shape[:k], dtype=np.int64))
    if n * inner > (1 << 31) - 1 or inner > (1 << 30) or batch * n * inner == 0:
        return None
    try:
        plan = _get_plan(ndim=2, batch=batch, ny=n, nx=inner, dtype=t.dtype, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=_lib.AXIS_Y | _lib.INVERSE | flags,
                         scale=scale, window_y=None, window_x=None, phase_y=phase, phase_x=None)
    except _lib.XrftHipError as e:
        if e.status in (_lib.UNSUPPORTED_LENGTH, _lib.BAD_ARG):
            return None
        raise
    out, _ = plan.execute(t.reshape(batch, n, inner))
    out = out.reshape(shape)
    if roll:
        out = engine.gather_axis(out, k, roll=roll)
    return out


def idft(daft, dim=None, true_phase=False, true_amplitude=False, **kwargs):
    """Deprecated alias of ``ifft`` with numpy-like defaults (xrft/xrft.py:253-266)."""
    warnings.warn("This function has been renamed and will disappear in the future. Please use `ifft` instead",
                  FutureWarning)
    return ifft(daft, dim=dim, true_phase=true_phase, true_amplitude=true_amplitude, **kwargs)
