"""Transform lengths no plan of the C ABI takes: Bluestein's algorithm through global memory, and the float64 detour of the compositions around it."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, engine
from ._hostside import _to_device
from ._plans import _get_plan, _plan_lock
from .labeled import DataArray


# ------------------------------------------------------------------------------------------------------
# Bluestein's algorithm through global memory: one transform axis (the last) whose length has a prime factor above 128 and exceeds
# what the in-tile Bluestein of the C ABI holds (numpy.fft takes any length, xrft.py:398-447).
#   X[k] = conj(c[k]) sum_j (x[j] conj(c[j])) c[k - j],   c[j] = exp(i pi j^2 / n)
# = chirp multiply with zero padding to a 2^a 3^b 5^c length m >= 2n - 1, a forward plan, the product with FFT_m(c wrapped) / m,
# an inverse plan, chirp multiply with truncation -- three table-multiply launches (xrfthip_table_mul) around two existing plans;
# detrend, window, flips and shifts, true-phase factors, scaling and |F|^2 are the same device calls the other paths use.
# ------------------------------------------------------------------------------------------------------
def _wide(da):
    """float32 data of a call that is composed of several device passes around a Bluestein axis (no two-axis plan exists for a long
    prime length): the whole composition runs in float64 -- detrending pass, chirp convolution, the other axis -- between two precision
    changes, so that its small bins hold the 1e-3 every fused path holds (stored float32 intermediates cost them 1.3e-3)."""
    t = _to_device(da.data)
    if t.dtype not in (torch.float32, torch.complex64) or not engine.bluestein_in_float64():
        return da, False
    w = engine.convert(t.contiguous(), torch.float64 if t.dtype == torch.float32 else torch.complex128)
    return DataArray(w, da.dims, da.coords, da.name, da.attrs), True


def _narrow(res, was_wide):
    if not was_wide or not isinstance(res.data, torch.Tensor) or res.data.dtype not in (torch.float64, torch.complex128):
        return res
    d = res.data
    n = engine.convert(d.contiguous(), torch.float32 if d.dtype == torch.float64 else torch.complex64)
    return DataArray(n, res.dims, res.coords, res.name, res.attrs)


_BLUE_TABLES = {}


def _blue_tables(n, cdt, dev, inverse=False):
    """(m, conj chirp as a HOST complex128 vector, FFT_m(chirp) / m on the device) of Bluestein's algorithm for length n, cached.
    The chirp's spectrum is taken by the engine's own length-m plan in complex128 (no numpy.fft in the product path)."""
    key = (n, str(cdt), str(dev), inverse)
    with _plan_lock:
        tb = _BLUE_TABLES.get(key)
    if tb is None:
        m = 2 * n - 1
        while True:
            q = m
            for p in (2, 3, 5):
                while q % p == 0:
                    q //= p
            if q == 1:
                break
            m += 1
        j = np.arange(n, dtype=np.int64)
        ang = np.pi * ((j * j) % (2 * n)).astype(np.float64) / n  # j^2 mod 2n: exact phases for long sequences
        chirp = np.exp((-1j if inverse else 1j) * ang)             # c[j] (conjugated for the inverse transform)
        b = np.zeros(m, dtype=np.complex128)
        b[:n] = chirp
        b[m - n + 1:] = chirp[1:][::-1]                            # c[-j] = c[j], wrapped
        plan = _get_plan(ndim=1, batch=1, ny=1, nx=m, dtype=torch.complex128, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=0,
                         scale=1.0 / m, window_y=None, window_x=None, phase_y=None, phase_x=None)
        bhat, _ = plan.execute(torch.from_numpy(b).to(dev).reshape(1, 1, m))
        tb = (m, np.conj(chirp), bhat.reshape(m).to(cdt))  # (one precision change of a table, once per length)
        with _plan_lock:
            if len(_BLUE_TABLES) > 8:
                _BLUE_TABLES.clear()
            _BLUE_TABLES[key] = tb
    return tb


def _bluestein_1d(t, n, mode, detrend_kind, flags, scale, win, ph, phase_in=None):
    """The 1-D plan's result for t[..., n] (real or complex) without a 1-D plan of length n.  With XRFTHIP_INVERSE in ``flags`` the
    unnormalised inverse transform (the same pipeline with conjugated chirps); ``phase_in`` multiplies the INPUT, indexed by source
    position (XRFTHIP_PHASE_IN, xrft.py:574-576).  float32 data run in float64 between two precision changes (engine.convert;
    engine.bluestein_in_float64): stored float32 intermediates between the five passes cost the small bins their 1e-3.  (Bluestein
    inside one tile of the C ABI's plans stays in float32: 1.2e-4 per bin.)"""
    if t.dtype in (torch.float32, torch.complex64) and engine.bluestein_in_float64():
        X = _bluestein_1d(engine.convert(t, torch.float64 if t.dtype == torch.float32 else torch.complex128), n, mode, detrend_kind, flags,
                          scale, win, ph, phase_in)
        return engine.convert(X, torch.float32 if X.dtype == torch.float64 else torch.complex64)
    shape = list(t.shape)
    x = t.reshape(-1, n).contiguous()
    real_in = not x.is_complex()
    cdt = torch.complex64 if x.dtype in (torch.float32, torch.complex64) else torch.complex128
    if detrend_kind != _lib.DETREND_NONE:  # per row, before the window (xrft.py:425-433)
        x = engine.detrend(x, 1, detrend_kind)
    idx = np.arange(n)
    if flags & _lib.FLIP_X:      # np.flip, then ifftshift (xrft.py:436-441)
        idx = idx[::-1]
    if flags & _lib.ISHIFT_X:
        idx = np.roll(idx, -(n // 2))
    if (flags & (_lib.FLIP_X | _lib.ISHIFT_X)):
        x = engine.gather_axis(x, 1, index=idx)
    m, cconj_chirp, bhat = _blue_tables(n, cdt, x.device, inverse=bool(flags & _lib.INVERSE))
    # the pointwise tables are composed on the host (length-n vectors, like the window vectors) and uploaded: no torch arithmetic
    tab_h = cconj_chirp
    if phase_in is not None:
        tab_h = tab_h * np.asarray(phase_in, dtype=np.complex128)[idx]
    if win is not None:  # the window rides on the first chirp multiply (it multiplies the samples where they lie AFTER flip / shift:
        tab_h = tab_h * np.asarray(win, dtype=np.float64)[idx]  # the reference windows first, then flips: window of the source sample)
    tab = torch.from_numpy(np.ascontiguousarray(tab_h.astype(np.complex64 if cdt == torch.complex64 else np.complex128))).to(x.device)
    a = engine.table_mul(x, tab.contiguous(), m)
    fwd = _get_plan(ndim=1, batch=a.shape[0], ny=1, nx=m, dtype=a.dtype, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=0, scale=1.0,
                    window_y=None, window_x=None, phase_y=None, phase_x=None)
    A, _ = fwd.execute(a.reshape(a.shape[0], 1, m))
    C = engine.table_mul(A.reshape(-1, m), bhat, m)
    inv = _get_plan(ndim=1, batch=a.shape[0], ny=1, nx=m, dtype=a.dtype, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=_lib.INVERSE, scale=1.0,
                    window_y=None, window_x=None, phase_y=None, phase_x=None)
    cc, _ = inv.execute(C.reshape(-1, 1, m))
    half = bool(flags & _lib.HALF_X)
    n_out = n // 2 + 1 if half else n
    fac = np.ones(n_out, dtype=np.complex128)
    if mode == _lib.OUT_COMPLEX:
        fac = fac * float(scale)
        if ph is not None:
            fac = fac * np.asarray(ph, dtype=np.complex128)[:n_out]
    tab2 = torch.from_numpy(np.ascontiguousarray((cconj_chirp[:n_out] * fac).astype(np.complex64 if cdt == torch.complex64 else np.complex128))).to(x.device)
    X = engine.table_mul(cc.reshape(-1, m), tab2, n_out)  # F[k] (x phase x scale), k < n_out
    if mode == _lib.OUT_POWER:
        if flags & _lib.REALDIM_X2:
            X = engine.spectrum_tail_axis(X, None, float(scale), 1, n % 2 == 0)
        else:
            X = engine.spectrum_tail(X, None, float(scale))
    elif flags & _lib.REALDIM_X2:
        d2 = np.full(n_out, 2.0); d2[0] = 1.0
        if n % 2 == 0:
            d2[-1] = 1.0
        X = engine.table_mul(X, torch.from_numpy(d2.astype(np.complex64 if cdt == torch.complex64 else np.complex128)).to(x.device), n_out)
    if flags & _lib.SHIFT_X:
        X = engine.gather_axis(X, 1, roll=n // 2)
    return X.reshape(shape[:-1] + [n_out])
