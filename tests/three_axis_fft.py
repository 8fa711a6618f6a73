"""Shared by the tests of the fused three-axis transform (tests/test_three_axis_fft_emulated.py on the emulated library, tests/test_gpu_three_axis_fft.py on the
MI355X): fields, the twin columns of a result, the numpy form of the field plan.  Not a conftest: imported by the tests that use it.

Coordinates: the origin is NOT an integer multiple of the spacing on t and on y (t = 0.3 + k, y = 1.1 + 0.5 k).  The true-phase factor of a Nyquist index n / 2 is
exp(+2 pi i lag / (2 dx)); with an integer origin / dx it is real, its conjugate is itself, and a twin that carried the conjugate of its sample's factor
instead of its own would not show."""
import numpy as np

from xrft_amd import _lib as L
from xrft_amd import api

import cases

# (nt, ny, nx): all even (Nyquist rows along t and y, a Nyquist column); all odd (no Nyquist anywhere); column blocks that straddle rows ky with whole 16-byte twin
# pieces; nt = 2 x 3 x 5; a cube
SHAPES = [(8, 6, 10), (9, 5, 7), (12, 7, 16), (30, 4, 6), (16, 16, 16)]
ORDERS = [["t", "y", "x"], ["x", "t", "y"]]
DIMS = ("b", "t", "y", "x")


def newest_plan():
    return next(reversed(api._plan_cache.values())).describe()


def no_fasth_plan():
    return all("[fasth]" not in p.describe() for p in api._plan_cache.values())


def coords(shape, batch):
    nt, ny, nx = shape
    return {"b": np.arange(batch), "t": 0.3 + np.arange(nt) * 1.0, "y": 1.1 + np.arange(ny) * 0.5, "x": np.arange(nx) * 2.0 + 3.0}


def field(shape, batch, dtype, seed=5):
    """A (b, t, y, x) field with a hyperplane under the noise, as the product's array and the oracle's (the same samples as float64)."""
    nt, ny, nx = shape
    rng = np.random.default_rng(seed)
    ramp = 0.05 * np.arange(nt).reshape(1, nt, 1, 1) + 0.03 * np.arange(ny).reshape(1, 1, ny, 1) - 0.02 * np.arange(nx).reshape(1, 1, 1, nx) + 1.0
    v = (rng.standard_normal((batch,) + tuple(shape)) + ramp).astype(dtype)
    return cases.pair(v, DIMS, coords(shape, batch))


def unshifted(v, shift):
    return np.fft.ifftshift(v, axes=(-3, -2, -1)) if shift else v


def twin_columns(v):
    """(the samples, their twins v[..., -kt, -ky, -kx]) of the columns 1 <= kx <= nx - (nx / 2 + 1) of an unshifted result: the columns the last pass writes twice,
    once as the sample and once, conjugated, as the twin."""
    nx = v.shape[-1]
    tw = np.roll(v[..., ::-1, ::-1, ::-1], 1, axis=(-3, -2, -1))
    return v[..., 1:nx - nx // 2], tw[..., 1:nx - nx // 2]


def nyquist_rows_of_twins(v):
    """The rows kt = nt / 2 and ky = ny / 2 (even lengths) of the columns kx > nx / 2 -- the twins -- of an unshifted result, as one vector (empty if both are odd)."""
    nt, ny, nx = v.shape[-3:]
    tw = v[..., nx // 2 + 1:]
    parts = ([tw[..., nt // 2, :, :].ravel()] if nt % 2 == 0 else []) + ([tw[..., :, ny // 2, :].ravel()] if ny % 2 == 0 else [])
    return np.concatenate(parts) if parts else np.zeros(0, dtype=v.dtype)


def herm_field_kw(shape, cdtype, flags=0, batch=2):
    """accuracy.make() arguments of the last pass of a three-axis transform: herm_ny / herm_nx with HERM_FIELD, complex output."""
    nt, ny, nx = shape
    return dict(batch=batch, ny=nt, nx=ny * (nx // 2 + 1), dtype=cdtype, out_mode=L.OUT_COMPLEX, flags=L.AXIS_Y | L.HERM_FIELD | flags, herm_ny=ny, herm_nx=nx)


def phase_tables(shape):
    """Three unit-modulus tables with no symmetry at all: nothing but the rule "an element carries the factors of its own indices" reproduces the result."""
    return [np.exp(1j * (0.37 * (a + 1) * np.arange(n) ** 2 + 0.11 * a)) for a, n in enumerate(shape)]


def half_spectrum(shape, batch, cdtype, seed=4):
    """The half spectrum [batch][nt][ny (nx/2 + 1)] of seeded real noise in the plan's dtype (a CPU tensor), and its exact complex128 image [batch][nt][ny][nx/2 + 1]."""
    import torch

    nt, ny, nx = shape
    h = np.fft.rfftn(np.random.default_rng(seed).standard_normal((batch, nt, ny, nx)), axes=(-2, -1))
    t = torch.from_numpy(np.ascontiguousarray(h)).to(cdtype).reshape(batch, nt, ny * (nx // 2 + 1))
    return t, t.to(torch.complex128).numpy().reshape(h.shape)


def field_plan_reference(h, shape, flags, window_t=None, phases=None):
    """What a herm_field_kw plan computes (scale 1) from its input h[batch][nt][ny][nx/2 + 1] (complex128): window along t by source row -> (ISHIFT_Y) rotation ->
    transform along t -> Hermitian extension -> phases by unshifted index -> shifts."""
    nt, ny, nx = shape
    if window_t is not None:
        h = h * np.asarray(window_t).reshape(1, nt, 1, 1)
    if flags & L.ISHIFT_Y:
        h = np.fft.ifftshift(h, axes=1)
    f = np.fft.fft(h, axis=1)
    nxh = nx // 2 + 1
    full = np.empty(h.shape[:3] + (nx,), dtype=np.complex128)
    full[..., :nxh] = f
    tw = f[:, (-np.arange(nt)) % nt][:, :, (-np.arange(ny)) % ny][..., nx - np.arange(nxh, nx)]
    full[..., nxh:] = np.conj(tw)
    if phases is not None:
        full = full * phases[0].reshape(1, nt, 1, 1) * phases[1].reshape(1, 1, ny, 1) * phases[2].reshape(1, 1, 1, nx)
    if flags & L.SHIFT_Y:
        full = np.fft.fftshift(full, axes=1)
    if flags & L.SHIFT_X:
        full = np.fft.fftshift(full, axes=(2, 3))
    return full
