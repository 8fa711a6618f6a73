"""xrft_amd -- the xrft spectral hot path (fft / dft / power_spectrum / cross_spectrum / isotropic_* / detrend)
on AMD MI355X (gfx950): hand-written HIP kernels in libxrft_hip.so behind the reference's call signatures.

    import xrft_amd as xrft
    ps = xrft.power_spectrum(da, dim=["y", "x"], detrend="linear", window="hann")

``da`` is an ``xrft_amd.DataArray`` (numpy or torch data) or, when xarray is installed, an ``xarray.DataArray``.
There is no CPU fallback: the compute entry points raise ``XrftHipUnavailable`` if the library is not built.
"""
from ._lib import XrftHipError, XrftHipUnavailable  # noqa: F401
from .labeled import Coordinate, DataArray  # noqa: F401
from .api import (clear_plan_cache, coherence, cross_phase, cross_spectrum, detrend, dft, fft, fit_loglog, idft, ifft,  # noqa: F401
                  isotropic_cross_spectrum, isotropic_power_spectrum, isotropize, mean_cross_spectrum, mean_power_spectrum, power_spectrum,
                  fir_filter, istft, multitaper_coherence, multitaper_cross_spectrum, multitaper_power_spectrum, spectrogram, stft, welch_coherence, welch_cross_spectrum, welch_power_spectrum)
from .engine import bluestein_in_float64, reuse_column_pass  # noqa: F401
from .padding import get_spacing, pad, unpad  # noqa: F401

__version__ = "0.1.0"
__all__ = ["DataArray", "Coordinate", "fft", "ifft", "dft", "idft", "detrend", "power_spectrum", "cross_spectrum",
           "cross_phase", "coherence", "isotropize",
           "isotropic_power_spectrum", "isotropic_cross_spectrum", "mean_power_spectrum", "mean_cross_spectrum", "welch_power_spectrum", "welch_cross_spectrum", "welch_coherence", "spectrogram", "stft", "istft", "fir_filter", "multitaper_power_spectrum", "multitaper_cross_spectrum", "multitaper_coherence", "fit_loglog", "pad", "unpad", "get_spacing", "XrftHipError",
           "XrftHipUnavailable", "clear_plan_cache", "bluestein_in_float64", "reuse_column_pass"]
