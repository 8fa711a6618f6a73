"""The accuracy ladder on the emulated library: every routing-table row (tests/accuracy.py ROWS, with its environment) and every mode of a
family (MODES) EXECUTED through engine.SpectralPlan and held to the rounding-level contract of tests/accuracy.py against the float64
transform of the same samples -- on seeded noise, single tones, a last-sample impulse, the Nyquist sequence and batches of unequal scale.
The family each case was written for is asserted first: a routing change fails the case instead of quietly testing another family."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import accuracy as A  # noqa: E402
import cases  # noqa: E402

L = _lib


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api._plan_cache.clear()
    _lib._load_for_testing(build_emu.build())
    yield
    api._plan_cache.clear()
    _lib._state.update(dll=None, path=None, device="cuda")


def _env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("XRFTHIP_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("kw,env,kind,tag,sig", [p[1:] for p in A.ladder_params(A.ROWS + A.MODES)], ids=[p[0] for p in A.ladder_params(A.ROWS + A.MODES)])
def test_ladder(monkeypatch, kw, env, kind, tag, sig):
    _env(monkeypatch, env)
    p, _c = A.run_ladder(kw, sig, "cpu")
    assert A.family(p) == (kind, tag)


def test_every_family_is_executed():
    """Every value of the Family enum (csrc/plan.h) and every xrfthip_kernel_kind value has at least one ladder case whose routed family
    is asserted: a Family added, or a form dropped from the ladder, fails here."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xrft_amd", "csrc", "plan.h")).read()
    body = src[src.index("enum class Family {"):]
    body = body[body.index("{") + 1:body.index("};")]
    names = [ln.split("//")[0].strip().rstrip(",") for ln in body.splitlines()]
    assert sorted(n for n in names if n) == sorted(A.FAMILY_FORMS)
    asserted = {(r[3], r[4]) for r in A.ROWS + A.MODES}
    missing = [f for f, forms in A.FAMILY_FORMS.items() if not forms & asserted]
    assert not missing, missing
    assert {k for k, _t in asserted} == set(range(14))


@pytest.mark.parametrize("n", [1 << 16, 1 << 20])
def test_four_step_input_phase_off_the_separable_form(n):
    """A PHASE_IN table that is exp(i theta n) but at one position: either the generic passes take the plan, or the result meets the
    bound against fft(x * phase)."""
    p = A.run_four_step_phase(n, A.four_step_phase(n), "cpu")
    if n == 1 << 20:
        assert A.family(p) == (L.K_GENERIC, "main")  # (a table off the separable form: the generic four-step passes)


def test_four_step_input_phase_separable_stays_on_the_fast_family():
    n = 1 << 20
    p = A.run_four_step_phase(n, np.exp(0.001j * np.arange(n)), "cpu", seed=4)
    assert A.family(p) == (L.K_FASTY, "fasty complex rows, four-step")


# ---------------------------------------------------------------------------------- the bound is tight enough (CPU only, no kernel)
class _Arr:
    """The smallest stand-in for a result that cases.check takes: values and dims, no coordinates."""

    def __init__(self, v):
        self.values, self.dims, self.coords = v, ("x",), {}


def _fft_radix2(x, bad_stage=None, bad_k=None, rel=0.0):
    """Iterative radix-2 decimation-in-time FFT in float64; twiddle W^bad_k of stage `bad_stage` (butterflies of half-length
    2^bad_stage) multiplied by (1 + rel)."""
    n = x.size
    lg = n.bit_length() - 1
    rev = np.zeros(n, dtype=np.int64)
    for b in range(lg):
        rev |= ((np.arange(n) >> b) & 1) << (lg - 1 - b)
    a = x[rev].astype(np.complex128)
    for s in range(lg):
        h = 1 << s
        w = np.exp(-2j * np.pi * np.arange(h) / (2 * h))
        if s == bad_stage:
            w[bad_k] *= 1.0 + rel
        a = a.reshape(-1, 2, h)
        t = a[:, 1, :] * w
        a = np.stack([a[:, 0, :] + t, a[:, 0, :] - t], axis=1).reshape(n)
    return a


def test_the_bound_is_sensitive():
    """Two faults that today's float32 bar (cases.check at TOL float32) lets through must fail the contract, and numpy.fft in float32 must
    pass it: the bound sits between a correct float32 transform and a subtly wrong one."""
    n = 1 << 16
    rng = np.random.default_rng(11)
    # a red spectrum (a random walk, as geophysical fields are): today's per-bin bar looks only at bins above 1e-3 of the peak, and a
    # fault of 1e-4 stays below it there; on white noise the per-bin bar would already catch these two
    x = np.cumsum(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    ref = np.fft.fft(x)
    assert np.abs(_fft_radix2(x) - ref).max() / np.abs(ref).max() < 1e-12  # (the radix-2 reference itself is right)
    scaled = ref * (1.0 + 1.0 / n)  # normalisation off by 1/N: 1.5e-5
    # W^1 of the butterflies of half-length 4 (stage 2) multiplies one point in every 8: N/8 of them, off by 1e-4
    twiddled = _fft_radix2(x, bad_stage=2, bad_k=1, rel=1e-4)
    for bad in (scaled, twiddled):
        cases.check(_Arr(bad), _Arr(ref), cases.TOL["complex64"])
        with pytest.raises(AssertionError):
            A.assert_accurate(bad, ref, "complex64", n)
    f32 = np.fft.fft(x.astype(np.complex64))
    assert f32.dtype == np.complex64  # (numpy >= 2 computes in float32)
    A.assert_accurate(f32, ref, "complex64", n)
