"""The decoration ladder (tests/decorations.py) on the emulated library: every kernel family with a window, a shift, an input rotation, a flip, a phase table, a
constant detrend with a scale, and all of them together, held to the rounding-level contract of tests/accuracy.py against a float64 numpy model of
include/xrft_hip.h.  The family each case runs on is asserted first, the demotions as recorded; a refused combination asserts its documented status."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import accuracy as A  # noqa: E402
import decorations as D  # noqa: E402

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


CASES = D.cases()


@pytest.mark.parametrize("kw,env,tokens,expect", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_decorations(monkeypatch, kw, env, tokens, expect):
    _env(monkeypatch, env)
    D.run(kw, tokens, expect, "cpu")


def test_every_family_has_a_decorated_case():
    """Every Family (accuracy.FAMILY_FORMS, held to csrc/plan.h by test_every_family_is_executed) has at least one case here whose ASSERTED family is that
    family: the demotions do not hollow the table out."""
    asserted = {c[4] for c in CASES if not isinstance(c[4], int)}
    missing = [f for f, forms in A.FAMILY_FORMS.items() if not forms & asserted]
    assert not missing, missing
    # ... and under a window with an input rotation, the combination the specialised inverse kernels once indexed by destination, in the families that keep it
    # (the one-axis families hand it to the generic passes: decorations.DEMOTED)
    rotated = {c[4] for c in CASES if {"win", "ishift"} <= set(c[3]) and not isinstance(c[4], int) and c[1].get("flags", 0) & L.INVERSE}
    for fam in ("FastYC", "FastG", "Generic"):
        assert A.FAMILY_FORMS[fam] & rotated, fam


def test_ids_are_unique_and_the_tables_name_cases():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids))
    assert set(D.DEMOTED) <= set(ids) and set(D.REFUSED) <= set(ids) and not set(D.DEMOTED) & set(D.REFUSED)


# ---------------------------------------------------------------------------------- the reference discriminates (CPU only, no kernel)
# (make() arguments, tokens) on which each mutation of the reference is visible
_SENSITIVE = {
    "window-after-flip": (dict(dtype=A.C128, out_mode=L.OUT_COMPLEX), "win+flip"),
    "window-by-destination": (dict(dtype=A.C128, out_mode=L.OUT_COMPLEX, flags=L.INVERSE), "win+ishift"),
    "fftshift-for-ifftshift": (dict(dtype=A.C128, out_mode=L.OUT_COMPLEX, flags=L.INVERSE), "ishift"),
    "phase-by-shifted-index": (dict(dtype=A.C128, out_mode=L.OUT_COMPLEX), "phase+shift"),
    "flips-swapped": (dict(dtype=A.F64, out_mode=L.OUT_CROSS), "win+shift+ishift+flip+flip0+phase+scale+const"),
    "scale-omitted": (dict(dtype=A.F64, out_mode=L.OUT_COMPLEX), "const+scale"),
}


@pytest.mark.parametrize("mutation", D.MUTATIONS)
@pytest.mark.parametrize("ny,nx", [(50, 50), (45, 49)], ids=["even", "odd"])
def test_the_reference_is_sensitive(mutation, ny, nx):
    """Each mistake a kernel's load or store code can make -- the window applied behind the flip, or indexed by the destination of the input rotation; fftshift
    for ifftshift (an odd length tells them apart); the output phase indexed by shifted frequency; FLIP0 and FLIP swapped between the fields; the scale left
    out -- misses the bound against the unmutated reference on the ladder's own inputs, in float64 AND at float32's bound; the unmutated reference meets both."""
    base, toks = _SENSITIVE[mutation]
    kw, tab = D.decorate(dict(base, ny=ny, nx=nx), toks.split("+"))
    xs = D.inputs(kw)
    x1 = xs[1] if len(xs) == 2 else None
    ref, _ = D.reference(kw, tab, xs[0], x1)
    bad, _ = D.reference(kw, tab, xs[0], x1, mutate=mutation)
    if mutation == "fftshift-for-ifftshift" and ny % 2 == 0:
        assert np.array_equal(bad, ref)  # (even lengths: the two rotations are one -- why the ladder has odd shapes)
        return
    det = kw.get("detrend", L.DETREND_NONE)
    shape, axes, _ = A._axes(kw)
    kap = A.kappa(xs[0].reshape(shape), A.detrended(xs[0].reshape(shape), axes, det)) if det else 0.0
    for dt in ("complex128", "complex64"):
        A.assert_accurate(ref.astype(dt), ref, dt, ny * nx, kap)
        with pytest.raises(AssertionError):
            A.assert_accurate(bad, ref, dt, ny * nx, kap)
