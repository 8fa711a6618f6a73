"""The extent ladder's CPU side (tests/extents.py): the checker shown to bite -- no library, synthetic outputs --, rung D (the host guards at the limit and one
step past it: plan creation only), the group rule of the fused radial sums, and a few cases of rungs A and B through the whole harness at a batch of 96 on the
emulated library (the MI355X runs them at 70 080 slabs and beyond 2^31 elements: tests/test_gpu_extents.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402

from xrft_amd import _lib, api  # noqa: E402

import accuracy as A  # noqa: E402
import extents as E  # noqa: E402

L = _lib


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    api._plan_cache.clear()
    _lib._load_for_testing(build_emu.build())
    yield
    api._plan_cache.clear()
    _lib._state.update(dll=None, path=None, device="cuda")


# ---------------------------------------------------------------------------------- the checker bites (no library)
SLABS, WRAP, BOUNDARY, POINTS = 480, 100, 250, 8


def _synthetic():
    """480 tiny slabs of a period of 48, as a float32 kernel would leave them; two guard bands; a pretend wrap distance of 100 slabs from slab 250 on."""
    rng = np.random.default_rng(21)
    ref = rng.standard_normal((E.PERIOD, POINTS)) * (1.0 + np.arange(E.PERIOD) / E.PERIOD).reshape(-1, 1)
    out = torch.from_numpy(np.tile(ref, (SLABS // E.PERIOD, 1))).to(torch.float32)
    bands = [torch.full((64,), E.PATTERN, dtype=torch.uint8) for _ in range(2)]
    return ref, out, bands


def _check(ref, out, bands, bounds, exact=False):
    return E.check(out, ref, A.bound(A.F32, POINTS), bounds, E.plain_accurate(A.F32, POINTS, 0.0), exact=exact, bands=bands, what="synthetic")


def test_the_checker_passes_the_clean_array():
    assert WRAP % E.PERIOD != 0
    ref, out, bands = _synthetic()
    assert _check(ref, out, bands, {"pretend wrap": BOUNDARY}, exact=True) is True
    out[300, 3] = float(np.nextafter(np.float32(out[300, 3]), np.float32(np.inf)))  # one ulp: within the bound, not the same bits
    assert _check(ref, out, bands, {"pretend wrap": BOUNDARY}) is False
    with pytest.raises(AssertionError, match="differs in its bits"):
        _check(ref, out, bands, {"pretend wrap": BOUNDARY}, exact=True)


def test_the_checker_fails_on_a_wrapped_index():
    """Every slab from the boundary on replaced by the slab one wrap distance earlier: the boundary's window catches it against float64; where no window looks
    (the boundary not known, the wrap confined to the middle of the batch), the comparison of every slab with its member of the period does."""
    ref, out, bands = _synthetic()
    out[BOUNDARY:] = out[BOUNDARY - WRAP:SLABS - WRAP].clone()
    with pytest.raises(AssertionError, match="pretend wrap"):
        _check(ref, out, bands, {"pretend wrap": BOUNDARY})
    with pytest.raises(AssertionError, match="last"):
        _check(ref, out, bands, {})
    ref, out, bands = _synthetic()
    out[BOUNDARY:400] = out[BOUNDARY - WRAP:400 - WRAP].clone()
    with pytest.raises(AssertionError, match=f"slab {BOUNDARY} is .* of the first period"):
        _check(ref, out, bands, {})


def test_the_checker_fails_on_one_zeroed_slab():
    ref, out, bands = _synthetic()
    out[200] = 0.0  # (period 4: in no window)
    with pytest.raises(AssertionError, match="slab 200 is"):
        _check(ref, out, bands, {"pretend wrap": BOUNDARY})


def test_the_checker_fails_on_a_flipped_guard_word():
    ref, out, bands = _synthetic()
    bands[1].view(torch.int32)[5] ^= 1
    with pytest.raises(AssertionError, match="guard band 1"):
        _check(ref, out, bands, {"pretend wrap": BOUNDARY})


def test_the_checker_fails_on_an_unwritten_last_slab():
    ref, out, bands = _synthetic()
    out[-1] = float("nan")
    with pytest.raises(AssertionError, match="slab 479"):
        _check(ref, out, bands, {"pretend wrap": BOUNDARY})
    ref, out, bands = _synthetic()
    out[335] = float("nan")  # ... and in no window: the device pass
    with pytest.raises(AssertionError, match="slab 335 holds a value that is not finite"):
        _check(ref, out, bands, {"pretend wrap": BOUNDARY})


def test_boundaries_and_batches():
    """The first slab at or beyond each limit, only where the case reaches it; the rung B batch leaves one whole period beyond 2^31 elements on both sides."""
    b = E.batch_beyond(256 * 256, 256 * 256)
    assert b == 32832 and b % E.PERIOD == 0
    bd = E.boundaries(b, 256 * 256, 4, 256 * 256, 4)
    assert bd == {"input 2^31 elements": 32768, "input 2^32 bytes": 16384, "input 2^33 bytes": 32768, "output 2^31 elements": 32768, "output 2^32 bytes": 16384, "output 2^33 bytes": 32768}
    assert b - E.PERIOD >= 32768 > b - 2 * E.PERIOD  # (the last period lies beyond the boundary whole, the one before it does not)
    assert E.boundaries(E.COUNT, 64 * 64, 4, 64 * 64, 4) == {}
    assert E.boundaries(200000, 4096, 4, 4096, 8) == {"output 2^32 bytes": 131072}
    with pytest.raises(AssertionError):  # a period that divides a power of two hides a wrap of whole slabs
        E.boundaries(b, 256 * 256, 4, 256 * 256, 4, period=32)


# ---------------------------------------------------------------------------------- rung D: the guards
def test_the_guards_at_the_limit_and_one_step_past_it():
    E.check_guards()


def test_a_group_of_the_fused_radial_sums_stays_within_grid_y():
    E.check_iso_group_limit()


def test_radial_sums_over_several_groups():
    E.run_iso_in_groups("cpu")


def test_the_y_only_rows_are_the_narrowest():
    """Rung A runs the y-only families at the narrowest nx at which they still take the plan at 70 080 slabs: every narrower one routes elsewhere."""
    for rid, nx, tag in (("fastmy-linear", E.FASTMY_NX, "fastm y-only"), ("fastgy-linear", E.FASTGY_NX, "fastg y-only")):
        kw, env, kind, _ = E.row(rid)
        assert not env
        assert A.family(A.make(**dict(kw, nx=nx, batch=E.COUNT))) == (kind, tag)
        for narrower in range(1, nx):
            assert A.family(A.make(**dict(kw, nx=narrower, batch=E.COUNT)))[1] != tag, narrower


def test_the_bit_identical_families_are_tags_of_the_routing_table():
    tags = {r[4] for r in A.ROWS + A.MODES}
    assert set(E.EXACT) <= tags and all(E.EXACT.values())


# ---------------------------------------------------------------------------------- the harness itself, at a batch of 96
SMALL = ["fasts-linear-windows-shifts", "fasts-iso", "fastmx-complex", "fusedi-33x32-half-y", "fasth-shifts", "fastgy-linear"]


@pytest.mark.parametrize("cid", SMALL)
def test_rung_a_cases_through_the_harness(cid):
    kw, env, kind, tag = E.RUNG_A[cid]
    E.run_plain(cid, kw, env, kind, tag, 2 * E.PERIOD, "cpu")


def test_averaged_forms_through_the_harness():
    E.run_mean("fasts-mean", 64, 64, 2, 2 * E.PERIOD, {"XRFTHIP_MEAN_ALL": "1"}, L.K_FASTS, "cpu")
    E.run_welch_rows("welch-rows", 64, 32, 3, 2 * E.PERIOD, "cpu")
    E.run_welch_cols("welch-columns", 64, 32, 3, 3, 2 * E.PERIOD, "cpu")


def test_strided_boxes_through_the_harness():
    """Rung C's runner at strides a CPU holds (the MI355X runs it at 2^30 + 16 elements between the slabs and at the largest pitch)."""
    E.run_strided("fasts", "fasts", 3, 0, 64 * 128 + 16, "cpu")
    E.run_strided("fastg-pitch", "fastg-f32", 2, 60, 50 * 60, "cpu")
    E.run_welch_rows_pitched("welch-rows-pitch", "cpu", pitch=128 + 5)
    E.run_welch_cols_strided("welch-columns-stride", "cpu", s=64, c=(64, 32, 5, 2, 40), beyond=0)
