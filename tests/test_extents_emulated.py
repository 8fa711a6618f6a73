"""The extent ladder's CPU side (tests/extents.py): the checker shown to bite -- no library, synthetic outputs --, rung D (the host guards at the limit and one
step past it: plan creation only), the group rule of the fused radial sums, and a few cases of rungs A and B through the whole harness at a batch of 96 on the
emulated library (the MI355X runs them at 70 080 slabs and beyond 2^31 elements: tests/test_gpu_extents.py).  The spectrogram, istft and fir_filter runners -- the
period along ONE series, across the batch, through the pitch -- each run once at four to six periods and 96 series, and the checker's form for them (extents.Along:
edge periods, an interior member, a tail) has its own mutants."""
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


# ---- ... with the period along a series (extents.Along): the first and the last period differ from the interior, a tail lies behind the last whole period
TAIL = 5


def _synthetic_along():
    """The same 480 slabs as the segments of ONE series: period 0 and period 9 are edges (values of their own), periods 1 .. 8 repeat; 5 values behind them.  The
    reference is that of a short series of four periods: first, interior, interior, last."""
    rng = np.random.default_rng(22)
    scale = (1.0 + np.arange(E.PERIOD) / E.PERIOD).reshape(-1, 1)
    first, inner, last = (rng.standard_normal((E.PERIOD, POINTS)) * scale for _ in range(3))
    ref = np.concatenate([first, inner, inner, last])
    out = torch.from_numpy(np.concatenate([first] + [inner] * (SLABS // E.PERIOD - 2) + [last])).to(torch.float32)
    tail_ref = rng.standard_normal(TAIL)
    tail = torch.from_numpy(tail_ref).to(torch.float32)
    bands = [torch.full((64,), E.PATTERN, dtype=torch.uint8) for _ in range(2)]
    return ref, out, tail, tail_ref, bands


def _check_along(ref, out, tail, tail_ref, bands, bounds, exact=False):
    def tail_ok(got, what):
        assert np.abs(got - tail_ref).max() <= 2.0 ** -23 * np.abs(tail_ref).max(), what
    along = E.Along(1, {0: 0, SLABS // E.PERIOD - 1: 3}, (tail, tail_ok))
    return E.check(out, ref, A.bound(A.F32, POINTS), bounds, E.plain_accurate(A.F32, POINTS, 0.0), exact=exact, bands=bands, what="synthetic", along=along)


def test_the_checker_passes_a_clean_series_whose_ends_differ():
    ref, out, tail, tail_ref, bands = _synthetic_along()
    assert not torch.equal(out[:E.PERIOD], out[E.PERIOD:2 * E.PERIOD]) and not torch.equal(out[-E.PERIOD:], out[E.PERIOD:2 * E.PERIOD])
    assert _check_along(ref, out, tail, tail_ref, bands, {"pretend wrap": BOUNDARY}, exact=True) is True
    with pytest.raises(AssertionError):  # (without the argument the first period is the member: the interior differs from it)
        _check(ref[:E.PERIOD], out, bands, {})


def test_the_checker_fails_on_an_index_wrapped_along_the_series():
    """Every period from the boundary's on replaced by the one a wrap distance earlier (100 slabs: another member of the period)."""
    ref, out, tail, tail_ref, bands = _synthetic_along()
    out[BOUNDARY:] = out[BOUNDARY - WRAP:SLABS - WRAP].clone()
    with pytest.raises(AssertionError, match="pretend wrap"):
        _check_along(ref, out, tail, tail_ref, bands, {"pretend wrap": BOUNDARY})
    with pytest.raises(AssertionError, match="last"):
        _check_along(ref, out, tail, tail_ref, bands, {})
    ref, out, tail, tail_ref, bands = _synthetic_along()
    out[BOUNDARY:400] = out[BOUNDARY - WRAP:400 - WRAP].clone()  # (confined to the middle, the boundary not known: the device pass)
    with pytest.raises(AssertionError, match=f"slab {BOUNDARY} is .* of period 1"):
        _check_along(ref, out, tail, tail_ref, bands, {})


def test_the_checker_fails_on_one_zeroed_interior_period():
    ref, out, tail, tail_ref, bands = _synthetic_along()
    out[4 * E.PERIOD:5 * E.PERIOD] = 0.0  # (period 4: in no window)
    with pytest.raises(AssertionError, match=f"slab {4 * E.PERIOD} is"):
        _check_along(ref, out, tail, tail_ref, bands, {"pretend wrap": BOUNDARY})


def test_the_checker_fails_on_an_unwritten_tail():
    ref, out, tail, tail_ref, bands = _synthetic_along()
    tail[-1] = float("nan")
    with pytest.raises(AssertionError, match="the tail behind the last whole period"):
        _check_along(ref, out, tail, tail_ref, bands, {"pretend wrap": BOUNDARY})
    ref, out, tail, tail_ref, bands = _synthetic_along()
    tail[2] = 0.0  # (written, wrong)
    with pytest.raises(AssertionError, match="synthetic tail"):
        _check_along(ref, out, tail, tail_ref, bands, {"pretend wrap": BOUNDARY})


def test_the_checker_fails_on_one_flipped_bit_of_an_interior_period():
    ref, out, tail, tail_ref, bands = _synthetic_along()
    out[7 * E.PERIOD + 11].view(torch.int32)[3] ^= 1  # (period 7: in no window; one ulp: within the bound)
    assert _check_along(ref, out, tail, tail_ref, bands, {"pretend wrap": BOUNDARY}) is False
    with pytest.raises(AssertionError, match="an interior period differs in its bits"):
        _check_along(ref, out, tail, tail_ref, bands, {"pretend wrap": BOUNDARY}, exact=True)
    ref, out, tail, tail_ref, bands = _synthetic_along()
    out[3].view(torch.int32)[3] ^= 1  # (an edge is held to float64 only)
    assert _check_along(ref, out, tail, tail_ref, bands, {"pretend wrap": BOUNDARY}, exact=True) is True


def test_the_checker_takes_whole_periods_under_a_norm_wise_bound():
    """The form of istft and fir_filter: one absolute bound per period of the reference, the window check on a whole period."""
    ref, out, tail, tail_ref, bands = _synthetic_along()
    bnd = [A.bound(A.F32, POINTS) * float(np.sqrt((ref[q * E.PERIOD:(q + 1) * E.PERIOD] ** 2).sum())) for q in range(4)]

    def accurate(got, r, rp, what):
        assert got.shape == r.shape == (E.PERIOD, POINTS) and np.sqrt(((got - r) ** 2).sum()) <= bnd[rp], what

    def run(exact=True):
        along = E.Along(1, {0: 0, SLABS // E.PERIOD - 1: 3}, None, whole=True)
        return E.check(out, ref, bnd, {"pretend wrap": BOUNDARY}, accurate, exact=exact, bands=bands, what="synthetic", along=along)

    assert run() is True
    out[4 * E.PERIOD + 7] = 0.0
    with pytest.raises(AssertionError, match="period 4 is"):
        run(exact=False)
    out[4 * E.PERIOD + 7] = out[E.PERIOD + 7]
    out[BOUNDARY] = out[BOUNDARY - WRAP]
    with pytest.raises(AssertionError, match="pretend wrap"):
        run()


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


# ---- the segment kernels (spectrogram, istft, fir_filter): every new runner once, at four to six periods along the series and 2 x PERIOD series
ALONG = {
    "spectrogram-64-37-complex": (lambda: E.keep_along(64, 37, L.OUT_COMPLEX), 5),
    "spectrogram-64-32-power": (lambda: E.keep_along(64, 32, L.OUT_POWER), 6),
    "spectrogram-256-128-power": (lambda: E.keep_along(256, 128, L.OUT_POWER), 4),
    "istft-64-16-hann": (lambda: E.synth_along(64, 16, "hann"), 5),
    "istft-64-37-boxcar": (lambda: E.synth_along(64, 37, None), 6),
    "istft-256-128-hann": (lambda: E.synth_along(256, 128, "hann"), 4),
    "fir-64-8-same": (lambda: E.filter_along(64, 8, "same"), 5),
    "fir-64-8-full": (lambda: E.filter_along(64, 8, "full"), 5),
    "fir-256-65-valid": (lambda: E.filter_along(256, 65, "valid"), 4),
}


@pytest.mark.parametrize("cid", list(ALONG))
def test_one_long_series_through_the_harness(cid):
    """The period along the series: the MI355X runs these runners at 2^26 segments (rung B), here four to six periods."""
    make, q = ALONG[cid]
    _plan, bounds, same = E.run_along(cid, make(), q, "cpu")
    assert bounds == {} and same


def test_segment_kernels_across_the_batch_through_the_harness():
    """Rung A's four cases at 96 series (columns)."""
    for cid, c in (("spectrogram-rows", E.keep_batch(64, 37, 130, L.OUT_COMPLEX)), ("istft", E.synth_batch(64, 37, 130, "hann")),
                   ("fir_filter", E.filter_batch(64, 8, 8000, "same"))):
        assert E.run_batch(cid, c, 2 * E.PERIOD, "cpu")[2]
    assert E.run_keep_cols("spectrogram-columns", 64, 37, 9, 3, 2 * E.PERIOD, "cpu")[2]
    assert E.run_keep_cols("spectrogram-columns-one-block", 64, 32, 20, 1, 2 * E.PERIOD, "cpu")[2]


def test_segment_kernels_through_the_pitch_through_the_harness():
    """Rung C's four runners at pitches a CPU holds (the MI355X: 2^30 + 5 between the series, a sample stride of 2^20)."""
    E.run_keep_rows_pitched("spectrogram-rows-pitch", "cpu", pitch=128 + 5)
    E.run_keep_cols_strided("spectrogram-columns-stride", "cpu", s=64, c=(64, 32, 5, 2, 40), beyond=0)
    E.run_synth_pitched("istft-pitch", "cpu", pitch=3 * 33 + 5)
    E.run_filter_pitched("fir-pitch", "cpu", pitch=700 + 5)


def test_the_one_series_shapes_of_rung_b():
    """The lengths rung B runs at: one whole period beyond 2^31 elements, the boundaries they reach, and that a wrap lands on another member (boundaries() asserts)."""
    m = E.batch_beyond(32, 64)
    assert m % E.PERIOD == 0 and (m - E.PERIOD) * 32 >= 1 << 31 > (m - 2 * E.PERIOD) * 32
    bd = E.boundaries(m, 32, 4, 64, 4)
    assert set(bd) == {f"{s} {n}" for s in ("input", "output") for n in ("2^31 elements", "2^32 bytes", "2^33 bytes")}
    assert bd["input 2^31 elements"] == bd["input 2^33 bytes"] == 1 << 26 and bd["output 2^31 elements"] == 1 << 25
    m = E.batch_beyond(33, None)
    assert (m - E.PERIOD) * 33 >= 1 << 31 and (m - 1) * 16 + 64 < (1 << 31) - 1  # (the span stays under the span guard)
    bd = E.boundaries(m, 33, 8, 16, 4, limits=E.MORE_LIMITS)
    assert {"input 2^31 elements", "input 2^33 bytes", "input 2^34 bytes"} <= set(bd) and not [k for k in bd if k.startswith("output 2^3")]
    assert bd["input 2^34 bytes"] == bd["input 2^31 elements"] == -(-(1 << 31) // 33)
    n = E.batch_beyond(57, 57)
    assert (n - E.PERIOD) * 57 >= 1 << 31
    assert set(E.boundaries(n, 57, 4, 57, 4)) == {f"{s} {x}" for s in ("input", "output") for x in ("2^31 elements", "2^32 bytes", "2^33 bytes")}
    assert set(E.SEGMENT_EXACT) == {"spectrogram", "istft", "fir_filter"} and all(E.SEGMENT_EXACT.values()) and not set(E.SEGMENT_EXACT) & set(E.EXACT)


def test_strided_boxes_through_the_harness():
    """Rung C's runner at strides a CPU holds (the MI355X runs it at 2^30 + 16 elements between the slabs and at the largest pitch)."""
    E.run_strided("fasts", "fasts", 3, 0, 64 * 128 + 16, "cpu")
    E.run_strided("fastg-pitch", "fastg-f32", 2, 60, 50 * 60, "cpu")
    E.run_welch_rows_pitched("welch-rows-pitch", "cpu", pitch=128 + 5)
    E.run_welch_cols_strided("welch-columns-stride", "cpu", s=64, c=(64, 32, 5, 2, 40), beyond=0)
