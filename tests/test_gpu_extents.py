"""GPU (-m gpu): the extent ladder on an MI355X (tests/extents.py) -- per kernel family, the smallest extents at which an index that wraps can show.

* rung A: 70 080 slabs, rows or series -- more than one grid dimension holds;
* rung B: dense batches whose last period lies beyond element offset 2^31 (float32: byte offset 2^33) in input and output, 11 to 83 GiB per case;
* rung C: the same offsets through the descriptor's strides -- 2^30 + 16 elements between the slabs, the largest pitch a plan accepts, a Welch series pitch of
  2^30 + 5 samples, a Welch sample stride of 2^20 --, in buffers that are allocated and never filled;
* rung D: the host guards at the limit and one step past it (plan creation only), as on the CPU;
* the spectrogram, istft and fir_filter kernels on each rung: 70 080 series or columns with several workgroups each (A); ONE series of 2^26 segments per kernel, whose
  sample offsets pass 2^31 inside the series, dense batches of short series, and a column-layout output beyond 2^31 elements inside one block (B, 17 to 26 GiB); a
  series pitch of 2^30 + 5 and a sample stride of 2^20 (C); their guards (D).  Along a series the first and last periods are edges held to float64, every interior
  period has the bits of the first interior one.  Not covered: API-level calls at these sizes (a span past 2^31 - 1: the composed route), 2^32 complex elements of
  istft input, L = 4096 variants of the one-series cases.

Every case of rungs A and B asserts its family, whole periods (the first, the last, every one that holds the first slab beyond a boundary) slab by slab against the
float64 reference at rounding level, every slab on the device against its member of the first period, and the guard bands around output, radial sums and workspace.
Each states the device memory it needs and skips only if less is free."""
import warnings

import pytest

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

torch = pytest.importorskip("torch")

import extents as E  # noqa: E402
import strided as S  # noqa: E402
from xrft_amd import _lib as L  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def real_library():
    from xrft_amd import api

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    api.clear_plan_cache()
    L._state.update(dll=None, path=None, device="cuda")
    L.load()  # raises XrftHipUnavailable if the HIP library is missing: no fallback
    assert L._state["path"].endswith("libxrft_hip.so") and L.device() == "cuda"
    yield
    E.teardown("cuda")  # the plan cache and the engine's grow-only scratch: the rest of the suite sees the memory it saw before


def _run(f, *args, **kw):
    try:
        return f(*args, **kw)
    except E.NeedsMemory as e:
        pytest.skip(str(e))
    except RuntimeError as e:  # a HIP error (the library's status with hipGetLastError behind it, or torch's): nothing more is started on this device
        if getattr(e, "hip_error", 0) or "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"a HIP error ends the module: {e}", returncode=3)
        raise


# ---------------------------------------------------------------------------------- rung A: counts
@pytest.mark.parametrize("cid", list(E.RUNG_A))
def test_rung_a_counts(cid):
    kw, env, kind, tag = E.RUNG_A[cid]
    _run(E.run_plain, cid, kw, env, kind, tag, E.COUNT, "cuda")


def test_rung_a_fasts_mean():
    """mean_batch = 2 over 140 160 slabs of 64 x 64 (70 080 outputs), the mean form forced where the default composes (XRFTHIP_MEAN_ALL)."""
    _run(E.run_mean, "fasts-mean", 64, 64, 2, 2 * E.COUNT, {"XRFTHIP_MEAN_ALL": "1"}, L.K_FASTS, "cuda")


def test_rung_a_welch_rows():
    _run(E.run_welch_rows, "welch-rows", 64, 32, 3, E.COUNT, "cuda")


def test_rung_a_welch_columns():
    _run(E.run_welch_cols, "welch-columns", 64, 32, 3, 3, E.COUNT, "cuda")


def test_radial_sums_over_several_groups():
    _run(E.run_iso_in_groups, "cuda")


# ---------------------------------------------------------------------------------- rung B: dense extents
def _beyond(bounds, sides=("input", "output")):
    for side in sides:
        assert f"{side} 2^31 elements" in bounds, bounds


@pytest.mark.parametrize("cid", list(E.RUNG_B))
def test_rung_b_dense(cid):
    kw, env, kind, tag = E.RUNG_B[cid]
    _plan, bounds = _run(E.run_plain, cid, kw, env, kind, tag, E.dense_batch(kw, env), "cuda")
    _beyond(bounds)
    if E.esize(kw.get("dtype", E.A.F32)) >= 4:
        assert "input 2^33 bytes" in bounds
    assert "output 2^33 bytes" in bounds


def test_rung_b_fasty_mean():
    """256 x 512, mean_batch = 2: the float64 partials [output][run] and the halved output both pass 2^31 elements."""
    _plan, bounds = _run(E.run_mean, "fasty-mean", 256, 512, 2, E.batch_beyond(256 * 512, 256 * 512 // 2), {}, L.K_FASTY, "cuda")
    _beyond(bounds)


def test_rung_b_fasty_coherence():
    _plan, bounds = _run(E.run_mean, "fasty-coherence", 256, 512, 2, E.batch_beyond(256 * 512, 256 * 512 // 2), {}, L.K_FASTY, "cuda", coherence=True)
    _beyond(bounds)


def test_rung_b_welch_rows():
    """Dense series, P x span beyond 2^31 samples.  A Welch plan takes (2^31 - 1) / 1024 outputs at most (extents.check_guards), so the series have 32 segments
    (a span of 1056 samples): 2 033 664 of them."""
    p = E.batch_beyond(31 * 32 + 64, None)
    assert p <= E.WELCH_OUTPUTS
    _plan, bounds = _run(E.run_welch_rows, "welch-rows-dense", 64, 32, 32, p, "cuda")
    _beyond(bounds, ("input",))
    assert "input 2^33 bytes" in bounds


# ---------------------------------------------------------------------------------- rung C: offsets through the descriptor's strides
@pytest.mark.parametrize("fam", list(E.RUNG_C_BATCH_STRIDE))
def test_rung_c_huge_batch_stride(fam):
    """batch = 3 with 2^30 + 16 elements between the slabs: slab 2 starts beyond element 2^31 and byte 2^33 (FastG rows: 300 rows at the largest stride)."""
    rid = E.RUNG_C_BATCH_STRIDE[fam]
    assert rid in S.FAMILIES[fam]
    if fam == "FastG-rows":  # 32-bit offsets among the rows of one workgroup: the largest stride the plan accepts, and more rows than a workgroup takes
        _run(E.run_strided, f"{fam}-batch-stride", rid, E.ROWS_BATCH, 0, E.largest_rows_stride(rid, E.ROWS_BATCH), "cuda", beyond=1 << 31)
    else:
        _run(E.run_strided, f"{fam}-batch-stride", rid, 3, 0, E.HUGE_STRIDE, "cuda", beyond=1 << 31)


@pytest.mark.parametrize("fam", list(E.RUNG_C_PITCH))
def test_rung_c_largest_pitch(fam):
    """The largest in_stride_y the plan accepts (ny x pitch x 4 within 16 bytes x ny of 2^32): the kernels' 32-bit row x pitch + column sums come within one row of
    wrapping.  One 16-byte step further is XRFTHIP_UNSUPPORTED_LENGTH: extents.check_guards."""
    rid = E.RUNG_C_PITCH[fam]
    kw, _, _ = S.table_row(rid)
    pitch = E.largest_pitch(kw["ny"], 4)
    _run(E.run_strided, f"{fam}-largest-pitch", rid, 2, pitch, kw["ny"] * pitch, "cuda")


def test_rung_c_welch_rows_with_a_huge_series_pitch():
    _run(E.run_welch_rows_pitched, "welch-rows-pitch", "cuda")


def test_rung_c_welch_columns_with_a_huge_sample_stride():
    _run(E.run_welch_cols_strided, "welch-columns-stride", "cuda")


# ---------------------------------------------------------------------------------- the segment kernels: spectrogram (fastk.h), istft (fasto.h), fir_filter (fastf.h)
# Every case asserts K_FASTW and its own describe line (spectrogram.assert_keep_plan, istft.assert_synth_plan, fir_filter.assert_filter_plan), a workspace of 0
# bytes, and bit identity (extents.SEGMENT_EXACT): the third value the runners return.
def _segments(f, *args, **kw):
    _plan, bounds, same = _run(f, *args, **kw)
    assert same is True
    return bounds


# ---- rung A: 70 080 series (columns), several workgroups per series, the last one short
SEGMENT_RUNG_A = {
    "spectrogram-rows": lambda: E.keep_batch(64, 37, 130, L.OUT_COMPLEX),  # 2 rounds per series, the second nearly empty
    "istft": lambda: E.synth_batch(64, 37, 130, "hann"),                   # 2 workgroups per series
    "fir_filter": lambda: E.filter_batch(64, 8, 8000, "same"),             # V = 57, unaligned; 141 segments: 2 workgroups per series
}


@pytest.mark.parametrize("cid", list(SEGMENT_RUNG_A))
def test_rung_a_segment_counts(cid):
    _segments(E.run_batch, cid, SEGMENT_RUNG_A[cid](), E.COUNT, "cuda")  # (the complex spectrogram's output also passes 2^32 bytes: a window of its own)


def test_rung_a_spectrogram_columns():
    """3 blocks of 70 080 columns, seg_stride = inner, POWER; block b scaled by 2^b and taken out again."""
    _segments(E.run_keep_cols, "spectrogram-columns", 64, 37, 9, 3, E.COUNT, "cuda")


# ---- rung B: each term at its smallest shape.  One series: the offsets grow INSIDE it
def _reached(bounds, *names):
    for name in names:
        assert name in bounds, (name, bounds)


def test_rung_b_spectrogram_one_series():
    """(64, 32, M, 1), POWER, full output: segment s starts at s H >= 2^31 samples and writes at s 64 >= 2^31 elements (2^33 bytes) -- seg_tile.h:77, fastk.h:60."""
    m = E.batch_beyond(32, 64)
    bounds = _segments(E.run_along, "spectrogram-one-series", E.keep_along(64, 32, L.OUT_POWER), m // E.PERIOD, "cuda")
    _beyond(bounds)
    _reached(bounds, "input 2^33 bytes", "output 2^33 bytes")


def test_rung_b_spectrogram_many_series():
    """(64, 32, 32, P): blk * pitch and blk * M * nxo."""
    bounds = _segments(E.run_batch, "spectrogram-many-series", E.keep_batch(64, 32, 32, L.OUT_POWER), E.batch_beyond(1056, 32 * 64), "cuda")
    _beyond(bounds)
    _reached(bounds, "input 2^33 bytes", "output 2^33 bytes")


def test_rung_b_spectrogram_columns_output():
    """(64, 32, 480), one block of 70 080 columns: (obase + r) inner + c0 + col passes 2^31 elements (fastk.h:75) in every column's last segments."""
    bounds = _segments(E.run_keep_cols, "spectrogram-columns-output", 64, 32, 480, 1, E.COUNT, "cuda")
    _beyond(bounds, ("output",))
    _reached(bounds, "output 2^33 bytes")


def test_rung_b_istft_one_series():
    """(64, 16, M, 1): 33 M beyond 2^31 complex elements (2^34 bytes) through s0 (n + 1) with s0 an int (fasto.h:45-48); R = 4, F = 125; the span of about 2^30
    samples stays under the span guard."""
    m = E.batch_beyond(33, None)
    bounds = _segments(E.run_along, "istft-one-series", E.synth_along(64, 16, "hann"), m // E.PERIOD, "cuda")
    _beyond(bounds, ("input",))
    _reached(bounds, "input 2^33 bytes", "input 2^34 bytes")


def test_rung_b_istft_many_series():
    """(64, 32, 32, P): series * pitch, series * span (fasto.h:48, :77)."""
    bounds = _segments(E.run_batch, "istft-many-series", E.synth_batch(64, 32, 32, "hann"), E.batch_beyond(32 * 33, 1056), "cuda")
    _beyond(bounds)
    _reached(bounds, "input 2^34 bytes", "output 2^33 bytes")


def test_rung_b_fir_filter_one_series():
    """(64, 8, N, 1), "same": first, idx < N and o0 (fastf.h:52-58, :104-107) beyond sample 2^31."""
    q = E.batch_beyond(57, 57) // E.PERIOD
    bounds = _segments(E.run_along, "fir-one-series", E.filter_along(64, 8, "same"), q, "cuda")
    _beyond(bounds)
    _reached(bounds, "input 2^33 bytes", "output 2^33 bytes")


def test_rung_b_fir_filter_many_series():
    """(64, 8, 8000, P): series * pitch, series * n_out."""
    bounds = _segments(E.run_batch, "fir-many-series", E.filter_batch(64, 8, 8000, "same"), E.batch_beyond(8000, 8000), "cuda")
    _beyond(bounds)
    _reached(bounds, "input 2^33 bytes", "output 2^33 bytes")


# ---- rung C: through the pitch
def test_rung_c_spectrogram_rows_with_a_huge_series_pitch():
    _run(E.run_keep_rows_pitched, "spectrogram-rows-pitch", "cuda")


def test_rung_c_spectrogram_columns_with_a_huge_sample_stride():
    _run(E.run_keep_cols_strided, "spectrogram-columns-stride", "cuda")


def test_rung_c_istft_with_a_huge_series_pitch():
    _run(E.run_synth_pitched, "istft-pitch", "cuda")


def test_rung_c_fir_filter_with_a_huge_series_pitch():
    _run(E.run_filter_pitched, "fir-pitch", "cuda")


# ---------------------------------------------------------------------------------- rung D: the guards
def test_rung_d_guards():
    E.check_guards()
    E.check_iso_group_limit()
