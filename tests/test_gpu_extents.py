"""GPU (-m gpu): the extent ladder on an MI355X (tests/extents.py) -- per kernel family, the smallest extents at which an index that wraps can show.

* rung A: 70 080 slabs, rows or series -- more than one grid dimension holds;
* rung B: dense batches whose last period lies beyond element offset 2^31 (float32: byte offset 2^33) in input and output, 11 to 83 GiB per case;
* rung C: the same offsets through the descriptor's strides -- 2^30 + 16 elements between the slabs, the largest pitch a plan accepts, a Welch series pitch of
  2^30 + 5 samples, a Welch sample stride of 2^20 --, in buffers that are allocated and never filled;
* rung D: the host guards at the limit and one step past it (plan creation only), as on the CPU.

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


# ---------------------------------------------------------------------------------- rung D: the guards
def test_rung_d_guards():
    E.check_guards()
    E.check_iso_group_limit()
