"""The accuracy ladder and the layout x parity matrix (tests/accuracy.py) through the real libxrft_hip.so on the MI355X, plus the shapes
the emulator cannot afford: a 4096^2 float32 slab on the headline path, (1024, 65536) float32 rows, (64, 1440, 720) float64, 2^20-point
real and complex rows, and the resident-set walkers.  GPU-only arithmetic (cross-lane reductions, line-group rendezvous) is reached only
here.  Nothing here reads files outside the repository."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import accuracy as A  # noqa: E402

from xrft_amd import _lib as L  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def real_library():
    from xrft_amd import api

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    api._plan_cache.clear()
    L._state.update(dll=None, path=None, device="cuda")
    L.load()
    assert L._state["path"].endswith("libxrft_hip.so") and L.device() == "cuda"
    yield
    api._plan_cache.clear()


def _env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("XRFTHIP_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


LADDER = A.ladder_params(A.ROWS + A.MODES, every_signal_to=1 << 20)  # (every signal up to 2^20 points per transform here: the GPU affords it)


@pytest.mark.parametrize("kw,env,kind,tag,sig", [p[1:] for p in LADDER], ids=[p[0] for p in LADDER])
def test_ladder(monkeypatch, kw, env, kind, tag, sig):
    _env(monkeypatch, env)
    p, _c = A.run_ladder(kw, sig, "cuda")
    assert A.family(p) == (kind, tag)


@pytest.mark.parametrize("order,ny,nx,dim,rd", [p[1:] for p in A.matrix_params()], ids=[p[0] for p in A.matrix_params()])
def test_layout_matrix(order, ny, nx, dim, rd):
    for dtype in ("float64", "float32"):
        A.run_matrix_cell(order, ny, nx, dim, rd, dtype)


@pytest.mark.parametrize("op", ["fft", "power_spectrum", "cross_spectrum"])
@pytest.mark.parametrize("order", [("y", "x", "t"), ("y", "t", "x")])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_odd_real_axis_first_in_memory_on_the_fused_passes(order, dtype, op):
    A.run_odd_real_axis_first(order, dtype, op)


@pytest.mark.parametrize("n", [1 << 16, 1 << 20])
def test_four_step_input_phase_off_the_separable_form(n):
    p = A.run_four_step_phase(n, A.four_step_phase(n), "cuda")
    if n == 1 << 20:
        assert A.family(p) == (L.K_GENERIC, "main")  # (a table off the separable form: the generic four-step passes)


def test_four_step_input_phase_separable_stays_on_the_fast_family():
    p = A.run_four_step_phase(1 << 20, np.exp(0.001j * np.arange(1 << 20)), "cuda", seed=4)
    assert A.family(p) == (L.K_FASTY, "fasty complex rows, four-step")


def _run(kw, x, dev="cuda", x1=None, rows=None, env=None):
    """Execute make(**kw) on x (float64 / complex128 samples rounded to the plan's dtype) and hold it to the contract; `rows`: compare
    only these batch entries (the reference of the rest would cost the CPU more than the test is worth)."""
    p = A.make(**kw)
    dt = kw.get("dtype", A.F32)
    t, x64 = A.tensor(x, dt)
    t1 = x164 = None
    if x1 is not None:
        t1, x164 = A.tensor(x1, dt)
        t1 = t1.to(dev)
    out, _ = p.execute(t.to(dev), t1)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    if rows is not None:
        kw = dict(kw, batch=len(rows))
        x64 = x64[rows]
        x164 = None if x164 is None else x164[rows]
        out = out[rows]
    ref, _ = A.reference(kw, x64, x164)
    flat = kw.get("out_mode", L.OUT_POWER) == L.OUT_COMPLEX
    return p, A.assert_accurate(out.reshape(ref.shape), ref, dt, A.points(kw), flat=flat, what=str(A.family(p)))


def test_headline_slab_4096():
    rng = np.random.default_rng(21)
    p, _ = _run(dict(ny=4096, nx=4096, batch=1, out_mode=L.OUT_COMPLEX), rng.standard_normal((1, 4096, 4096)))
    assert A.family(p) == (L.K_FASTY, "fasty")


def test_long_float32_rows_subset():
    rng = np.random.default_rng(22)
    x = rng.standard_normal((1024, 65536))
    rows = [0, 1, 511, 1022, 1023]
    p, _ = _run(dict(ndim=1, nx=65536, batch=1024, out_mode=L.OUT_COMPLEX), x, rows=rows)
    assert A.family(p) == (L.K_FASTR, "fastr")


def test_fastm_float64_64x1440x720():
    rng = np.random.default_rng(23)
    p, _ = _run(dict(ny=1440, nx=720, batch=64, dtype=A.F64, out_mode=L.OUT_COMPLEX), rng.standard_normal((64, 1440, 720)))
    assert A.family(p)[0] in (L.K_FASTM, L.K_FASTN)


@pytest.mark.parametrize("cplx", [False, True])
def test_rows_of_2_20_points(cplx):
    rng = np.random.default_rng(24)
    n = 1 << 20
    x = rng.standard_normal((2, n)) + (1j * rng.standard_normal((2, n)) if cplx else 0.0)
    p, _ = _run(dict(ndim=1, nx=n, batch=2, dtype=A.C64 if cplx else A.F32, out_mode=L.OUT_COMPLEX), x)
    assert A.family(p) == ((L.K_FASTY, "fasty complex rows, four-step") if cplx else (L.K_FASTY, "fasty four-step"))


@pytest.mark.parametrize("shape", [(7, 256, 256), (5, 128, 256), (9, 64, 64)])
def test_small_slabs_walked_by_a_resident_set(monkeypatch, shape):
    _env(monkeypatch, {"XRFTHIP_FASTS_GRID": "2"})
    rng = np.random.default_rng(25)
    b, ny, nx = shape
    x = rng.standard_normal(shape) * (np.arange(b) + 1.0)[:, None, None]
    p, _ = _run(dict(ny=ny, nx=nx, batch=b, out_mode=L.OUT_COMPLEX), x)
    assert A.family(p) == (L.K_FASTS, "fasts")


def test_long_rows_walked_by_a_resident_set():
    rng = np.random.default_rng(26)
    x = rng.standard_normal((600, 32768)) * (np.arange(600) + 1.0)[:, None]
    p, _ = _run(dict(ndim=1, nx=32768, batch=600, out_mode=L.OUT_COMPLEX), x, rows=[0, 1, 299, 598, 599])
    assert A.family(p) == (L.K_FASTR, "fastr")
