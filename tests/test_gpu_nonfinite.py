"""A NaN / inf stays inside its own transform (tests/nonfinite.py), through the real libxrft_hip.so on the MI355X: the cross-lane and cross-wave meeting of a
sequence's marks exists only here.  Every case is a small shape; nothing here reads files outside the repository."""
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import nonfinite as N  # noqa: E402

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


@pytest.mark.parametrize("rid,batch,B,inpos,bad,detrend,field", [p[1:] for p in N.params()], ids=[p[0] for p in N.params()])
def test_a_bad_sample_stays_in_its_transform(monkeypatch, rid, batch, B, inpos, bad, detrend, field):
    _env(monkeypatch, N.ROWS[rid][2])
    N.run_case(rid, batch, B, inpos, bad, detrend, field, "cuda")


@pytest.mark.parametrize("size,order,dim", [p[1:] for p in N.api_params()], ids=[p[0] for p in N.api_params()])
def test_land_mask_through_the_api(monkeypatch, size, order, dim):
    _env(monkeypatch, {})
    for dtype in ("float64", "float32"):
        fams = N.run_api_land_mask(size, order, dim, dtype)
        assert fams == N.API_FAMILY[f"{'x'.join(map(str, size))}-{''.join(order)}-{''.join(dim)}"], fams
