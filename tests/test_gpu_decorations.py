"""The decoration ladder (tests/decorations.py) through the real libxrft_hip.so on the MI355X: the cases, inputs, reference, bounds and recorded routing of
tests/test_decorations_emulated.py, one parametrisation for both.  Nothing here reads files outside the repository."""
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decorations as D  # noqa: E402

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


CASES = D.cases()


@pytest.mark.parametrize("kw,env,tokens,expect", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_decorations(monkeypatch, kw, env, tokens, expect):
    _env(monkeypatch, env)
    D.run(kw, tokens, expect, "cuda")
