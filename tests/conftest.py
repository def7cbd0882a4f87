import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run by the driver with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "gpu_exclusive: times the GPU, so no other GPU test may run next to it")


# ---- a test that times the GPU reads the load of other GPU tests as its own failure (another process's kernels look like a
# shared hardware pipe to tests/test_gpu_queues.py).  When the suite runs in several processes (pytest-xdist), every GPU test holds
# a shared lock for its duration and a gpu_exclusive test an exclusive one; while an exclusive test waits, the turnstile keeps new
# shared holders out.  In a single process the locks are never contended.
@pytest.fixture(autouse=True)
def _gpu_lock(request, tmp_path_factory):
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    import fcntl

    root = tmp_path_factory.getbasetemp().parent   # shared by the xdist workers of one run
    exclusive = request.node.get_closest_marker("gpu_exclusive") is not None
    with open(root / "gpu_turnstile.lock", "a") as turnstile, open(root / "gpu.lock", "a") as lock:
        fcntl.flock(turnstile, fcntl.LOCK_EX)
        try:
            fcntl.flock(lock, fcntl.LOCK_EX if exclusive else fcntl.LOCK_SH)
        finally:
            fcntl.flock(turnstile, fcntl.LOCK_UN)
        try:
            yield
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def pytest_collection_modifyitems(config, items):
    if _has_gpu():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


# ---- the library reads its RFLU_* tuning variables once per handle (rflu_create); tests switch them between calls through
# monkeypatch: let every setenv / delenv / undo make the default handles read the environment again (rflu_reload_tuning)
def _reload_library_tuning():
    mod = sys.modules.get("recursivefactorization.jl_amd._ffi")
    if mod is not None and getattr(mod, "_lib", None) is not None:
        try:
            mod.reload_tuning()
        except Exception:
            pass


def _wrap_monkeypatch(name):
    orig = getattr(pytest.MonkeyPatch, name)

    def wrapped(self, *a, **k):
        r = orig(self, *a, **k)
        _reload_library_tuning()
        return r

    setattr(pytest.MonkeyPatch, name, wrapped)


for _n in ("setenv", "delenv", "undo"):
    _wrap_monkeypatch(_n)
