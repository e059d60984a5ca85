import sys
from pathlib import Path

import pytest

REPO_ROOT = Path(__file__).resolve().parent.parent
if str(REPO_ROOT) not in sys.path:
    sys.path.insert(0, str(REPO_ROOT))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires a real MI355X GPU (run via gpurun)"
    )


@pytest.fixture
def repo_root() -> Path:
    return REPO_ROOT


def _short_tmp_root() -> str:
    """Shortest writable temp directory on this host."""
    import os
    import tempfile

    candidates = [tempfile.gettempdir(), "/tmp", "/var/tmp", "/dev/shm"]
    usable = [c for c in candidates
              if os.path.isdir(c) and os.access(c, os.W_OK | os.X_OK)]
    return min(usable, key=len)


@pytest.fixture
def tmp_path():
    """Per-test scratch directory with a short absolute path.

    Most suites bind AF_UNIX sockets under tmp_path, and sockaddr_un caps
    the path at 107 bytes. pytest's own tmp_path nests
    <TMPDIR>/pytest-of-<user>/pytest-N/<test-name>N/, which overflows that
    limit under a deep TMPDIR or a long user name — the plugin then cannot
    bind and every socket test fails. This override keeps the same
    contract (fresh empty directory per test, removed afterwards) but
    stays a few dozen bytes long wherever the suite runs.
    """
    import shutil
    import tempfile

    d = Path(tempfile.mkdtemp(prefix="k3samd-", dir=_short_tmp_root()))
    try:
        yield d
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session", autouse=True)
def build_native():
    """Every suite needs the native tree once per session (no-op when
    up to date)."""
    import subprocess
    subprocess.run(["make", "-C", str(REPO_ROOT / "native"), "-j8"],
                   check=True, capture_output=True)
