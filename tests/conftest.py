import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# torch before the product library, in every test process: torch carries its own HIP runtime under another file name than the one
# libslide_gpu.so links, so the library loaded first leaves two HIP (and HSA) runtimes in the process, and the one initialised second
# sees no device (a CPU test that loads the library, then the GPU tests of the same session).  torch loaded first, the library binds
# to torch's runtime, as in bench.py and __graft_entry__.smoke().
import torch  # noqa: E402,F401


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (gfx950); run with -m gpu on the GPU box")


@pytest.fixture(scope="session")
def oracle_lib():
    from oracle import pyoracle
    return pyoracle.lib()


@pytest.fixture(scope="session")
def gpu():
    """The product library on a gfx950 device; the tests FAIL (not skip) when it is unusable."""
    import slide_slam_amd as s
    s.device_check()
    return s
