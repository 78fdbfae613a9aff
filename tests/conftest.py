import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The CPU oracle is pinned to golden vectors at 2e-6 in fp32.  MKL picks its fp32 kernels by CPU vendor and model, and
# its branches round differently, so the tests ask for its generic branch, the one every x86 CPU can run and the one
# tests/golden/make_golden.py uses (unless the caller chose one).  MKL reads this when it initialises, after this file
# is imported.
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    d = os.path.join(ROOT, "tests", "golden")
    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = dict(np.load(os.path.join(d, name + ".npz")))
        return cache[name]

    return load
