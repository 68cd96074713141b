import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def _has_gpu():
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


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle as O
    O.build()
    return O


@pytest.fixture(scope="session")
def ref_point_layout(oracle):
    """Layout facts of the reference's own Point.h as the probe built from it prints them.  build() makes the probe only where the
    reference tree is at hand (oracle/_ref/); its output is recorded in tests/golden/ref_point_layout.json, and a fresh probe run
    must still equal that record."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "ref_point_layout.json")) as f:
        recorded = json.load(f)
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "point_layout.json")):
        live = oracle.ref_point_layout()
        assert live == recorded, "the probe's output differs from tests/golden/ref_point_layout.json: %s" % live
        return live
    return recorded


@pytest.fixture(scope="session")
def pkg():
    import torch  # noqa: F401  -- before libpt_hip.so, so both share one HIP runtime
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="session")
def golden():
    import numpy as np
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_knn.npz"))


@pytest.fixture(scope="session")
def golden_cases():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.cases()
