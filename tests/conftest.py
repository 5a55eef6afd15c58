import glob
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "yolo-continuous_amd")
GOLD = os.path.join(REPO, "tests", "golden")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950) device and the built HIP library")


@pytest.fixture(scope="session")
def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)


def _golden_parts(stem):
    """The arrays of <stem>.<i>.npz, i = 0, 1, ...: make_golden.py writes the larger
    fixtures in parts so that no committed file exceeds 1 MiB."""
    parts = sorted(glob.glob(os.path.join(GOLD, stem + ".[0-9]*.npz")))
    assert parts, f"no {stem}.<i>.npz under {GOLD}"
    out = {}
    for p in parts:
        out.update(np.load(p))
    return out


@pytest.fixture(scope="session")
def g1():
    return _golden_parts("g1_ops")


@pytest.fixture(scope="session")
def g2():
    return _golden_parts("g2_nets")


@pytest.fixture(scope="session")
def g3():
    return dict(np.load(os.path.join(GOLD, "g3_post.npz")))


@pytest.fixture(scope="session")
def device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")
