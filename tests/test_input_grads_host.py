"""tests/golden/dit_input_grads.npz (made by tests/make_golden_input_grads.py from the REAL reference): the fixture
loads with the keys and shapes its cases promise; where the reference tree is present it regenerates in memory, and
the CPU oracle's autograd through the same graphs agrees with it."""
import os

import numpy as np
import pytest

import make_golden_input_grads as MG
from oracle import ref_import

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_input_grads.npz")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def test_fixture_matches_its_cases():
    g = np.load(GOLD)
    want = MG.expected_keys()
    assert {k: tuple(g[k].shape) for k in g.files} == want
    assert os.path.getsize(GOLD) < 340_000
    for k in g.files:
        assert np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0, k       # every input gradient is non-zero


@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
def test_fixture_regenerates_and_oracle_agrees():
    g = np.load(GOLD)
    again = MG.compute(MG.reference_forward)
    for k in g.files:
        assert _rel(again[k], g[k]) < 1e-6, k
    orc = MG.compute(MG.oracle_forward)
    for k in g.files:
        assert _rel(orc[k], g[k]) < 1e-4, (k, _rel(orc[k], g[k]))
