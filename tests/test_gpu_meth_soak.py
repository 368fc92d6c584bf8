"""Randomised check of the methylation calls: tools/soak.py's run_soak_meth on a fixed set of genomes (pattern 3), both
conversions, calls, counts and totals of every read equal to the restatement of the contract (tests/test_gpu_meth.py)."""
import os
import sys

import pytest

import refio

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(refio.ROOT, "tools"))


def test_meth_soak_pattern3():
    import soak
    line = soak.run_soak_meth(range(1, 21), pattern=3)
    assert line.startswith("soak ok"), line
