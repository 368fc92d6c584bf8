"""Randomised check of single-end random PBAT: tools/soak.py's run_soak_rpbat on a fixed set of genomes (pattern 3),
reads of either conversion drawn at random, records and conversions equal to the rule on the oracle's two runs."""
import os
import sys

import pytest

import refio

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(refio.ROOT, "tools"))


def test_random_pbat_soak_pattern3():
    import soak
    line = soak.run_soak_rpbat(range(1, 21), pattern=3)
    assert line.startswith("soak ok"), line
