"""Randomised check of the per-cytosine pile-up: tools/soak.py's run_soak_pileup on a fixed set of genomes (pattern 3),
many of them with hundreds of short chromosomes; reads of both conversions and both strands, some with call_len, and
the whole table of every genome equal to the restatement of the contract (tests/test_gpu_pileup.py)."""
import os
import sys

import pytest

import refio

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(refio.ROOT, "tools"))

GENOMES = 12  # the only knob


def test_pileup_soak_pattern3():
    import soak
    line = soak.run_soak_pileup(range(1, GENOMES + 1), pattern=3)
    assert line.startswith("soak ok"), line
