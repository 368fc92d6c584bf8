"""Paired-end random PBAT on random genomes (tools/soak.py run_soak_pe_rpbat): pairs of either orientation with random
m, b, k and L, every record and conversion identical to the rule applied to the oracle's two orientations."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_soak_pe_random_pbat_20_genomes():
    import soak
    line = soak.run_soak_pe_rpbat(range(1, 21))
    print(line)
    assert line.startswith("soak ok")
