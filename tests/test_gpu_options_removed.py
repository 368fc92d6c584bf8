"""The options of the superseded single-end schedules are gone from the product library: their names are refused like
any unknown name, by the C ABI and by the command line, and se_lit_side no longer takes the value 2."""
import os
import subprocess

import pytest

import refio

pytestmark = pytest.mark.gpu

REMOVED = ["se_lit_staged", "se_lit_ablate", "se_stagger", "se_stage_blocks", "se_verify_blocks"]
WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")


@pytest.fixture(scope="module")
def idx(g1_index_path):
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    index = walt_amd.Index.open(g1_index_path, device=0)
    yield index
    index.close()


@pytest.mark.parametrize("name", REMOVED)
def test_removed_option_names_are_refused(idx, name):
    import walt_amd
    with pytest.raises(walt_amd.WaltError) as e:
        idx.set_option(name, 1)
    assert e.value.code == walt_amd.WALT_EINVAL and name in str(e.value)
    with pytest.raises(walt_amd.WaltError) as e:
        idx.get_option(name)
    assert e.value.code == walt_amd.WALT_EINVAL and name in str(e.value)


def test_se_lit_side_2_is_out_of_range(idx):
    import walt_amd
    with pytest.raises(walt_amd.WaltError) as e:
        idx.set_option("se_lit_side", 2)
    assert e.value.code == walt_amd.WALT_EINVAL and "se_lit_side" in str(e.value) and "outside" in str(e.value)
    assert idx.get_option("se_lit_side") == 1


def test_cli_refuses_a_removed_option(g1_index_path, scratch):
    r = subprocess.run([WALT_BIN, "-i", g1_index_path, "-r", os.path.join(refio.GOLDEN, "sp_short.fastq"), "-o",
                        os.path.join(scratch, "removed_option.sam"), "-X", "se_lit_staged=1"], capture_output=True, text=True)
    assert r.returncode != 0 and "se_lit_staged" in r.stderr
