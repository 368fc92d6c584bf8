"""Single-end random PBAT (-R, walt_map_se_rpbat_batch) without a GPU: the command line refuses the combinations the
mode does not define before it opens a device, and every library and the Python binding carry the new calls."""
import ctypes
import os
import subprocess

import pytest

import refio

WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
RPBAT_SYMBOLS = ("walt_se_rpbat_workspace_bytes", "walt_map_se_rpbat_batch", "walt_map_se_rpbat_batch_device")


@pytest.mark.parametrize("extra, word", [
    (["-r", "reads.fq", "-A"], "-A"),
    (["-r", "reads.fq", "-P"], "-P"),
    (["-1", "r1.fq", "-2", "r2.fq"], "-1"),
    (["--random-pbat", "-1", "r1.fq", "-2", "r2.fq"], "-1"),
])
def test_cli_refuses_random_pbat_combinations(tmp_path, extra, word):
    # neither the index nor the reads exist: the refusal comes from the option check, before any file or device
    cmd = [WALT_BIN, "-i", str(tmp_path / "none.dbindex"), "-o", str(tmp_path / "out.mr")]
    cmd += extra if "--random-pbat" in extra else ["-R"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode != 0
    assert "-R" in p.stderr and word in p.stderr, p.stderr
    assert "index file missing" not in p.stderr
    assert not os.path.exists(tmp_path / "out.mr")


def test_cli_knows_the_option(tmp_path):
    # -R alone passes the option check and stops at the missing index, like any other single-end run
    p = subprocess.run([WALT_BIN, "-i", str(tmp_path / "none.dbindex"), "-o", str(tmp_path / "out.mr"), "-R", "-r",
                        "reads.fq"], capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode != 0 and "index file missing" in p.stderr, p.stderr
    p = subprocess.run([WALT_BIN], capture_output=True, text=True)
    assert " -R " in p.stderr


def test_index_has_random_pbat_methods():
    import walt_amd
    assert callable(getattr(walt_amd.Index, "map_se_rpbat_batch", None))
    assert callable(getattr(walt_amd.Index, "map_se_rpbat_batch_device", None))
    assert callable(getattr(walt_amd, "se_rpbat_workspace_bytes", None))


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_random_pbat_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    for nm in RPBAT_SYMBOLS:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)


@pytest.mark.parametrize("n, read_len", [(1, 100), (1800, 150), (100000, 100)])
def test_workspace_holds_the_second_record_array(n, read_len):
    """walt_se_rpbat_workspace_bytes = walt_se_workspace_bytes plus n aligned 16-byte records (host arithmetic only)."""
    import walt_amd
    L = walt_amd.lib(3)
    one = L.walt_se_workspace_bytes(n, read_len)
    both = L.walt_se_rpbat_workspace_bytes(n, read_len)
    assert both == (one + 15) // 16 * 16 + 16 * n
    assert walt_amd.se_rpbat_workspace_bytes(n, read_len) == both
