"""walt_amd -- MI355X-native seed-and-extend hot path of WALT behind a C ABI.

This package is only the thin Python binding of ``lib/libwalt_amd.so`` (built
from ``csrc/`` by ``python -m walt_amd.build`` / ``__graft_entry__.build()``);
the product is the HIP library declared in ``include/walt_amd.h``.  There is
no CPU fallback: if the library is missing the import fails loudly, and the
mapping calls return WALT_EHIP when no GPU is present.

Function names and argument meaning follow the reference call sites they
replace (smithlabcode/walt v1.0): ``map_se_batch`` is the strand loop + OpenMP
loop over ``SingleEndMapping`` (mapping.cpp:486-500), ``map_pe_batch`` the
loops over ``PairEndMapping`` plus ``MergePairedEndResults``
(paired.cpp:642-699), ``Index`` is ``ReadIndexHeadInfo``/``ReadIndex``
(reference.cpp:324-417), ``makedb`` is makedb.cpp:128-159.
"""
import ctypes
import functools
import inspect
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# Seed pattern: a compile-time choice of the library, like the reference's -D SEEDPATTERN3 / 5 / 7
# (src/walt/Makefile:34, FAQ.md:5-13): libwalt_amd.so is pattern 3 (the default), libwalt_amd_sp5.so /
# libwalt_amd_sp7.so the other two.  set_pattern() (or WALT_AMD_PATTERN) selects the library that lib(),
# makedb() and the Index constructors use; an Index keeps the library it was made with.
PATTERN = int(os.environ.get("WALT_AMD_PATTERN", "3"))


def set_pattern(p):
    global PATTERN
    if p not in (3, 5, 7):
        raise ValueError("seed pattern must be 3, 5 or 7")
    PATTERN = p


def lib_path(pattern=None):
    pattern = PATTERN if pattern is None else pattern
    # WALT_AMD_LIB: another build of the default library (A/B timing of two builds on one GPU box; diagnostic)
    if pattern == 3 and os.environ.get("WALT_AMD_LIB"):
        return os.environ["WALT_AMD_LIB"]
    return os.path.join(_HERE, "lib", "libwalt_amd%s.so" % ("" if pattern == 3 else "_sp%d" % pattern))


LIB_PATH = lib_path(3)

WALT_OK = 0
STRAND_CT00, STRAND_CT01, STRAND_GA10, STRAND_GA11 = 1, 2, 4, 8
STRANDS_CT, STRANDS_GA, STRANDS_ALL = 3, 12, 15
WITH_REFERENCE = 16  # Index.open: also build the unconverted reference the methylation calls need


def effective_cpus():
    """CPUs this process may use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()
        if q != "max":
            n = min(n, max(1, -(-int(q) // int(p))))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                p = int(f.read())
            if q > 0 and p > 0:
                n = min(n, max(1, -(-q // p)))
        except (OSError, ValueError):
            pass
    return n

# numpy views of the C structs (include/walt_amd.h)
best_match_dtype = np.dtype(
    [("genome_pos", "<u4"), ("times", "<u4"), ("strand", "S1"), ("pad", "V3"), ("mismatch", "<u4")])
candidate_dtype = np.dtype([("genome_pos", "<u4"), ("strand", "S1"), ("pad", "V3"), ("mismatch", "<u4")])
pair_result_dtype = np.dtype(
    [("m1", best_match_dtype), ("m2", best_match_dtype), ("best_times", "<u4"), ("frag_len", "<i4"),
     ("best_i", "<i4"), ("best_j", "<i4"), ("pair_mm", "<u4"), ("pad", "V12")])
batch_stats_dtype = np.dtype(
    [("too_short", "<u8"), ("probes", "<u8"), ("candidates", "<u8"), ("big_regions", "<u8")])
meth_counts_dtype = np.dtype([("meth", "<u2", (4,)), ("unmeth", "<u2", (4,))])  # contexts: CpG, CHG, CHH, unknown
meth_stats_dtype = np.dtype([("reads", "<u8"), ("meth", "<u8", (4,)), ("unmeth", "<u8", (4,))])
METH_CONTEXTS = ("CpG", "CHG", "CHH", "unknown")
# walt_meth_site: one covered cytosine of the pile-up (strand ord('+') / ord('-'), context an index into METH_CONTEXTS)
meth_site_dtype = np.dtype([("pos", "<u4"), ("meth", "<u4"), ("unmeth", "<u4"), ("strand", "u1"), ("context", "u1"),
                            ("reserved", "<u2")])
assert meth_site_dtype.itemsize == 16
# walt_variant_site: a position the opposite-strand evidence flags (include/walt_amd.h, "opposite-strand evidence")
variant_site_dtype = np.dtype([("pos", "<u4"), ("meth", "<u4"), ("unmeth", "<u4"), ("strand", "u1"), ("context", "u1"),
                               ("reserved", "<u2"), ("match", "<u4"), ("other", "<u4")])
assert variant_site_dtype.itemsize == 24
# walt_levels: the genome-wide summary of a pile-up (include/walt_amd.h, "methylation levels"); rows CpG, CHG, CHH,
# unknown (METH_CONTEXTS) and CpG pairs
level_row_dtype = np.dtype([("sites", "<u8"), ("covered", "<u8"), ("meth", "<u8"), ("unmeth", "<u8"), ("max_depth", "<u8"),
                            ("level_sum", "<u8"), ("hist", "<u8", (10,))])
levels_dtype = np.dtype([("row", level_row_dtype, (5,)), ("offref", "<u8", (2,))])
LEVEL_ROWS = METH_CONTEXTS + ("CpG_symmetric",)
assert level_row_dtype.itemsize == 128 and levels_dtype.itemsize == 656
# walt_region / walt_region_levels (include/walt_amd.h, "methylation levels per region"); rows as levels_dtype's
region_dtype = np.dtype([("lo", "<u4"), ("hi", "<u4")])
region_row_dtype = np.dtype([("sites", "<u4"), ("covered", "<u4"), ("meth", "<u8"), ("unmeth", "<u8"), ("level_sum", "<u8")])
region_levels_dtype = np.dtype([("row", region_row_dtype, (5,))])
REGIONS_MAX = 1 << 22  # regions of one Pileup.regions_device call at most (WALT_REGIONS_MAX)
assert region_dtype.itemsize == 8 and region_row_dtype.itemsize == 32 and region_levels_dtype.itemsize == 160
# called sites (include/walt_amd.h, "called sites"): the joint histogram of (depth, meth) per context and its bins
SITECALL_DEPTH = 127   # WALT_SITECALL_DEPTH: depths 1 .. 127 are histogrammed, deeper sites are "deep"
SITECALL_BINS = 8255   # WALT_SITECALL_BINS: bins per context


def sitecall_bin(d, m):
    """The bin of a site of depth d (1 .. SITECALL_DEPTH) with m methylated calls (0 .. d)."""
    if not (1 <= d <= SITECALL_DEPTH and 0 <= m <= d):
        raise ValueError("sitecall_bin: depth %r is not 1 to %d, or meth %r is not 0 to the depth" % (d, SITECALL_DEPTH, m))
    return (d - 1) * (d + 2) // 2 + m


# walt_nonconv_tally / walt_nonconv_rule (include/walt_amd.h, "non-converted reads")
nonconv_tally_dtype = np.dtype([("meth", "<u2"), ("total", "<u2"), ("run", "<u2"), ("reserved", "<u2")])
nonconv_rule_dtype = np.dtype([("min_meth", "<u4"), ("min_run", "<u4"), ("min_percent", "<u4"), ("min_total", "<u4")])
assert nonconv_tally_dtype.itemsize == 8 and nonconv_rule_dtype.itemsize == 16
# walt_cpgpair_site: one non-zero entry of a pair table (include/walt_amd.h, "adjacent CpG pairs"); n: MM, MU, UM, UU
cpgpair_site_dtype = np.dtype([("pos", "<u4"), ("next", "<u4"), ("n", "<u4", (4,))])
assert cpgpair_site_dtype.itemsize == 24
# walt_epiallele_site: one entry of a window table (include/walt_amd.h, "four-CpG epialleles"); n: MMMM, MMMU, .. UUUU
epiallele_site_dtype = np.dtype([("pos", "<u4"), ("last", "<u4"), ("n", "<u4", (16,))])
assert epiallele_site_dtype.itemsize == 72
assert meth_counts_dtype.itemsize == 16 and meth_stats_dtype.itemsize == 72
assert best_match_dtype.itemsize == 16 and candidate_dtype.itemsize == 12
assert pair_result_dtype.itemsize == 64 and batch_stats_dtype.itemsize == 32


# status codes of include/walt_amd.h
WALT_OK, WALT_EINVAL, WALT_EIO, WALT_EHIP, WALT_EBASE, WALT_ENOMEM, WALT_EFORMAT = 0, -1, -2, -3, -4, -5, -6


class WaltError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("walt_amd error %d: %s" % (code, msg))
        self.code = code


_libs = {}


def _preload_hip_runtime():
    """One process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own
    libamdhip64 (same SONAME as /opt/rocm's); if libwalt_amd.so pulled in the system
    copy first, a later `import torch` would load a second runtime and find no GPU.
    So when torch is installed, its bundled runtime is loaded first (by path, without
    importing torch) and libwalt_amd.so's NEEDED libamdhip64.so.7 resolves to it.
    WALT_AMD_HIP_RUNTIME=<path> overrides; empty string disables the preload."""
    import importlib.util
    path = os.environ.get("WALT_AMD_HIP_RUNTIME")
    if path is None:
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        if spec is not None and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                path = cand
    if path:
        ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def diag_lib():
    """libwalt_amd_diag.so (make -C walt_amd/csrc diag): the pattern-3 library with the in-kernel phase stamps and
    the WALT_AMD_ABLATE / WALT_AMD_STAMPS / WALT_AMD_SYNC_DEBUG switches, which the product library does not have."""
    return lib("diag")


def lib(pattern=None):
    """Load libwalt_amd.so / its _sp5 / _sp7 variant (fails loudly when it has not been built)."""
    pattern = PATTERN if pattern is None else pattern
    if pattern in _libs:
        return _libs[pattern]
    diag = pattern == "diag"
    path = os.path.join(_HERE, "lib", "libwalt_amd_diag.so") if diag else lib_path(pattern)
    if diag:
        pattern = 3
    if not os.path.exists(path):
        raise ImportError(
            "walt_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the hot path)" % path)
    _preload_hip_runtime()
    L = ctypes.CDLL(path)
    c = ctypes
    vp, u32, u64, ci = c.c_void_p, c.c_uint32, c.c_uint64, c.c_int
    L.walt_last_error.restype = c.c_char_p
    L.walt_device_count.restype = ci
    L.walt_min_read_len.restype = u32
    L.walt_max_read_len.restype = u32
    if L.walt_seed_pattern() != pattern:
        raise ImportError("walt_amd: %s was built for seed pattern %d, not %d" % (path, L.walt_seed_pattern(), pattern))
    L.walt_index_open.argtypes = [c.c_char_p, ci, c.c_uint, ci, c.POINTER(vp)]
    L.walt_index_from_host.argtypes = [u32, vp, vp, vp, vp, vp, vp, ci, ci, c.POINTER(vp)]
    L.walt_index_close.argtypes = [vp]
    L.walt_index_close.restype = None
    L.walt_index_n_chrom.argtypes = [vp]
    L.walt_index_n_chrom.restype = u32
    L.walt_index_chrom_len.argtypes = [vp, u32]
    L.walt_index_chrom_len.restype = u32
    L.walt_index_chrom_name.argtypes = [vp, u32]
    L.walt_index_chrom_name.restype = c.c_char_p
    L.walt_index_genome_len.argtypes = [vp]
    L.walt_index_genome_len.restype = u64
    L.walt_index_device_bytes.argtypes = [vp]
    L.walt_index_device_bytes.restype = u64
    L.walt_index_dir_bits.argtypes = [vp]
    L.walt_index_dir_bits.restype = ci
    L.walt_index_bad_buckets.argtypes = [vp, ci]
    L.walt_index_bad_buckets.restype = u64
    L.walt_index_outliers.argtypes = [vp, ci]
    L.walt_index_outliers.restype = u64
    L.walt_index_window_entries.argtypes = [vp, ci]
    L.walt_index_window_entries.restype = u64
    L.walt_index_window_eligible.argtypes = [vp, ci]
    L.walt_index_window_eligible.restype = u64
    L.walt_map_se_batch.argtypes = [vp, vp, vp, u32, ci, u32, u32, vp, vp]
    L.walt_se_workspace_bytes.argtypes = [u32, u32]
    L.walt_se_workspace_bytes.restype = c.c_size_t
    L.walt_map_se_batch_device.argtypes = [vp, vp, vp, u32, u32, ci, u32, u32, vp, vp, vp, c.c_size_t, vp]
    L.walt_batch_check.argtypes = [vp, vp]
    L.walt_se_rpbat_workspace_bytes.argtypes = [u32, u32]
    L.walt_se_rpbat_workspace_bytes.restype = c.c_size_t
    L.walt_map_se_rpbat_batch.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.walt_map_se_rpbat_batch_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, c.c_size_t, vp]
    L.walt_map_pe_batch.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, ci, vp, vp, vp, vp, vp, vp]
    L.walt_pe_workspace_bytes.argtypes = [u32, u32, u32]
    L.walt_pe_workspace_bytes.restype = c.c_size_t
    L.walt_pe_workspace_bytes_best.argtypes = [vp, u32, u32, u32]
    L.walt_pe_workspace_bytes_best.restype = c.c_size_t
    L.walt_map_pe_batch_device.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, u32, ci, vp, vp, vp, c.c_size_t, vp]
    L.walt_pe_rpbat_workspace_bytes.argtypes = [u32, u32, u32]
    L.walt_pe_rpbat_workspace_bytes.restype = c.c_size_t
    L.walt_pe_rpbat_workspace_bytes_best.argtypes = [vp, u32, u32, u32]
    L.walt_pe_rpbat_workspace_bytes_best.restype = c.c_size_t
    L.walt_map_pe_rpbat_batch.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, ci, vp, vp, vp]
    L.walt_map_pe_rpbat_batch_device.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, u32, ci, vp, vp, vp, vp,
                                                 c.c_size_t, vp]
    L.walt_index_enable_reference.argtypes = [vp]
    L.walt_index_has_reference.argtypes = [vp]
    L.walt_meth_call_batch.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp]
    L.walt_meth_call_batch_device.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp]
    L.walt_pileup_create.argtypes = [vp, c.POINTER(vp)]
    L.walt_pileup_destroy.argtypes = [vp]
    L.walt_pileup_destroy.restype = None
    L.walt_pileup_clear.argtypes = [vp]
    L.walt_pileup_device_bytes.argtypes = [vp]
    L.walt_pileup_device_bytes.restype = u64
    L.walt_meth_pileup_batch.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp]
    L.walt_meth_pileup_batch_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp]
    L.walt_pileup_extract.argtypes = [vp, u32, u32, vp, u64, c.POINTER(u64), vp]
    L.walt_pileup_extract_device.argtypes = [vp, u32, u32, vp, u64, vp, vp, vp]
    L.walt_pileup_levels.argtypes = [vp, u32, u32, vp]
    L.walt_pileup_levels_device.argtypes = [vp, u32, u32, vp, vp]
    L.walt_pileup_depth_hist.argtypes = [vp, u32, u32, vp, vp]
    L.walt_pileup_depth_hist_device.argtypes = [vp, u32, u32, vp, vp, vp]
    L.walt_pileup_call_sites.argtypes = [vp, u32, u32, vp, vp, u64, c.POINTER(u64)]
    L.walt_pileup_call_sites_device.argtypes = [vp, u32, u32, vp, vp, u64, vp, vp]
    L.walt_pileup_read.argtypes = [vp, u32, u32, vp, vp]
    L.walt_pileup_add.argtypes = [vp, u32, u32, vp, vp]
    L.walt_pileup_regions_workspace_bytes.argtypes = [u32]
    L.walt_pileup_regions_workspace_bytes.restype = u64
    L.walt_pileup_regions.argtypes = [vp, vp, u64, vp]
    L.walt_pileup_regions_device.argtypes = [vp, vp, u32, vp, vp, vp]
    L.walt_dedup_create.argtypes = [ci, u64, c.POINTER(vp)]
    L.walt_dedup_destroy.argtypes = [vp]
    L.walt_dedup_destroy.restype = None
    L.walt_dedup_clear.argtypes = [vp]
    L.walt_dedup_reserve.argtypes = [vp, u64]
    L.walt_dedup_count.argtypes = [vp, c.POINTER(u64), c.POINTER(u64)]
    L.walt_dedup_device_bytes.argtypes = [vp]
    L.walt_dedup_device_bytes.restype = u64
    L.walt_dedup_batch.argtypes = [vp, vp, c.c_size_t, vp, c.c_size_t, ci, ci, u32, vp]
    L.walt_dedup_pairs_batch.argtypes = [vp, vp, vp, ci, u32, vp]
    L.walt_dedup_batch_device.argtypes = [vp, vp, c.c_size_t, vp, c.c_size_t, ci, ci, u32, vp, vp]
    L.walt_dedup_pairs_batch_device.argtypes = [vp, vp, vp, ci, u32, vp, vp]
    L.walt_meth_pileup_batch_skip.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp,
                                              c.c_size_t]
    L.walt_meth_pileup_batch_skip_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                     vp, c.c_size_t, vp]
    L.walt_pair_overlap_batch.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.walt_pair_overlap_batch_device.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.walt_meth_pileup_batch_excl.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp,
                                              c.c_size_t, vp]
    L.walt_meth_pileup_batch_excl_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                     vp, c.c_size_t, vp, vp]
    L.walt_mbias_create.argtypes = [ci, u32, c.POINTER(vp)]
    L.walt_mbias_destroy.argtypes = [vp]
    L.walt_mbias_destroy.restype = None
    L.walt_mbias_clear.argtypes = [vp]
    L.walt_mbias_device_bytes.argtypes = [vp]
    L.walt_mbias_device_bytes.restype = u64
    L.walt_mbias_read.argtypes = [vp, u32, vp]
    L.walt_mbias_batch.argtypes = [vp, u32, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t]
    L.walt_mbias_batch_device.argtypes = [vp, u32, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, vp]
    L.walt_meth_pileup_batch_mbias.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp,
                                               c.c_size_t, vp, vp, u32]
    L.walt_meth_pileup_batch_mbias_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                      vp, c.c_size_t, vp, vp, u32, vp]
    L.walt_meth_pileup_batch_trim.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp,
                                              c.c_size_t, vp, vp, u32, u32, u32]
    L.walt_meth_pileup_batch_trim_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                     vp, c.c_size_t, vp, vp, u32, u32, u32, vp]
    L.walt_pair_overlap_batch_trim.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, u32, u32, u32]
    L.walt_pair_overlap_batch_trim_device.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, u32, u32, u32, vp]
    L.walt_nonconv_batch.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, vp, c.c_size_t, vp]
    L.walt_nonconv_batch_device.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, vp, c.c_size_t, vp, vp]
    L.walt_meth_nonconv_batch.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, c.c_size_t, vp]
    L.walt_meth_nonconv_batch_device.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, c.c_size_t,
                                                 vp, vp]
    L.walt_nonconv_pairs_batch.argtypes = [vp, vp, u32, vp]
    L.walt_nonconv_pairs_batch_device.argtypes = [vp, vp, u32, vp, vp]
    L.walt_cpgpairs_create.argtypes = [vp, c.POINTER(vp)]
    L.walt_cpgpairs_destroy.argtypes = [vp]
    L.walt_cpgpairs_destroy.restype = None
    L.walt_cpgpairs_clear.argtypes = [vp]
    L.walt_cpgpairs_device_bytes.argtypes = [vp]
    L.walt_cpgpairs_device_bytes.restype = u64
    L.walt_cpgpairs_n_pairs.argtypes = [vp]
    L.walt_cpgpairs_n_pairs.restype = u64
    L.walt_cpgpairs_batch.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t]
    L.walt_cpgpairs_batch_device.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, vp]
    L.walt_cpgpairs_extract.argtypes = [vp, u32, u32, vp, u64, c.POINTER(u64)]
    L.walt_cpgpairs_extract_device.argtypes = [vp, u32, u32, vp, u64, vp, vp]
    L.walt_meth_pileup_batch_pairs.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp,
                                               c.c_size_t, vp, vp, u32, u32, u32, vp]
    L.walt_meth_pileup_batch_pairs_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                      vp, c.c_size_t, vp, vp, u32, u32, u32, vp, vp]
    L.walt_epialleles_create.argtypes = [vp, c.POINTER(vp)]
    L.walt_epialleles_destroy.argtypes = [vp]
    L.walt_epialleles_destroy.restype = None
    L.walt_epialleles_clear.argtypes = [vp]
    L.walt_epialleles_device_bytes.argtypes = [vp]
    L.walt_epialleles_device_bytes.restype = u64
    L.walt_epialleles_n_pairs.argtypes = [vp]
    L.walt_epialleles_n_pairs.restype = u64
    L.walt_epialleles_batch.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t]
    L.walt_epialleles_batch_device.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, vp]
    L.walt_epialleles_extract.argtypes = [vp, u32, u32, u64, vp, u64, c.POINTER(u64)]
    L.walt_epialleles_extract_device.argtypes = [vp, u32, u32, u64, vp, u64, vp, vp]
    L.walt_meth_pileup_batch_epi.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp,
                                             c.c_size_t, vp, vp, u32, u32, u32, vp, vp]
    L.walt_meth_pileup_batch_epi_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                    vp, c.c_size_t, vp, vp, u32, u32, u32, vp, vp, vp]
    L.walt_meth_evidence_batch.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, c.c_size_t]
    L.walt_meth_evidence_batch_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, c.c_size_t, vp]
    L.walt_meth_pileup_batch_ev.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp,
                                            c.c_size_t, vp, vp, u32, u32, u32, vp, vp, vp]
    L.walt_meth_pileup_batch_ev_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                   vp, c.c_size_t, vp, vp, u32, u32, u32, vp, vp, vp, vp]
    L.walt_meth_pileup_batch_qual.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, vp,
                                              c.c_size_t, vp, vp, u32, u32, u32, vp, vp, vp, vp, u32]
    L.walt_meth_pileup_batch_qual_device.argtypes = [vp, vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                     vp, c.c_size_t, vp, vp, u32, u32, u32, vp, vp, vp, vp, u32, vp]
    L.walt_meth_nonconv_batch_qual.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp, c.c_size_t, vp,
                                               vp, u32]
    L.walt_meth_nonconv_batch_qual_device.argtypes = [vp, vp, vp, u32, vp, c.c_size_t, vp, c.c_size_t, ci, vp, vp, vp, vp,
                                                      c.c_size_t, vp, vp, u32, vp]
    L.walt_pileup_variants.argtypes = [vp, vp, u32, u32, u32, u32, vp, u64, c.POINTER(u64)]
    L.walt_pileup_variants_device.argtypes = [vp, vp, u32, u32, u32, u32, vp, u64, vp, vp]
    L.walt_pileup_mask_variants.argtypes = [vp, vp, u32, u32, u32, u32, vp]
    L.walt_pileup_mask_variants_device.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp]
    L.walt_index_set_option.argtypes = [vp, c.c_char_p, c.c_longlong]
    L.walt_index_get_option.argtypes = [vp, c.c_char_p, c.POINTER(c.c_longlong)]
    L.walt_makedb.argtypes = [c.c_char_p, c.c_char_p, ci]
    L.walt_index_build_device.argtypes = [vp, u32, vp, vp, ci, c.c_uint, ci, c.POINTER(vp)]
    L.walt_index_size.argtypes = [vp, ci]
    L.walt_index_size.restype = u32
    L.walt_index_export_strand.argtypes = [vp, ci, vp, vp, vp]
    L.walt_index_write.argtypes = [vp, c.c_char_p]
    L.walt_profile_enable.argtypes = [vp, ci]
    L.walt_profile_last.argtypes = [vp, c.POINTER(c.c_float), c.POINTER(c.c_float)]
    L.walt_profile_detail.argtypes = [vp, c.POINTER(c.c_float)]
    L.walt_comm_available.argtypes = []
    L.walt_comm_unique_id.argtypes = [vp]
    L.walt_comm_init.argtypes = [ci, ci, ci, vp, c.POINTER(vp)]
    L.walt_stats_allreduce.argtypes = [vp, vp, c.c_size_t]
    L.walt_comm_rank.argtypes = [vp]
    L.walt_comm_world.argtypes = [vp]
    L.walt_comm_close.argtypes = [vp]
    L.walt_comm_close.restype = None
    _libs["diag" if diag else pattern] = L
    return L


def _check(rc):
    if rc != WALT_OK:
        raise WaltError(rc, lib().walt_last_error().decode("utf-8", "replace"))


def device_count():
    return lib().walt_device_count()


def makedb(fasta_path, out_dbindex_path, threads=1):
    """makedb -c <fasta_path> -o <out_dbindex_path> (makedb.cpp:128-159)."""
    _check(lib().walt_makedb(os.fsencode(fasta_path), os.fsencode(out_dbindex_path), int(threads)))


def _ptr(a):
    return None if a is None else a.ctypes.data


# What the methylation-side calls take: a 1-d array or strided view with n elements, read in place.  Each helper returns
# (the array to keep alive, its address or None when n == 0, its stride in bytes).
def _records_arg(records, n=None):
    records = np.asarray(records)
    if records.dtype != best_match_dtype or records.ndim != 1 or (n is not None and records.shape[0] != n):
        raise ValueError("records: a 1-d best_match_dtype array (or view)" + (" with one element per read" if n is not None else ""))
    n = records.shape[0]
    stride = records.strides[0] if n > 1 else best_match_dtype.itemsize
    if stride < 0:
        records, stride = np.ascontiguousarray(records), best_match_dtype.itemsize
    return records, records.ctypes.data if n else None, stride


def _bytes_arg(a, n, error):
    """conv or skip: uint8, any positive stride"""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 1 or a.shape[0] != n:
        raise ValueError(error)
    stride = a.strides[0] if n > 1 else 1
    if stride <= 0:
        a, stride = np.ascontiguousarray(a), 1
    return a, a.ctypes.data if n else None, stride


def _conv_arg(conv, n, per="read"):
    """'T' / 'A' for the whole batch, or one byte per read -> (array to keep alive, address, stride, conversion)"""
    if isinstance(conv, (str, bytes)):
        return None, None, 0, ord(conv)
    return _bytes_arg(conv, n, "conv: 'T', 'A' or a 1-d uint8 array with one element per %s" % per) + (0,)


def _skip_arg(skip, n):
    if skip is None:
        return None, None, 1
    return _bytes_arg(skip, n, "skip: a 1-d uint8 array with one element per read")


def _trim_arg(trim5, trim3):
    """the ignored read ends of a call -> (trim5, trim3) when one is non-zero, else None; any uint32 value is legal"""
    trim5, trim3 = int(trim5), int(trim3)
    if not (0 <= trim5 < 1 << 32 and 0 <= trim3 < 1 << 32):
        raise ValueError("trim5, trim3: 0 .. 2^32 - 1")
    return (trim5, trim3) if trim5 or trim3 else None


def nonconv_rule(min_meth=0, min_run=0, min_percent=0, min_total=0):
    """A walt_nonconv_rule (include/walt_amd.h, "non-converted reads") as a 1-element nonconv_rule_dtype array: a read
    fails with min_meth or more methylated non-CpG calls, with a run of min_run or more of them, or with min_percent
    percent or more of its non-CpG calls methylated when it has at least max(min_total, 1); 0 switches a test off.  Any
    uint32 is taken here: the library refuses min_percent above 100."""
    r = np.zeros(1, dtype=nonconv_rule_dtype)
    for name, v in (("min_meth", min_meth), ("min_run", min_run), ("min_percent", min_percent), ("min_total", min_total)):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError("%s: 0 .. 2^32 - 1" % name)
        r[name] = int(v)
    return r


def _rule_arg(rule):
    rule = np.ascontiguousarray(rule, dtype=nonconv_rule_dtype)
    if rule.size != 1:
        raise ValueError("rule: one nonconv_rule_dtype element (walt_amd.nonconv_rule(...))")
    return rule


def _meth_form(L, device, pile, skip=None, excl=None, mbias=None, skip_alone="skip", trim=None, pairs=None, epi=None, ev=None,
               qual=None):
    """The C form of a methylation call, by what the call is composed with: pile (a handle or None), skip = (address,
    stride), excl = (address,), mbias = (handle, table), trim = (trim5, trim3), pairs = (handle,), epi = (handle,), ev = (handle,),
    qual = (address, min_qual), each None when the caller gave none.  The
    narrowest form that takes them all is the one called -- its name is what a refusal shows; skip_alone: the form of a
    call with skip only.  Returns (the function, its arguments between the index and bases, its arguments behind stats)."""
    widest = "qual" if qual else "ev" if ev else "epi" if epi else "pairs" if pairs else "trim" if trim else "mbias" if mbias else "excl" if excl else skip_alone if skip else None
    if widest is None:
        name, head, tail = ("walt_meth_pileup_batch", (pile,), ()) if pile is not None else ("walt_meth_call_batch", (), ())
    else:  # (these three take a null pile-up, a null skip and a null excl)
        name, head, tail = "walt_meth_pileup_batch_" + widest, (pile,), skip or (None, 1)
        if widest != "skip":
            tail += excl or (None,)
        if widest in ("mbias", "trim", "pairs", "epi", "ev", "qual"):
            tail += mbias or (None, 0)
        if widest in ("trim", "pairs", "epi", "ev", "qual"):
            tail += trim or (0, 0)
        if widest in ("pairs", "epi", "ev", "qual"):
            tail += pairs or (None,)
        if widest in ("epi", "ev", "qual"):
            tail += epi or (None,)
        if widest in ("ev", "qual"):
            tail += ev or (None,)
        if widest == "qual":
            tail += qual
    return getattr(L, name + ("_device" if device else "")), head, tail


def pack_reads(seqs):
    """list of str/bytes -> (bases uint8[total], offsets uint64[n+1])."""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offsets[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    bases = np.frombuffer(b"".join(bs), dtype=np.uint8).copy() if bs else np.zeros(0, dtype=np.uint8)
    return bases, offsets


def pack_quals(quals):
    """list of str/bytes, the quality lines of the reads given to pack_reads in the same order -> quals uint8[total]: one
    raw byte per base at the offsets pack_reads returns (include/walt_amd.h, "minimum base quality")."""
    bs = [q.encode("latin-1") if isinstance(q, str) else bytes(q) for q in quals]
    return np.frombuffer(b"".join(bs), dtype=np.uint8).copy() if bs else np.zeros(0, dtype=np.uint8)


def se_rpbat_workspace_bytes(n, max_read_len):
    """Bytes of the workspace Index.map_se_rpbat_batch_device needs (walt_se_rpbat_workspace_bytes)."""
    return lib().walt_se_rpbat_workspace_bytes(int(n), int(max_read_len))


def regions_workspace_bytes(n):
    """Bytes of the workspace Pileup.regions_device needs for n regions (walt_pileup_regions_workspace_bytes)."""
    return lib().walt_pileup_regions_workspace_bytes(int(n))


def pe_rpbat_workspace_bytes(n, max_read_len, top_k):
    """Least bytes of the workspace Index.map_pe_rpbat_batch_device needs (walt_pe_rpbat_workspace_bytes)."""
    return lib().walt_pe_rpbat_workspace_bytes(int(n), int(max_read_len), int(top_k))


COMM_ID_BYTES = 128


def comm_available():
    """True when librccl loads in this process (walt_comm_available; no communication)."""
    return lib().walt_comm_available() == 0


def comm_unique_id():
    """128-byte RCCL id made by rank 0 (ncclGetUniqueId); the caller hands it to the other ranks."""
    buf = (ctypes.c_ubyte * COMM_ID_BYTES)()
    _check(lib().walt_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
    return bytes(buf)


class Comm:
    """RCCL communicator of the one-process-per-GPU path; its only use is stats_allreduce()."""

    def __init__(self, device, rank, world, unique_id):
        self._L = lib()
        h = ctypes.c_void_p()
        buf = (ctypes.c_ubyte * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _check(self._L.walt_comm_init(int(device), int(rank), int(world), ctypes.cast(buf, ctypes.c_void_p),
                                      ctypes.byref(h)))
        self._h = h

    def stats_allreduce(self, vec):
        """Sum a vector of counters over the ranks (walt_stats_allreduce); returns a numpy uint64 array."""
        v = np.ascontiguousarray(np.asarray(vec), dtype=np.uint64).copy()
        _check(self._L.walt_stats_allreduce(self._h, v.ctypes.data, v.size))
        return v

    @property
    def rank(self):
        return self._L.walt_comm_rank(self._h)

    @property
    def world(self):
        return self._L.walt_comm_world(self._h)

    def close(self):
        if self._h:
            self._L.walt_comm_close(self._h)
            self._h = None


def _keyword_only_epi(plain):
    """Index.meth_call_batch with one more, keyword-only argument epi=.  The argument cannot stand in the method's own
    parameter list: a keyword-only parameter is listed behind every other, and the end of that list is pinned
    (tests/test_nonconv_cpu.py), so inspect.signature goes on showing the list as it was.  plain's parameters are
    Index._meth_batch's by name."""
    signature = inspect.signature(plain)

    @functools.wraps(plain)
    def call(self, *args, epi=None, **kw):
        if epi is None:
            return plain(self, *args, **kw)
        bound = signature.bind(self, *args, **kw)
        bound.apply_defaults()
        named = dict(bound.arguments)
        del named["self"]
        return self._meth_batch(None, epi=epi, **named)

    return call


def _keyword_only_evidence(plain):
    """Pileup.add_batch[_device] with one more, keyword-only argument evidence=, in the way _keyword_only_epi adds epi=: the
    end of their parameter lists is pinned too (tests/test_epialleles_cpu.py), so inspect.signature goes on showing the
    lists as they were.  The method "_" + plain's name takes the evidence object's handle in front of plain's parameters."""
    signature = inspect.signature(plain)

    @functools.wraps(plain)
    def call(self, *args, evidence=None, **kw):
        if evidence is None:
            return plain(self, *args, **kw)
        bound = signature.bind(self, *args, **kw)
        bound.apply_defaults()
        named = dict(bound.arguments)
        del named["self"]
        return getattr(self, "_" + plain.__name__)(evidence.handle, **named)

    return call


# The base qualities of the call in progress on this thread, (quals, min_qual), or None: set by _keyword_only_quals, read
# where the C call is composed (Index._qual_arg).
_qual_call = threading.local()


def _keyword_only_quals(plain):
    """A methylation call with two more, keyword-only arguments quals=None, min_qual=0 (include/walt_amd.h, "minimum base
    quality"), in the way _keyword_only_epi adds epi=: the parameter lists are pinned, so inspect.signature goes on
    showing them as they were.  quals: a uint8 array with offsets[n] elements (walt_amd.pack_quals), or for a device form
    the address of one; min_qual: 0 .. 127, compared with the raw byte.  Without the two the call is the old one."""

    @functools.wraps(plain)
    def call(self, *args, quals=None, min_qual=0, **kw):
        if quals is None and not min_qual:
            return plain(self, *args, **kw)
        if getattr(_qual_call, "now", None) is not None:
            raise RuntimeError("a methylation call with quals= inside another")
        _qual_call.now = (quals, int(min_qual))
        try:
            return plain(self, *args, **kw)
        finally:
            _qual_call.now = None

    return call


def _qual_arg(total=None, first=0):
    """The (address, min_qual) of the call in progress, or None without quals= / min_qual=.  total: a host form's
    offsets[n] (the array's length is checked; first = offsets[0] .. total are the bytes read); None: a device form, quals an address.
    -> (array to keep alive, (address or None, min_qual))"""
    now = getattr(_qual_call, "now", None)
    if now is None:
        return None, None
    quals, min_qual = now
    if not 0 <= min_qual < 1 << 32:
        raise ValueError("min_qual: 0 .. 127")
    if quals is None or total is None:
        return None, (quals, min_qual)
    arr = np.ascontiguousarray(quals)
    if arr.dtype != np.uint8 or arr.ndim != 1 or arr.shape[0] != total:
        raise ValueError("quals: a 1-d uint8 array with offsets[n] = %d elements, one per base (walt_amd.pack_quals)" % total)
    return arr, (arr.ctypes.data, min_qual)


class Index:
    """Device-resident index (all selected strands stay in HBM)."""

    def __init__(self, handle, L=None):
        self._h = handle
        self._L = L if L is not None else lib()

    def _ck(self, rc):
        if rc != WALT_OK:
            raise WaltError(rc, self._L.walt_last_error().decode("utf-8", "replace"))

    @classmethod
    def open(cls, dbindex_path, device=0, strands=STRANDS_ALL, dir_bits=-1):
        h = ctypes.c_void_p()
        _check(lib().walt_index_open(os.fsencode(dbindex_path), int(device), int(strands), int(dir_bits),
                                     ctypes.byref(h)))
        return cls(h, lib())

    @classmethod
    def from_host(cls, chrom_len, genome, counter, index, chrom_names=None, device=0, dir_bits=-1, diag=False):
        """genome/counter/index: 4-lists (CT00, CT01, GA10, GA11) of numpy arrays or None.
        diag: through the diagnostic build of the library (diag_lib)."""
        n = len(chrom_len)
        cl = np.ascontiguousarray(chrom_len, dtype=np.uint32)
        names = None
        keep = []
        if chrom_names is not None:
            arr = (ctypes.c_char_p * n)(*[os.fsencode(x) for x in chrom_names])
            names = ctypes.cast(arr, ctypes.c_void_p)
            keep.append(arr)
        g = (ctypes.c_void_p * 4)()
        cn = (ctypes.c_void_p * 4)()
        ix = (ctypes.c_void_p * 4)()
        sz = (ctypes.c_uint32 * 4)()
        for s in range(4):
            if genome[s] is None:
                continue
            ga = np.ascontiguousarray(genome[s], dtype=np.uint8)
            ca = np.ascontiguousarray(counter[s], dtype=np.uint32)
            ia = np.ascontiguousarray(index[s], dtype=np.uint32)
            keep += [ga, ca, ia]
            g[s], cn[s], ix[s], sz[s] = ga.ctypes.data, ca.ctypes.data, ia.ctypes.data, ia.size
        h = ctypes.c_void_p()
        L = diag_lib() if diag else lib()
        rc = L.walt_index_from_host(n, cl.ctypes.data, names, ctypes.cast(g, ctypes.c_void_p),
                                    ctypes.cast(cn, ctypes.c_void_p), ctypes.cast(ix, ctypes.c_void_p),
                                    ctypes.cast(sz, ctypes.c_void_p), int(device), int(dir_bits), ctypes.byref(h))
        if rc != WALT_OK:
            raise WaltError(rc, L.walt_last_error().decode("utf-8", "replace"))
        return cls(h, L)

    @classmethod
    def build_device(cls, d_genome_ascii, chrom_len, chrom_names=None, device=0, strands=STRANDS_ALL,
                     dir_bits=-1):
        """GPU makedb: d_genome_ascii is an HBM address of the ACGT genome (makedb.cpp:46-85)."""
        n = len(chrom_len)
        cl = np.ascontiguousarray(chrom_len, dtype=np.uint32)
        names = None
        if chrom_names is not None:
            arr = (ctypes.c_char_p * n)(*[os.fsencode(x) for x in chrom_names])
            names = ctypes.cast(arr, ctypes.c_void_p)
        h = ctypes.c_void_p()
        _check(lib().walt_index_build_device(d_genome_ascii, n, cl.ctypes.data, names, int(device), int(strands),
                                             int(dir_bits), ctypes.byref(h)))
        return cls(h, lib())

    def index_size(self, strand):
        return self._L.walt_index_size(self._h, strand)

    def export_strand(self, strand, want_genome=True):
        """(genome bytes, counter, index) numpy arrays of a resident strand (reference.cpp:302-322 layout)."""
        g = np.empty(self.genome_len, dtype=np.uint8) if want_genome else None
        cnt = np.empty((1 << 24) + 1, dtype=np.uint32)
        ix = np.empty(self.index_size(strand), dtype=np.uint32)
        self._ck(self._L.walt_index_export_strand(self._h, strand, _ptr(g), _ptr(cnt), _ptr(ix)))
        return g, cnt, ix

    def write(self, dbindex_path):
        self._ck(self._L.walt_index_write(self._h, os.fsencode(dbindex_path)))

    def profile_enable(self, on=True):
        self._ck(self._L.walt_profile_enable(self._h, int(on)))

    def profile_last(self):
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        self._ck(self._L.walt_profile_last(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def profile_detail(self):
        """ms of the last single-end call by kernel group: pass 1, heavy stages, region verifier, literal pass"""
        buf = (ctypes.c_float * 4)()
        self._ck(self._L.walt_profile_detail(self._h, buf))
        return [float(x) for x in buf]

    def close(self):
        if self._h:
            self._L.walt_index_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def n_chrom(self):
        return self._L.walt_index_n_chrom(self._h)

    @property
    def chrom_lengths(self):
        return [self._L.walt_index_chrom_len(self._h, i) for i in range(self.n_chrom)]

    @property
    def chrom_names(self):
        return [self._L.walt_index_chrom_name(self._h, i).decode() for i in range(self.n_chrom)]

    @property
    def genome_len(self):
        return self._L.walt_index_genome_len(self._h)

    @property
    def device_bytes(self):
        return self._L.walt_index_device_bytes(self._h)

    @property
    def dir_bits(self):
        return self._L.walt_index_dir_bits(self._h)

    def bad_buckets(self, strand):
        return self._L.walt_index_bad_buckets(self._h, strand)

    def outliers(self, strand):
        return self._L.walt_index_outliers(self._h, strand)

    def window_entries(self, strand):
        return self._L.walt_index_window_entries(self._h, strand)

    def window_eligible(self, strand):
        return self._L.walt_index_window_eligible(self._h, strand)

    # -- single-end -----------------------------------------------------------
    def map_se_batch(self, bases, offsets, ag_wildcard=False, max_mismatches=6, b=5000):
        """Host-buffer form.  Returns (best_match[n], stats)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        out = np.zeros(n, dtype=best_match_dtype)
        stats = np.zeros(1, dtype=batch_stats_dtype)
        self._ck(self._L.walt_map_se_batch(self._h, _ptr(bases), _ptr(offsets), n, int(bool(ag_wildcard)),
                                       int(max_mismatches), int(b), _ptr(out), _ptr(stats)))
        return out, stats[0]

    def map_se_batch_device(self, d_bases, d_offsets, n, max_read_len, d_out, d_stats, d_workspace, workspace_bytes,
                            stream=0, ag_wildcard=False, max_mismatches=6, b=5000):
        """Device-pointer form (ints are HBM addresses, stream a hipStream_t value); workspace_bytes = what
        d_workspace holds (at least se_workspace_bytes(n, max_read_len))."""
        self._ck(self._L.walt_map_se_batch_device(self._h, d_bases, d_offsets, int(n), int(max_read_len),
                                              int(bool(ag_wildcard)), int(max_mismatches), int(b), d_out, d_stats,
                                              d_workspace, int(workspace_bytes), stream))

    # -- single-end random PBAT: every read under both conversions (include/walt_amd.h states the rules) ----------
    def map_se_rpbat_batch(self, bases, offsets, max_mismatches=6, b=5000):
        """Host-buffer form.  Returns (best_match[n], conv uint8[n] of ord('T') / ord('A'), stats); the index must
        hold all four strands."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        out = np.zeros(n, dtype=best_match_dtype)
        conv = np.zeros(n, dtype=np.uint8)
        stats = np.zeros(1, dtype=batch_stats_dtype)
        self._ck(self._L.walt_map_se_rpbat_batch(self._h, _ptr(bases), _ptr(offsets), n, int(max_mismatches), int(b),
                                             _ptr(out), _ptr(conv), _ptr(stats)))
        return out, conv, stats[0]

    def map_se_rpbat_batch_device(self, d_bases, d_offsets, n, max_read_len, d_out, d_conv, d_stats, d_workspace,
                                  workspace_bytes, stream=0, max_mismatches=6, b=5000):
        """Device-pointer form (ints are HBM addresses, stream a hipStream_t value); workspace_bytes = what
        d_workspace holds (at least the module's se_rpbat_workspace_bytes(n, max_read_len))."""
        self._ck(self._L.walt_map_se_rpbat_batch_device(self._h, d_bases, d_offsets, int(n), int(max_read_len),
                                                    int(max_mismatches), int(b), d_out, d_conv, d_stats, d_workspace,
                                                    int(workspace_bytes), stream))

    # -- methylation calls (include/walt_amd.h states the rules) -------------------------------------------------
    @property
    def has_reference(self):
        return bool(self._L.walt_index_has_reference(self._h))

    def enable_reference(self):
        """Builds the unconverted reference on an index that holds all four strands (walt_index_enable_reference)."""
        self._ck(self._L.walt_index_enable_reference(self._h))

    @_keyword_only_quals
    @_keyword_only_epi
    def meth_call_batch(self, bases, offsets, records, conv="T", call_len=None, want_calls=True, want_counts=True,
                        stats=None, want_stats=True, pairs=None, skip=None, excl=None, mbias=None, mbias_table=0, trim5=0, trim3=0):
        """Host-buffer form.  records: a best_match_dtype array, or the m1 / m2 field of a pair_result_dtype array (a
        strided view: read in place).  conv: 'T' / 'A' for the whole batch, or a uint8 array of ord('T') / ord('A') per
        read (any stride, e.g. conv[:, 0] of map_pe_rpbat_batch).  Returns (calls uint8[total bases], counts
        meth_counts_dtype[n], stats meth_stats_dtype scalar array); an output that is not wanted is None.  stats: an
        existing 1-element meth_stats_dtype array to accumulate into.  skip: a uint8 array with one element per read
        (any stride, e.g. dup[:, 0] of Dedup.add_pairs): a read with a non-zero byte is called but left out of stats.
        excl: a uint32 array with one word per read, as Index.pair_overlap returns it: the read positions
        [excl & 0xFFFF, excl >> 16) get no call (walt_meth_pileup_batch_excl; only when given).  mbias: an MBias set on
        this index's device; the calls of the batch are added to its table mbias_table under the same skip
        (walt_meth_pileup_batch_mbias; only when given; want_calls may be False).  trim5 / trim3: the first trim5 read
        positions and the last trim3 before the clip point get no call (include/walt_amd.h, "ignored read ends":
        walt_meth_pileup_batch_trim; only when one is non-zero).  pairs: a CpgPairs table of this index; the calls of the
        batch are folded into it under the same skip (walt_meth_pileup_batch_pairs; only when given; want_calls may be
        False).  epi (keyword only): an Epialleles table of this index, likewise (walt_meth_pileup_batch_epi).  quals,
        min_qual (keyword only): one quality byte per base (walt_amd.pack_quals) and the floor below which a base gets no
        call (include/walt_amd.h, "minimum base quality": walt_meth_pileup_batch_qual; only when given)."""
        return self._meth_batch(None, bases, offsets, records, conv, call_len, want_calls, want_counts, stats, want_stats,
                                skip, excl, mbias, mbias_table, trim5, trim3, pairs)

    # -- non-converted reads (include/walt_amd.h states the rules) ------------------------------------------------
    def nonconv_batch(self, calls, offsets, records, rule, want_tally=True):
        """Host-buffer form of walt_nonconv_batch.  calls: the uint8 array Index.meth_call_batch returned (indexed from
        offsets[0]); records: a best_match_dtype array or strided view; rule: walt_amd.nonconv_rule(...).  Returns (filt
        uint8[n]: 1 for a read the rule fails, tally nonconv_tally_dtype[n] or None).  Waits for the result."""
        calls = np.ascontiguousarray(calls, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        rule = _rule_arg(rule)
        n = offsets.size - 1
        records, rec_ptr, rec_stride = _records_arg(records, n)
        filt = np.zeros(n, dtype=np.uint8)
        tally = np.zeros(n, dtype=nonconv_tally_dtype) if want_tally else None
        calls_ptr = calls.ctypes.data - int(offsets[0]) if n else None
        self._ck(self._L.walt_nonconv_batch(self._h, calls_ptr, _ptr(offsets), n, rec_ptr, rec_stride, _ptr(rule),
                                            _ptr(filt) if n else None, 1, _ptr(tally) if n else None))
        return filt, tally

    def nonconv_batch_device(self, d_calls, d_offsets, n, d_records, rule, d_filt, record_stride=16, filt_stride=1, d_tally=None,
                             stream=0):
        """Device-pointer form (ints are HBM addresses on this index's device, stream a hipStream_t value); asynchronous."""
        rule = _rule_arg(rule)
        self._ck(self._L.walt_nonconv_batch_device(self._h, d_calls, d_offsets, int(n), d_records, int(record_stride), _ptr(rule),
                                                   d_filt, int(filt_stride), d_tally, stream))

    def nonconv_pairs(self, pairs, filt):
        """The pair rule in place (walt_nonconv_pairs_batch).  pairs: a pair_result_dtype array; filt: a contiguous uint8
        array of 2 n bytes (shape [2n] or [n, 2]), mate k + 1 of pair i at 2 i + k.  Returns filt."""
        pairs = np.ascontiguousarray(pairs, dtype=pair_result_dtype)
        n = pairs.size
        if not isinstance(filt, np.ndarray) or filt.dtype != np.uint8 or filt.size != 2 * n or not filt.flags.c_contiguous:
            raise ValueError("filt: a contiguous uint8 array with two bytes per pair")
        self._ck(self._L.walt_nonconv_pairs_batch(self._h, _ptr(pairs) if n else None, n, _ptr(filt) if n else None))
        return filt

    def nonconv_pairs_device(self, d_pairs, n, d_filt, stream=0):
        """Device-pointer form of the pair rule; asynchronous."""
        self._ck(self._L.walt_nonconv_pairs_batch_device(self._h, d_pairs, int(n), d_filt, stream))

    @_keyword_only_quals
    def meth_nonconv_batch(self, bases, offsets, records, rule, conv="T", call_len=None, want_calls=False, want_tally=True):
        """Calls and judges in one step (walt_meth_nonconv_batch): the arguments of meth_call_batch plus the rule.  Returns
        (filt uint8[n], tally nonconv_tally_dtype[n] or None, calls uint8[total bases] or None).  quals, min_qual (keyword
        only): as in meth_call_batch; the verdict is made from the masked calls (walt_meth_nonconv_batch_qual)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        rule = _rule_arg(rule)
        n = offsets.size - 1
        records, rec_ptr, rec_stride = _records_arg(records, n)
        conv_arr, conv_ptr, conv_stride, conversion = _conv_arg(conv, n)
        cl = None if call_len is None else np.ascontiguousarray(call_len, dtype=np.uint32)
        if cl is not None and cl.size != n:
            raise ValueError("call_len: one element per read")
        total = int(offsets[n] - offsets[0]) if n else 0
        calls = np.zeros(total, dtype=np.uint8) if want_calls else None
        calls_ptr = None if calls is None else calls.ctypes.data - int(offsets[0]) if n else calls.ctypes.data
        filt = np.zeros(n, dtype=np.uint8)
        tally = np.zeros(n, dtype=nonconv_tally_dtype) if want_tally else None
        quals_arr, qual = _qual_arg(int(offsets[n]) if n else 0)
        form = self._L.walt_meth_nonconv_batch_qual if qual else self._L.walt_meth_nonconv_batch
        self._ck(form(self._h, bases.ctypes.data, _ptr(offsets), n, rec_ptr, rec_stride, conv_ptr, conv_stride, conversion,
                      _ptr(cl), calls_ptr, _ptr(rule), _ptr(filt) if n else None, 1, _ptr(tally) if n else None, *(qual or ())))
        return filt, tally, calls

    @_keyword_only_quals
    def meth_nonconv_batch_device(self, d_bases, d_offsets, n, d_records, rule, d_calls, d_filt, record_stride=16, d_conv=None,
                                  conv_stride=1, conversion="T", d_call_len=None, filt_stride=1, d_tally=None, stream=0):
        """Device-pointer form: the calling kernel, then the judging kernel on the calls it wrote, on `stream`; d_calls
        must be given.  quals, min_qual (keyword only): the address of the device array of quality bytes and the floor
        (walt_meth_nonconv_batch_qual_device; only when given)."""
        rule = _rule_arg(rule)
        _, qual = _qual_arg()  # (quals: the address of the device array)
        form = self._L.walt_meth_nonconv_batch_qual_device if qual else self._L.walt_meth_nonconv_batch_device
        self._ck(form(self._h, d_bases, d_offsets, int(n), d_records, int(record_stride), d_conv, int(conv_stride),
                      ord(conversion), d_call_len, d_calls, _ptr(rule), d_filt, int(filt_stride), d_tally, *(qual or ()), stream))

    # -- overlap of a pair (include/walt_amd.h states the rules) --------------------------------------------------
    def pair_overlap(self, pairs, offsets1, offsets2, call_len1=None, call_len2=None, trim1=(0, 0), trim2=(0, 0)):
        """Host-buffer form of walt_pair_overlap_batch.  pairs: a pair_result_dtype array; offsets1 / offsets2: the two
        mates' offsets (n + 1 each).  Returns (excl uint32[n]: per pair the read positions of mate 2 that mate 1 already
        calls, ex_lo | ex_hi << 16, 0 for none; totals uint64[2]: pairs with a non-empty interval, mate-2 bases
        excluded).  trim1 / trim2: (trim5, trim3) of mate 1 / mate 2, the ignored read ends their calling calls get
        (walt_pair_overlap_batch_trim; only when one is non-zero)."""
        trim = (_trim_arg(*trim1) or (0, 0)) + (_trim_arg(*trim2) or (0, 0))
        pairs = np.ascontiguousarray(pairs, dtype=pair_result_dtype)
        offsets1 = np.ascontiguousarray(offsets1, dtype=np.uint64)
        offsets2 = np.ascontiguousarray(offsets2, dtype=np.uint64)
        n = pairs.size
        if pairs.ndim != 1 or offsets1.size != n + 1 or offsets2.size != n + 1:
            raise ValueError("pairs: a 1-d pair_result_dtype array; offsets1 and offsets2: one more element than pairs")
        cl = []
        for a in (call_len1, call_len2):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
            if a is not None and a.size != n:
                raise ValueError("call_len: one element per pair")
            cl.append(a)
        excl = np.zeros(n, dtype=np.uint32)
        totals = np.zeros(2, dtype=np.uint64)
        form, tail = (self._L.walt_pair_overlap_batch_trim, trim) if any(trim) else (self._L.walt_pair_overlap_batch, ())
        self._ck(form(self._h, _ptr(pairs) if n else None, _ptr(offsets1), _ptr(offsets2), n,
                      _ptr(cl[0]) if n else None, _ptr(cl[1]) if n else None, _ptr(excl) if n else None, _ptr(totals), *tail))
        return excl, totals

    def pair_overlap_device(self, d_pairs, d_offsets1, d_offsets2, n, d_excl, d_call_len1=None, d_call_len2=None,
                            d_totals=None, stream=0, trim1=(0, 0), trim2=(0, 0)):
        """Device-pointer form (ints are HBM addresses, stream a hipStream_t value); asynchronous.  d_totals
        (uint64[2]) is accumulated into, not cleared.  trim1 / trim2: as in pair_overlap
        (walt_pair_overlap_batch_trim_device; only when one is non-zero)."""
        trim = (_trim_arg(*trim1) or (0, 0)) + (_trim_arg(*trim2) or (0, 0))
        form, tail = (self._L.walt_pair_overlap_batch_trim_device, trim) if any(trim) else (self._L.walt_pair_overlap_batch_device, ())
        self._ck(form(self._h, d_pairs, d_offsets1, d_offsets2, int(n), d_call_len1, d_call_len2, d_excl, d_totals, *tail, stream))

    def cpg_pairs(self):
        """A table of adjacent-CpG state pairs on this index's device (walt_cpgpairs_create); the index must hold the
        reference."""
        return CpgPairs(self)

    def epialleles(self):
        """A table of four-CpG epiallele patterns on this index's device (walt_epialleles_create); the index must hold
        the reference."""
        return Epialleles(self)

    def pileup(self):
        """A per-cytosine pile-up on this index's device (walt_pileup_create); the index must hold the reference."""
        return Pileup(self)

    def _meth_batch(self, pile, bases, offsets, records, conv="T", call_len=None, want_calls=True, want_counts=True,
                    stats=None, want_stats=True, skip=None, excl=None, mbias=None, mbias_table=0, trim5=0, trim3=0, pairs=None,
                    epi=None, ev=None):
        """Index.meth_call_batch; pile: null, or the handle of a pile-up that takes the calls too; skip: null, or the
        records that are not counted (walt_meth_pileup_batch_skip, which takes a null pile-up); excl: null, or the read
        positions that get no call (walt_meth_pileup_batch_excl, which takes a null pile-up and a null skip)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        records, rec_ptr, rec_stride = _records_arg(records, n)
        conv_arr, conv_ptr, conv_stride, conversion = _conv_arg(conv, n)
        cl = None if call_len is None else np.ascontiguousarray(call_len, dtype=np.uint32)
        if cl is not None and cl.size != n:
            raise ValueError("call_len: one element per read")
        total = int(offsets[n] - offsets[0]) if n else 0
        calls = np.zeros(total, dtype=np.uint8) if want_calls else None
        counts = np.zeros(n, dtype=meth_counts_dtype) if want_counts else None
        if stats is None and want_stats:
            stats = np.zeros(1, dtype=meth_stats_dtype)
        # calls is indexed like bases: offsets[0] bytes in front of the first read belong to neither
        calls_ptr = None if calls is None else calls.ctypes.data - int(offsets[0]) if n else calls.ctypes.data
        skip_arr, skip_ptr, skip_stride = _skip_arg(skip, n)
        excl_arr = None
        if excl is not None:
            excl_arr = np.ascontiguousarray(excl, dtype=np.uint32)
            if excl_arr.ndim != 1 or excl_arr.shape[0] != n:
                raise ValueError("excl: a 1-d uint32 array with one word per read")
        quals_arr, qual = _qual_arg(int(offsets[n]) if n else 0)
        form, head, tail = _meth_form(self._L, False, pile, skip is not None and (skip_ptr, skip_stride),
                                      excl is not None and (_ptr(excl_arr) if n else None,),
                                      mbias is not None and (mbias.handle, int(mbias_table)), trim=_trim_arg(trim5, trim3),
                                      pairs=pairs is not None and (pairs.handle,), epi=epi is not None and (epi.handle,),
                                      ev=ev is not None and (ev,), qual=qual)
        self._ck(form(self._h, *head, bases.ctypes.data, _ptr(offsets), n, rec_ptr, rec_stride, conv_ptr, conv_stride,
                      conversion, _ptr(cl), calls_ptr, _ptr(counts), _ptr(stats), *tail))
        return calls, counts, stats

    @_keyword_only_quals
    def meth_call_batch_device(self, d_bases, d_offsets, n, d_records, record_stride=16, d_conv=None, conv_stride=1,
                               conversion="T", d_call_len=None, d_calls=None, d_counts=None, d_stats=None, stream=0,
                               d_skip=None, skip_stride=1, d_excl=None, mbias=None, mbias_table=0, trim5=0, trim3=0, pairs=None,
                               *, epi=None):
        """Device-pointer form (ints are HBM addresses, stream a hipStream_t value); asynchronous.  mbias: an MBias set
        whose table mbias_table takes the calls too (walt_meth_pileup_batch_mbias_device with a null pile-up; d_calls
        must be given); d_skip / d_excl: as in Pileup.add_batch_device (walt_meth_pileup_batch_excl_device with a null
        pile-up); trim5 / trim3: as in meth_call_batch (walt_meth_pileup_batch_trim_device); pairs: a CpgPairs table of
        this index that takes the calls too (walt_meth_pileup_batch_pairs_device; d_calls must be given); epi: an Epialleles
        table of this index, likewise (walt_meth_pileup_batch_epi_device).  quals, min_qual (keyword only): the address of the
        device array of quality bytes, one per base, and the floor (walt_meth_pileup_batch_qual_device; only when given)."""
        batch = (d_bases, d_offsets, int(n), d_records, int(record_stride), d_conv, int(conv_stride), ord(conversion), d_call_len,
                 d_calls, d_counts, d_stats)
        self._meth_batch_device(None, "excl", batch, stream, d_skip, skip_stride, d_excl, mbias, mbias_table, trim5, trim3, pairs, epi)

    def _meth_batch_device(self, pile, skip_alone, batch, stream, d_skip, skip_stride, d_excl, mbias, mbias_table, trim5=0,
                           trim3=0, pairs=None, epi=None, ev=None):
        """Index.meth_call_batch_device (pile null) and Pileup.add_batch_device.  batch: the C arguments from d_bases to
        d_stats; skip_alone: the form a call with d_skip only goes to (the index's: walt_meth_pileup_batch_excl_device, a
        pile-up's: walt_meth_pileup_batch_skip_device)."""
        form, head, tail = _meth_form(self._L, True, pile, d_skip is not None and (d_skip, int(skip_stride)),
                                      d_excl is not None and (d_excl,), mbias is not None and (mbias.handle, int(mbias_table)),
                                      skip_alone, _trim_arg(trim5, trim3), pairs is not None and (pairs.handle,),
                                      epi is not None and (epi.handle,), ev is not None and (ev,), _qual_arg()[1])
        self._ck(form(self._h, *head, *batch, *tail, stream))

    # -- options: tuning values and test hooks (include/walt_amd.h; the library reads no environment on the mapping path)
    def set_option(self, name, value):
        self._ck(self._L.walt_index_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = ctypes.c_longlong(0)
        self._ck(self._L.walt_index_get_option(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    def pe_workspace_bytes(self, n, max_read_len, top_k):
        """What a paired-end call uses best on this index's device now (never less than the module-level minimum)."""
        return self._L.walt_pe_workspace_bytes_best(self._h, int(n), int(max_read_len), int(top_k))

    @staticmethod
    def check_batch(d_workspace, stream=0):
        """Waits for `stream`; raises if the last device-resident call on this workspace met an invalid read."""
        _check(lib().walt_batch_check(d_workspace, stream))

    def map_pe_batch_device(self, d_bases1, d_offsets1, d_bases2, d_offsets2, n, max_read_len, d_out, d_stats,
                            d_workspace, workspace_bytes, stream=0, max_mismatches=6, b=5000, top_k=50, frag_range=1000):
        self._ck(self._L.walt_map_pe_batch_device(self._h, d_bases1, d_offsets1, d_bases2, d_offsets2, int(n),
                                              int(max_read_len), int(max_mismatches), int(b), int(top_k),
                                              int(frag_range), d_out, d_stats, d_workspace, int(workspace_bytes), stream))

    # -- paired-end -----------------------------------------------------------
    def map_pe_batch(self, bases1, offsets1, bases2, offsets2, max_mismatches=6, b=5000, top_k=50,
                     frag_range=1000, want_ranked=False):
        bases1 = np.ascontiguousarray(bases1, dtype=np.uint8)
        bases2 = np.ascontiguousarray(bases2, dtype=np.uint8)
        offsets1 = np.ascontiguousarray(offsets1, dtype=np.uint64)
        offsets2 = np.ascontiguousarray(offsets2, dtype=np.uint64)
        n = offsets1.size - 1
        if offsets2.size - 1 != n:
            raise ValueError("The number of reads in paired-end files should be the same.")  # paired.cpp:673-677
        out = np.zeros(n, dtype=pair_result_dtype)
        stats = np.zeros(2, dtype=batch_stats_dtype)
        r1 = r2 = n1 = n2 = None
        if want_ranked:
            r1 = np.zeros((n, top_k), dtype=candidate_dtype)
            r2 = np.zeros((n, top_k), dtype=candidate_dtype)
            n1 = np.zeros(n, dtype=np.uint32)
            n2 = np.zeros(n, dtype=np.uint32)
        self._ck(self._L.walt_map_pe_batch(self._h, _ptr(bases1), _ptr(offsets1), _ptr(bases2), _ptr(offsets2), n,
                                       int(max_mismatches), int(b), int(top_k), int(frag_range), _ptr(out),
                                       _ptr(r1), _ptr(n1), _ptr(r2), _ptr(n2), _ptr(stats)))
        if want_ranked:
            return out, stats, (r1, n1, r2, n2)
        return out, stats

    # -- paired-end random PBAT: every pair in both orientations (include/walt_amd.h states the rules) -------------
    def map_pe_rpbat_batch(self, bases1, offsets1, bases2, offsets2, max_mismatches=6, b=5000, top_k=50,
                           frag_range=1000):
        """Host-buffer form.  Returns (pair_result[n], conv uint8[n, 2] of ord('T') / ord('A') per mate, stats[2])."""
        bases1 = np.ascontiguousarray(bases1, dtype=np.uint8)
        bases2 = np.ascontiguousarray(bases2, dtype=np.uint8)
        offsets1 = np.ascontiguousarray(offsets1, dtype=np.uint64)
        offsets2 = np.ascontiguousarray(offsets2, dtype=np.uint64)
        n = offsets1.size - 1
        if offsets2.size - 1 != n:
            raise ValueError("The number of reads in paired-end files should be the same.")
        out = np.zeros(n, dtype=pair_result_dtype)
        conv = np.zeros((n, 2), dtype=np.uint8)
        stats = np.zeros(2, dtype=batch_stats_dtype)
        self._ck(self._L.walt_map_pe_rpbat_batch(self._h, _ptr(bases1), _ptr(offsets1), _ptr(bases2), _ptr(offsets2),
                                             n, int(max_mismatches), int(b), int(top_k), int(frag_range), _ptr(out),
                                             _ptr(conv), _ptr(stats)))
        return out, conv, stats

    def map_pe_rpbat_batch_device(self, d_bases1, d_offsets1, d_bases2, d_offsets2, n, max_read_len, d_out, d_conv,
                                  d_stats, d_workspace, workspace_bytes, stream=0, max_mismatches=6, b=5000, top_k=50,
                                  frag_range=1000):
        """Device-pointer form; d_conv holds 2n bytes, d_stats two walt_batch_stats; workspace_bytes = what d_workspace
        holds (at least pe_rpbat_workspace_bytes(n, max_read_len, top_k))."""
        self._ck(self._L.walt_map_pe_rpbat_batch_device(self._h, d_bases1, d_offsets1, d_bases2, d_offsets2, int(n),
                                                    int(max_read_len), int(max_mismatches), int(b), int(top_k),
                                                    int(frag_range), d_out, d_conv, d_stats, d_workspace,
                                                    int(workspace_bytes), stream))

    def pe_rpbat_workspace_bytes(self, n, max_read_len, top_k):
        """What a random-PBAT paired-end call uses best on this index's device now (walt_pe_rpbat_workspace_bytes_best)."""
        return self._L.walt_pe_rpbat_workspace_bytes_best(self._h, int(n), int(max_read_len), int(top_k))


class Pileup:
    """Per-cytosine methylation pile-up of an Index (include/walt_amd.h, "methylation pile-up"): two exact 32-bit
    counters per forward position on the index's device, fed by the methylation calls of uniquely mapped records."""

    def __init__(self, index):
        self._index = index
        self._L = index._L
        h = ctypes.c_void_p()
        index._ck(self._L.walt_pileup_create(index._h, ctypes.byref(h)))
        self._h = h

    @_keyword_only_quals
    @_keyword_only_evidence
    def add_batch(self, bases, offsets, records, conv="T", call_len=None, want_calls=True, want_counts=True, stats=None,
                  want_stats=True, pairs=None, skip=None, excl=None, mbias=None, mbias_table=0, trim5=0, trim3=0, *, epi=None):
        """Index.meth_call_batch with the pile-up as one more destination: same arguments, same returns.  evidence (keyword
        only): another Pileup of the index that takes the batch's opposite-strand evidence (include/walt_amd.h,
        "opposite-strand evidence": walt_meth_pileup_batch_ev; only when given).  quals, min_qual (keyword only): as in
        Index.meth_call_batch (walt_meth_pileup_batch_qual; only when given); in add_batch_device quals is the address of
        the device array."""
        return self._add_batch(None, bases, offsets, records, conv, call_len, want_calls, want_counts, stats, want_stats, pairs,
                               skip, excl, mbias, mbias_table, trim5, trim3, epi=epi)

    def _add_batch(self, ev, bases, offsets, records, conv, call_len, want_calls, want_counts, stats, want_stats, pairs, skip, excl,
                   mbias, mbias_table, trim5, trim3, epi):
        """add_batch; ev: null, or the handle of the evidence object"""
        return self._index._meth_batch(self._h, bases, offsets, records, conv, call_len, want_calls, want_counts, stats,
                                       want_stats, skip, excl, mbias, mbias_table, trim5, trim3, pairs, epi, ev)

    @_keyword_only_quals
    @_keyword_only_evidence
    def add_batch_device(self, d_bases, d_offsets, n, d_records, record_stride=16, d_conv=None, conv_stride=1,
                         conversion="T", d_call_len=None, d_calls=None, d_counts=None, d_stats=None, stream=0, d_skip=None,
                         skip_stride=1, d_excl=None, mbias=None, mbias_table=0, trim5=0, trim3=0, pairs=None, *, epi=None):
        """Index.meth_call_batch_device with the pile-up as one more destination; asynchronous.  d_skip: one byte per
        record (a non-zero byte: not counted); d_excl: one uint32 per record (Index.pair_overlap_device's); mbias: an
        MBias set whose table mbias_table takes the calls too (d_calls must be given); pairs: a CpgPairs table of the
        index that takes them as well; epi: an Epialleles table of the index, likewise; evidence (keyword only): as in
        add_batch (walt_meth_pileup_batch_ev_device); quals, min_qual (keyword only): the address of the device array of quality
        bytes, one per base, and the floor (walt_meth_pileup_batch_qual_device)."""
        self._add_batch_device(None, d_bases, d_offsets, n, d_records, record_stride, d_conv, conv_stride, conversion, d_call_len,
                               d_calls, d_counts, d_stats, stream, d_skip, skip_stride, d_excl, mbias, mbias_table, trim5, trim3,
                               pairs, epi=epi)

    def _add_batch_device(self, ev, d_bases, d_offsets, n, d_records, record_stride, d_conv, conv_stride, conversion, d_call_len,
                          d_calls, d_counts, d_stats, stream, d_skip, skip_stride, d_excl, mbias, mbias_table, trim5, trim3, pairs,
                          epi):
        """add_batch_device; ev: null, or the handle of the evidence object"""
        batch = (d_bases, d_offsets, int(n), d_records, int(record_stride), d_conv, int(conv_stride), ord(conversion), d_call_len,
                 d_calls, d_counts, d_stats)
        self._index._meth_batch_device(self._h, "skip", batch, stream, d_skip, skip_stride, d_excl, mbias, mbias_table, trim5, trim3,
                                       pairs, epi, ev)

    # -- opposite-strand evidence (include/walt_amd.h states the rules): this object holds the evidence ----------------
    @_keyword_only_quals
    def add_evidence_batch(self, bases, offsets, records, conv="T", call_len=None, skip=None):
        """The evidence kernel alone (walt_meth_evidence_batch): the batch as Index.meth_call_batch takes it; this object's
        plane 0 counts the matches, plane 1 the other bases.  Nothing is returned.  quals, min_qual (keyword only): a base
        below the floor adds to neither plane (walt_meth_pileup_batch_qual with this object as its only destination)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        records, rec_ptr, rec_stride = _records_arg(records, n)
        conv_arr, conv_ptr, conv_stride, conversion = _conv_arg(conv, n)
        cl = None if call_len is None else np.ascontiguousarray(call_len, dtype=np.uint32)
        if cl is not None and cl.size != n:
            raise ValueError("call_len: one element per read")
        skip_arr, skip_ptr, skip_stride = _skip_arg(skip, n)
        quals_arr, qual = _qual_arg(int(offsets[n]) if n else 0)
        if qual:
            self._index._ck(self._L.walt_meth_pileup_batch_qual(self._index._h, None, bases.ctypes.data, _ptr(offsets), n, rec_ptr,
                                                                rec_stride, conv_ptr, conv_stride, conversion, _ptr(cl), None, None,
                                                                None, skip_ptr, skip_stride, None, None, 0, 0, 0, None, None,
                                                                self._h, *qual))
            return
        self._index._ck(self._L.walt_meth_evidence_batch(self._index._h, self._h, bases.ctypes.data, _ptr(offsets), n, rec_ptr,
                                                         rec_stride, conv_ptr, conv_stride, conversion, _ptr(cl), skip_ptr,
                                                         skip_stride))

    @_keyword_only_quals
    def add_evidence_batch_device(self, d_bases, d_offsets, n, d_records, record_stride=16, d_conv=None, conv_stride=1,
                                  conversion="T", d_call_len=None, d_skip=None, skip_stride=1, stream=0):
        """Device-pointer form (walt_meth_evidence_batch_device); asynchronous.  quals, min_qual (keyword only): the address
        of the device array of quality bytes and the floor (walt_meth_pileup_batch_qual_device)."""
        _, qual = _qual_arg()
        if qual:
            self._index._ck(self._L.walt_meth_pileup_batch_qual_device(self._index._h, None, d_bases, d_offsets, int(n), d_records,
                                                                       int(record_stride), d_conv, int(conv_stride), ord(conversion),
                                                                       d_call_len, None, None, None, d_skip, int(skip_stride), None,
                                                                       None, 0, 0, 0, None, None, self._h, *qual, stream))
            return
        self._index._ck(self._L.walt_meth_evidence_batch_device(self._index._h, self._h, d_bases, d_offsets, int(n), d_records,
                                                                int(record_stride), d_conv, int(conv_stride), ord(conversion),
                                                                d_call_len, d_skip, int(skip_stride), stream))

    def variants(self, ev, pos_lo=0, pos_hi=None, min_depth=5, max_percent=50):
        """The positions of [pos_lo, pos_hi) that the evidence object `ev` flags (walt_pileup_variants), ascending:
        variant_site_dtype[n], meth / unmeth from this pile-up, match / other from ev."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        args = (self._h, ev.handle, int(pos_lo), int(pos_hi), int(min_depth), int(max_percent))
        n = ctypes.c_uint64(0)
        rc = self._L.walt_pileup_variants(*args, None, 0, ctypes.byref(n))
        if rc != WALT_OK and n.value == 0:
            self._index._ck(rc)
        out = np.zeros(n.value, dtype=variant_site_dtype)
        if n.value:
            self._index._ck(self._L.walt_pileup_variants(*args, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def variants_device(self, ev, pos_lo, pos_hi, min_depth, max_percent, d_out, cap, d_n_out, stream=0):
        """Device-pointer form (walt_pileup_variants_device); asynchronous."""
        self._index._ck(self._L.walt_pileup_variants_device(self._h, ev.handle, int(pos_lo), int(pos_hi), int(min_depth),
                                                            int(max_percent), d_out, int(cap), d_n_out, stream))

    def mask_variants(self, ev, pos_lo=0, pos_hi=None, min_depth=5, max_percent=50):
        """Zeroes this pile-up's counters at the positions of [pos_lo, pos_hi) that `ev` flags (walt_pileup_mask_variants);
        returns uint64[5]: judged, flagged, masked sites, methylated calls removed, unmethylated calls removed."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        out = np.zeros(5, dtype=np.uint64)
        self._index._ck(self._L.walt_pileup_mask_variants(self._h, ev.handle, int(pos_lo), int(pos_hi), int(min_depth),
                                                          int(max_percent), _ptr(out)))
        return out

    def mask_variants_device(self, ev, pos_lo, pos_hi, min_depth, max_percent, d_out, stream=0):
        """Device-pointer form (walt_pileup_mask_variants_device): 40 bytes at d_out; asynchronous."""
        self._index._ck(self._L.walt_pileup_mask_variants_device(self._h, ev.handle, int(pos_lo), int(pos_hi), int(min_depth),
                                                                 int(max_percent), d_out, stream))

    def extract(self, pos_lo=0, pos_hi=None):
        """(sites meth_site_dtype[n] of the forward positions [pos_lo, pos_hi), ascending; offref uint64[2]: the
        methylated / unmethylated calls of the range that lie on an A or T of the reference)."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        n = ctypes.c_uint64(0)
        offref = np.zeros(2, dtype=np.uint64)
        rc = self._L.walt_pileup_extract(self._h, int(pos_lo), int(pos_hi), None, 0, ctypes.byref(n), _ptr(offref))
        if rc != WALT_OK and n.value == 0:
            self._index._ck(rc)
        sites = np.zeros(n.value, dtype=meth_site_dtype)
        if n.value:
            self._index._ck(self._L.walt_pileup_extract(self._h, int(pos_lo), int(pos_hi), _ptr(sites), n.value,
                                                        ctypes.byref(n), _ptr(offref)))
        return sites, offref

    def extract_device(self, pos_lo, pos_hi, d_sites, cap, d_n_sites, d_offref=None, stream=0):
        """Device-pointer form (walt_pileup_extract_device); asynchronous."""
        self._index._ck(self._L.walt_pileup_extract_device(self._h, int(pos_lo), int(pos_hi), d_sites, int(cap), d_n_sites,
                                                           d_offref, stream))

    def levels(self, pos_lo=0, pos_hi=None):
        """The summary of the forward positions [pos_lo, pos_hi) (walt_pileup_levels): one levels_dtype record."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        out = np.zeros(1, dtype=levels_dtype)
        self._index._ck(self._L.walt_pileup_levels(self._h, int(pos_lo), int(pos_hi), _ptr(out)))
        return out[0]

    def levels_device(self, pos_lo, pos_hi, d_out, stream=0):
        """Device-pointer form (walt_pileup_levels_device): 656 bytes at d_out; asynchronous."""
        self._index._ck(self._L.walt_pileup_levels_device(self._h, int(pos_lo), int(pos_hi), d_out, stream))

    def depth_hist(self, pos_lo=0, pos_hi=None):
        """The joint histogram of the sites of [pos_lo, pos_hi) (walt_pileup_depth_hist): (hist uint64[4][SITECALL_BINS] by
        context and sitecall_bin(depth, meth), deep uint64[4]: the sites deeper than SITECALL_DEPTH)."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        hist = np.zeros((4, SITECALL_BINS), dtype=np.uint64)
        deep = np.zeros(4, dtype=np.uint64)
        self._index._ck(self._L.walt_pileup_depth_hist(self._h, int(pos_lo), int(pos_hi), _ptr(hist), _ptr(deep)))
        return hist, deep

    def depth_hist_device(self, pos_lo, pos_hi, d_hist, d_deep, stream=0):
        """Device-pointer form (walt_pileup_depth_hist_device): 8 * 4 * SITECALL_BINS bytes at d_hist, 32 at d_deep, both
        zeroed by the call; asynchronous."""
        self._index._ck(self._L.walt_pileup_depth_hist_device(self._h, int(pos_lo), int(pos_hi), d_hist, d_deep, stream))

    @staticmethod
    def _min_meth_arg(min_meth):
        table = np.ascontiguousarray(min_meth, dtype=np.uint32)
        if table.shape != (4, SITECALL_DEPTH + 1):
            raise ValueError("min_meth must have shape (4, %d): context by depth" % (SITECALL_DEPTH + 1))
        return table

    def call_sites(self, min_meth, pos_lo=0, pos_hi=None):
        """The sites of [pos_lo, pos_hi) with meth >= min_meth[context][depth] (reserved 0), and every site deeper than
        SITECALL_DEPTH (reserved 1), ascending (walt_pileup_call_sites): meth_site_dtype[n]."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        table = self._min_meth_arg(min_meth)
        args = (self._h, int(pos_lo), int(pos_hi), _ptr(table))
        n = ctypes.c_uint64(0)
        rc = self._L.walt_pileup_call_sites(*args, None, 0, ctypes.byref(n))
        if rc != WALT_OK and n.value == 0:
            self._index._ck(rc)
        out = np.zeros(n.value, dtype=meth_site_dtype)
        if n.value:
            self._index._ck(self._L.walt_pileup_call_sites(*args, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def call_sites_device(self, pos_lo, pos_hi, d_min_meth, d_out, cap, d_n_out, stream=0):
        """Device-pointer form (walt_pileup_call_sites_device): d_min_meth uint32[4][128]; asynchronous."""
        self._index._ck(self._L.walt_pileup_call_sites_device(self._h, int(pos_lo), int(pos_hi), d_min_meth, d_out, int(cap),
                                                              d_n_out, stream))

    def regions(self, regions):
        """The summaries of many ranges in one call (walt_pileup_regions): `regions` is an (n, 2) integer array of
        [lo, hi) or a region_dtype array; returns n region_levels_dtype records, record i equal to levels(lo, hi) of
        region i in the fields it has."""
        if isinstance(regions, np.ndarray) and regions.dtype == region_dtype:
            regs = np.ascontiguousarray(regions).reshape(-1)
        else:
            arr = np.asarray(regions)
            if arr.size == 0:
                arr = np.zeros((0, 2), dtype=np.uint32)
            if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype.kind not in "iu":
                raise ValueError("Pileup.regions wants an (n, 2) integer array or a region_dtype array")
            if arr.size and (int(arr.min()) < 0 or int(arr.max()) > 0xFFFFFFFF):
                raise ValueError("Pileup.regions: positions are 32-bit and not negative")
            regs = np.ascontiguousarray(arr.astype(np.uint32)).view(region_dtype).reshape(-1)
        out = np.zeros(regs.size, dtype=region_levels_dtype)
        self._index._ck(self._L.walt_pileup_regions(self._h, _ptr(regs), regs.size, _ptr(out)))
        return out

    def regions_device(self, d_regions, n, d_out, d_work, stream=0):
        """Device-pointer form (walt_pileup_regions_device): n region_dtype records at d_regions, 160 * n bytes at d_out,
        regions_workspace_bytes(n) bytes at d_work; asynchronous.  A region outside the genome gives a zero record."""
        self._index._ck(self._L.walt_pileup_regions_device(self._h, d_regions, int(n), d_out, d_work, stream))

    def read(self, pos_lo=0, pos_hi=None):
        """(meth, unmeth) uint32 arrays: the raw counters of [pos_lo, pos_hi) (walt_pileup_read)."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        n = max(0, int(pos_hi) - int(pos_lo))
        meth, unmeth = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._index._ck(self._L.walt_pileup_read(self._h, int(pos_lo), int(pos_hi), _ptr(meth), _ptr(unmeth)))
        return meth, unmeth

    def add(self, pos_lo, pos_hi, meth=None, unmeth=None):
        """Adds two uint32 arrays of pos_hi - pos_lo counts into the counters (walt_pileup_add); None: zeros."""
        arrs = []
        for a in (meth, unmeth):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint32)
                if a.size != int(pos_hi) - int(pos_lo):
                    raise ValueError("Pileup.add wants pos_hi - pos_lo counts per array")
            arrs.append(a)
        self._index._ck(self._L.walt_pileup_add(self._h, int(pos_lo), int(pos_hi), *[None if a is None else _ptr(a) for a in arrs]))

    def clear(self):
        self._index._ck(self._L.walt_pileup_clear(self._h))

    @property
    def handle(self):
        return self._h

    @property
    def device_bytes(self):
        return self._L.walt_pileup_device_bytes(self._h)

    def close(self):
        if self._h:
            self._L.walt_pileup_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dedup:
    """A duplicate set on one device (include/walt_amd.h, "duplicates"): PCR duplicates marked from mapped records alone.
    The set numbers the records it is fed; a record is a duplicate when an earlier one had the same key."""

    def __init__(self, device=0, initial_slots=0, pattern=None):
        self._L = lib(pattern)
        h = ctypes.c_void_p()
        self._h = None
        self._ck(self._L.walt_dedup_create(int(device), int(initial_slots), ctypes.byref(h)))
        self._h = h

    def _ck(self, rc):
        if rc != WALT_OK:
            raise WaltError(rc, self._L.walt_last_error().decode("utf-8", "replace"))

    def add_batch(self, records, conv="T", kind=0):
        """records: a best_match_dtype array or strided view (e.g. the m1 field of a pair_result_dtype array); conv: 'T' /
        'A' for all, or a uint8 array per record (any stride).  Returns dup uint8[n]."""
        records, rec_ptr, rec_stride = _records_arg(records)
        n = records.shape[0]
        conv_arr, conv_ptr, conv_stride, conversion = _conv_arg(conv, n, "record")
        dup = np.zeros(n, dtype=np.uint8)
        self._ck(self._L.walt_dedup_batch(self._h, rec_ptr, rec_stride, conv_ptr, conv_stride, conversion, int(kind), n, _ptr(dup)))
        return dup

    def add_pairs(self, pairs, conv="T"):
        """pairs: a pair_result_dtype array; conv: mate 1's conversion for all ('T' / 'A'; mate 2 has the other), or a
        uint8 array [n, 2] as map_pe_rpbat_batch returns it.  Returns dup uint8[n, 2]."""
        pairs = np.ascontiguousarray(pairs, dtype=pair_result_dtype)
        n = pairs.shape[0]
        conv_arr, conversion = None, 0
        if isinstance(conv, (str, bytes)):
            conversion = ord(conv)
        else:
            conv_arr = np.ascontiguousarray(conv, dtype=np.uint8)
            if conv_arr.shape != (n, 2):
                raise ValueError("conv: 'T', 'A' or a uint8 array [n, 2]")
        dup = np.zeros((n, 2), dtype=np.uint8)
        self._ck(self._L.walt_dedup_pairs_batch(self._h, _ptr(pairs), _ptr(conv_arr), conversion, n, _ptr(dup)))
        return dup

    def add_batch_device(self, d_records, n, d_dup, record_stride=16, d_conv=None, conv_stride=1, conversion="T", kind=0,
                         stream=0):
        """Device-pointer form (ints are HBM addresses on the set's device); asynchronous; reserve() first."""
        self._ck(self._L.walt_dedup_batch_device(self._h, d_records, int(record_stride), d_conv, int(conv_stride),
                                                 ord(conversion), int(kind), int(n), d_dup, stream))

    def add_pairs_device(self, d_pairs, n, d_dup, d_conv=None, conversion="T", stream=0):
        self._ck(self._L.walt_dedup_pairs_batch_device(self._h, d_pairs, d_conv, ord(conversion), int(n), d_dup, stream))

    def reserve(self, n_more):
        self._ck(self._L.walt_dedup_reserve(self._h, int(n_more)))

    def count(self):
        """(distinct keys held, records numbered since the last clear)"""
        keys, fed = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(self._L.walt_dedup_count(self._h, ctypes.byref(keys), ctypes.byref(fed)))
        return keys.value, fed.value

    def clear(self):
        self._ck(self._L.walt_dedup_clear(self._h))

    @property
    def handle(self):
        return self._h

    @property
    def device_bytes(self):
        return self._L.walt_dedup_device_bytes(self._h)

    def close(self):
        if self._h:
            self._L.walt_dedup_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MBias:
    """Methylation bias by read position on one device (include/walt_amd.h, "methylation bias by read position"):
    `tables` tables (1 to 8; one per mate) of exact 64-bit counts [context 4][methylated, unmethylated][position 1024],
    summed from the calls of uniquely mapped, unskipped records."""

    SHAPE = (4, 2, 1024)

    def __init__(self, device=0, tables=1, pattern=None):
        self._L = lib(pattern)
        h = ctypes.c_void_p()
        self._h = None
        self._ck(self._L.walt_mbias_create(int(device), int(tables), ctypes.byref(h)))
        self._h = h
        self.tables = int(tables)

    def _ck(self, rc):
        if rc != WALT_OK:
            raise WaltError(rc, self._L.walt_last_error().decode("utf-8", "replace"))

    def add(self, calls, offsets, records, skip=None, table=0):
        """calls: the uint8 array Index.meth_call_batch returned (indexed from offsets[0]); offsets: n + 1; records: a
        best_match_dtype array or strided view (e.g. the m2 field of a pair_result_dtype array); skip: a uint8 array per
        record, any stride.  Waits for the result."""
        calls = np.ascontiguousarray(calls, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        records, rec_ptr, rec_stride = _records_arg(records, n)
        skip_arr, skip_ptr, skip_stride = _skip_arg(skip, n)
        calls_ptr = calls.ctypes.data - int(offsets[0]) if n else None
        self._ck(self._L.walt_mbias_batch(self._h, int(table), calls_ptr, _ptr(offsets), n, rec_ptr, rec_stride, skip_ptr, skip_stride))

    def add_device(self, d_calls, d_offsets, n, d_records, record_stride=16, d_skip=None, skip_stride=1, table=0, stream=0):
        """Device-pointer form (ints are HBM addresses on the set's device, stream a hipStream_t value); asynchronous."""
        self._ck(self._L.walt_mbias_batch_device(self._h, int(table), d_calls, d_offsets, int(n), d_records, int(record_stride),
                                                 d_skip, int(skip_stride), stream))

    def read(self, table=0):
        """The table as a uint64 array [4, 2, 1024]: context (CpG, CHG, CHH, unknown), methylated / unmethylated, position."""
        out = np.zeros(self.SHAPE, dtype=np.uint64)
        self._ck(self._L.walt_mbias_read(self._h, int(table), _ptr(out)))
        return out

    def clear(self):
        self._ck(self._L.walt_mbias_clear(self._h))

    @property
    def handle(self):
        return self._h

    @property
    def device_bytes(self):
        return self._L.walt_mbias_device_bytes(self._h)

    def close(self):
        if self._h:
            self._L.walt_mbias_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CpgTable:
    """What CpgPairs and Epialleles share: a table keyed by CpG pair number on an Index's device (the C functions
    walt_<_prefix>_*).  Close it before the index."""
    _prefix = None

    def __init__(self, index):
        self._index = index
        self._L = index._L
        self._h = None
        h = ctypes.c_void_p()
        index._ck(self._fn("create")(index._h, ctypes.byref(h)))
        self._h = h

    def _fn(self, name):
        return getattr(self._L, "walt_%s_%s" % (self._prefix, name))

    def add(self, calls, offsets, records, skip=None):
        """calls: the uint8 array Index.meth_call_batch returned (indexed from offsets[0]); offsets: n + 1; records: a
        best_match_dtype array or strided view (e.g. the m2 field of a pair_result_dtype array); skip: a uint8 array per
        record, any stride.  Waits for the result."""
        calls = np.ascontiguousarray(calls, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        records, rec_ptr, rec_stride = _records_arg(records, n)
        skip_arr, skip_ptr, skip_stride = _skip_arg(skip, n)
        calls_ptr = calls.ctypes.data - int(offsets[0]) if n else None
        self._index._ck(self._fn("batch")(self._h, calls_ptr, _ptr(offsets), n, rec_ptr, rec_stride, skip_ptr, skip_stride))

    def add_device(self, d_calls, d_offsets, n, d_records, record_stride=16, d_skip=None, skip_stride=1, stream=0):
        """Device-pointer form (ints are HBM addresses on the index's device, stream a hipStream_t value); asynchronous."""
        self._index._ck(self._fn("batch_device")(self._h, d_calls, d_offsets, int(n), d_records, int(record_stride), d_skip,
                                                 int(skip_stride), stream))

    def _extract(self, dtype, *args):
        """extract(*args, out, cap, n_out) twice: for the count, then into an array of `dtype`."""
        n = ctypes.c_uint64(0)
        rc = self._fn("extract")(self._h, *args, None, 0, ctypes.byref(n))
        if rc != WALT_OK and n.value == 0:
            self._index._ck(rc)
        sites = np.zeros(n.value, dtype=dtype)
        if n.value:
            self._index._ck(self._fn("extract")(self._h, *args, _ptr(sites), n.value, ctypes.byref(n)))
        return sites

    @property
    def n_pairs(self):
        return int(self._fn("n_pairs")(self._h))

    def clear(self):
        self._index._ck(self._fn("clear")(self._h))

    @property
    def handle(self):
        return self._h

    @property
    def device_bytes(self):
        return self._fn("device_bytes")(self._h)

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CpgPairs(_CpgTable):
    """Adjacent-CpG state pairs of an Index (include/walt_amd.h, "adjacent CpG pairs"): for every two neighbouring CpG
    pairs of the genome, how often one read called them MM, MU, UM, UU -- exact 32-bit counters on the index's device,
    keyed by the number of the lower pair.  Close it before the index."""
    _prefix = "cpgpairs"

    def extract(self, pos_lo=0, pos_hi=None):
        """The non-zero entries whose lower pair starts in the forward positions [pos_lo, pos_hi), ascending:
        cpgpair_site_dtype[n] (pos, next, n[4] = MM, MU, UM, UU)."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        return self._extract(cpgpair_site_dtype, int(pos_lo), int(pos_hi))

    def extract_device(self, pos_lo, pos_hi, d_out, cap, d_n_out, stream=0):
        """Device-pointer form (walt_cpgpairs_extract_device); asynchronous."""
        self._index._ck(self._L.walt_cpgpairs_extract_device(self._h, int(pos_lo), int(pos_hi), d_out, int(cap), d_n_out, stream))


class Epialleles(_CpgTable):
    """Four-CpG epialleles of an Index (include/walt_amd.h, "four-CpG epialleles"): for every four neighbouring CpG pairs
    of the genome, how often one read showed each of their 16 methylation patterns (column 8 u0 + 4 u1 + 2 u2 + u3, u = 1
    unmethylated, the lowest position first) -- exact 32-bit counters on the index's device, keyed by the number of the
    lowest pair.  add and add_device take CpgPairs's arguments.  Close it before the index."""
    _prefix = "epialleles"

    def extract(self, pos_lo=0, pos_hi=None, min_total=1):
        """The entries whose lowest pair starts in the forward positions [pos_lo, pos_hi) and whose sixteen counters sum
        to at least min_total (>= 1), ascending: epiallele_site_dtype[n] (pos, last, n[16])."""
        pos_hi = self._index.genome_len if pos_hi is None else pos_hi
        return self._extract(epiallele_site_dtype, int(pos_lo), int(pos_hi), int(min_total))

    def extract_device(self, pos_lo, pos_hi, min_total, d_out, cap, d_n_out, stream=0):
        """Device-pointer form (walt_epialleles_extract_device); asynchronous."""
        self._index._ck(self._L.walt_epialleles_extract_device(self._h, int(pos_lo), int(pos_hi), int(min_total), d_out, int(cap),
                                                               d_n_out, stream))
