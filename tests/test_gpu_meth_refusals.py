"""What the methylation-side entry points refuse, and which of them Python calls (include/walt_amd.h: "methylation
calls", "methylation pile-up", "duplicates", "overlap of a pair", "methylation bias by read position").  One table of
(entry point, arguments, status, walt_last_error() text) over every host and device form: the ten walt_meth_* forms,
walt_mbias_batch, walt_dedup_batch, walt_dedup_pairs_batch, walt_pair_overlap_batch and their _device forms.  The texts
are literals: what a caller sees today is what it sees after the host code behind these forms moves.  Batches are three
reads with one mapped record; a refusal returns before any kernel, an accepting row launches on those three reads."""
import os

import numpy as np
import pytest

import refio

pytestmark = pytest.mark.gpu

EINVAL = -1
RECORD_STRIDE = ": record stride %d is smaller than a walt_best_match (16) or not a multiple of 4"
CONV_STRIDE = ": conv stride 0 is smaller than its element (1)"
CONVERSION_C = ": conversion 67 is neither 'T' nor 'A'"
SKIP_STRIDE = ": skip stride 0 is smaller than its element (1)"
METH_ALIGN = ": records and call_len must be 4-byte aligned, counts and stats 8-byte aligned"
EXCL_ALIGN = ": excl must be 4-byte aligned"
NULL_PILE = ": bad argument (null pile-up)"
OTHER_PILE = ": the pile-up belongs to another index"
TABLE_1_OF_1 = ": table 1 of a bias set with 1"
NO_CALLS = ": the bias table is counted from the calls: d_calls must not be NULL when a bias set is given"
DECREASING = "offsets not non-decreasing"
TOO_LONG = "read length above 1024 is not supported"

# the ten forms of the calling call: name -> (takes a pile-up, skip, excl, a bias set); "_device" appended for the device form
METH_FORMS = {
    "walt_meth_call_batch": (False, False, False, False),
    "walt_meth_pileup_batch": (True, False, False, False),
    "walt_meth_pileup_batch_skip": (True, True, False, False),
    "walt_meth_pileup_batch_excl": (True, True, True, False),
    "walt_meth_pileup_batch_mbias": (True, True, True, True),
}
PILE_REQUIRED = ("walt_meth_pileup_batch",)


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "refusals_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    return refio.DbIndex(path), path


@pytest.fixture(scope="module")
def g1_all(g1):
    import walt_amd
    idx = walt_amd.Index.open(g1[1], device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield idx
    idx.close()


class Batch:
    """three reads of 50 bases, record 0 mapped; the same batch on the host (h) and on the device (d), as addresses"""

    def __init__(self, wa, torch):
        dev = torch.device("cuda", 0)
        n = 3
        rec = np.zeros(n, dtype=wa.best_match_dtype)
        rec[0] = (100, 1, b"+", b"", 0)
        pairs = np.zeros(n, dtype=wa.pair_result_dtype)
        pairs["m1"][0], pairs["m2"][0] = (100, 1, b"+", b"", 0), (120, 1, b"-", b"", 0)
        pairs["best_times"][0], pairs["frag_len"][0] = 1, 70
        host = dict(
            bases=np.frombuffer((b"ACGTTGCATCGA" * 13)[:150], dtype=np.uint8).copy(),
            offsets=np.array([0, 50, 100, 150], dtype=np.uint64),
            records=rec, pairs=pairs,
            conv=np.full(n, ord("T"), dtype=np.uint8), conv2=np.full(2 * n, ord("T"), dtype=np.uint8),
            skip=np.zeros(n, dtype=np.uint8), excl=np.zeros(n, dtype=np.uint32),
            calls=np.zeros(150 + 16, dtype=np.uint8), counts=np.zeros(n, dtype=wa.meth_counts_dtype),
            stats=np.zeros(1, dtype=wa.meth_stats_dtype), dup=np.zeros(2 * n, dtype=np.uint8),
            totals=np.zeros(2, dtype=np.uint64),
            # a read of 1,025 bases in front of two of five; and read 1 ending before it starts
            bases_long=np.full(1035, ord("C"), dtype=np.uint8), offsets_long=np.array([0, 1025, 1030, 1035], dtype=np.uint64),
            calls_long=np.zeros(1035 + 16, dtype=np.uint8), offsets_dec=np.array([0, 50, 40, 150], dtype=np.uint64))
        self.host = host
        self.dev = {}
        for k, a in host.items():
            raw = np.zeros(a.nbytes + 64, dtype=np.uint8)  # (room behind every array: the kernels read whole slices)
            raw[:a.nbytes] = a.view(np.uint8).reshape(-1)
            self.dev[k] = torch.from_numpy(raw).to(dev)
        torch.cuda.synchronize()
        self.h = {k: a.ctypes.data for k, a in host.items()}
        self.d = {k: t.data_ptr() for k, t in self.dev.items()}
        assert all(p % 16 == 0 for p in self.d.values())


@pytest.fixture(scope="module")
def env(wa, g1, g1_all):
    import torch
    other = wa.Index.open(g1[1], device=0, strands=wa.STRANDS_ALL | wa.WITH_REFERENCE)
    e = dict(batch=Batch(wa, torch), idx=g1_all._h, pile=g1_all.pileup(), other_pile=other.pileup(), mb=wa.MBias(0, 1),
             dd=wa.Dedup(0, 1024))
    yield e
    torch.cuda.synchronize()
    for k in ("pile", "other_pile", "mb", "dd"):
        e[k].close()
    other.close()


def meth_args(name, device, src, env, **over):
    """the argument tuple of one of the ten forms: a valid call on the three reads, with `over` on top"""
    pile, skip, excl, mbias = METH_FORMS[name]
    a = dict(idx=env["idx"], p=env["pile"].handle if name in PILE_REQUIRED else None, bases=src["bases"], offsets=src["offsets"],
             n=3, records=src["records"], record_stride=16, conv=None, conv_stride=1, conversion=ord("T"), call_len=None,
             calls=src["calls"], counts=src["counts"], stats=src["stats"], skip=None, skip_stride=1, excl=None, mb=None,
             table=0, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    order = ["idx"] + (["p"] if pile else []) + ["bases", "offsets", "n", "records", "record_stride", "conv", "conv_stride",
                                                  "conversion", "call_len", "calls", "counts", "stats"]
    order += (["skip", "skip_stride"] if skip else []) + (["excl"] if excl else []) + (["mb", "table"] if mbias else [])
    order += ["stream"] if device else []
    return tuple(a[k] for k in order)


NULLS = dict(bases=None, offsets=None, n=0, records=None, calls=None, counts=None, stats=None)


def meth_rows(env):
    b = env["batch"]
    rows = []
    for name, (pile, skip, excl, mbias) in METH_FORMS.items():
        for device in (False, True):
            form = name + ("_device" if device else "")
            src = b.d if device else b.h

            def row(label, status, text, **over):
                rows.append((form, label, meth_args(name, device, src, env, **over), status, text))

            row("null handle", EINVAL, form + ": bad argument", idx=None)
            row("record stride 8", EINVAL, form + RECORD_STRIDE % 8, record_stride=8)
            row("conv stride 0", EINVAL, form + CONV_STRIDE, conv=src["conv"], conv_stride=0)
            row("conversion 'C'", EINVAL, form + CONVERSION_C, conversion=ord("C"))
            if skip:
                row("skip stride 0", EINVAL, form + SKIP_STRIDE, skip=src["skip"], skip_stride=0)
            if device:
                row("misaligned records", EINVAL, form + METH_ALIGN, records=src["records"] + 2)
                row("misaligned counts", EINVAL, form + METH_ALIGN, counts=src["counts"] + 4)
                if excl:
                    row("misaligned excl", EINVAL, form + EXCL_ALIGN, excl=src["excl"] + 2)
            if pile:
                row("a pile-up of another index", EINVAL, form + OTHER_PILE, p=env["other_pile"].handle)
                if name in PILE_REQUIRED:
                    row("null pile-up", EINVAL, form + NULL_PILE, p=None)
                else:
                    row("accepted with a pile-up", 0, None, p=env["pile"].handle)
            if mbias:
                row("table out of range", EINVAL, form + TABLE_1_OF_1, mb=env["mb"].handle, table=1)
                if device:
                    row("a bias set without d_calls", EINVAL, form + NO_CALLS, mb=env["mb"].handle, calls=None)
                else:  # (the host form counts from its own device copy)
                    row("a bias set without calls", 0, None, mb=env["mb"].handle, calls=None)
                row("accepted with a bias set", 0, None, mb=env["mb"].handle)
            if not device:  # (a device form leaves the offsets to the kernel: such a read gets no call)
                row("decreasing offsets", EINVAL, DECREASING, offsets=src["offsets_dec"])
                row("a read of 1,025 bases", EINVAL, TOO_LONG, bases=src["bases_long"], offsets=src["offsets_long"],
                    calls=src["calls_long"])
            row("n == 0 with null arrays", 0, None, **NULLS)
            row("accepted", 0, None)
            if skip:
                row("accepted with skip, conv and excl" if excl else "accepted with skip and conv", 0, None, skip=src["skip"],
                    conv=src["conv"], **(dict(excl=src["excl"]) if excl else {}))
    return rows


def other_rows(env):
    b = env["batch"]
    mb, dd, idx = env["mb"].handle, env["dd"].handle, env["idx"]
    rows = []
    for device in (False, True):
        s = b.d if device else b.h
        tail = (None,) if device else ()
        form = "walt_mbias_batch" + ("_device" if device else "")
        pre = "" if device else form + ": "
        rows += [
            (form, "null handle", (None, 0, s["calls"], s["offsets"], 3, s["records"], 16, None, 1) + tail, EINVAL,
             form + ": bad argument (null bias set)"),
            (form, "table out of range", (mb, 1, s["calls"], s["offsets"], 3, s["records"], 16, None, 1) + tail, EINVAL,
             form + TABLE_1_OF_1),
            (form, "record stride 8", (mb, 0, s["calls"], s["offsets"], 3, s["records"], 8, None, 1) + tail, EINVAL,
             form + RECORD_STRIDE % 8),
            (form, "skip stride 0", (mb, 0, s["calls"], s["offsets"], 3, s["records"], 16, s["skip"], 0) + tail, EINVAL,
             form + SKIP_STRIDE),
            (form, "null records", (mb, 0, s["calls"], s["offsets"], 3, None, 16, None, 1) + tail, EINVAL,
             form + ": bad argument (null calls, offsets or records)"),
            (form, "n == 0 with null arrays", (mb, 0, None, None, 0, None, 16, None, 1) + tail, 0, None),
            (form, "accepted", (mb, 0, s["calls"], s["offsets"], 3, s["records"], 16, s["skip"], 1) + tail, 0, None),
        ]
        if device:
            rows += [(form, "misaligned records", (mb, 0, s["calls"], s["offsets"], 3, s["records"] + 2, 16, None, 1) + tail, EINVAL,
                      form + ": records must be 4-byte aligned, offsets 8-byte aligned"),
                     (form, "misaligned offsets", (mb, 0, s["calls"], s["offsets"] + 4, 3, s["records"], 16, None, 1) + tail, EINVAL,
                      form + ": records must be 4-byte aligned, offsets 8-byte aligned")]
        else:
            rows += [(form, "decreasing offsets", (mb, 0, s["calls"], s["offsets_dec"], 3, s["records"], 16, None, 1), EINVAL,
                      pre + DECREASING),
                     (form, "a read of 1,025 calls", (mb, 0, s["calls_long"], s["offsets_long"], 3, s["records"], 16, None, 1), EINVAL,
                      pre + TOO_LONG)]

        form = "walt_dedup_batch" + ("_device" if device else "")
        rows += [
            (form, "null handle", (None, s["records"], 16, None, 1, ord("T"), 0, 3, s["dup"]) + tail, EINVAL,
             form + ": bad argument (null duplicate set)"),
            (form, "record stride 8", (dd, s["records"], 8, None, 1, ord("T"), 0, 3, s["dup"]) + tail, EINVAL, form + RECORD_STRIDE % 8),
            (form, "conv stride 0", (dd, s["records"], 16, s["conv"], 0, ord("T"), 0, 3, s["dup"]) + tail, EINVAL, form + CONV_STRIDE),
            (form, "conversion 'C'", (dd, s["records"], 16, None, 1, ord("C"), 0, 3, s["dup"]) + tail, EINVAL, form + CONVERSION_C),
            (form, "kind 3", (dd, s["records"], 16, None, 1, ord("T"), 3, 3, s["dup"]) + tail, EINVAL, form + ": kind 3 is not 0, 1 or 2"),
            (form, "n == 0 with null arrays", (dd, None, 16, None, 1, ord("T"), 0, 0, None) + tail, 0, None),
            (form, "accepted", (dd, s["records"], 16, s["conv"], 1, 0, 0, 3, s["dup"]) + tail, 0, None),
        ]
        if device:
            rows.append((form, "misaligned records", (dd, s["records"] + 2, 16, None, 1, ord("T"), 0, 3, s["dup"]) + tail, EINVAL,
                         form + ": records must be 4-byte aligned"))

        form = "walt_dedup_pairs_batch" + ("_device" if device else "")
        rows += [
            (form, "null handle", (None, s["pairs"], None, ord("T"), 3, s["dup"]) + tail, EINVAL, form + ": bad argument (null duplicate set)"),
            (form, "conversion 'C'", (dd, s["pairs"], None, ord("C"), 3, s["dup"]) + tail, EINVAL, form + CONVERSION_C),
            (form, "null pairs", (dd, None, None, ord("T"), 3, s["dup"]) + tail, EINVAL, form + ": bad argument"),
            (form, "n == 0 with null arrays", (dd, None, None, ord("T"), 0, None) + tail, 0, None),
            (form, "accepted", (dd, s["pairs"], s["conv2"], 0, 3, s["dup"]) + tail, 0, None),
        ]
        if device:
            rows.append((form, "misaligned pairs", (dd, s["pairs"] + 4, None, ord("T"), 3, s["dup"]) + tail, EINVAL,
                         form + ": pairs must be 16-byte aligned"))

        form = "walt_pair_overlap_batch" + ("_device" if device else "")
        rows += [
            (form, "null handle", (None, s["pairs"], s["offsets"], s["offsets"], 3, None, None, s["excl"], s["totals"]) + tail, EINVAL,
             form + ": bad argument (null index)"),
            (form, "null excl", (idx, s["pairs"], s["offsets"], s["offsets"], 3, None, None, None, s["totals"]) + tail, EINVAL,
             form + ": bad argument"),
            (form, "n == 0 with null arrays", (idx, None, None, None, 0, None, None, None, None) + tail, 0, None),
            (form, "accepted", (idx, s["pairs"], s["offsets"], s["offsets"], 3, None, None, s["excl"], s["totals"]) + tail, 0, None),
        ]
        if device:
            rows.append((form, "misaligned pairs", (idx, s["pairs"] + 2, s["offsets"], s["offsets"], 3, None, None, s["excl"], None) + tail,
                         EINVAL, form + ": pairs, call_len and excl must be 4-byte aligned, offsets and totals 8-byte aligned"))
        else:
            rows += [(form, "decreasing offsets", (idx, s["pairs"], s["offsets"], s["offsets_dec"], 3, None, None, s["excl"], None), EINVAL,
                      form + ": " + DECREASING),
                     # (no length limit here: only the differences of the offsets are used)
                     (form, "a read of 1,025 bases", (idx, s["pairs"], s["offsets_long"], s["offsets"], 3, None, None, s["excl"], None), 0, None)]
    return rows


def test_every_form_refuses_what_it_refused_and_says_it_the_same_way(wa, env):
    import torch
    L = wa.lib()
    rows = meth_rows(env) + other_rows(env)
    forms = {r[0] for r in rows}
    assert len(forms) == 18 and all(hasattr(L, f) for f in forms)
    wrong = []
    for form, label, args, status, text in rows:
        rc = getattr(L, form)(*args)
        got = None if rc == 0 else L.walt_last_error().decode()
        print("%s [%s]: %d %r" % (form, label, rc, got))
        if rc != status or got != text:
            wrong.append((form, label, rc, got, status, text))
    torch.cuda.synchronize()
    assert not wrong, "\n".join("%s [%s]: status %d %r, expected %d %r" % w for w in wrong)
    # every kind of refusal met every form it applies to
    assert sum(1 for r in rows if r[3] == 0) >= 2 * len(forms) and sum(1 for r in rows if r[3] != 0) >= 100


@pytest.mark.parametrize("case", ["conversion of read 0 before the length of read 1", "length before conversion, both at read 0",
                                  "order of read 1 before the conversion of read 2"])
def test_several_faults_in_one_batch_report_the_one_they_reported(wa, env, case):
    """walt_meth_call_batch goes read by read: read i's order, then its length, then its conversion byte, before anything
    of read i + 1"""
    b, L = env["batch"], wa.lib()
    conv = np.full(3, ord("T"), dtype=np.uint8)
    if case.startswith("conversion"):
        conv[0], offsets, want = ord("C"), np.array([0, 5, 1030, 1035], dtype=np.uint64), \
            "walt_meth_call_batch: conversion 67 of read 0 is neither 'T' nor 'A'"
    elif case.startswith("length"):
        conv[0], offsets, want = ord("C"), b.host["offsets_long"], TOO_LONG
    else:
        conv[2], offsets, want = ord("C"), np.array([0, 50, 40, 1035], dtype=np.uint64), DECREASING
    rc = L.walt_meth_call_batch(env["idx"], b.h["bases_long"], offsets.ctypes.data, 3, b.h["records"], 16, conv.ctypes.data, 1, 0,
                                None, b.h["calls_long"], b.h["counts"], b.h["stats"])
    print(rc, L.walt_last_error().decode())
    assert rc == EINVAL and L.walt_last_error().decode() == want


SHAPES = ("plain", "skip", "excl", "mbias")
PICKED = {  # which C form each Python method calls, by what the call is composed with
    "Index.meth_call_batch": ("walt_meth_call_batch", "walt_meth_pileup_batch_skip", "walt_meth_pileup_batch_excl",
                              "walt_meth_pileup_batch_mbias"),
    "Pileup.add_batch": ("walt_meth_pileup_batch", "walt_meth_pileup_batch_skip", "walt_meth_pileup_batch_excl",
                         "walt_meth_pileup_batch_mbias"),
    # (a device call on the index with d_skip alone goes to the excl form, one on a pile-up to the skip form)
    "Index.meth_call_batch_device": ("walt_meth_call_batch_device", "walt_meth_pileup_batch_excl_device",
                                     "walt_meth_pileup_batch_excl_device", "walt_meth_pileup_batch_mbias_device"),
    "Pileup.add_batch_device": ("walt_meth_pileup_batch_device", "walt_meth_pileup_batch_skip_device",
                                "walt_meth_pileup_batch_excl_device", "walt_meth_pileup_batch_mbias_device"),
}


@pytest.mark.parametrize("method", sorted(PICKED))
@pytest.mark.parametrize("shape", SHAPES)
def test_python_picks_the_c_form_it_picked(wa, g1_all, env, method, shape):
    """a record stride of 18 is refused by whichever form is called, and the refusal names it"""
    b = env["batch"]
    want = PICKED[method][SHAPES.index(shape)]
    target = g1_all if method.startswith("Index") else env["pile"]
    with pytest.raises(wa.WaltError) as ei:
        if method.endswith("_device"):
            kw = {"skip": dict(d_skip=b.d["skip"]), "excl": dict(d_excl=b.d["excl"]), "mbias": dict(mbias=env["mb"])}.get(shape, {})
            call = target.meth_call_batch_device if target is g1_all else target.add_batch_device
            call(b.d["bases"], b.d["offsets"], 3, b.d["records"], 18, None, 1, "T", None, b.d["calls"], None, None, **kw)
        else:
            raw = np.zeros(2 * 18 + 16, dtype=np.uint8)
            records = np.ndarray(shape=(3,), dtype=wa.best_match_dtype, buffer=raw, strides=(18,))
            kw = {"skip": dict(skip=b.host["skip"]), "excl": dict(excl=b.host["excl"]), "mbias": dict(mbias=env["mb"])}.get(shape, {})
            call = target.meth_call_batch if target is g1_all else target.add_batch
            call(b.host["bases"], b.host["offsets"], records, "T", **kw)
    print(str(ei.value))
    assert ei.value.code == EINVAL and str(ei.value) == "walt_amd error -1: " + want + RECORD_STRIDE % 18
