#!/usr/bin/env python3
"""Record what the REAL reference binary (oracle/_ref/{makedb,walt}, built by oracle/Makefile.ref) writes for the
inputs of the tests that compare with it, so that those tests need no reference binary: tests/golden/refbin.json.
Run where oracle/_ref/ is built (no GPU needed).  Commits DATA only:
  awkward    : per test_gpu_cli.py awkward case (mode, -N/-sam/-A, threads), md5 and size of every output file
  clip_short : per read of test_hostio_cpu.py's short clipped reads, the sequence the reference reports after -C
               clipping and N replacement; and the exit status of the reference on reads of fewer than 13 bases
It also checks that the reference's -sam -a -u output on se_ct.fastq is golden case se_sam_au."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)

import refio  # noqa: E402
from test_gpu_cli import AWKWARD_CASES, awkward_run  # noqa: E402
from test_hostio_cpu import CLIP_ADAPTOR, CLIP_TINY, clip_short_records  # noqa: E402


def clip_short(wd, index):
    recs = clip_short_records()
    fq = os.path.join(wd, "clip_short.fastq")
    with open(fq, "w") as f:
        for nm, sq in recs:
            f.write("@%s\n%s\n+\n%s\n" % (nm, sq, "I" * len(sq)))
    out = os.path.join(wd, "o.mr")
    subprocess.run([refio.REF_WALT, "-i", index, "-r", fq, "-o", out, "-C", CLIP_ADAPTOR, "-u", "-a", "-m", "0"],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ref_seq = {}
    for side in ("_unmapped", "_ambiguous", ""):
        for ln in open(out + side):
            f = ln.rstrip("\n").split("\t")
            if side == "_unmapped":
                ref_seq[f[0]] = f[1]
            else:
                ref_seq[f[3]] = f[6] if f[5] == "+" else refio.revcomp(f[6])
    fq2 = os.path.join(wd, "clip_tiny.fastq")
    with open(fq2, "w") as f:
        f.write(CLIP_TINY)
    r = subprocess.run([refio.REF_WALT, "-i", index, "-r", fq2, "-o", os.path.join(wd, "t.mr"), "-C", CLIP_ADAPTOR, "-u"],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return {"ref_seq": ref_seq, "tiny_reference_exit_status": r.returncode}


def main():
    if not (os.path.exists(refio.REF_WALT) and os.path.exists(refio.REF_MAKEDB)):
        sys.exit("build oracle/_ref first: make -f oracle/Makefile.ref")
    with tempfile.TemporaryDirectory(prefix="refbin_") as wd:
        index = os.path.join(wd, "g1.dbindex")
        subprocess.run([refio.REF_MAKEDB, "-c", os.path.join(HERE, "g1.fa"), "-o", index], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        awkward = {}
        for mode, extra in AWKWARD_CASES:
            for threads in ("1", "6"):
                tag, outs = awkward_run(refio.REF_WALT, index, wd, mode, extra, threads)
                awkward[tag] = {fn: [hashlib.md5(b).hexdigest(), len(b)] for fn, b in outs.items()}
        sam = os.path.join(wd, "se.sam")
        subprocess.run([refio.REF_WALT, "-i", index, "-r", os.path.join(HERE, "se_ct.fastq"), "-o", sam, "-sam", "-a", "-u"],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        assert open(sam).read() == refio.golden_file("se_sam_au", "out.sam"), "golden case se_sam_au is stale"
        res = {"awkward": awkward, "clip_short": clip_short(wd, index)}
    out = os.path.join(HERE, "refbin.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
