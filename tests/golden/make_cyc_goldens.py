"""Generator of the wtcyc fixtures and goldens: tests/golden/cyc_*.fa.gz (synthetic, seeded reads) and tests/golden/cyc_manifest.json (per option set: argv,
md5, line count and the text of the -o and -a outputs of the reference's `wtcyc -t 1`).

The reference is compiled WHERE ITS SOURCES LIE (REF, default /root/reference) into a temporary directory outside the repository, with the flags of
oracle/Makefile:12 (REFFLAGS, read from that file); nothing of it is kept.  What the reference does with an empty record is found out here by running it and
recorded in the manifest ("empty_record").

    python tests/golden/make_cyc_goldens.py"""
import gzip
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import cycsets  # noqa: E402

rng = np.random.default_rng(20261020)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rseq(n):
    return rng.integers(0, 4, n).astype(np.uint8)


def rc(s):
    return (3 - s[::-1]).astype(np.uint8)


def mutate(s, rate):
    out, i = [], 0
    while i < len(s):
        r = rng.random()
        if r < rate * 0.3:
            out.append(int(rng.integers(0, 4)))
        elif r < rate * 0.6:
            i += 1
            continue
        elif r < rate:
            out.append((int(s[i]) + 1 + int(rng.integers(0, 3))) % 4)
            i += 1
            continue
        out.append(int(s[i]))
        i += 1
    return np.array(out, dtype=np.uint8)


def text(s, lower=False):
    t = ACGT[np.asarray(s, dtype=np.uint8)].tobytes().decode()
    return t.lower() if lower else t


def hairpin(arm, err, adapter=40):
    s = rseq(arm)
    return np.concatenate([s, rseq(adapter), mutate(rc(s), err)])


def write_fa(path, records, width=0):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        for name, seq in records:
            f.write((">%s\n" % name).encode())
            if width and seq:
                for i in range(0, len(seq), width):
                    f.write((seq[i:i + width] + "\n").encode())
            else:
                f.write((seq + "\n").encode())


def main():
    reads = []
    for k, (arm, err) in enumerate(((300, 0.10), (700, 0.15), (1500, 0.20), (3000, 0.12), (450, 0.18))):
        reads.append(("hairpin_%d_e%d" % (arm, int(err * 100)), text(hairpin(arm, err))))
    reads.append(("plain_2000", text(rseq(2000))))
    reads.append(("short_63", text(rseq(63))))
    reads.append(("empty", ""))
    reads.append(("hairpin_lower_600", text(hairpin(600, 0.12), lower=True)))
    reads.append(("short_20", text(rseq(20))))
    # a palindrome in the middle of a read: the hit touches neither end (no -o line whatever the score)
    mid = hairpin(500, 0.10)
    reads.append(("inner_hit", text(np.concatenate([rseq(900), mid, rseq(1400)]))))
    reads.append(("plain_5000 with a description", text(rseq(5000))))
    s = hairpin(900, 0.15)
    reads.append(("hairpin_mixed_case", "".join(c.lower() if i % 3 == 0 else c for i, c in enumerate(text(s)))))
    reads.append(("hairpin_offset_1200", text(np.concatenate([hairpin(1200, 0.14), rseq(30)]))))
    write_fa(os.path.join(HERE, "cyc_reads.fa.gz"), reads, width=0)
    write_fa(os.path.join(HERE, "cyc_wrapped.fa.gz"), reads[:3], width=70)
    write_fa(os.path.join(HERE, "cyc_too_long.fa.gz"), [("ok_1", text(hairpin(300, 0.1))), ("too_long", text(rseq(65536))), ("ok_2", text(rseq(100)))])
    write_fa(os.path.join(HERE, "cyc_non_acgt.fa.gz"), [("ok_1", text(hairpin(300, 0.1))), ("has_N", text(rseq(200)) + "N" + text(rseq(200)))])

    flags = None
    for line in open(os.path.join(ROOT, "oracle", "Makefile")):
        m = re.match(r"REFFLAGS\s*=\s*(.*)", line)
        if m:
            flags = m.group(1).split()
    assert flags, "REFFLAGS not found in oracle/Makefile"
    td = tempfile.mkdtemp(prefix="cycref_")
    assert not os.path.abspath(td).startswith(ROOT + os.sep)
    try:
        exe = os.path.join(td, "wtcyc")
        subprocess.run(["gcc"] + flags + ["-o", exe] + [os.path.join(REF, f) for f in ("file_reader.c", "ksw.c", "wtcyc.c")] + ["-lm", "-lpthread"], check=True)
        man = {"reference": "wtcyc -t 1, compiled with the flags of oracle/Makefile:12", "cases": {}}
        for name, (inp, argv) in cycsets.SETS.items():
            got = cycsets.run(exe, ["-t", "1"], os.path.join(HERE, inp), argv, td)
            assert got["rc"] == 0, (name, got)
            man["cases"][name] = {"input": inp, "argv": argv,
                                  "o_md5": hashlib.md5(got["o"]).hexdigest(), "o_lines": got["o"].count(b"\n"), "o_text": got["o"].decode(),
                                  "a_md5": hashlib.md5(got["a"]).hexdigest(), "a_lines": got["a"].count(b"\n"), "a_text": got["a"].decode()}
            print("%-12s -o %3d lines  -a %3d lines" % (name, man["cases"][name]["o_lines"], man["cases"][name]["a_lines"]))
        a = man["cases"]["defaults"]["a_text"].splitlines()
        empty = [ln for ln in a if ln.startswith("empty\t")]
        assert empty == ["empty\t0\t0\t0.000\t0\t0\t0\t0"], empty
        man["empty_record"] = "the reference writes the -a line of a read without a hit (KSWX_NULL): '%s'; no -o line, exit status 0" % empty[0].replace("\t", " ")
        assert any(c["o_lines"] for c in man["cases"].values())
        with open(os.path.join(HERE, "cyc_manifest.json"), "w") as f:
            json.dump(man, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(td)


if __name__ == "__main__":
    main()
