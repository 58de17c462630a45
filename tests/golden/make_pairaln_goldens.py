"""Generator of the pairaln fixtures and goldens: tests/golden/pairaln_*.fa.gz / .fq.gz (synthetic, seeded records) and tests/golden/pairaln_manifest.json
(per option set: inputs, argv, md5, line count and the text of what the reference's `pairaln` wrote to standard output).

The reference is compiled WHERE ITS SOURCES LIE (REF, default /root/reference) into a temporary directory outside the repository, with the flags of
oracle/Makefile (REFFLAGS, read from that file); nothing of it is kept.  What the reference does with an empty record is found out here by running it and
recorded in the manifest ("empty_record").

    python tests/golden/make_pairaln_goldens.py"""
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
import pairalnsets  # noqa: E402

SEED = int(os.environ.get("PAIRALN_SEED", "20261024"))
rng = np.random.default_rng(SEED)
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


def mixed(t):
    return "".join(c.lower() if i % 3 == 0 else c for i, c in enumerate(t))


def write(path, records, width=0, fastq=False):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        for name, seq in records:
            if fastq:
                f.write(("@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq))).encode())
                continue
            f.write((">%s\n" % name).encode())
            if width and seq:
                for i in range(0, len(seq), width):
                    f.write((seq[i:i + width] + "\n").encode())
            else:
                f.write((seq + "\n").encode())


def pairs():
    """the pairs of the main file: short, so that the pictures of the -a sets stay a few kilobytes each"""
    P = []
    a = rseq(200)
    P += [("similar_200_q", text(a)), ("similar_200_t", text(mutate(a, 0.12)))]
    P += [("nohit_q", text(np.zeros(80, dtype=np.uint8))), ("nohit_t", text(np.ones(90, dtype=np.uint8)))]      # all A against all C: no positive cell
    a = rseq(250)
    P += [("minus_only_q", text(a)), ("minus_only_t", text(rc(mutate(a, 0.10))))]
    a = rseq(150)
    P += [("inner_q", text(np.concatenate([rseq(100), a, rseq(80)]))), ("inner_t", text(np.concatenate([rseq(60), mutate(a, 0.08), rseq(140)])))]
    a, b = rseq(130), rseq(140)
    P += [("long_ins_q", text(np.concatenate([a, rseq(75), b]))), ("long_ins_t", text(np.concatenate([mutate(a, 0.05), mutate(b, 0.05)])))]
    a, b = rseq(140), rseq(120)
    P += [("long_del_q", text(np.concatenate([mutate(a, 0.05), mutate(b, 0.05)]))), ("long_del_t", text(np.concatenate([a, rseq(70), b])))]
    a = rseq(150)
    P += [("lower_q", text(a, lower=True)), ("lower_t", text(mutate(a, 0.15), lower=True))]
    a = rseq(180)
    P += [("mixed_q with a description", mixed(text(a))), ("mixed_t\tdescribed too", mixed(text(mutate(a, 0.18))))]
    a = rseq(60)
    P += [("short_60_q", text(a)), ("short_60_t", text(mutate(a, 0.05)))]
    a = rseq(400)
    P += [("contained_q", text(a[100:260])), ("contained_t", text(mutate(a, 0.10)))]
    return P


def long_pairs():
    """the one long pair: its picture spans 25 tiles of the renderer"""
    a = rseq(12000)
    return [("long_12000_q", text(a)), ("long_12000_t", text(mutate(a, 0.15)))]


def main():
    P = pairs()
    write(os.path.join(HERE, "pairaln_pairs.fa.gz"), P)
    write(os.path.join(HERE, "pairaln_long.fa.gz"), long_pairs())
    write(os.path.join(HERE, "pairaln_wrapped.fa.gz"), P[:10], width=70)
    write(os.path.join(HERE, "pairaln_pairs.fq.gz"), P[:8] + P[12:16], fastq=True)
    write(os.path.join(HERE, "pairaln_odd.fa.gz"), P[4:8] + P[16:19])
    write(os.path.join(HERE, "pairaln_too_long.fa.gz"), P[:2] + [("ok_q", text(rseq(100))), ("too_long", text(rseq(65536)))])
    a = rseq(300)
    write(os.path.join(HERE, "pairaln_non_acgt.fa.gz"), P[:2] + [("has_N", text(a[:150]) + "N" + text(a[150:])), ("ok_t", text(mutate(a, 0.1)))])
    write(os.path.join(HERE, "pairaln_empty.fa.gz"), P[:2] + [("empty", ""), ("after_empty", text(rseq(100)))])

    flags = None
    for line in open(os.path.join(ROOT, "oracle", "Makefile")):
        m = re.match(r"REFFLAGS\s*=\s*(.*)", line)
        if m:
            flags = m.group(1).split()
    assert flags, "REFFLAGS not found in oracle/Makefile"
    td = tempfile.mkdtemp(prefix="pairalnref_")
    assert not os.path.abspath(td).startswith(ROOT + os.sep)
    try:
        exe = os.path.join(td, "pairaln")
        subprocess.run(["gcc"] + flags + ["-o", exe] + [os.path.join(REF, f) for f in ("file_reader.c", "ksw.c", "pairaln.c")] + ["-lm", "-lpthread"], check=True)
        man = {"reference": "pairaln, compiled with the flags of oracle/Makefile (REFFLAGS)", "cases": {}}
        seen = set()
        for name, (inputs, argv, stdin) in pairalnsets.SETS.items():
            got = pairalnsets.run(exe, [], inputs, argv, stdin)
            assert got["rc"] == 0, (name, got["rc"], got["err"])
            out = got["out"]
            # a hit whose extended rectangle lies off the diagonal by more than the band of kswx.h:1452-1461: ksw_global2 returns MINUS_INF and walks back through
            # bytes it never wrote.  What the reference prints there is not defined, so no fixture may hold such a pair (the seed is chosen accordingly)
            assert b"-1073741824" not in out, (name, [ln for ln in out.decode().splitlines() if "-1073741824" in ln])
            man["cases"][name] = {"inputs": inputs, "argv": argv, "stdin": stdin, "md5": hashlib.md5(out).hexdigest(), "lines": out.count(b"\n"), "stdout": out.decode()}
            print("%-10s %4d lines %8d bytes" % (name, out.count(b"\n"), len(out)))
            if "-a" in argv:
                lines = out.decode().split("\n")
                for k in range(0, len(lines) - 3, 4):
                    a, m, b = lines[k + 1:k + 4]
                    seen |= set(m)
                    if "-" * 65 in a:
                        seen.add("long gap in the query line")
                    if "-" * 65 in b:
                        seen.add("long gap in the target line")
        assert {"|", "*", "-", "long gap in the query line", "long gap in the target line"} <= seen, seen
        d = man["cases"]["s"]["stdout"].splitlines()
        nohit = [ln for ln in d if ln.startswith("nohit_q\t")]
        assert len(nohit) == 2 and nohit[0].split("\t")[10] == "0", nohit
        man["no_hit"] = nohit[0]
        minus = [ln.split("\t") for ln in d if ln.startswith("minus_only_q\t")]
        assert int(minus[0][10]) < 100 < int(minus[1][10]) and minus[1][6] == "-", minus
        # with the default T = -100 the extensions run to the reads' ends through unrelated sequence; the hit alone (-T 0) starts and ends inside both reads
        inner = [ln.split("\t") for ln in man["cases"]["T0_a"]["stdout"].splitlines() if ln.startswith("inner_q\t")][0]
        assert 0 < int(inner[3]) and int(inner[4]) < int(inner[2]) and 0 < int(inner[8]) and int(inner[9]) < int(inner[7]), inner
        r = subprocess.run([exe, "-a", os.path.join(HERE, "pairaln_empty.fa.gz")], capture_output=True)
        if r.returncode == 0:
            ln = [x for x in r.stdout.decode().split("\n") if x.startswith("empty\t")]
            man["empty_record"] = {"defined": True, "exit_status": 0, "line": ln[0] if ln else None, "stdout": r.stdout.decode()}
        else:
            man["empty_record"] = {"defined": False, "exit_status": r.returncode, "stderr_tail": r.stderr.decode(errors="replace")[-200:],
                                   "note": "the reference does not survive an empty record: pairaln of this project refuses it like a character outside ACGTacgt"}
        print("empty record:", {k: v for k, v in man["empty_record"].items() if k != "stdout"})
        with open(os.path.join(HERE, "pairaln_manifest.json"), "w") as f:
            json.dump(man, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(td)


if __name__ == "__main__":
    main()
