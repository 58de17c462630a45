"""The option sets of the pairaln goldens (tests/golden/make_pairaln_goldens.py, tests/test_pairaln.py, tests/test_gpu_pairaln.py) and the one way they are run.

A set is (inputs, argv, stdin): the input files are arguments, or, where stdin is True, the one input is piped in (the files are gzip: piped decompressed)."""
import gzip
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SETS = {
    "defaults":  (["pairaln_pairs.fa.gz"], [], False),
    "s":         (["pairaln_pairs.fa.gz"], ["-s"], False),
    "a":         (["pairaln_pairs.fa.gz"], ["-a"], False),
    "s_a":       (["pairaln_pairs.fa.gz"], ["-s", "-a"], False),
    "T0_a":      (["pairaln_pairs.fa.gz"], ["-T", "0", "-a"], False),
    "W100_a":    (["pairaln_pairs.fa.gz"], ["-W", "100", "-a"], False),
    "scores_a":  (["pairaln_pairs.fa.gz"], ["-M", "1", "-X", "-3", "-O", "-2", "-E", "-2", "-a"], False),
    "T-30_s":    (["pairaln_pairs.fa.gz"], ["-T", "-30", "-s"], False),
    "stdin":     (["pairaln_pairs.fa.gz"], [], True),
    "wrapped":   (["pairaln_wrapped.fa.gz"], ["-s"], False),
    "fastq":     (["pairaln_pairs.fq.gz"], [], False),
    "odd_s":     (["pairaln_odd.fa.gz"], ["-s"], False),
    "two_files": (["pairaln_wrapped.fa.gz", "pairaln_odd.fa.gz"], [], False),
    "long_a":    (["pairaln_long.fa.gz"], ["-a"], False),
}


def run(exe, extra, inputs, argv, stdin=False):
    """one run: {"rc", "out", "err"}"""
    paths = [os.path.join(GOLDEN, f) for f in inputs]
    if stdin:
        r = subprocess.run([exe] + extra + argv, input=gzip.open(paths[0], "rb").read(), capture_output=True)
    else:
        r = subprocess.run([exe] + extra + argv + paths, stdin=subprocess.DEVNULL, capture_output=True)
    return {"rc": r.returncode, "out": r.stdout, "err": r.stderr.decode(errors="replace")}
