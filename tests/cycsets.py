"""The option sets of the wtcyc goldens (tests/golden/make_cyc_goldens.py, tests/test_wtcyc.py, tests/test_gpu_wtcyc.py) and the one way they are run.

An argv is a template: {o} / {a} are files in the run's own directory, a "-" is standard output; where a set does not name -o, the regions go to standard
output too (the tool's default)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SETS = {
    "defaults":    ("cyc_reads.fa.gz", ["-a", "{a}"]),
    "W50":         ("cyc_reads.fa.gz", ["-W", "50", "-fo", "{o}", "-a", "{a}"]),
    "T0":          ("cyc_reads.fa.gz", ["-T", "0", "-o", "{o}", "-a", "{a}"]),
    "T-30":        ("cyc_reads.fa.gz", ["-T", "-30", "-o", "{o}", "-a", "{a}"]),
    "s100_m0.5":   ("cyc_reads.fa.gz", ["-s", "100", "-m", "0.5", "-o", "{o}", "-a", "{a}"]),
    "scores":      ("cyc_reads.fa.gz", ["-M", "1", "-X", "-3", "-O", "-2", "-E", "-2", "-o", "{o}", "-a", "{a}"]),
    "P2_p1":       ("cyc_reads.fa.gz", ["-P", "2", "-p", "1", "-o", "{o}", "-a", "{a}"]),
    "a_stdout":    ("cyc_reads.fa.gz", ["-a", "-", "-o", "{o}"]),
    "wrapped":     ("cyc_wrapped.fa.gz", ["-o", "{o}", "-a", "{a}"]),
}


def run(exe, extra, inp, argv, workdir, tag="run"):
    """one run: {"rc", "o", "a", "err"}; -o / -a as bytes, wherever the set sends them"""
    o, a = os.path.join(workdir, tag + ".o"), os.path.join(workdir, tag + ".a")
    for f in (o, a):
        if os.path.exists(f):
            os.remove(f)
    args = [x.format(o=o, a=a) for x in argv]
    r = subprocess.run([exe] + extra + args + [inp], capture_output=True)
    out = {"rc": r.returncode, "err": r.stderr.decode(errors="replace")}
    a_stdout = any(args[i] == "-a" and args[i + 1] == "-" for i in range(len(args) - 1))
    o_file = any(x in ("-o", "-fo") for x in args)
    out["o"] = open(o, "rb").read() if o_file and os.path.exists(o) else (b"" if o_file or a_stdout else r.stdout)
    out["a"] = r.stdout if a_stdout else (open(a, "rb").read() if os.path.exists(a) else b"")
    return out
