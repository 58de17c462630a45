"""bench.py without a GPU: its read-set generator writes the bytes of smartdenovo_amd/synth.py (the goldens of big_manifest.json pin the md5 of those bytes),
--dump-outputs turns an .ovl and its .contained into the arrays it promises, and the plain / --full options are there."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench
from smartdenovo_amd import synth


@pytest.mark.parametrize("genome,coverage,seed", [(200000, 20.0, 3), (1500, 3.0, 1), (50001, 4.0, 11)])
def test_generator_writes_the_bytes_of_synth(tmp_path, genome, coverage, seed):
    """1500 bp: the genome draw leaves half of a 64-bit draw buffered; 200 kb: several stream windows"""
    names, seqs = synth.synth_reads(genome, coverage, seed=seed)
    md5 = synth.write_fasta(str(tmp_path / "ref.fa"), names, seqs)
    reads, bases, got = bench.synth_fasta(str(tmp_path / "fast.fa"), genome, coverage, seed, threads=3)
    assert (reads, bases, got) == (len(names), int(sum(s.size for s in seqs)), md5)
    assert hashlib.md5(open(str(tmp_path / "fast.fa"), "rb").read()).hexdigest() == md5


def test_dump_outputs_reads_back_the_ovl(tmp_path):
    recs = [("pb000000000106", "+", 19843, 0, 16066, "pb000000000016", "-", 16554, 538, 16554, 12565, "0.750", 13432, 742, 1842, 1892, "7M1D2M2I8M"),
            ("pb000000000007", "-", 9000, 10, 8000, "pb000000000106", "+", 19843, 0, 7990, 6000, "0.812", 7000, 300, 120, 130, "12M3D")]
    ovl = tmp_path / "o.ovl"
    ovl.write_bytes(b"".join(("\t".join(str(x) for x in r) + "\n").encode() for r in recs))
    (tmp_path / "o.ovl.contained").write_bytes(b"pb000000000007\npb000000000042\n")
    d = tmp_path / "dump"
    assert bench.dump_outputs(str(d), str(ovl)) == 2
    got = {f: np.load(str(d / f)) for f in os.listdir(str(d))}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    rec = got["ovl_records.npy"]
    assert rec.dtype == np.float32 and rec.shape == (2, 16)
    assert rec[0].tolist()[:11] == [106, 0, 19843, 0, 16066, 16, 1, 16554, 538, 16554, 12565] and abs(rec[0, 11] - 0.75) < 1e-6
    assert rec[1, 0] == 7 and rec[1, 1] == 1 and rec[1, 15] == 130
    assert got["ovl_rows.npy"].tolist() == [0, 1]
    import zlib
    assert got["ovl_cigar.npy"].tolist() == [[10, zlib.crc32(b"7M1D2M2I8M")], [5, zlib.crc32(b"12M3D")]]
    assert got["ovl_cigar_ops.npy"].tolist() == [[0, 17, 2, 1, 5], [1, 12, 0, 3, 2]]
    assert got["contained.npy"].tolist() == [7, 42]


def test_dump_outputs_samples_a_large_output_the_same_way(tmp_path):
    ovl = tmp_path / "o.ovl"
    ovl.write_bytes(b"".join(b"pb%012d\t+\t100\t0\t90\tpb%012d\t+\t100\t5\t95\t80\t0.900\t85\t5\t1\t2\t%dM\n" % (i, i + 1, i + 1) for i in range(50)))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), str(ovl), max_rows=7, cigar_sample=4)
    bench.dump_outputs(str(b), str(ovl), max_rows=7, cigar_sample=4)
    for f in ("ovl_records.npy", "ovl_cigar.npy", "ovl_rows.npy", "ovl_cigar_ops.npy", "contained.npy"):
        assert np.array_equal(np.load(str(a / f)), np.load(str(b / f)))
    rows = np.load(str(a / "ovl_rows.npy")).astype(int)
    assert len(rows) == 7 and list(rows) == sorted(set(rows))
    assert np.load(str(a / "ovl_records.npy"))[:, 0].tolist() == rows.tolist()
    assert np.load(str(a / "ovl_cigar_ops.npy")).shape == (4, 5)


def test_plain_and_full_runs_are_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, timeout=120)
    assert r.returncode == 0
    h = r.stdout.decode()
    assert "--full" in h and "--dump-outputs" in h and "--steps" in h
