"""bin/wtcyc on the GPU: every option set of tests/golden/cyc_manifest.json byte for byte against what the reference's `wtcyc -t 1` wrote, one set again with a
block budget that cuts the input into more than three blocks, and the routes that end a run.  Reads nothing of the reference's tree."""
import os
import subprocess

import pytest

import cycsets
from test_wtcyc import MAN, check_case

pytestmark = pytest.mark.gpu
EXE = os.path.join(cycsets.ROOT, "bin", "wtcyc")
EXTRA = ["--gpu", "0", "--pool-gb", "2"]


@pytest.fixture(scope="module")
def exe():
    assert os.path.exists(EXE), "bin/wtcyc is not built: run build()"
    return EXE


@pytest.mark.parametrize("name", sorted(cycsets.SETS))
def test_every_set_is_byte_identical_to_the_reference(exe, name, tmp_path):
    check_case(exe, EXTRA, name, str(tmp_path))


def test_three_blocks_give_the_same_bytes(exe, tmp_path):
    check_case(exe, EXTRA + ["--block-bytes", "9000"], "defaults", str(tmp_path))


def test_runs_that_end_early(exe, tmp_path):
    for inp, word in (("cyc_too_long.fa.gz", "too_long"), ("cyc_non_acgt.fa.gz", "has_N")):
        got = cycsets.run(exe, EXTRA, os.path.join(cycsets.GOLDEN, inp), ["-o", "{o}", "-a", "{a}"], str(tmp_path), tag=word)
        assert got["rc"] == 1 and word in got["err"] and got["a"] == b"" and got["o"] == b""
    keep = tmp_path / "keep"
    keep.write_text("mine\n")
    r = subprocess.run([exe] + EXTRA + ["-o", str(keep), os.path.join(cycsets.GOLDEN, "cyc_wrapped.fa.gz")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("File exists! '%s'\n\n" % keep) and keep.read_text() == "mine\n"
    assert MAN["cases"]["wrapped"]["o_lines"] == 3


def test_a_pool_too_small_for_one_read_ends_the_run(exe, tmp_path):
    """--pool-mb 1 (tests/test_halving.py): the call is halved down to one read and the run ends; the fixture has no pool at which halves succeed"""
    got = cycsets.run(exe, ["--gpu", "0", "--pool-mb", "1"], os.path.join(cycsets.GOLDEN, "cyc_reads.fa.gz"), ["-o", "{o}", "-a", "{a}"], str(tmp_path))
    assert got["rc"] == 1 and "scratch pool too small even for one read: " in got["err"] and got["err"].endswith(" (use --pool-gb) --\n")
    assert got["a"] == b"" and got["o"] == b""
