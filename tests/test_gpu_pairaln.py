"""bin/pairaln on the GPU: every option set of tests/golden/pairaln_manifest.json byte for byte against what the reference's pairaln wrote, two sets again with a
block budget that puts every pair into a block of its own, and the routes that end a run.  Reads nothing of the reference's tree."""
import os

import pytest

import pairalnsets
from test_pairaln import MAN, check_case

pytestmark = pytest.mark.gpu
EXE = os.path.join(pairalnsets.ROOT, "bin", "pairaln")
EXTRA = ["--gpu", "0", "--pool-gb", "2"]


@pytest.fixture(scope="module")
def exe():
    assert os.path.exists(EXE), "bin/pairaln is not built: run build()"
    return EXE


@pytest.mark.parametrize("name", sorted(pairalnsets.SETS))
def test_every_set_is_byte_identical_to_the_reference(exe, name):
    check_case(exe, EXTRA, name)


def test_small_blocks_give_the_same_bytes(exe):
    check_case(exe, EXTRA + ["--block-bytes", "700"], "s_a")


def test_runs_that_end_early(exe):
    for inp, word in (("pairaln_too_long.fa.gz", "too_long"), ("pairaln_non_acgt.fa.gz", "has_N")):
        got = pairalnsets.run(exe, EXTRA, [inp], ["-a"])
        assert got["rc"] == 1 and word in got["err"] and got["out"] == b""
    got = pairalnsets.run(exe, EXTRA, ["pairaln_wrapped.fa.gz"], ["-W", "2000"])
    assert got["rc"] == 1 and "-W 2000" in got["err"] and got["out"] == b""
    got = pairalnsets.run(exe, EXTRA, ["pairaln_empty.fa.gz"], ["-a"])
    assert got["rc"] == 0 and got["out"].decode() == MAN["empty_record"]["stdout"]


def test_a_pool_too_small_for_one_pair_ends_the_run(exe):
    """--pool-mb 1 (tests/test_halving.py): the file is one pair, so the first call is the call of one item and the run ends there, without a halving; the
    fixtures have no pool at which a call fails and its halves succeed"""
    got = pairalnsets.run(exe, ["--gpu", "0", "--pool-mb", "1"], ["pairaln_long.fa.gz"], ["-a"])
    assert got["rc"] == 1 and "scratch pool too small even for one pair: " in got["err"] and got["err"].endswith(" (use --pool-gb) --\n")
    assert got["out"] == b""
    got = pairalnsets.run(exe, ["--gpu", "0", "--pool-mb", "1"], ["pairaln_pairs.fa.gz"], ["-a"])
    assert got["rc"] == 0 and got["out"].decode() == MAN["cases"]["a"]["stdout"]
