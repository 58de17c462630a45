"""The driver that halves a block on WTZ_E_POOL (ht_halving, smartdenovo_amd/csrc/host/wtz_tool.h) under wtcyc, pairaln and wtext, on the host emulation of the
device library.  --pool-mb (a test hook no usage text names) gives the context a pool of whole MiB; the main pool is half of it.  Needs no GPU.

(a) a pool too small for one item ends the run with status 1, the tool's own text and no output;
(b) a pool in which the whole block fails with WTZ_E_POOL and its halves succeed gives the golden's bytes.

What the fixtures reach (found on the emulation with a print in the driver's halving branch that is not committed):
  wtcyc, cyc_reads.fa.gz: (a) up to 12 MiB (the trace of the 6 043-base read needs 6 236 416 bytes of the main pool); from 13 MiB on no call fails.  (b) is out
      of reach: the only request of wtz_alignx_batch that is summed over the call is the strip boundaries of K-local, 8 bytes per base of a read of more than
      1 024 bases (about 200 KB for the whole file), and the global stage cuts its own launch groups, so a call only fails where one read alone does.
  pairaln -a: pairaln_pairs.fa.gz (records of at most 404 bases) fits a 1 MiB pool, the smallest the hook can ask for, without a failing call, so neither (a)
      nor (b) is in reach with it; (a) is reached with pairaln_long.fa.gz.  That file is ONE pair: the first call is the call of one item and the run ends
      without a halving.  (b) is out of reach for the reason above, and wtz_pwtext_batch cuts its launch groups by the same budget it refuses a single picture
      by.  So NO committed test reaches what pairaln does after a halving (the CIGAR offsets moved behind those of the part before in pa_align, a part's own
      stretch of the text buffer in pa_render); the block tests with --block-bytes reach the same code with step == m only.
  wtext, case dmo_hard (72 extensions in one block): (a) at 1 MiB; at 2 .. 14 MiB the call over all 72 fails ("ran out of scratch") and the run completes on
      halves, from 15 MiB on no call fails.  (b) runs at 14 MiB: one halving, 72 -> 36 + 36, seen in the print."""
import os

import pytest

import cycsets
import emultools
import pairalnsets
from test_pairaln import MAN as PAIRALN_MAN
from test_wtext import ext_cmd, overlap_inputs, run_ext

GIVE_UP = "scratch pool too small even for one %s: "


@pytest.fixture(scope="module")
def wtcyc():
    return emultools.build("wtcyc")


@pytest.fixture(scope="module")
def pairaln():
    return emultools.build("pairaln")


@pytest.fixture(scope="module")
def wtext():
    return emultools.build("wtext")


def test_wtcyc_gives_up_at_one_read(wtcyc, tmp_path):
    got = cycsets.run(wtcyc, ["--pool-mb", "1"], os.path.join(cycsets.GOLDEN, "cyc_reads.fa.gz"), ["-o", "{o}", "-a", "{a}"], str(tmp_path))
    assert got["rc"] == 1 and GIVE_UP % "read" in got["err"] and got["err"].endswith(" (use --pool-gb) --\n")
    assert got["a"] == b"" and got["o"] == b""


def test_pairaln_gives_up_at_one_pair(pairaln):
    got = pairalnsets.run(pairaln, ["--pool-mb", "1"], ["pairaln_long.fa.gz"], ["-a"])
    assert got["rc"] == 1 and GIVE_UP % "pair" in got["err"] and got["err"].endswith(" (use --pool-gb) --\n")
    assert got["out"] == b""


def test_pairaln_small_records_fit_the_smallest_pool(pairaln):
    got = pairalnsets.run(pairaln, ["--pool-mb", "1"], ["pairaln_pairs.fa.gz"], ["-a"])
    assert got["rc"] == 0 and got["out"].decode() == PAIRALN_MAN["cases"]["a"]["stdout"]


def test_wtext_gives_up_at_one_extension(wtext, oracle_exe, tmp_path_factory, tmp_path):
    out = os.path.join(str(tmp_path), "x.ovl")
    r = ext_cmd(wtext, "dmo_hard", overlap_inputs(oracle_exe, tmp_path_factory, "ora"), out, ["--pool-mb", "1"])
    err = r.stderr.decode()
    assert r.returncode == 1 and GIVE_UP % "extension" in err and "--pool-gb" not in err and err.endswith(" --\n")
    assert open(out, "rb").read() == b""


def test_wtext_halves_a_block_and_writes_the_same_bytes(wtext, oracle_exe, tmp_path_factory, tmp_path):
    """14 MiB: the largest pool (of whole MiB) at which the one call over dmo_hard's 72 extensions fails and its halves succeed"""
    run_ext(wtext, "dmo_hard", overlap_inputs(oracle_exe, tmp_path_factory, "ora"), tmp_path, ["--pool-mb", "14"])
