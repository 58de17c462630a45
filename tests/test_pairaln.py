"""The drop-in pairaln (smartdenovo_amd/csrc/host/pairaln_main.c) on the host emulation of the device library: every option set of
tests/golden/pairaln_manifest.json byte for byte against what the reference's pairaln wrote (tests/golden/make_pairaln_goldens.py), and the routes that end a
run.  Needs no GPU."""
import hashlib
import json
import os
import subprocess

import pytest

import emultools
import pairalnsets

ROOT = pairalnsets.ROOT
MAN = json.load(open(os.path.join(pairalnsets.GOLDEN, "pairaln_manifest.json")))
EXTRA = ["--pool-gb", "1"]


@pytest.fixture(scope="module")
def exe():
    """pairaln_emul: the same main against the libwtz_emul.so that tests/emul/build_emul.sh produces"""
    return emultools.build("pairaln")


def check_case(exe, extra, name):
    case = MAN["cases"][name]
    got = pairalnsets.run(exe, extra, case["inputs"], case["argv"], case["stdin"])
    assert got["rc"] == 0, got["err"]
    assert got["out"].decode() == case["stdout"]
    assert hashlib.md5(got["out"]).hexdigest() == case["md5"] and got["out"].count(b"\n") == case["lines"]


def test_manifest_holds_the_sets_and_the_content_the_feature_names():
    assert set(pairalnsets.SETS) == set(MAN["cases"]) and len(MAN["cases"]) >= 12
    for name, (inputs, argv, stdin) in pairalnsets.SETS.items():
        c = MAN["cases"][name]
        assert c["argv"] == argv and c["inputs"] == inputs and c["stdin"] == stdin
    assert MAN["no_hit"].split("\t")[10:] == ["0", "-nan", "0", "0", "0", "0"]
    assert MAN["empty_record"]["defined"] and MAN["empty_record"]["line"].split("\t")[10:] == ["0", "-nan", "0", "0", "0", "0"]
    s = [ln.split("\t") for ln in MAN["cases"]["s"]["stdout"].splitlines()]
    assert [ln[6] for ln in s] == ["+", "-"] * 10      # both strands of a pair adjacent
    minus = [ln for ln in s if ln[0] == "minus_only_q"]
    assert int(minus[0][10]) < 100 < int(minus[1][10])
    pics = MAN["cases"]["a"]["stdout"].split("\n")
    assert any("-" * 65 in pics[k + 1] for k in range(0, 40, 4)) and any("-" * 65 in pics[k + 3] for k in range(0, 40, 4))
    assert any("mixed_q\t" in ln and "\tmixed_t\t" in ln for ln in pics)      # the descriptions are not part of the names
    assert MAN["cases"]["odd_s"]["lines"] == 3 * 2      # seven records: three pairs
    assert max(len(ln) for ln in MAN["cases"]["long_a"]["stdout"].split("\n")) > 12000


@pytest.mark.parametrize("name", sorted(pairalnsets.SETS))
def test_every_set_is_byte_identical_to_the_reference(exe, name):
    check_case(exe, EXTRA, name)


@pytest.mark.parametrize("name", ["s_a", "two_files"])
def test_small_blocks_give_the_same_bytes(exe, name):
    """a byte budget of 700 bases: nearly every pair is a block of its own"""
    check_case(exe, EXTRA + ["--block-bytes", "700"], name)


def test_an_empty_record_gives_the_reference_s_lines(exe):
    got = pairalnsets.run(exe, EXTRA, ["pairaln_empty.fa.gz"], ["-a"])
    assert got["rc"] == 0 and got["out"].decode() == MAN["empty_record"]["stdout"]
    assert got["out"].endswith(MAN["empty_record"]["line"].encode() + b"\n\n\n\n")


@pytest.mark.parametrize("inp,word,text", [("pairaln_too_long.fa.gz", "too_long", "65536"), ("pairaln_non_acgt.fa.gz", "has_N", "ACGTacgt")])
def test_records_the_tool_refuses_end_the_run_without_a_partial_block(exe, inp, word, text):
    got = pairalnsets.run(exe, EXTRA, [inp], ["-a"])
    assert got["rc"] == 1 and word in got["err"] and text in got["err"]
    assert got["out"] == b""      # the first pair of the file is in the refused record's block: nothing of it is written
    got = pairalnsets.run(exe, EXTRA + ["--block-bytes", "1000"], [inp], [])
    assert got["rc"] == 1 and got["out"] == b""      # a record is looked at when it is read: the block before it has not been written either


def test_bandwidths_the_tool_refuses(exe):
    for argv, word in ((["-W", "2000"], "-W 2000"), (["-W", "1024"], "-W 1024"), (["-W", "-50"], "-T")):
        got = pairalnsets.run(exe, EXTRA, ["pairaln_wrapped.fa.gz"], argv)
        assert got["rc"] == 1 and word in got["err"] and got["out"] == b""
    got = pairalnsets.run(exe, EXTRA, ["pairaln_wrapped.fa.gz"], ["-W", "1023"])
    assert got["rc"] == 0 and got["out"].count(b"\n") == 5


def test_usage_text_is_the_reference_s(exe):
    for argv in (["-h"], ["-Z"], ["-W"]):
        r = subprocess.run([exe] + argv, stdin=subprocess.DEVNULL, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout.startswith("Program: pairaln\n pairaln read paired sequences (fasta or fastq) from STDIN") and r.stdout.endswith(" -a          Output alignment\n\n")
        assert " -T <int>    Alignment penalty: read end clipping, 0: distable HSP extension, otherwise set to -100 or other [-100]\n" in r.stdout
