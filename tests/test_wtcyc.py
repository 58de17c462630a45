"""The drop-in wtcyc (smartdenovo_amd/csrc/host/wtcyc_main.c) on the host emulation of the device library: every option set of tests/golden/cyc_manifest.json
byte for byte against what the reference's `wtcyc -t 1` wrote (tests/golden/make_cyc_goldens.py), and the routes that end a run.  Needs no GPU."""
import hashlib
import json
import os
import subprocess

import pytest

import cycsets
import emultools

ROOT = cycsets.ROOT
MAN = json.load(open(os.path.join(cycsets.GOLDEN, "cyc_manifest.json")))
EXTRA = ["--pool-gb", "1"]


@pytest.fixture(scope="module")
def exe():
    """wtcyc_emul: the same main against the libwtz_emul.so that tests/emul/build_emul.sh produces"""
    return emultools.build("wtcyc")


def check_case(exe, extra, name, workdir):
    case = MAN["cases"][name]
    got = cycsets.run(exe, extra, os.path.join(cycsets.GOLDEN, case["input"]), case["argv"], workdir)
    assert got["rc"] == 0, got["err"]
    assert got["a"].decode() == case["a_text"]
    assert got["o"].decode() == case["o_text"]
    assert hashlib.md5(got["a"]).hexdigest() == case["a_md5"] and hashlib.md5(got["o"]).hexdigest() == case["o_md5"]
    assert got["a"].count(b"\n") == case["a_lines"] and got["o"].count(b"\n") == case["o_lines"]


def test_manifest_holds_the_sets_the_feature_names():
    assert set(cycsets.SETS) == set(MAN["cases"]) and len(MAN["cases"]) >= 8
    for name, (inp, argv) in cycsets.SETS.items():
        assert MAN["cases"][name]["argv"] == argv and MAN["cases"][name]["input"] == inp
    assert "KSWX_NULL" in MAN["empty_record"]
    assert "empty\t0\t0\t0.000\t0\t0\t0\t0\n" in MAN["cases"]["defaults"]["a_text"]


@pytest.mark.parametrize("name", sorted(cycsets.SETS))
def test_every_set_is_byte_identical_to_the_reference(exe, name, tmp_path):
    check_case(exe, EXTRA, name, str(tmp_path))


def test_three_blocks_give_the_same_bytes(exe, tmp_path):
    """a byte budget of 9 000 bases cuts the 14 reads into more than three blocks"""
    check_case(exe, EXTRA + ["--block-bytes", "9000"], "defaults", str(tmp_path))


def test_a_read_beyond_65535_bases_ends_the_run(exe, tmp_path):
    got = cycsets.run(exe, EXTRA, os.path.join(cycsets.GOLDEN, "cyc_too_long.fa.gz"), ["-o", "{o}", "-a", "{a}"], str(tmp_path))
    assert got["rc"] == 1 and "too_long" in got["err"] and "65536" in got["err"]
    assert got["a"] == b"" and got["o"] == b""      # the read's block is not written


def test_a_character_outside_acgt_ends_the_run(exe, tmp_path):
    got = cycsets.run(exe, EXTRA, os.path.join(cycsets.GOLDEN, "cyc_non_acgt.fa.gz"), ["-o", "{o}", "-a", "{a}"], str(tmp_path))
    assert got["rc"] == 1 and "has_N" in got["err"] and "ACGTacgt" in got["err"]
    assert got["a"] == b"" and got["o"] == b""


def test_existing_output_is_refused_without_f(exe, tmp_path):
    inp = os.path.join(cycsets.GOLDEN, "cyc_wrapped.fa.gz")
    for opt in ("-o", "-a"):
        keep = tmp_path / ("keep" + opt)
        keep.write_text("mine\n")
        r = subprocess.run([exe] + EXTRA + [opt, str(keep), inp], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("File exists! '%s'\n\n" % keep) and r.stdout.startswith("WTCYC: Align long read")
        assert keep.read_text() == "mine\n"
    r = subprocess.run([exe] + EXTRA + ["-f", "-o", str(keep), "-a", str(tmp_path / "a"), inp], capture_output=True, text=True)
    assert r.returncode == 0 and keep.read_text() == MAN["cases"]["wrapped"]["o_text"]


def test_usage_text_is_the_reference_s(exe):
    for argv in (["-h"], [], ["-Z"]):
        r = subprocess.run([exe] + argv, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout.startswith("WTCYC: Align long read against its reverse complementary\n") and r.stdout.endswith("-a wt.zmo.cyc.info\n\n")
        assert " -T <int>    Alignment penalty: read end clipping, 0: distable HSP extension, otherwise set to -30 or other [-100]\n" in r.stdout
