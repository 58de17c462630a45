"""wtz_pwtext_batch without a GPU: the bodies of smartdenovo_amd/csrc/wtz_pwtext.h compiled into the host emulation of the library (tests/emul: one lane that
walks every column group of a tile) against tests/pwtextref.py, and that restatement against the `-a` blocks the reference's pairaln wrote
(tests/golden/pairaln_manifest.json).  The lane-crossing parts (the scans, the 65-way search, the ballots) are the identity here: tests/test_gpu_pwtext.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import pwtextref as pw
import pairalnsets

ROOT = pw.ROOT


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


@pytest.fixture(scope="module")
def cases():
    return pw.Cases()


@pytest.fixture(scope="module")
def ctx(emul_lib, cases):
    c = pw.context(cases, emul_lib)
    yield c
    c.close()


def test_case_list_holds_the_shapes_the_feature_names(cases):
    cols = set(len(w) // 3 - 1 for w in cases.want)
    assert {0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513} <= cols and max(cols) >= 20000
    nops = set(n for _, n in cases.slices)
    assert {0, 1, 63, 64, 65} <= nops and max(nops) >= 15000
    assert all(any(ch in w for w in cases.want) for ch in (b"|", b"*", b"-"))
    at = lambda side: set((int(cases.offs[int(p[side + "_read"])]) + int(p[side + "_from"])) % 32 for p, n in zip(cases.pr, cases.names) if n.startswith("from_"))
    assert at("q") == set(range(32)) and at("t") == set(range(32))


def test_restatement_equals_the_reference_s_pictures():
    """every `-a` block of the manifest, rebuilt from the two gapped lines the reference printed: its marker line and its ungapped bases must come back"""
    man = json.load(open(os.path.join(pairalnsets.GOLDEN, "pairaln_manifest.json")))
    n = 0
    for name, case in man["cases"].items():
        if "-a" not in case["argv"]:
            continue
        lines = case["stdout"].split("\n")
        k = 0
        while k + 3 < len(lines):
            a, m, b = lines[k + 1:k + 4]
            cig, code = [], {"A": 0, "C": 1, "G": 2, "T": 3}
            for x, y in zip(a, b):
                op = 2 if x == "-" else 1 if y == "-" else 0
                if cig and cig[-1] & 15 == op:
                    cig[-1] += 16
                else:
                    cig.append(16 | op)
            q = [code[x] for x in a if x != "-"]
            t = [code[y] for y in b if y != "-"]
            assert pw.picture(q, t, cig) == (a + "\n" + m + "\n" + b + "\n").encode(), (name, lines[k][:60])
            n += 1
            k += 4
    assert n >= 20


def test_emulation_equals_the_restatement_on_every_case(ctx, cases):
    pw.check_whole_batch(ctx, cases)


def test_reversed_batch_and_single_alignments_give_the_same_bytes(ctx, cases):
    pw.check_batching_does_not_matter(ctx, cases)


def test_argument_errors_leave_the_context_usable(ctx, cases):
    pw.check_argument_errors(ctx, cases)


def test_a_small_pool_cuts_the_call_into_launch_groups(emul_lib, cases):
    pw.check_small_pool(cases, emul_lib)


def test_one_alignment_larger_than_the_pool_is_a_pool_error(emul_lib, cases):
    pw.check_pool_error(cases, emul_lib)


def test_pwtext_bodies_stand_alone(tmp_path):
    """tests/emul/check_pwtext.cpp: wtz_pwtext_scan / wtz_pwtext_tile over random CIGARs and views against a scalar restatement written in that file, buffers of
    exactly the planned size"""
    exe = os.path.join(str(tmp_path), "check_pwtext")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DWTZ_EMUL", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "smartdenovo_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "emul", "check_pwtext.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 bad" in r.stdout, r.stdout + r.stderr
