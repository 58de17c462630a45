"""The lane forms of K-sw1 / K-sw2 (wtz_sw_lane.h) on the MI355X as the product runs them - 64 problems per wavefront in an order the TEST chooses, K-sw1 in the
relative mode with the fold's rule, forward DP and traceback in two launches around a lane-interleaved trace block in the transient pool: form 65 of wtz_test_dp on
tests/golden/lane_vectors.npz (recorded from the reference's own kswx_extend_align_core and ksw_global2; the conditions on the file: tests/test_lane_vectors_cpu.py).
The file's waves are what the product's shape sort avoids: ragged rows, ragged bands beside the block-skip and store-guard edges, idle lanes, a short last wave.
One context per cost block, one call per kind with all its waves.  Beside the record: the same answered / declined set as the one-lane host emulation (the rule is
per lane: it must not depend on a lane's neighbours), and form 64 (one problem per wavefront, absolute mode) wherever both forms answer."""
import os
import subprocess

import pytest

import lanevec as lv
from conftest import ROOT
from smartdenovo_amd import hipabi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


def open_ctx(vec, lib_path=None, w=50):
    ctx = hipabi.Context(hipabi.Params.defaults(w=w), pool_bytes=(2 << 30) if lib_path is None else (1 << 30), lib_path=lib_path)
    ctx.upload(*hipabi.pack_reads(vec.reads()))
    if (vec.I, vec.D) != (ctx.params.O, ctx.params.O):
        ctx.set_gap_open(vec.I, vec.D)
    return ctx


@pytest.fixture(scope="module", params=[0, 1])
def run(request, emul_lib):
    """per cost block: form 65 of both kinds on the GPU and on the emulation, one call each"""
    vec = lv.Block(request.param)
    res = {}
    for name, lib in (("gpu", None), ("emul", emul_lib)):
        ctx = open_ctx(vec, lib)
        try:
            for kind in (1, 2):
                res[(name, kind)] = ctx.test_dp(kind, 65, lv.problems(hipabi, vec, vec.of_kind(kind), True))
        finally:
            ctx.close()
    return vec, res


@pytest.mark.parametrize("kind", [1, 2])
def test_waves_equal_the_record(kind, run):
    vec, res = run
    idx = vec.of_kind(kind)
    out, cigs = res[("gpu", kind)]
    answered = lv.check_lane_form(vec, idx, out, cigs, "form 65")
    declined = [i for i in idx if vec.live[i] and i not in answered]
    if kind == 1:
        assert all(not vec.high[i] for i in declined) and sum(not vec.rel_ok[i] for i in declined) >= 8
    else:
        assert not declined


@pytest.mark.parametrize("kind", [1, 2])
def test_same_set_as_one_lane_per_wavefront(kind, run):
    """what a lane answers does not depend on who sits beside it: the emulation runs every problem alone"""
    vec, res = run
    idx = vec.of_kind(kind)
    g, e = res[("gpu", kind)][0]["form_used"], res[("emul", kind)][0]["form_used"]
    diff = [i for k, i in enumerate(idx) if int(g[k]) != int(e[k])]
    assert not diff, "form 65 on the GPU and on the emulation answer different sets: %s" % "; ".join("%s: GPU %s" % (vec.where(i), "declined" if g[idx.index(i)] == 0 else "answered") for i in diff[:5])
    assert (e == 65).sum() >= 0.75 * sum(vec.live[i] for i in idx)


@pytest.mark.parametrize("kind", [1, 2])
def test_form_64_agrees(kind, run):
    """form 64: the same lane bodies with lane 0 alone in its wavefront, K-sw1 in the absolute mode"""
    vec, res = run
    out65, cig65 = res[("gpu", kind)]
    pos = {i: k for k, i in enumerate(vec.of_kind(kind))}
    both = 0
    for w in ((50, 5, 20) if kind == 1 else (50,)):
        idx = vec.of_kind(kind, w if kind == 1 else None)
        ctx = open_ctx(vec, w=w)
        try:
            out, cigs = ctx.test_dp(kind, 64, lv.problems(hipabi, vec, idx, False))
        finally:
            ctx.close()
        for k, i in enumerate(idx):
            if int(out["form_used"][k]) == 0:
                continue
            assert int(out["form_used"][k]) == 64
            if vec.live[i]:
                lv.equals_record(vec, i, out, cigs, k, "form 64")
            k65 = pos[i]
            if int(out65["form_used"][k65]) == 65:
                both += 1
                a, b = tuple(int(out[f][k]) for f in lv.FIELDS), tuple(int(out65[f][k65]) for f in lv.FIELDS)
                assert a == b and cigs[k].tolist() == cig65[k65].tolist(), "forms 64 and 65 differ, %s: %s != %s" % (vec.where(i), a, b)
    assert both >= 0.75 * sum(vec.live[i] for i in pos)
