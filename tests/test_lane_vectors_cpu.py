"""tests/golden/lane_vectors.npz (make_lane_vectors.py: whole wavefronts of K-sw1 / K-sw2 problems, recorded from the reference's own kswx_extend_align_core and
ksw_global2 at the cost pairs (-3, -3) and (-2, -3)): the conditions on the file, and form 65 of wtz_test_dp - the lane bodies of wtz_sw_lane.h, K-sw1 in the RELATIVE
mode with the fold's rule - on the host emulation, where a "wavefront" has one lane.  What the emulation cannot see - 64 lanes with their own trip counts, band
ends and trace offsets - is tests/test_gpu_lane_waves.py on the same file.  Form 255 (the scalar bodies) on the same problems keeps the file independent of the lane code."""
import os
import subprocess

import numpy as np
import pytest

import lanevec as lv
from conftest import ROOT


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


@pytest.fixture(scope="module", params=[0, 1])
def vec(request):
    return lv.Block(request.param)


def open_ctx(vec, lib_path, w=50):
    from smartdenovo_amd import hipabi
    ctx = hipabi.Context(hipabi.Params.defaults(w=w), pool_bytes=1 << 30, lib_path=lib_path)
    ctx.upload(*hipabi.pack_reads(vec.reads()))
    if (vec.I, vec.D) != (ctx.params.O, ctx.params.O):
        ctx.set_gap_open(vec.I, vec.D)
    return ctx


def test_the_file_meets_its_conditions(vec):
    assert (vec.I, vec.D) == lv.COSTS[vec.b] and os.path.getsize(os.path.join(ROOT, "tests", "golden", "lane_vectors.npz")) < (1 << 20)
    seen = {}
    for kind in (1, 2):
        idx = vec.of_kind(kind)
        nwave = int(vec.wave[idx].max()) + 1
        for k in range(nwave):
            w = [i for i in idx if vec.wave[i] == k]
            # a wavefront is 64 consecutive problems of a call, lane after lane; only the last one of a kind may be short
            assert [int(vec.lane[i]) for i in w] == list(range(len(w))) and (len(w) == 64 or k == nwave - 1) and w == idx[64 * k:64 * k + len(w)]
            nc, comp = int(vec.nc[w[0]]), str(vec.comp[w[0]])
            assert all(vec.nc[i] == nc and vec.comp[i] == comp for i in w)
            live = [i for i in w if vec.live[i]]
            shp = {i: lv.shape(vec, i) for i in live}
            assert live and all(shp[i] for i in live), "a live problem outside the lane envelope"
            assert all(vec.qlen[i] == 0 or vec.tlen[i] == 0 for i in w if not vec.live[i])
            widest = max(s[1] for s in shp.values())
            assert widest <= nc and (nc == 16 or widest > {32: 16, 64: 32, 104: 64}[nc]), "the wave's class is the class of its widest live problem"
            seen.setdefault((kind, nc), []).append((comp, len(live)))
            if kind == 1:
                high = [i for i in live if vec.high[i]]
                assert 4 * len(high) >= 3 * len(live), "fewer than three quarters of the lanes at a high init_score"
                assert all(8 * (vec.qlen[i] + vec.tlen[i]) + 64 <= vec.init[i] <= 1 << 20 for i in high) and all(0 <= vec.init[i] <= 60 for i in live if not vec.high[i])
                assert all(vec.rel_ok[i] for i in high)
            key = lambda i: (shp[i][1], shp[i][0])
            if comp == "sorted":
                assert len(live) == 64 and [key(i) for i in w] == sorted((key(i) for i in w), reverse=True)
            if comp == "ragged_rows":
                r = [shp[i][0] for i in w]
                assert len(w) == 64 and r[0] == 1 == min(r) and r[63] > max(r[:63]) and r[1:63] != sorted(r[1:63]) and r[63] >= (30 if nc == 16 else 60)
                assert nc != 104 or r[63] == (lv.LN_MAXROWS if kind == 1 else lv.LG_MAXROWS)
            if comp == "ragged_cols":
                c = [shp[i][1] for i in w]
                top = {16: 16, 32: 32, 64: 64, 104: 101}[nc]
                assert max(c) == top and any((a <= 8 and b == top) or (b <= 8 and a == top) for a, b in zip(c, c[1:]))
                assert all(e in c for e in (8, 9, 16, 17, 32, 33, 64, 65, 96, 97) if e <= top)
            if comp == "partial":
                assert len(live) in (1, 37, 63) and vec.lane[max(live, key=key)] != 0
        assert len(idx) % 64 != 0 or kind == 1, "the last K-sw2 wave is short"
    for kind in (1, 2):
        for nc in lv.CLASSES:
            comps = [c for c, _ in seen[(kind, nc)]]
            assert set(lv.COMPOSITIONS) <= set(comps), (kind, nc, comps)
            assert sorted(n for c, n in seen[(kind, nc)] if c == "partial") == [1, 37, 63]
    assert {"w5", "w20"} <= {c for v in seen.values() for c, _ in v} and set(vec.w_param[vec.kind == 1].tolist()) == {50, 5, 20}
    low = (vec.kind == 1) & vec.live & ~vec.high
    assert (low & ~vec.rel_ok).sum() >= 8, "fewer than 8 low problems whose answer is not translation invariant"
    assert len(set(vec.W[(vec.kind == 2) & vec.live].tolist())) == 4


@pytest.mark.parametrize("kind", [1, 2])
def test_lane_forms_on_the_emulation(kind, vec, emul_lib):
    """form 65, one problem per "wavefront": relative mode + the fold's rule (K-sw1), the band width each problem names (K-sw2)"""
    from smartdenovo_amd import hipabi
    idx = vec.of_kind(kind)
    ctx = open_ctx(vec, emul_lib)
    try:
        out, cigs = ctx.test_dp(kind, 65, lv.problems(hipabi, vec, idx, True))
    finally:
        ctx.close()
    answered = lv.check_lane_form(vec, idx, out, cigs, "form 65 (emulation)")
    declined = [i for i in idx if vec.live[i] and i not in answered]
    if kind == 1:
        assert all(not vec.high[i] for i in declined) and sum(not vec.rel_ok[i] for i in declined) >= 8
        assert any(vec.rel_ok[i] for i in answered if not vec.high[i]), "no low problem was answered: the rule declines too much to be tested"
    else:
        assert not declined


@pytest.mark.parametrize("kind", [1, 2])
def test_scalar_bodies_equal_the_record(kind, vec, emul_lib):
    """form 255 answers every problem of the file, fillers included, with the record"""
    from smartdenovo_amd import hipabi
    for w in ((50, 5, 20) if kind == 1 else (50,)):
        idx = vec.of_kind(kind, w if kind == 1 else None)
        assert idx
        ctx = open_ctx(vec, emul_lib, w=w)
        try:
            out, cigs = ctx.test_dp(kind, 255, lv.problems(hipabi, vec, idx, False))
        finally:
            ctx.close()
        for k, i in enumerate(idx):
            assert int(out["form_used"][k]) == 255
            lv.equals_record(vec, i, out, cigs, k, "form 255 (emulation)")
