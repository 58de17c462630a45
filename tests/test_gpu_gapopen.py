"""wtz_set_gap_open on the MI355X: every device form of the three banded DPs at two pairs of SEPARATE gap-open costs against the reference's own routines
(tests/golden/dpid_vectors.npz: the problems of dp_vectors.npz at (I, D) = (-2, -3) and (-3, -2)), one context per cost pair; and align_hzmaux as wtmsa runs it
(tests/golden/hzmid_vectors.npz: windows by chaining_hzmps, I = -2, D = -3) through the service and the stage path - which runs the split-cost instantiation of
the K-sw3 register forms inside the fused stitch launch - with the switch back to equal costs in the same context.  The checks, the problem lists and the
`must` sets are those of tests/test_gpu_dp_forms.py; what is and is not pinned on the host: tests/test_gapopen_cpu.py."""
import numpy as np
import pytest

import dpidvec
import hzmchainvec as cv
import hzmidvec as iv
from smartdenovo_amd import hipabi
from test_gpu_dp_forms import SHIFT_MUST, check, make_ctx, problems

pytestmark = pytest.mark.gpu

# classes the packed form (7) answers at I == D and may decline at I != D because the wider window - its |O| is max(|I|, |D|) - no longer fits 16 bits: none.
# At the vectors' scores the window of wtz_pk_window is the one of O = -3 (the costs of both blocks have max(|I|, |D|) = 3 = |O| of dp_vectors.npz), so form 7
# answers at I != D exactly what it answers at I == D.
PK_DECLINES = set()


@pytest.fixture(scope="module", params=[0, 1], ids=["I-2_D-3", "I-3_D-2"])
def blk(request):
    return dpidvec.Block(request.param)


def gap_ctx(vec, **kw):
    ctx = make_ctx(vec, **kw)
    ctx.set_gap_open(vec.I, vec.D)
    return ctx


def test_shift_extension_forms(blk):
    """K-sw3: forms 0, 3, 4, 5, 7 in one context per cost pair; 5 and 7 run their split-cost instantiation"""
    idx = [int(i) for i in np.nonzero(blk.kind == 0)[0]]
    ctx = gap_ctx(blk)
    res = {}
    try:
        for form in (0, 3, 4, 5, 7):
            res[form] = ctx.test_dp(hipabi.DP_SHIFT, form, problems(blk, idx))
    finally:
        ctx.close()
    for form, (out, cigs) in res.items():
        must = (lambda c: True) if form in (0, 3, 4) else (lambda c, f=form: c in SHIFT_MUST[f] - (PK_DECLINES if f == 7 else set()))
        ans = check(blk, idx, out, cigs, 0, form, must)
        if form == 0:
            used = {str(blk.cls[i]): int(out["form_used"][k]) for k, i in enumerate(idx)}
            assert used["s_wide"] == 3 and used["s_keyovf"] in (3, 7) and used["s_longt"] == 3 and used["s_c4"] in (5, 7)
        if form in (5, 7):
            for cls in ("s_wide", "s_longt", "s_empty") + (() if form == 7 else ("s_keyovf",)):
                assert ans[cls][0] == 0, "form %d should decline %s" % (form, cls)
            # what the form answered includes problems that tell the two costs apart, in every class it must answer
            for cls in SHIFT_MUST[form]:
                assert any(blk.differs[i] and out["form_used"][k] == form for k, i in enumerate(idx) if str(blk.cls[i]) == cls), "form %d class %s" % (form, cls)


@pytest.mark.parametrize("w", [50, 20, 5, 100, 200])
def test_fixed_extension_forms(w, blk):
    idx = [int(i) for i in np.nonzero((blk.kind == 1) & (blk.w_param == w))[0]]
    assert idx
    ctx = gap_ctx(blk, w=w)
    total = {}
    try:
        for form in (0, 1, 2, 17, 18, 20, 24, 64, 255):
            out, cigs = ctx.test_dp(hipabi.DP_FIXED, form, problems(blk, idx))
            ans = check(blk, idx, out, cigs, 1, form, (lambda c: True) if form in (0, 255) else (lambda c: False))
            total[form] = sum(a for a, _ in ans.values())
            if form == 0:
                total["auto_forms"] = {int(u) for u in out["form_used"]}
    finally:
        ctx.close()
    assert total[0] == len(idx) and total[255] == len(idx)
    if w == 50:
        assert {1, 2, 18, 255} <= total["auto_forms"] and total[1] > 0 and total[2] > 0 and total[17] > 0 and total[18] > 0
    if w in (50, 20, 5):
        assert total[64] > 0.5 * len(idx), "the lane form answered only %d of %d problems" % (total[64], len(idx))
    if w == 100:
        assert total[20] > 0 and 20 in total["auto_forms"]
    if w == 200:
        assert total[24] > 0 and 24 in total["auto_forms"]


def test_global_forms(blk):
    idx = [int(i) for i in np.nonzero(blk.kind == 2)[0]]
    ctx = gap_ctx(blk)
    total = {}
    try:
        for form in (0, 1, 2, 17, 18, 20, 24, 32, 33, 64, 255):
            out, cigs = ctx.test_dp(hipabi.DP_GLOBAL, form, problems(blk, idx))
            ans = check(blk, idx, out, cigs, 2, form, (lambda c: True) if form in (0, 255) else (lambda c: False))
            total[form] = sum(a for a, _ in ans.values())
            if form == 0:
                used = {str(blk.cls[i]): set() for i in idx}
                for k, i in enumerate(idx):
                    used[str(blk.cls[i])].add(int(out["form_used"][k]))
                assert used["g_c4"] <= {18, 20} and 20 in used["g_c4"] and used["g_c8"] <= {20, 24} and 24 in used["g_c8"] and used["g_long"] <= {17, 18} and 255 in used["g_empty"]
            if form == 33:
                cls33 = {str(blk.cls[i]) for k, i in enumerate(idx) if out["form_used"][k] == 33}
                assert {"g_ring", "g_ringwide"} <= cls33
    finally:
        ctx.close()
    assert total[0] == len(idx) and total[255] == len(idx)
    for form in (1, 2, 17, 18, 20, 24, 32, 33, 64):
        assert total[form] > 0, "form %d answered nothing" % form


def test_recorded_calls_at_wtmsas_defaults_and_back():
    """hzmid_vectors.npz through the service and the stage path in one context (one parameter set, one call each); then set_gap_open(-3, -3) in the same
    context: the committed hzmchain records of the same calls"""
    lays = iv.load_vectors()
    ctx, lens, tid, rid, beg, end = iv.open_all(None, lays, -2)
    try:
        ctx.set_gap_open(iv.I, iv.D)
        svc = iv.run(ctx, "service", lens, tid, rid, beg, end, lays[0]["min_sm"])
        stg = iv.run(ctx, "stages", lens, tid, rid, beg, end, lays[0]["min_sm"])
        ctx.set_gap_open(-3, -3)
        back = iv.run(ctx, "service", lens, tid, rid, beg, end, lays[0]["min_sm"])
    finally:
        ctx.close()
    want = iv.wants(lays)
    assert sum(w is not None for w in want) >= 40
    for name, got in (("service", svc), ("stages", stg)):
        for k, (g, w) in enumerate(zip(got, want)):
            assert cv.equal(g, w), "%s, call %d: %s != %s" % (name, k, g and g[0], w and w[0])
    for k, (g, w) in enumerate(zip(back, iv.chain_wants(lays))):
        assert cv.equal(g, w), "back at (-3, -3), call %d: %s != %s" % (k, g and g[0], w and w[0])
