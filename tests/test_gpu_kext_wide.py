"""wtz_kext_batch and wtz_align_batch on the GPU against tests/golden/kext_wide_vectors.npz (tests/golden/make_kext_wide_vectors.py): the two widest
kernel forms with every exit and a moving band, 64 C - 1 / 64 C / 64 C + 1 live diagonals for every form, views inside longer reads on both strands
and through q_rev / t_rev, views on the first and the last uploaded base, 20 000 rows, and chain rows whose extension stages run in the wide forms.

The host emulation runs the same DP body on one lane; what crosses lanes (the prefix maximum that carries F, the shift that hands E to the left
neighbour, the four reductions of the band trim, the per-lane query window) is checked here and nowhere else.  Exact equality everywhere; nothing
here reads the reference's tree."""
import numpy as np
import pytest

import kextvec as kv
import localvec as lv
from smartdenovo_amd import hipabi

pytestmark = pytest.mark.gpu

V = kv.load_vectors(kv.WIDE_VECTORS)
NAMES = [str(x) for x in V["f_names"]]
ALONE = [n for n in NAMES if n.startswith(("edge_", "view_", "rows_"))]
NINE = kv.FIELDS + ("form_used", "rows", "cells")


@pytest.fixture(scope="module")
def ctx():
    c = lv.make_context(V["words"], V["offs"], V["lens"], int(V["M"]), int(V["X"]))
    yield c
    c.close()


@pytest.fixture(scope="module")
def problems():
    return kv.problems_of(V)


def _run(ctx, problems, idx):
    return kv.run_by_group(ctx, problems[idx], V["f_gap"][idx], V["f_end_bonus"][idx], V["f_zdrop"][idx])


@pytest.fixture(scope="module")
def whole_set(ctx, problems):
    """the whole function-level set in one call per setting; shared by the tests below and never modified"""
    out = _run(ctx, problems, np.arange(len(NAMES)))
    out.setflags(write=False)
    return out


def _assert_equal(got6, idx, what):
    exp = V["f_expect"][idx].astype(np.int64)
    bad = np.nonzero((got6 != exp).any(axis=1))[0]
    assert bad.size == 0, "%s: %s" % (what, [(NAMES[int(np.atleast_1d(idx)[b])], got6[b].tolist(), exp[b].tolist()) for b in bad[:8]])


def test_whole_set_equals_reference(ctx, whole_set):
    _assert_equal(kv.six(whole_set), np.arange(len(NAMES)), "whole set")
    bad = np.nonzero((whole_set["rows"] != V["f_rows"]) | (whole_set["cells"] != V["f_cells"].astype(np.uint64)))[0]
    assert bad.size == 0, [(NAMES[b], int(whole_set["rows"][b]), int(V["f_rows"][b]), int(whole_set["cells"][b]), int(V["f_cells"][b])) for b in bad[:8]]
    assert (whole_set["form_used"] == V["f_form"]).all()
    assert lv.pool_info(ctx).main_used == 0


@pytest.mark.parametrize("name", ALONE)
def test_edge_case(name, ctx, problems, whole_set):
    """every form-edge problem, every view and the two long problems alone in a call of its own: the reference's ints, and what it gave inside the set"""
    i = NAMES.index(name)
    alone = _run(ctx, problems, np.array([i]))
    _assert_equal(kv.six(alone), np.array([i]), name)
    assert alone[0] == whole_set[i], (name, alone[0], whole_set[i])


@pytest.mark.parametrize("batch", [1, 37])
def test_reversed_order_and_batches_give_the_same(ctx, problems, whole_set, batch):
    idx = np.arange(len(NAMES) - 1, -1, -1)
    got = np.zeros(idx.size, dtype=hipabi.KEXT_RESULT)
    for b in range(0, idx.size, batch):
        sel = idx[b:b + batch]
        got[b:b + batch] = _run(ctx, problems, sel)
    _assert_equal(kv.six(got), idx, "batches of %d, reversed order" % batch)
    assert (got == whole_set[idx]).all()


def test_chain_equals_the_chain_table(ctx):
    pr = kv.chain_problems(V["c_q_read"], V["c_t_read"], V["c_t_rev"], V["lens"])
    c0 = ctx.counters()
    out = kv.run_chain_by_group(ctx, pr, V["c_w"], V["c_T"])
    got, exp = kv.chain_six(out), V["c_expect"].astype(np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(str(V["c_names"][b]), got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    loc = np.stack([out[f] for f in ("local_score", "local_tb", "local_te", "local_qb", "local_qe")], axis=1).astype(np.int64)
    assert (loc == V["c_local"]).all()
    c1 = ctx.counters()
    ran = ((V["c_flags"] & kv.F_LEFT_RAN) != 0).sum() + ((V["c_flags"] & kv.F_RIGHT_RAN) != 0).sum()
    assert ran == (V["c_slots"] > 0).sum() and c1.n_kext - c0.n_kext == ran and c1.n_local - c0.n_local == len(pr)
    assert lv.pool_info(ctx).main_used == 0


@pytest.mark.parametrize("ql,w,h0,form", [(50, 10, 30, 1), (1100, 1023, 400, 32)])
def test_views_equal_uploaded_sequences(ql, w, h0, form):
    """needs no table: a problem on a sub-range of a read gives the nine result fields of the same bases uploaded as a read of their own, and q_rev / t_rev
    on an uploaded reverse complement gives what the forward read gives, walked forwards from its first base and backwards from its last"""
    rng = np.random.default_rng(7 + ql)
    q = rng.integers(0, 4, ql).astype(np.uint8)
    t = q.copy()
    t[::9] = (t[::9] + 1) % 4
    t = np.concatenate([t[:ql // 3], t[ql // 3 + 3:]])
    rc = lambda s: (3 - s[::-1]).astype(np.uint8)
    pad = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    seqs = [np.concatenate([pad(77), q, pad(45)]), np.concatenate([pad(13), t, pad(101)]), q, t, rc(q), rc(t)]
    words, offs, lens = hipabi.pack_reads(seqs)
    c = lv.make_context(words, offs, lens, 2, -5)
    try:
        pr = lv.whole_read_problems([2, 0, 2, 0, 4, 2, 4, 2, 4, 2, 4], [3, 1, 1, 3, 3, 5, 5, 3, 3, 5, 5], lens)
        pr["W"], pr["init_score"] = w, h0
        for k in (1, 3):                                                              # = 0: sub-range of the query's read
            pr[k]["q_from"], pr[k]["q_len"] = 77, q.size
        for k in (1, 2):                                                              # = 0: sub-range of the target's read
            pr[k]["t_from"], pr[k]["t_len"] = 13, t.size
        for k in (4, 6, 8, 10):                                                       # q_rev of the uploaded reverse complement
            pr[k]["q_rev"] = 1
        for k in (5, 6, 9, 10):                                                       # t_rev of the uploaded reverse complement
            pr[k]["t_rev"] = 1
        for k in (7, 8, 9, 10):                                                       # = 7: both sides walked backwards from their last base
            pr[k]["q_from"], pr[k]["t_from"], pr[k]["q_strand"], pr[k]["t_strand"] = q.size - 1, t.size - 1, -1, -1
        out = c.kext_batch(pr, 3, 1, 3, 1, 100, -1)
        assert out["form_used"][0] == form and out["tle"][0] > ql // 2 and out["rows"][7] > ql // 4
        for same, as_ in ((1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (8, 7), (9, 7), (10, 7)):
            assert [out[f][same] for f in NINE] == [out[f][as_] for f in NINE], (same, as_, out[same], out[as_])
    finally:
        c.close()
