"""wtz_local_batch on the GPU (K-local, smartdenovo_amd/csrc/wtz_sw_local.h) against tests/golden/local_vectors.npz, the five ints that the
reference's own ksw_align2(..., KSW_XSTART) returned (tests/golden/make_local_vectors.py).  Exact equality everywhere; nothing here reads the
reference's tree.  The gap costs are arguments of the call, so "one call" is one call per gap-cost setting of the set (localvec.GAPS)."""
import numpy as np
import pytest

import localvec as lv
from smartdenovo_amd import hipabi

pytestmark = pytest.mark.gpu

V = lv.load_vectors()
NAMES = [str(x) for x in V["names"]]
# the cases a failure should name: query lengths around a lane of eight, the 64 lanes, the switch between four and sixteen columns per lane (256),
# the strip of 1 024 columns and two strips; maximal ties; saturation
EDGE = [n for n in NAMES if n.startswith(("qlen_", "tlen_", "all_A_", "identical_17000"))]


@pytest.fixture(scope="module")
def ctx():
    c = lv.make_context(V["words"], V["offs"], V["lens"], int(V["M"]), int(V["X"]), pool_bytes=2 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def problems():
    return lv.whole_read_problems(V["q_read"], V["t_read"], V["lens"])


@pytest.fixture(scope="module")
def whole_set(ctx, problems):
    """the whole set in one call per gap setting; shared by the tests below and never modified"""
    out = lv.run_by_gap(ctx, problems, V["gap"])
    out.setflags(write=False)
    return out


def _assert_equal(got5, idx, what):
    exp = V["expect"][idx].astype(np.int64)
    bad = np.nonzero((got5 != exp).any(axis=1))[0]
    assert bad.size == 0, "%s: %s" % (what, [(NAMES[int(np.atleast_1d(idx)[b])], got5[b].tolist(), exp[b].tolist()) for b in bad[:8]])


def test_whole_set_in_one_call_equals_reference(ctx, whole_set):
    _assert_equal(lv.five(whole_set), np.arange(len(NAMES)), "whole set")
    lens = V["lens"].astype(np.uint64)
    assert (whole_set["cells"] >= lens[V["q_read"]] * lens[V["t_read"]]).all()
    assert set(int(f) for f in whole_set["form_used"]) == {4, 16}
    p = lv.pool_info(ctx)
    assert p.main_used == 0 and p.main_cap > 0      # no WTZ_E_POOL with the 2 GB pool (the call above would have raised), and the pool is handed back empty


@pytest.mark.parametrize("name", EDGE)
def test_edge_case(name, ctx, problems, whole_set):
    """the named problem alone in a call of its own: nothing it shares a launch with (boundary offsets, launch order) can hide or cause a fault; and it
    gives what it gave inside the whole set, cells included"""
    i = NAMES.index(name)
    alone = lv.run_by_gap(ctx, problems[i:i + 1], V["gap"][i:i + 1])
    _assert_equal(lv.five(alone), np.array([i]), name)
    assert alone[0] == whole_set[i], (name, alone[0], whole_set[i])


@pytest.mark.parametrize("batch", [1, 37])
def test_reversed_order_and_batches_give_the_same(ctx, problems, whole_set, batch):
    idx = np.arange(len(NAMES) - 1, -1, -1)      # every problem of the set, the two 17 000-base pairs included
    got = np.zeros(idx.size, dtype=hipabi.LOCAL_RESULT)
    for b in range(0, idx.size, batch):
        sel = idx[b:b + batch]
        got[b:b + batch] = lv.run_by_gap(ctx, problems[sel], V["gap"][sel])
    _assert_equal(lv.five(got), idx, "batches of %d, reversed order" % batch)
    assert (got["cells"] == whole_set["cells"][idx]).all()


def test_only_queries_beyond_one_strip_take_pool(ctx, problems):
    """include/wtzmo_hip.h: a problem takes 8 * t_len bytes of the main pool when its query exceeds one strip (1 024 columns on the device), and none
    otherwise.  counters.pool_peak is the high-water mark since reset_counters.  A request above a quarter slab is rounded to 256 bytes, a smaller one
    takes one slab (at most 2 MB, wtz_pool_init): that is the only slack allowed here."""
    ql, tl = problems["q_len"].astype(np.int64), problems["t_len"].astype(np.int64)
    short = np.nonzero(ql <= 1024)[0]
    assert (ql[short] == 1024).any() and short.size > 100
    ctx.reset_counters()
    lv.run_by_gap(ctx, problems[short], V["gap"][short])
    assert ctx.counters().pool_peak == 0
    one = np.array([NAMES.index("qlen_1025_inside")])
    lv.run_by_gap(ctx, problems[one], V["gap"][one])
    assert 8 * int(tl[one[0]]) <= ctx.counters().pool_peak <= (2 << 20)
    ctx.reset_counters()
    g0 = np.nonzero((ql > 1024) & (V["gap"] == 0))[0]      # one call: the boundaries of all its long queries in one block
    need = 8 * int(tl[g0].sum())
    assert need > (2 << 20) // 4      # above a quarter slab: the request itself, rounded to 256 bytes
    lv.run_by_gap(ctx, problems[g0], V["gap"][g0])
    assert need <= ctx.counters().pool_peak <= need + 256
    assert lv.pool_info(ctx).main_used == 0


def test_views_equal_uploaded_sequences():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, 3000).astype(np.uint8)
    b = np.concatenate([rng.integers(0, 4, 333).astype(np.uint8), a[500:2700], rng.integers(0, 4, 77).astype(np.uint8)])
    b[::9] = (b[::9] + 1) % 4
    rc = lambda s: (3 - s[::-1]).astype(np.uint8)
    seqs = [a, b, a[401:2802].copy(), b[100:1500].copy(), rc(a), rc(b)]
    words, offs, lens = hipabi.pack_reads(seqs)
    c = lv.make_context(words, offs, lens, 2, -5)
    try:
        pr = lv.whole_read_problems([0, 2, 0, 0, 0, 4, 0, 4, 5], [1, 1, 1, 3, 1, 1, 5, 5, 0], lens)
        pr[2]["q_from"], pr[2]["q_len"] = 401, 2401                                   # = 1: sub-range of the query
        pr[4]["t_from"], pr[4]["t_len"] = 100, 1400                                   # = 3: sub-range of the target
        pr[5]["q_rev"] = 1                                                            # = 0: q_rev of the uploaded reverse complement
        pr[6]["t_rev"] = 1                                                            # = 0
        pr[7]["q_rev"], pr[7]["t_rev"] = 1, 1                                         # = 0
        out = lv.five(c.local_batch(pr, *lv.GAPS[0]))
        assert out[0, 0] > 1000
        for same, as_ in ((2, 1), (4, 3), (5, 0), (6, 0), (7, 0)):
            assert (out[same] == out[as_]).all(), (same, as_, out[same].tolist(), out[as_].tolist())
        # q_rev AND t_rev with the roles kept: the alignment of the two reverse complements mirrors the coordinates of the forward one where the
        # optimum is unique in its end points - here only the score is asserted
        rr = lv.five(c.local_batch(lv.whole_read_problems([4], [5], lens), *lv.GAPS[0]))
        assert rr[0, 0] == out[0, 0]
    finally:
        c.close()


def test_problem_beyond_the_limit_is_an_argument_error_and_the_context_survives():
    big = np.zeros(hipabi.LOCAL_MAXLEN + 1, dtype=np.uint8)      # A ... A C A
    big[hipabi.LOCAL_MAXLEN - 1] = 1
    a = np.array([0, 1, 2, 3] * 30, dtype=np.uint8)
    words, offs, lens = hipabi.pack_reads([big, a, np.ones(5, dtype=np.uint8)])
    c = lv.make_context(words, offs, lens, 2, -5)
    try:
        for q, t in ((0, 1), (1, 0)):
            with pytest.raises(RuntimeError, match="error -1"):
                c.local_batch(lv.whole_read_problems([1, q], [1, t], lens), *lv.GAPS[0])
        out = lv.five(c.local_batch(lv.whole_read_problems([1], [1], lens), *lv.GAPS[0]))
        assert out[0].tolist() == [240, 119, 119, 0, 0]
        assert lv.pool_info(c).main_used == 0
        # exactly at the limit the call is accepted, and the last column / the last row can hold the answer:
        # columns: A...AC against ACGTACGT...: the final "AC" on the target's first two bases; rows: the only C of the target against CCCCC
        pr = lv.whole_read_problems([0, 2], [1, 0], lens)
        pr[0]["q_len"] = hipabi.LOCAL_MAXLEN
        pr[1]["t_len"] = hipabi.LOCAL_MAXLEN
        o = c.local_batch(pr, *lv.GAPS[0])
        last = hipabi.LOCAL_MAXLEN - 1
        assert lv.five(o).tolist() == [[4, 1, last, 0, last - 1], [2, last, 0, last, 0]]
        assert o["form_used"].tolist() == [16, 4]
    finally:
        c.close()
