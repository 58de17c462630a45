"""wtz_kext_batch and wtz_align_batch on the GPU (K-kext, smartdenovo_amd/csrc/wtz_sw_kext.h) against tests/golden/kext_vectors.npz: the six ints
that the reference's own ksw_extend2 returned, and the chain table (tests/golden/make_kext_vectors.py, tests/kextvec.py).  Exact equality everywhere;
nothing here reads the reference's tree.  Gap costs, end bonus and zdrop are arguments of the call, so "one call" is one call per setting present."""
import numpy as np
import pytest

import kextvec as kv
import localvec as lv
from smartdenovo_amd import hipabi

pytestmark = pytest.mark.gpu

V = kv.load_vectors()
NAMES = [str(x) for x in V["f_names"]]
EDGE = [n for n in NAMES if n.startswith(("qlen_", "w_", "runoff_", "all_A_"))]


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
    assert (whole_set["rows"] == V["f_rows"]).all() and (whole_set["cells"] == V["f_cells"].astype(np.uint64)).all()
    assert set(int(f) for f in whole_set["form_used"]) == {1, 2, 4, 8, 16, 32}
    assert (whole_set["cells"] > 0).all()
    assert lv.pool_info(ctx).main_used == 0


@pytest.mark.parametrize("name", EDGE)
def test_edge_case(name, ctx, problems, whole_set):
    """the named problem alone in a call of its own gives what it gave inside the set, rows and cells included"""
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
    for i in np.nonzero([str(n).startswith("all_A_all_C") for n in V["c_names"]])[0]:
        assert not any(out[int(i)].tolist())      # found = 0 and zeros
    c1 = ctx.counters()
    ran = ((V["c_flags"] & kv.F_LEFT_RAN) != 0).sum() + ((V["c_flags"] & kv.F_RIGHT_RAN) != 0).sum()
    assert c1.n_kext - c0.n_kext == ran and c1.n_local - c0.n_local == len(pr)
    assert lv.pool_info(ctx).main_used == 0


def test_limits_are_argument_errors_and_the_context_survives(ctx, problems, whole_set):
    one = problems[:2].copy()
    for field, value in (("W", hipabi.KEXT_MAXW + 1), ("q_len", 0), ("t_len", 0)):
        bad = one.copy()
        bad[field][1] = value
        with pytest.raises(RuntimeError, match="error -1"):
            ctx.kext_batch(bad, 3, 1, 3, 1, 100, -1)
    with pytest.raises(RuntimeError, match="error -1"):
        ctx.kext_batch(one, 3, 0, 3, 1, 100, -1)
    with pytest.raises(RuntimeError, match="error -1"):
        ctx.align_batch(one, hipabi.KEXT_MAXW + 1, -3, -3, -1, -100)
    again = _run(ctx, problems, np.array([0, 1]))
    assert (again == whole_set[:2]).all()
    assert lv.pool_info(ctx).main_used == 0
