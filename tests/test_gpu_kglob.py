"""wtz_global_batch and wtz_alignx_batch on the GPU (K-glob, smartdenovo_amd/csrc/wtz_sw_kglob.h, and the wide forms beyond 2 047 band slots) against
tests/golden/kglob_vectors.npz: the score, the five counts and the CIGAR that the reference's own ksw_global2 returned, and the chain table
(tests/golden/make_kglob_vectors.py, tests/kglobvec.py).  Exact equality everywhere; nothing here reads the reference's tree.
The F carry across lanes, the E hand-over, the full-width trace stores and the cooperative staging of the traceback are the identity in the host
emulation: only this module covers them (the form-edge problems keep the last register of lane 63 live)."""
import numpy as np
import pytest

import kglobvec as gv
import localvec as lv
from smartdenovo_amd import hipabi

pytestmark = pytest.mark.gpu

V = gv.load_vectors()
NAMES = [str(x) for x in V["f_names"]]
N = len(NAMES)


@pytest.fixture(scope="module")
def ctx():
    c = lv.make_context(V["words"], V["offs"], V["lens"], int(V["M"]), int(V["X"]))
    yield c
    c.close()


@pytest.fixture(scope="module")
def problems():
    return gv.problems_of(V)


@pytest.fixture(scope="module")
def whole_set(ctx, problems):
    """the whole function-level set in one call per gap setting; shared by the tests below and never modified"""
    out, cigs = gv.run_by_gap(ctx, problems, V["f_gap"])
    out.setflags(write=False)
    return out, cigs


def check_rows(out, cigs, idx):
    exp = V["f_expect"][idx].astype(np.int64)
    got = gv.six(out)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(NAMES[int(idx[b])], got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    assert (out["cells"] == V["f_cells"][idx]).all()
    assert [int(f) for f in out["form_used"]] == gv.forms_of(V, idx)
    wrong = [NAMES[int(i)] for k, i in enumerate(idx) if not np.array_equal(cigs[k], gv.decode_cigar(V["f_cigar"], V["f_cig_off"], int(i)))]
    assert not wrong, wrong[:8]


def test_whole_set_equals_reference(ctx, whole_set):
    out, cigs = whole_set
    check_rows(out, cigs, np.arange(N))
    assert set(int(f) for f in out["form_used"]) == {1, 2, 4, 8, 16, 32, 33}
    assert lv.pool_info(ctx).main_used == 0


def test_every_problem_alone(ctx, problems, whole_set):
    for i in range(N):
        out, cigs = gv.run_by_gap(ctx, problems[i:i + 1], V["f_gap"][i:i + 1])
        check_rows(out, cigs, np.array([i]))
        assert out[0] == whole_set[0][i], NAMES[i]


@pytest.mark.parametrize("batch", [1, 37])
def test_reversed_order_and_batches_give_the_same(ctx, problems, whole_set, batch):
    idx = np.arange(N - 1, -1, -1)
    for b in range(0, N, batch):
        sel = idx[b:b + batch]
        out, cigs = gv.run_by_gap(ctx, problems[sel], V["f_gap"][sel])
        check_rows(out, cigs, sel)
        assert (out == whole_set[0][sel]).all()


def test_a_small_pool_splits_the_call_into_launch_groups(problems):
    idx = np.array([k for k, n in enumerate(NAMES) if n.startswith(("edge_1025", "edge_2047", "edge_513", "tb_")) and V["f_gap"][k] == 0])
    assert sum(int(V["f_t_len"][k]) * 1024 for k in idx if V["f_slots"][k] > 1024) > (3 << 20)      # the C = 32 traces alone do not fit the 3 MB main pool together
    c = lv.make_context(V["words"], V["offs"], V["lens"], int(V["M"]), int(V["X"]), pool_bytes=6 << 20)
    try:
        out, cigs = gv.run_by_gap(c, problems[idx], V["f_gap"][idx])
        check_rows(out, cigs, idx)
        big = np.array([NAMES.index("rows_6000_slots_2047")])
        with pytest.raises(RuntimeError, match="error -3"):
            c.global_batch(problems[big], *gv.GAPS[0])
        out, cigs = gv.run_by_gap(c, problems[idx[:3]], V["f_gap"][idx[:3]])
        check_rows(out, cigs, idx[:3])
    finally:
        c.close()


def test_statistics_only_calls_equal_the_full_calls(ctx, problems, whole_set):
    out, _ = gv.run_by_gap(ctx, problems, V["f_gap"], cigar=False)
    full = whole_set[0].copy()
    full["cigar_len"] = 0
    assert (out == full).all()


def test_chain_equals_the_chain_table(ctx):
    pr = gv.chain_problems(V)
    c0 = ctx.counters()
    out, cigs = gv.run_chain_by_group(ctx, pr, V["c_w"], V["c_T"])
    got, exp = gv.twelve(out), V["c_expect"].astype(np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(str(V["c_names"][b]), got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    wrong = [str(V["c_names"][i]) for i in range(len(pr)) if not np.array_equal(cigs[i], gv.decode_cigar(V["c_cigar"], V["c_cig_off"], i))]
    assert not wrong, wrong
    i = [str(n) for n in V["c_names"]].index("all_A_all_C")
    assert not any(out[i].tolist())      # found = 0: KSWX_NULL
    i = [str(n) for n in V["c_names"]].index("skew_800")
    assert out["band"][i] > 1023 and out["form_used"][i] == 33      # the wide route from the chain
    c1 = ctx.counters()
    assert c1.n_kglob - c0.n_kglob == int(exp[:, 0].sum()) and c1.n_local - c0.n_local == len(pr)
    assert lv.pool_info(ctx).main_used == 0


def test_view_identities(ctx, problems, whole_set):
    """the same bases reached as a view inside a longer read and as whole reads of their own give the same result"""
    reads = lv.unpack_reads(V["words"], V["offs"], V["lens"])
    idx = np.array([k for k, n in enumerate(NAMES) if n.startswith("view_")])
    own = []
    for k in idx:
        p = problems[k]
        own.append(gv.view(reads, int(p["q_read"]), int(p["q_rev"]), int(p["q_from"]), int(p["q_strand"]), int(p["q_len"])))
        own.append(gv.view(reads, int(p["t_read"]), int(p["t_rev"]), int(p["t_from"]), int(p["t_strand"]), int(p["t_len"])))
    words, offs, lens = hipabi.pack_reads(own)
    c = lv.make_context(words, offs, lens, int(V["M"]), int(V["X"]))
    try:
        pr = lv.whole_read_problems(np.arange(0, 2 * idx.size, 2), np.arange(1, 2 * idx.size, 2), lens)
        pr["W"] = problems["W"][idx]
        out, cigs = gv.run_by_gap(c, pr, V["f_gap"][idx])
        assert (out == whole_set[0][idx]).all()
        assert all(np.array_equal(cigs[k], whole_set[1][int(i)]) for k, i in enumerate(idx))
    finally:
        c.close()


def test_limits_are_argument_errors_and_the_context_survives(ctx, problems, whole_set):
    one = problems[:2].copy()
    for field, value in (("q_len", 0), ("t_len", 65536), ("W", -1)):
        bad = one.copy()
        bad[field][1] = value
        with pytest.raises(RuntimeError, match="error -1"):
            ctx.global_batch(bad, 3, 1, 3, 1)
    with pytest.raises(RuntimeError, match="error -1"):
        ctx.alignx_batch(gv.chain_problems(V)[:2], hipabi.KEXT_MAXW + 1, -3, -3, -1, -100)
    sel = np.array([0, 1])
    out, cigs = gv.run_by_gap(ctx, problems[sel], V["f_gap"][sel])
    check_rows(out, cigs, sel)
    assert lv.pool_info(ctx).main_used == 0
