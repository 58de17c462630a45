"""The region form of align_hzmaux on the MI355X (wtz_pairs_seed_region = K_pair_region, wtz_hzmaux_batch): the vectors recorded from the reference's own
compiled routine (tests/golden/hzmreg_vectors.npz), field for field and CIGAR word for CIGAR word; the wave-cooperative match stage against the model
of the reference's walk and against the same task bodies run with one lane (the host emulation), the degenerate intervals against the whole form and the
reference's compiled align_hzmaux, the one-call service against the stage-level path, and one layout - a backbone and all of its reads, each with its own
interval - in one call.  What is and is not pinned: tests/test_hzmreg_cpu.py."""
import os
import subprocess

import pytest

import hzmregvec as hv
from conftest import ROOT
from test_hzmaux_functions import SHIM, WTGBO, make_pairs, run_cpu, same

pytestmark = pytest.mark.gpu
Z, HZ, ZMAX, ZVAR = WTGBO[0], WTGBO[1], WTGBO[5], WTGBO[6]


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


@pytest.fixture(scope="module")
def big_layout():
    """the layout shape of INTEGRATION: one backbone of 20 kb with an exact 1.8 kb duplicate, ten reads"""
    return hv.layout(seed=21, glen=20000, nreads=10, repeat=(1800, 5000))


def test_recorded_vectors():
    """tests/golden/hzmreg_vectors.npz (the reference's compiled align_hzmaux with beg / end, 81 calls) through the service and through the stage-level path"""
    from test_hzmreg_cpu import check_vectors
    assert check_vectors(None, hv.load_vectors()) >= 2 * 60


def test_recorded_layout_in_one_call_from_a_subset_index():
    """the layout shape of INTEGRATION on the largest recorded backbone: the z-index holds the backbone and its reads only, one call"""
    lay = max(hv.load_vectors(), key=lambda x: x["backbone"].size)
    cs = lay["cases"]
    ctx = hv.open_ctx(None, [lay["backbone"]] + [c["read"] for c in cs] + [lay["backbone"][::-1].copy()], subset=range(len(cs) + 1), prm=lay["prm"], min_sm=lay["min_sm"])
    try:
        got = hv.service(ctx, [0] * len(cs), list(range(1, len(cs) + 1)), [c["beg"] for c in cs], [c["end"] for c in cs])
    finally:
        ctx.close()
    assert same([c["want"] for c in cs], got, "reference vs one call per layout") >= len(cs) - 2


def _layout_call(lib_path, lay):
    G, reads, iv = lay
    n = len(reads)
    seqs = [G] + reads
    lens = [s.size for s in seqs]
    tid, rid = [0] * (n + 2), list(range(1, n + 1)) + [1, 2]
    beg, end = [b for b, _ in iv] + [0, 0], [e for _, e in iv] + [-1, -1]      # the last two as N reads: the whole backbone (wtmsa.c:472-475)
    ctx = hv.open_ctx(lib_path, seqs, subset=range(n + 1))
    try:
        svc = hv.service(ctx, tid, rid, beg, end)
        stg = hv.stages(ctx, lens, tid, rid, beg, end)
        summ = ctx.pairs_seed_region(tid, rid, beg, end)
    finally:
        ctx.close()
    return svc, stg, [int(v) for v in summ["n_hits"]], (G, seqs, tid, rid, beg, end)


def test_layout_in_one_call(big_layout, emul_lib):
    svc, stg, nh, (G, seqs, tid, rid, beg, end) = _layout_call(None, big_layout)
    assert nh == [len(hv.model_matches(G, seqs[r], Z, HZ, ZMAX, ZVAR, b, e)) for r, b, e in zip(rid, beg, end)]
    assert nh[0] < nh[-2] and nh[1] < nh[-1], "the interval excluded nothing"
    assert same(svc, stg, "service vs stages") >= 10
    e_svc, e_stg, e_nh, _ = _layout_call(emul_lib, big_layout)
    assert nh == e_nh
    same(e_svc, svc, "one lane vs wavefront, service")
    same(e_stg, stg, "one lane vs wavefront, stages")
    for i, r in enumerate(svc):
        if r is not None:
            x, cig = r
            assert hv.fold_cigar(G, seqs[rid[i]], x, cig) == (x[2], x[4], x[6], x[7], x[8], x[9]) and x[5] == x[6] + x[7] + x[8] + x[9]


@pytest.mark.parametrize("refine", [0, 1])
def test_degenerate_intervals_give_the_whole_form(refine):
    pairs = make_pairs(59, 48)
    seqs = [s for tq in pairs for s in tq]
    lens = [s.size for s in seqs]
    n = len(pairs)
    tid, rid = [2 * i for i in range(n)], [2 * i + 1 for i in range(n)]
    ctx = hv.open_ctx(None, seqs, refine=refine)
    try:
        whole = hv.whole_form(ctx, lens, tid, rid, refine=refine)
        for beg, end in ([0] * n, [0] * n), ([-5] * n, [-1] * n), ([0] * n, [lens[t] + 100 for t in tid]):
            assert same(whole, hv.service(ctx, tid, rid, beg, end), "whole form vs service") >= 15
            same(whole, hv.stages(ctx, lens, tid, rid, beg, end, refine=refine), "whole form vs stages")
    finally:
        ctx.close()
    if os.path.exists(SHIM):
        import ctypes as C
        same(run_cpu(C.CDLL(SHIM).ref_align_hzmaux, pairs, WTGBO, hv.MIN_SM, refine), whole, "reference vs whole form")


def test_empty_interval_and_argument_errors(big_layout):
    G, reads, iv = big_layout
    seqs = [G] + reads[:2]
    ctx = hv.open_ctx(None, seqs, subset=[0, 1])
    try:
        res, cig = ctx.hzmaux_batch([0, 0], [1, 1], [700, G.size + 5], [700, G.size + 9])
        assert not res["found"].any() and cig.size == 0
        with pytest.raises(RuntimeError, match="error -4"):
            ctx.hzmaux_batch([0], [2], [0], [0])
    finally:
        ctx.close()
    ctx = hv.open_ctx(None, seqs, aux_strand=0)
    try:
        with pytest.raises(RuntimeError, match="error -1"):
            ctx.hzmaux_batch([0], [1], [0], [0])
    finally:
        ctx.close()
