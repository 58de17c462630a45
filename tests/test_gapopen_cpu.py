"""wtz_set_gap_open (separate insertion / deletion gap-open costs: the I and D of align_hzmaux, hzm_aln.h:1684) on the host emulation of the device library.

The pins: tests/golden/hzmid_vectors.npz (make_hzmid_vectors.py) - 42 calls of the reference's own compiled align_hzmaux as wtmsa runs it, windows by
chaining_hzmps and I = -2, D = -3 (wtmsa.c:617, 633-634) - through the one-call service and through the stage path: the ten fields and every CIGAR word; and
tests/golden/dpid_vectors.npz (make_dpid_vectors.py) - the 200 problems of dp_vectors.npz through the reference's three DP routines at (-2, -3) and at (-3, -2) -
through the scalar bodies behind wtz_test_dp.  Every hzmid call differs from the same call at (-2, -2) and at (-3, -3): with the setter not called, whatever
params.O is, exactly those are missed (asserted - this is what fails without the feature).  Beside it: (O, O) reproduces the committed I = D vectors, the clone,
the errors, the symbol."""
import os
import subprocess

import numpy as np
import pytest

import dpidvec
import hzmidvec as iv
import hzmchainvec as cv
from conftest import ROOT
from dpvec import Vectors
from test_hzmaux_functions import same

FIELDS = ("score", "tb", "te", "qb", "qe", "aln", "mat", "mis", "ins", "del")
SCALAR_FORM = {0: 4, 1: 255, 2: 255}


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


@pytest.fixture(scope="module")
def vectors():
    return iv.load_vectors()


def test_the_files_meet_their_conditions(vectors):
    cases = [c for lay in vectors for c in lay["cases"]]
    reg = [c for c in cases if c["is_region"]]
    hits = [c for c in cases if c["want"] is not None]
    assert len(vectors) == 4 and len(cases) >= 30 and 0 < len(reg) < len(cases)
    assert sum(c["want"] is None for c in reg) * 4 <= len(reg) and sum(c["differs"] for c in hits) * 2 >= len(hits)
    assert all(c["differs"] == (c["differs_m2"] and c["differs_m3"]) for c in cases)
    assert all((lay["prm"][13], lay["prm"][14]) == (iv.I, iv.D) for lay in vectors)
    from test_gpu_dp_forms import SHIFT_MUST
    for b, costs in enumerate(((-2, -3), (-3, -2))):
        blk = dpidvec.Block(b)
        assert (blk.I, blk.D) == costs and blk.n == Vectors().n and (blk.cls == Vectors().cls).all()
        for kind in (0, 1, 2):
            assert blk.differs[blk.kind == kind].sum() * 3 >= (blk.kind == kind).sum()
        for cls in set().union(*SHIFT_MUST.values()):
            assert blk.differs[blk.cls == cls].any(), "no problem of class %s tells the two costs apart" % cls


@pytest.mark.parametrize("how", ["service", "stages"])
def test_recorded_calls_at_wtmsas_defaults(how, vectors, emul_lib):
    """set_gap_open(-2, -3) + set_window_chaining(0): the record in every field and CIGAR word; params.O (here -3) is read by nothing"""
    ctx, lens, tid, rid, beg, end = iv.open_all(emul_lib, vectors, -3)
    try:
        ctx.set_gap_open(iv.I, iv.D)
        got = iv.run(ctx, how, lens, tid, rid, beg, end, vectors[0]["min_sm"])
    finally:
        ctx.close()
    assert same(iv.wants(vectors), got, "reference vs " + how) >= 40
    assert all(cv.equal(g, w) for g, w in zip(got, iv.wants(vectors)))


@pytest.mark.parametrize("O", [-2, -3])
def test_one_cost_misses_exactly_the_differs_cases(O, vectors, emul_lib):
    """the setter not called, params.O at -2 or at -3: exactly the calls recorded as differing from that single cost are missed"""
    ctx, lens, tid, rid, beg, end = iv.open_all(emul_lib, vectors, O)
    try:
        got = iv.run(ctx, "service", lens, tid, rid, beg, end, vectors[0]["min_sm"])
    finally:
        ctx.close()
    key = "differs_m2" if O == -2 else "differs_m3"
    cases = [c for lay in vectors for c in lay["cases"]]
    nmiss = 0
    for c, g in zip(cases, got):
        assert cv.equal(g, c["want"]) != c[key]
        nmiss += c[key]
    assert nmiss >= 20


def test_equal_costs_reproduce_the_committed_vectors(vectors, emul_lib):
    """set_gap_open(-3, -3) in a context made with params.O = -2: the (-3, -3) records of the same calls in hzmchain_vectors.npz; and back to (-2, -3)"""
    ctx, lens, tid, rid, beg, end = iv.open_all(emul_lib, vectors, -2)
    try:
        ctx.set_gap_open(-3, -3)
        got33 = iv.run(ctx, "service", lens, tid, rid, beg, end, vectors[0]["min_sm"])
        ctx.set_gap_open(iv.I, iv.D)
        got23 = iv.run(ctx, "stages", lens, tid, rid, beg, end, vectors[0]["min_sm"])
    finally:
        ctx.close()
    assert all(cv.equal(g, w) for g, w in zip(got33, iv.chain_wants(vectors)))
    assert all(cv.equal(g, w) for g, w in zip(got23, iv.wants(vectors)))


def _dp_problems(vec, idx):
    from test_gpu_dp_forms import problems
    return problems(vec, idx)


def _check_dp(vec, kind, out, cigs, idx):
    from test_gpu_dp_forms import check
    ans = check(vec, idx, out, cigs, kind, SCALAR_FORM[kind], lambda c: True)
    assert sum(a for a, _ in ans.values()) == len(idx)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_scalar_forms_at_both_cost_pairs(kind, emul_lib):
    """wtz_test_dp's scalar forms (SHIFT 4, FIXED 255, GLOBAL 255) == the reference's routines at (-2, -3) and at (-3, -2), every problem of the file"""
    from smartdenovo_amd import hipabi
    for b in (0, 1):
        vec = dpidvec.Block(b)
        for w in (sorted(set(vec.w_param[vec.kind == 1].tolist())) if kind == 1 else [50]):
            idx = [int(i) for i in np.nonzero((vec.kind == kind) & ((vec.w_param == w) | (kind != 1)))[0]]
            assert idx
            ctx = hipabi.Context(hipabi.Params.defaults(w=w), pool_bytes=1 << 30, lib_path=emul_lib)
            try:
                ctx.upload(*hipabi.pack_reads(vec.reads()))
                ctx.set_gap_open(vec.I, vec.D)
                out, cigs = ctx.test_dp(kind, SCALAR_FORM[kind], _dp_problems(vec, idx))
                _check_dp(vec, kind, out, cigs, idx)
            finally:
                ctx.close()


def test_equal_costs_reproduce_the_dp_vectors(emul_lib):
    """set_gap_open(O, O), and the setter not called: dp_vectors.npz (recorded at I = D = O)"""
    from smartdenovo_amd import hipabi
    vec = Vectors()
    idx = [int(i) for i in np.nonzero(vec.kind == 0)[0]]
    for setter in (False, True):
        ctx = hipabi.Context(hipabi.Params.defaults(), pool_bytes=1 << 30, lib_path=emul_lib)
        try:
            ctx.upload(*hipabi.pack_reads(vec.reads()))
            if setter:
                ctx.set_gap_open(-2, -3)
                ctx.set_gap_open(vec.meta["scores"]["O"], vec.meta["scores"]["O"])
            out, cigs = ctx.test_dp(0, 4, _dp_problems(vec, idx))
            _check_dp(vec, 0, out, cigs, idx)
        finally:
            ctx.close()


def test_clone_inherits_the_setting(vectors, emul_lib):
    lays = vectors[:1]
    ctx, lens, tid, rid, beg, end = iv.open_all(emul_lib, lays, -3)
    try:
        ctx.set_gap_open(iv.I, iv.D)
        twin = ctx.clone()
        try:
            ctx.set_gap_open(-3, -3)      # the clone keeps what it copied
            got = iv.run(twin, "service", lens, tid, rid, beg, end, lays[0]["min_sm"])
        finally:
            twin.close()
    finally:
        ctx.close()
    assert all(cv.equal(g, w) for g, w in zip(got, iv.wants(lays)))


def test_argument_errors(vectors, emul_lib):
    from smartdenovo_amd import hipabi
    lays = vectors[:1]
    ctx, lens, tid, rid, beg, end = iv.open_all(emul_lib, lays, -3)
    try:
        ctx.set_gap_open(iv.I, iv.D)
        for bad in ((1, -3), (-2, 1), (3, 3), (-2, -(1 << 20) - 1)):
            with pytest.raises(RuntimeError, match="error -1.*wtz_set_gap_open"):      # WTZ_E_ARG
                ctx.set_gap_open(*bad)
        got = iv.run(ctx, "service", lens, tid, rid, beg, end, lays[0]["min_sm"])      # the setting stayed as it was
        ctx.set_gap_open(0, 0)                                                          # a cost of zero is a setting like any other
    finally:
        ctx.close()
    assert all(cv.equal(g, w) for g, w in zip(got, iv.wants(lays)))
    lib = hipabi.load(emul_lib)
    lib.wtz_set_gap_open.argtypes = [hipabi.C.c_void_p, hipabi.C.c_int32, hipabi.C.c_int32]
    assert lib.wtz_set_gap_open(None, -2, -3) == -1


def test_symbol_is_exported(emul_lib):
    from smartdenovo_amd import hipabi
    assert "wtz_set_gap_open" in hipabi.SYMBOLS
    hipabi.check_symbols(emul_lib)
    assert "wtz_set_gap_open" in open(os.path.join(ROOT, "include", "wtzmo_hip.h")).read()
    P = hipabi.Params.defaults()
    assert hipabi.C.sizeof(P) == 36 * 4, "wtz_params_c changed its size"
