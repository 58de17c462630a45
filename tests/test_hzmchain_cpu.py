"""wtz_set_window_chaining (HZM_FAST_WINDOW_KMER_CHAINING of the reference, hzm_aln.h:36) on the host emulation of the device library: with 0 every window of a
scan is built by chaining_hzmps (hzm_aln.h:351-408, 544-561), as wtmsa and wtcns run align_hzmaux (wtmsa.c:617, wtcns.c:806).

The pin: tests/golden/hzmchain_vectors.npz (make_hzmchain_vectors.py), 101 calls of the reference's own compiled align_hzmaux with the flag at 0 - the 81 of
hzmreg_vectors.npz and 20 on two backbones with a tandem duplicate inside one window.  The ten kswx_t fields, every CIGAR word and the boxes of the chain windows
must be equal, through the one-call service and through the stage-level path.  All 81 calls with an interval (and all 20 without) differ from the flag-1 run of the
same recorder: with the switch left at 1 - or ignored - every one of them is missed (asserted).  91 calls have two matches of equal off2 less than zwin apart
(`tie`): the order inside a tie group is observable in the chain form and comes from the scan's exact path.  Beside it: the switch back, the clone, the errors, the
symbol, and what a call leaves behind when the pool runs out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hzmchainvec as cv
import hzmregvec as hv
from conftest import ROOT
from test_hzmaux_functions import same


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


@pytest.fixture(scope="module")
def vectors():
    return cv.load_vectors()


def test_the_file_meets_its_conditions(vectors):
    cases = [c for lay in vectors for c in lay["cases"]]
    reg = [c for c in cases if c["is_region"]]
    assert len(vectors) == 10 and len(reg) >= 50 and sum(c["want"] is None for c in reg) * 4 <= len(reg) and sum(c["differs"] for c in reg) * 4 >= 3 * len(reg)
    assert sum(c["tie"] for c in cases) >= 4
    assert {lay["prm"][13] for lay in vectors} == {-2, -3} and all(lay["prm"][13] == lay["prm"][14] for lay in vectors)
    assert all(c["tie"] for lay in vectors[8:] for c in lay["cases"][:6]), "a read across both copies of a tandem duplicate has off2 ties"


def test_recorded_vectors(vectors, emul_lib):
    assert cv.check_vectors(emul_lib, vectors) >= 2 * 90


@pytest.mark.parametrize("fast", [None, 1])
def test_the_fast_windows_miss_the_vectors(fast, vectors, emul_lib):
    """the switch untouched, or set to 1: exactly the cases recorded as differs_from_fast are missed"""
    nmiss = 0
    for lay, (got, _) in zip(vectors, cv.run_vectors(emul_lib, vectors, fast, "service")):
        for c, g in zip(lay["cases"], got):
            assert cv.equal(g, c["want"]) != c["differs"]
            nmiss += c["differs"]
    assert nmiss >= 60


def test_tie_cases_are_present_and_equal(vectors, emul_lib):
    """the calls with equal off2 values inside one window, alone: the tandem layouts (every read across both copies has them)"""
    lays = [dict(lay, cases=[c for c in lay["cases"] if c["tie"]]) for lay in vectors[8:]]
    assert sum(len(lay["cases"]) for lay in lays) >= 4
    assert cv.check_vectors(emul_lib, lays) >= 2 * 4


def test_switch_back_restores_the_fast_windows(emul_lib):
    """wtz_set_window_chaining(1) after (0): the calls of hzmreg_vectors.npz (flag 1) equal their record again; in between they do not"""
    lay = hv.load_vectors()[0]
    cs = lay["cases"]
    n = len(cs)
    tid, rid, beg, end = [0] * n, list(range(1, n + 1)), [c["beg"] for c in cs], [c["end"] for c in cs]
    ctx = hv.open_ctx(emul_lib, [lay["backbone"]] + [c["read"] for c in cs], prm=lay["prm"], min_sm=lay["min_sm"])
    try:
        ctx.set_window_chaining(0)
        chained = hv.service(ctx, tid, rid, beg, end)
        ctx.set_window_chaining(1)
        back = hv.service(ctx, tid, rid, beg, end)
    finally:
        ctx.close()
    want = [c["want"] for c in cs]
    assert same(want, back, "reference (flag 1) vs the switch set back") >= n - 1
    assert not any(cv.equal(g, w) for g, w in zip(chained, want))


def test_clone_inherits_the_setting(vectors, emul_lib):
    lay = vectors[8]
    cs = lay["cases"]
    n = len(cs)
    ctx = hv.open_ctx(emul_lib, [lay["backbone"]] + [c["read"] for c in cs], prm=lay["prm"], min_sm=lay["min_sm"])
    try:
        ctx.set_window_chaining(0)
        twin = ctx.clone()
        try:
            ctx.set_window_chaining(1)      # the clone keeps what it copied
            got = hv.service(twin, [0] * n, list(range(1, n + 1)), [c["beg"] for c in cs], [c["end"] for c in cs])
        finally:
            twin.close()
    finally:
        ctx.close()
    assert same([c["want"] for c in cs], got, "reference vs the clone") >= n - 1


def test_argument_errors(emul_lib):
    from smartdenovo_amd import hipabi
    for kw in (dict(aux_strand=0), dict(dot_matrix=1)):
        P = hv.params()
        for k, v in kw.items():
            setattr(P, k, v)
        ctx = hipabi.Context(P, pool_bytes=64 << 20, lib_path=emul_lib)
        try:
            with pytest.raises(RuntimeError, match="error -1.*aux_strand"):      # WTZ_E_ARG
                ctx.set_window_chaining(0)
            ctx.set_window_chaining(1)                                            # the default is always allowed
        finally:
            ctx.close()
    assert hipabi.load(emul_lib).wtz_set_window_chaining(None, 0) == -1


def test_symbol_is_exported(emul_lib):
    from smartdenovo_amd import hipabi
    assert "wtz_set_window_chaining" in hipabi.SYMBOLS
    hipabi.check_symbols(emul_lib)
    assert "wtz_set_window_chaining" in open(os.path.join(ROOT, "include", "wtzmo_hip.h")).read()


def test_pool_exhaustion_leaves_nothing_and_the_halves_equal_the_record(vectors, emul_lib):
    """the 8 MiB shape of test_hzmreg_cpu.py in chain form: the one call over the first layout fails (WTZ_E_POOL), the main pool is empty afterwards, no batch is left,
    and the calls over its halves equal the record"""
    lay = vectors[0]
    cs = lay["cases"]
    n = len(cs)
    ctx = hv.open_ctx(emul_lib, [lay["backbone"]] + [c["read"] for c in cs], pool_bytes=8 << 20, prm=lay["prm"], min_sm=lay["min_sm"])
    try:
        ctx.set_window_chaining(0)
        tid, rid, beg, end = [0] * n, list(range(1, n + 1)), [c["beg"] for c in cs], [c["end"] for c in cs]
        with pytest.raises(RuntimeError, match="error -3"):      # WTZ_E_POOL
            ctx.hzmaux_batch(tid, rid, beg, end)
        info = np.zeros(4, dtype=np.uint64)      # wtz_pool_info_t: main_cap, main_used, transient_cap, transient_peak
        ctx.lib.wtz_pool_info.argtypes = [C.c_void_p, C.c_void_p]
        assert ctx.lib.wtz_pool_info(ctx.h, info.ctypes.data) == 0 and info[1] == 0, "the main pool is still in use"
        with pytest.raises(RuntimeError, match="error -4"):      # no batch left to continue
            ctx.pairs_align([0], [0])
        h = n // 2
        got = hv.service(ctx, tid[:h], rid[:h], beg[:h], end[:h]) + hv.service(ctx, tid[h:], rid[h:], beg[h:], end[h:])
    finally:
        ctx.close()
    assert same([c["want"] for c in cs], got, "reference vs the halves") >= n - 1
