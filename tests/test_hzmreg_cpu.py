"""The region form of align_hzmaux (hzm_aln.h:1684-1775 with beg / end: wtz_pairs_seed_region, wtz_hzmaux_batch) on the host emulation of the device
library: the product's own task bodies with one lane.

The pin: tests/golden/hzmreg_vectors.npz, 65 calls with an interval and 16 with (0, -1), recorded from the reference's own compiled align_hzmaux
(tests/golden/make_hzmreg_vectors.py: a driver of a few lines around hzm_aln.h, not wtmsa - wtmsa.c:617 sets HZM_FAST_WINDOW_KMER_CHAINING = 0 and so switches the
window scan to the chaining_hzmps branch, hzm_aln.h:544-, which the device does not have).  58 of the 65 differ from what the whole form gives on the same pair: an
implementation that ignores the interval misses them (asserted).  The ten kswx_t fields and every CIGAR word must be equal, through the one-call service and
through the stage-level path.  Beside it: n_hits of the seed stage against a model of query_single_read_seeds_by_region (hzm_aln.h:117-171) written from the
reference's text (tests/hzmregvec.py), the degenerate intervals against the whole form and the reference's compiled routine, the empty interval, the errors, and
what a call leaves behind when the pool runs out.

Break, not continue (hzm_aln.h:161): inside one run of the index, off + len never decreases (off + len = j + 1 for the z-mer ending at base j, hzm_aln.h:98-99, runs
are in off order, i.e. in j order; the cap at 0xFFFF keeps that), so on an index built by index_single_read_seeds no later occurrence can fit once one has ended
behind `end`: the two walks keep the same matches, and no case can tell them apart.  test_run_cut_at_every_boundary asserts that on its hand-built run and
pins the count at every cut position instead."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hzmregvec as hv
from conftest import ROOT
from test_hzmaux_functions import SHIM, WTGBO, Aln, make_pairs, run_cpu, same  # noqa: F401

Z, HZ, ZMAX, ZVAR = WTGBO[0], WTGBO[1], WTGBO[5], WTGBO[6]


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


@pytest.fixture(scope="module")
def vectors():
    return hv.load_vectors()


def check_vectors(lib_path, lays):
    """shared with test_gpu_hzmreg.py: the service and the stage-level path equal the record, field for field and CIGAR word for CIGAR word; the CIGARs fold"""
    nhit = 0
    for how in ("service", "stages"):
        for lay, (got, want) in zip(lays, hv.run_vectors(lib_path, lays, how)):
            nhit += same(want, got, "reference vs " + how)
            for c, g in zip(lay["cases"], got):
                if g is not None:
                    x, cig = g
                    assert hv.fold_cigar(lay["backbone"], c["read"], x, cig) == (x[2], x[4], x[6], x[7], x[8], x[9]) and x[5] == x[6] + x[7] + x[8] + x[9]
    return nhit


def test_recorded_vectors(vectors, emul_lib):
    cases = [c for lay in vectors for c in lay["cases"]]
    reg = [c for c in cases if c["is_region"]]
    assert len(reg) >= 40 and sum(c["want"] is None for c in reg) * 4 <= len(reg) and sum(c["differs"] for c in reg) >= 4
    assert {lay["prm"][13] for lay in vectors} == {-2, -3} and all(lay["prm"][13] == lay["prm"][14] for lay in vectors)
    assert check_vectors(emul_lib, vectors) >= 2 * 60


def test_ignoring_the_interval_misses_the_vectors(vectors, emul_lib):
    """the whole form on the same pairs: it must miss every case recorded as differs_from_whole and meet every other"""
    for lay, (got, want) in zip(vectors, hv.run_vectors(emul_lib, vectors, "whole")):
        for c, g, w in zip(lay["cases"], got, want):
            eq = (g is None) == (w is None) and (g is None or (g[0] == w[0] and np.array_equal(g[1], w[1])))
            assert eq != c["differs"]


LAYOUTS = [dict(seed=11, glen=12000, nreads=6), dict(seed=12, glen=16000, nreads=6, repeat=(1800, 4000)), dict(seed=13, glen=14000, nreads=6, repeat=(1500, 3000))]


@pytest.fixture(scope="module")
def layouts():
    return [hv.layout(**kw) for kw in LAYOUTS]


@pytest.mark.parametrize("k", range(len(LAYOUTS)))
def test_match_counts_equal_the_reference_walk(k, layouts, emul_lib):
    G, reads, iv = layouts[k]
    n = len(reads)
    ctx = hv.open_ctx(emul_lib, [G] + reads)
    try:
        tid, rid = [0] * n, list(range(1, n + 1))
        reg = ctx.pairs_seed_region(tid, rid, [b for b, _ in iv], [e for _, e in iv])
        assert ctx.lib.wtz_batch_begin(ctx.h) == 0
        whole = ctx.pairs_seed(tid, rid)
    finally:
        ctx.close()
    want = [len(hv.model_matches(G, reads[i], Z, HZ, ZMAX, ZVAR, *iv[i])) for i in range(n)]
    full = [len(hv.model_matches(G, reads[i], Z, HZ, ZMAX, ZVAR, 0, 0)) for i in range(n)]
    assert [int(v) for v in reg["n_hits"]] == want
    assert [int(v) for v in whole["n_hits"]] == full
    assert sum(w < f for w, f in zip(want, full)) >= n - 1, "the intervals of this layout exclude nothing: the case shows nothing"
    assert min(want) > 50


def test_service_equals_stage_path_and_cigars_fold(layouts, emul_lib):
    G, reads, iv = layouts[1]
    n = len(reads)
    seqs = [G] + reads
    lens = [s.size for s in seqs]
    tid, rid = [0] * n + [0], list(range(1, n + 1)) + [1]
    beg, end = [b for b, _ in iv] + [0], [e for _, e in iv] + [-1]      # the last pair: an N read's whole form (wtmsa.c:472-475)
    ctx = hv.open_ctx(emul_lib, seqs)
    try:
        a = hv.service(ctx, tid, rid, beg, end)
        b = hv.stages(ctx, lens, tid, rid, beg, end)
    finally:
        ctx.close()
    assert same(a, b, "service vs stages") >= n - 1
    for i, r in enumerate(a):
        if r is None:
            continue
        x, cig = r
        assert hv.fold_cigar(G, seqs[rid[i]], x, cig) == (x[2], x[4], x[6], x[7], x[8], x[9])
        assert x[5] == x[6] + x[7] + x[8] + x[9]


@pytest.mark.parametrize("refine", [0, 1])
def test_degenerate_intervals_give_the_whole_form(refine, emul_lib):
    pairs = make_pairs(53, 16)
    seqs = [s for tq in pairs for s in tq]
    lens = [s.size for s in seqs]
    n = len(pairs)
    tid, rid = [2 * i for i in range(n)], [2 * i + 1 for i in range(n)]
    ctx = hv.open_ctx(emul_lib, seqs, refine=refine)
    try:
        whole = hv.whole_form(ctx, lens, tid, rid, refine=refine)
        nhit = 0
        for beg, end in ([0] * n, [0] * n), ([-5] * n, [-1] * n), ([0] * n, [lens[t] + 100 for t in tid]):
            nhit = same(whole, hv.service(ctx, tid, rid, beg, end), "whole form vs service")
            same(whole, hv.stages(ctx, lens, tid, rid, beg, end, refine=refine), "whole form vs stages")
    finally:
        ctx.close()
    assert nhit >= 5
    if os.path.exists(SHIM):
        import ctypes as C
        same(run_cpu(C.CDLL(SHIM).ref_align_hzmaux, pairs, WTGBO, hv.MIN_SM, refine), whole, "reference vs whole form")


def test_empty_interval_finds_nothing(layouts, emul_lib):
    G, reads, _ = layouts[0]
    ctx = hv.open_ctx(emul_lib, [G] + reads[:3])
    try:
        beg, end = [500, 3000, G.size + 10], [500, 2000, G.size + 20]
        summ = ctx.pairs_seed_region([0] * 3, [1, 2, 3], beg, end)
        res, cig = ctx.hzmaux_batch([0] * 3, [1, 2, 3], beg, end)
    finally:
        ctx.close()
    assert not summ["n_hits"].any() and not summ["gate"].any()
    assert not res["found"].any() and cig.size == 0


def test_run_cut_at_every_boundary(emul_lib):
    """one z-mer at three offsets of the target, the middle occurrence two bases longer (a homopolymer run inside it, within -l 2); `end` at, one in front of and
    one behind the end of each occurrence.  The expected counts come from the model of hzm_aln.h:158-168; the walk with `continue` for the break keeps the same
    matches at every position (module docstring), which is asserted, not assumed."""
    rng = np.random.default_rng(5)

    def rnd(n):
        s = rng.integers(0, 4, size=n, dtype=np.uint8)
        for i in range(1, n):      # no homopolymers in the filler: every length is its compressed length
            while s[i] == s[i - 1]:
                s[i] = rng.integers(0, 4)
        return s
    U = np.array([0, 1, 2, 3, 1, 0, 2, 1, 3, 0], dtype=np.uint8)          # ACGTCAGCTA: not its own reverse complement
    U2 = np.array([0, 1, 2, 3, 1, 1, 1, 0, 2, 1, 3, 0], dtype=np.uint8)    # the same z-mer with CCC for its second C: len 12
    sep, st = np.array([2], dtype=np.uint8), np.array([3], dtype=np.uint8)  # keep the fillers from extending a run of U; different in T and Q, so that no z-mer across an edge of U matches
    T = np.concatenate([rnd(300), st, U, st, rnd(200), st, U2, st, rnd(200), st, U, st, rnd(300)])
    Q = np.concatenate([rnd(150), sep, U, sep, rnd(150)])
    occ = [(o, ln) for m, d, o, ln in hv.zmers(T, Z, HZ) if (m, d) == hv.zmers(U, Z, HZ)[0][:2]]
    assert [ln for _, ln in occ] == [10, 12, 10]
    ends = sorted({o + ln + d for o, ln in occ for d in (-1, 0, 1)})
    begs = [0] * len(ends) + [occ[0][0] + 1, occ[1][0], occ[1][0] + 1]
    ends = ends + [0, 0, occ[2][0] + 9]
    kept = [hv.model_matches(T, Q, Z, HZ, ZMAX, ZVAR, b, e) for b, e in zip(begs, ends)]
    assert kept == [hv.model_matches(T, Q, Z, HZ, ZMAX, ZVAR, b, e, cut="continue") for b, e in zip(begs, ends)]
    assert sorted({sum(m[1] == 151 for m in k) for k in kept}) == [0, 1, 2, 3]      # of the run of U (at base 151 of Q); the fillers add a few chance matches
    want = [len(k) for k in kept]
    ctx = hv.open_ctx(emul_lib, [T, Q])
    try:
        got = ctx.pairs_seed_region([0] * len(begs), [1] * len(begs), begs, ends)
    finally:
        ctx.close()
    assert [int(v) for v in got["n_hits"]] == want


def test_pool_exhaustion_leaves_nothing_and_the_halves_equal_the_record(vectors, emul_lib):
    """8 MiB: on the emulation the largest pool (of 1, 2, 3, 4, 6, 8, 12 MiB tried) at which the one call over the first layout fails, in wtz_pairs_align, and the calls over
    its halves succeed: what a caller's halving loop (ht_halving) goes through"""
    lay = vectors[0]
    cs = lay["cases"]
    n = len(cs)
    ctx = hv.open_ctx(emul_lib, [lay["backbone"]] + [c["read"] for c in cs], pool_bytes=8 << 20, prm=lay["prm"], min_sm=lay["min_sm"])
    try:
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


def test_argument_errors(layouts, emul_lib):
    G, reads, iv = layouts[0]
    seqs = [G] + reads[:2]
    ctx = hv.open_ctx(emul_lib, seqs, aux_strand=0)
    try:
        with pytest.raises(RuntimeError, match="error -1"):      # WTZ_E_ARG
            ctx.hzmaux_batch([0], [1], [0], [0])
        with pytest.raises(RuntimeError, match="error -1"):
            ctx.pairs_seed_region([0], [1], [0], [0])
    finally:
        ctx.close()
    ctx = hv.open_ctx(emul_lib, seqs, subset=[1, 2])
    try:
        with pytest.raises(RuntimeError, match="error -4"):      # WTZ_E_STATE: the target has no z-index
            ctx.hzmaux_batch([0], [1], [0], [0])
        ctx.zindex_build_subset([0, 1])
        assert ctx.hzmaux_batch([0], [1], [iv[0][0]], [iv[0][1]])[0]["found"][0] == 1
        with pytest.raises(RuntimeError, match="error -4"):      # ... nor may the read be missing: its z-mers are read from the index too
            ctx.hzmaux_batch([0], [2], [0], [0])
        from smartdenovo_amd import hipabi
        out = np.zeros(1, dtype=hipabi.HZMAUX_RESULT); one = np.zeros(1, dtype=np.uint32)
        args = [np.array([v], dtype=t) for v, t in ((0, np.uint32), (1, np.uint32), (0, np.int32), (0, np.int32))]
        rc = ctx.lib.wtz_hzmaux_batch(ctx.h, *[a.ctypes.data for a in args], 1, out.ctypes.data, one.ctypes.data, 1)
        assert rc == -1 and b"words needed" in ctx.lib.wtz_last_error() and out["found"][0] == 1 and out["cigar_len"][0] > 1
    finally:
        ctx.close()
