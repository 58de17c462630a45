"""wtz_local_batch without a GPU: the DP body of smartdenovo_amd/csrc/wtz_sw_local.h, compiled into the host emulation of the library (tests/emul,
one lane instead of 64: strips of 4 / 16 columns, every strip boundary through the pool), is the CPU restatement of the reference's
ksw_align2(..., KSW_XSTART) (ksw.c:344-366 over ksw_i16).  It must give the five ints of the reference
  - for every problem of tests/golden/local_vectors.npz (dumped from the reference routine by tests/golden/make_local_vectors.py), and
  - where oracle/_ref/libref_shim.so exists, for 2 000 fresh seeded pairs against the routine called live.  That second check is the one that decides
    the two points the restatement rests on: the reference feeds E from H before its lazy-F loop, and it pads the query with zero-score cells."""
import os
import subprocess

import numpy as np
import pytest

import localvec as lv
from smartdenovo_amd import hipabi

ROOT = lv.ROOT


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


def test_vector_file_holds_the_cases_the_feature_names():
    v = lv.load_vectors()
    names = [str(x) for x in v["names"]]
    lens = v["lens"].astype(np.int64)
    ql, tl = lens[v["q_read"]], lens[v["t_read"]]
    assert len(names) >= 300 and len(set(names)) == len(names)
    assert max(ql.max(), tl.max()) <= 20000
    assert os.path.getsize(lv.VECTORS) < (1 << 19)
    assert {1, 7, 8, 9, 63, 64, 65, 1025} <= set(int(x) for x in ql)
    for prefix in ("unrelated_", "shared_same_", "shared_opposite_", "cyc_palindrome_", "all_A_", "gap_80_columns", "gap_600_columns", "gap_80_rows", "gap_600_rows", "identical_17000"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert set(int(g) for g in v["gap"]) == {0, 1, 2, 3} and lv.GAPS[1][0] != lv.GAPS[1][2]
    e = v["expect"]
    assert (e[[names.index("identical_17000_saturating"), names.index("identical_17000_one_substitution_at_16500")], 0] == 32767).all()
    # the long gaps are really crossed: the alignment spans more than the two flanks minus the gap on one sequence
    for n in ("gap_600_columns_g0", "gap_600_rows_g0"):
        i = names.index(n)
        assert abs((e[i, 1] - e[i, 3]) - (e[i, 2] - e[i, 4])) >= 512


def test_restatement_equals_reference_vectors(emul_lib):
    v = lv.load_vectors()
    ctx = lv.make_context(v["words"], v["offs"], v["lens"], int(v["M"]), int(v["X"]), lib_path=emul_lib)
    try:
        out = lv.run_by_gap(ctx, lv.whole_read_problems(v["q_read"], v["t_read"], v["lens"]), v["gap"])
    finally:
        ctx.close()
    got = lv.five(out)
    bad = np.nonzero((got != v["expect"]).any(axis=1))[0]
    assert bad.size == 0, [(str(v["names"][b]), got[b].tolist(), v["expect"][b].tolist()) for b in bad[:8]]
    assert (out["cells"] >= v["lens"][v["q_read"]].astype(np.uint64) * v["lens"][v["t_read"]].astype(np.uint64)).all()


def _mutate(rng, s, rate):
    out, i = [], 0
    while i < len(s):
        r = rng.random()
        if r < rate * 0.4:
            out.append(int(rng.integers(4)))
            out.append(int(s[i]))
        elif r < rate * 0.8:
            i += int(rng.integers(6)) if rng.random() < 0.3 else 0
        elif r < rate:
            out.append((int(s[i]) + 1 + int(rng.integers(3))) % 4)
        else:
            out.append(int(s[i]))
        i += 1
    return np.array(out if out else [0], dtype=np.uint8)


@pytest.mark.skipif(not lv.have_shim(), reason="needs oracle/_ref/libref_shim.so (the reference's ksw.c compiled where its sources are)")
def test_restatement_equals_live_ksw_align2_on_fresh_pairs(emul_lib):
    """2 000 pairs, lengths 1-300, gap-rich (a quarter unrelated, the rest mutated at 12 % / 25 % with deletion runs, a third over a two-letter
    alphabet: many ties), both gap-cost settings (equal and unequal opening costs).  Mismatches allowed: 0."""
    rng = np.random.default_rng(7)
    seqs, gi = [], []
    N = 2000
    for n in range(N):
        a = rng.integers(0, 4 if n % 3 else 2, int(rng.integers(1, 301))).astype(np.uint8)
        if n % 4 == 0:
            b = rng.integers(0, 4, int(rng.integers(1, 301))).astype(np.uint8)
        else:
            b = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.uint8), _mutate(rng, a, 0.25 if n % 2 else 0.12)])[:300]
        seqs += [a, b]
        gi.append((n // 4) % 2)
    words, offs, lens = hipabi.pack_reads(seqs)
    ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=emul_lib)
    try:
        got = lv.five(lv.run_by_gap(ctx, lv.whole_read_problems(np.arange(0, 2 * N, 2), np.arange(1, 2 * N, 2), lens), gi))
    finally:
        ctx.close()
    ref = np.array([lv.ref_align(seqs[2 * n], seqs[2 * n + 1], 2, -5, lv.GAPS[gi[n]]) for n in range(N)], dtype=np.int64)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, [(int(b), got[b].tolist(), ref[b].tolist()) for b in bad[:8]]
    assert (ref[:, 0] > 50).sum() > N // 3      # the set is not trivially empty of alignments


def test_views_and_limits_on_the_emulated_device(emul_lib):
    """sub-range and reverse-complement views equal the cut / reversed sequence uploaded as a read; a problem beyond the documented limit is
    WTZ_E_ARG and the context goes on working"""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 4, 700).astype(np.uint8)
    b = np.concatenate([rng.integers(0, 4, 50).astype(np.uint8), _mutate(rng, a[100:600], 0.1), rng.integers(0, 4, 80).astype(np.uint8)])
    big = np.zeros(hipabi.LOCAL_MAXLEN + 1, dtype=np.uint8)
    seqs = [a, b, a[100:600].copy(), (3 - a[::-1]).astype(np.uint8), (3 - b[::-1]).astype(np.uint8), big]
    words, offs, lens = hipabi.pack_reads(seqs)
    ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=emul_lib)
    try:
        pr = lv.whole_read_problems([0, 2, 0, 3, 3], [1, 1, 1, 1, 4], lens)
        pr[2]["q_from"], pr[2]["q_len"] = 100, 500                                  # = problem 1
        pr[3]["q_rev"] = 1                                                           # revcomp of the revcomp = problem 0
        pr[4]["q_rev"], pr[4]["t_rev"] = 1, 1                                        # = problem 0
        out = lv.five(ctx.local_batch(pr, *lv.GAPS[0]))
        assert out[0, 0] > 500 and (out[2] == out[1]).all() and (out[3] == out[0]).all() and (out[4] == out[0]).all()
        over = lv.whole_read_problems([5], [1], lens)
        with pytest.raises(RuntimeError, match="error -1"):
            ctx.local_batch(over, *lv.GAPS[0])
        assert (lv.five(ctx.local_batch(pr[:1], *lv.GAPS[0]))[0] == out[0]).all()
        assert lv.pool_info(ctx).main_used == 0
    finally:
        ctx.close()


_BAD_PROBLEMS = [
    ("read id out of range", lambda p, lens: p.__setitem__("q_read", len(lens)), "read id out of range"),
    ("strand 0", lambda p, lens: p.__setitem__("t_strand", 0), r"strand must be \+1 or -1"),
    ("region past the read end walking forwards", lambda p, lens: (p.__setitem__("q_from", 10), p.__setitem__("q_len", int(lens[0]) - 9)), "region outside its read"),
    ("region past the read start walking backwards", lambda p, lens: (p.__setitem__("t_strand", -1), p.__setitem__("t_from", 20), p.__setitem__("t_len", 22)), "region outside its read"),
    ("negative start", lambda p, lens: p.__setitem__("q_from", -1), "region outside its read"),
]


@pytest.mark.parametrize("entry", ["local", "extend"])
@pytest.mark.parametrize("what,spoil,message", _BAD_PROBLEMS, ids=[b[0].replace(" ", "_") for b in _BAD_PROBLEMS])
def test_bad_problems_are_the_same_argument_error_in_both_batch_entries(emul_lib, entry, what, spoil, message):
    """wtz_local_batch and wtz_extend_batch turn a wtz_dp_problem_t into its two views by the same routine: the same bad problem (second of two, so the
    message names problem 1) is WTZ_E_ARG (-1) with the same text from either, and the context goes on working"""
    import ctypes as C
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, 4, 120).astype(np.uint8), rng.integers(0, 4, 90).astype(np.uint8)]
    words, offs, lens = hipabi.pack_reads(seqs)
    ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=emul_lib)

    def run(pr):
        if entry == "local":
            return ctx.local_batch(pr, *lv.GAPS[0])
        pr = np.ascontiguousarray(pr, dtype=hipabi.DP_PROBLEM)
        out = np.zeros(pr.size, dtype=hipabi.DP_RESULT)
        cig = np.zeros(1 << 12, dtype=np.uint32)
        ctx.lib.wtz_extend_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
        ctx._chk(ctx.lib.wtz_extend_batch(ctx.h, pr.ctypes.data, pr.size, out.ctypes.data, cig.ctypes.data, cig.size))
        return out

    try:
        pr = lv.whole_read_problems([0, 0], [1, 1], lens)
        good = run(pr)
        spoil(pr[1], lens)
        with pytest.raises(RuntimeError, match=r"error -1: problem 1: " + message):
            run(pr)
        again = run(lv.whole_read_problems([0, 0], [1, 1], lens))
        assert (again["score"] == good["score"]).all()
    finally:
        ctx.close()
