"""wtz_global_batch and wtz_alignx_batch without a GPU: the body of smartdenovo_amd/csrc/wtz_sw_kglob.h, compiled into the host emulation of the library
(tests/emul: one lane that holds all 64 * C band slots; bands beyond 2 047 slots run the scalar body), is the CPU restatement of the reference's
ksw_global2 (ksw.c:503-586).  It must give the score, the five counts of kswx.h:1468-1477 and the CIGAR word for word
  - for every row of tests/golden/kglob_vectors.npz (tests/golden/make_kglob_vectors.py), and
  - where oracle/_ref/libref_shim.so exists, for 1 000 fresh function-level pairs and 200 fresh chain pairs against the routines called live: mismatches allowed, 0.
The lane-crossing parts of the kernel (the F carry, the E hand-over, the wide trace stores, the cooperative staging) are the identity here: tests/test_gpu_kglob.py."""
import os
import subprocess

import numpy as np
import pytest

import kglobvec as gv
import localvec as lv
from smartdenovo_amd import hipabi

ROOT = lv.ROOT
needs_shim = pytest.mark.skipif(not gv.have_shim(), reason="needs oracle/_ref/libref_shim.so (the reference's ksw.c compiled where its sources are)")


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


@pytest.fixture(scope="module")
def V():
    return gv.load_vectors()


@pytest.fixture(scope="module")
def vctx(emul_lib, V):
    c = lv.make_context(V["words"], V["offs"], V["lens"], int(V["M"]), int(V["X"]), lib_path=emul_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def whole_set(vctx, V):
    return gv.run_by_gap(vctx, gv.problems_of(V), V["f_gap"])


def check_rows(V, out, cigs, idx, emul=True):
    exp = V["f_expect"][idx].astype(np.int64)
    got = gv.six(out)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(str(V["f_names"][idx[b]]), got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    assert (out["cells"] == V["f_cells"][idx]).all()
    assert [int(f) for f in out["form_used"]] == gv.forms_of(V, idx, emul)
    if cigs is not None:
        for k, i in enumerate(idx):
            want = gv.decode_cigar(V["f_cigar"], V["f_cig_off"], int(i))
            assert cigs[k].size == want.size and (cigs[k] == want).all(), str(V["f_names"][i])
            assert int(out["cigar_len"][k]) == want.size


def test_vector_file_holds_the_cases_the_feature_names(V):
    names = [str(x) for x in V["f_names"]]
    assert len(set(names)) == len(names) and os.path.getsize(gv.VECTORS) < 256 * 1024
    assert int(V["M"]) == 2 and int(V["X"]) == -5
    slots = set(int(s) for s in V["f_slots"])
    assert {64 * c + d for c in (1, 2, 4, 8, 16) for d in (-1, 0, 1)} | {2047, 2049, 2400} <= slots
    for var in ("copy", "unrelated", "all_A", "two_letter", "short_q", "short_t"):
        assert sum(1 for n in names if n.startswith("edge_") and n.endswith(var)) >= 18
    i = names.index("rows_20000_w40")
    assert V["f_t_len"][i] >= 20000 and V["f_W"][i] == 40
    i = names.index("rows_6000_slots_2047")
    assert V["f_t_len"][i] >= 6000 and V["f_slots"][i] == 2047
    assert set(int(g) for g in V["f_gap"]) == {0, 1, 2, 3} and (V["f_W"] == 0).sum() >= 8
    d = np.abs(V["f_q_len"].astype(np.int64) - V["f_t_len"])
    assert ((d == V["f_W"]) & (V["f_q_len"] > V["f_t_len"])).sum() >= 6 and ((d == V["f_W"]) & (V["f_q_len"] < V["f_t_len"])).sum() >= 6
    at = set()      # where base 0 of the query view lies in the uploaded words
    for k in (k for k, n in enumerate(names) if n.startswith("view_")):
        r, f = int(V["f_q_read"][k]), int(V["f_q_from"][k])
        at.add((int(V["offs"][r]) + (int(V["lens"][r]) - 1 - f if V["f_q_rev"][k] else f)) & 31)
    assert at == set(range(32))
    i = names.index("view_wtcyc_shape")
    assert V["f_q_read"][i] == V["f_t_read"][i] and V["f_q_rev"][i] == 1 and V["f_t_rev"][i] == 0
    br = V["c_branch"]
    assert all((br == b).sum() >= 1 for b in (gv.B_DIFF, gv.B_W2, gv.B_LIFT, gv.B_EXACT))
    assert (V["c_expect"][:, 0] == 0).sum() >= 1 and (V["c_T"] == 0).sum() >= 1 and (V["c_w"] < 0).sum() >= 2 and V["c_expect"][:, 11].max() > 1023


def test_emulation_equals_the_file_on_every_row(vctx, V, whole_set):
    out, cigs = whole_set
    check_rows(V, out, cigs, np.arange(len(out)))
    assert set(int(f) for f in out["form_used"]) == {1, 2, 4, 8, 16, 32, 255}
    assert lv.pool_info(vctx).main_used == 0
    c = vctx.counters()
    assert c.n_kglob >= len(out) and c.cells_kglob >= int(V["f_cells"].sum())


def test_statistics_only_calls_equal_the_full_calls(vctx, V, whole_set):
    out, _ = gv.run_by_gap(vctx, gv.problems_of(V), V["f_gap"], cigar=False)
    full = whole_set[0].copy()
    full["cigar_len"] = 0
    assert (out == full).all()


def test_chain_equals_the_chain_table(vctx, V):
    pr = gv.chain_problems(V)
    out, cigs = gv.run_chain_by_group(vctx, pr, V["c_w"], V["c_T"])
    got, exp = gv.twelve(out), V["c_expect"].astype(np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(str(V["c_names"][b]), got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    for i in range(len(pr)):
        want = gv.decode_cigar(V["c_cigar"], V["c_cig_off"], i)
        assert cigs[i].size == want.size and (cigs[i] == want).all(), str(V["c_names"][i])
    i = [str(n) for n in V["c_names"]].index("all_A_all_C")
    assert not any(out[i].tolist())      # found = 0: KSWX_NULL
    sel = (V["c_w"] == 50) & (V["c_T"] == -100)
    stat = vctx.alignx_batch(pr[sel], 50, -3, -3, -1, -100, cigar=False)      # statistics only
    assert sel.sum() >= 2 and (gv.twelve(stat) == exp[sel]).all() and (stat["cigar_len"] == 0).all()
    assert lv.pool_info(vctx).main_used == 0


def test_limits_are_argument_errors_and_the_context_survives(vctx, V, whole_set):
    pr = gv.problems_of(V)
    one = pr[:2].copy()
    for field, value in (("q_len", 0), ("t_len", 0), ("q_len", 65536), ("t_len", 65536), ("W", -1)):
        bad = one.copy()
        bad[field][1] = value
        with pytest.raises(RuntimeError, match="error -1"):
            vctx.global_batch(bad, 3, 1, 3, 1)
    k = int(np.nonzero(pr["q_len"] != pr["t_len"])[0][0])
    bad = pr[[0, k]].copy()
    bad["W"][1] = abs(int(bad["q_len"][1]) - int(bad["t_len"][1])) - 1      # the corner outside the band by one
    assert bad["W"][1] >= 0
    with pytest.raises(RuntimeError, match="error -1"):
        vctx.global_batch(bad, 3, 1, 3, 1)
    with pytest.raises(RuntimeError, match="error -1"):
        vctx.global_batch(one, -1, 1, 3, 1)
    for w in (hipabi.KEXT_MAXW + 1, -hipabi.KEXT_MAXW - 1):
        with pytest.raises(RuntimeError, match="error -1"):
            vctx.alignx_batch(gv.chain_problems(V)[:2], w, -3, -3, -1, 0)
    with pytest.raises(RuntimeError, match="error -1"):
        vctx.alignx_batch(gv.chain_problems(V)[:2], -40, -3, -3, -1, -100)
    sel = np.array([0, 1])
    again, cg = gv.run_by_gap(vctx, pr[sel], V["f_gap"][sel])
    check_rows(V, again, cg, sel)
    assert lv.pool_info(vctx).main_used == 0


def test_a_pool_too_small_for_one_problem_is_a_pool_error(emul_lib, V):
    names = [str(x) for x in V["f_names"]]
    i = names.index("rows_6000_slots_2047")      # 6 020 rows x 1 024 bytes of trace: more than half of an 8 MB pool
    small = names.index("w0_64")
    c = lv.make_context(V["words"], V["offs"], V["lens"], int(V["M"]), int(V["X"]), lib_path=emul_lib, pool_bytes=8 << 20)
    try:
        pr = gv.problems_of(V)
        with pytest.raises(RuntimeError, match="error -3"):
            c.global_batch(pr[[small, i]], *gv.GAPS[int(V["f_gap"][i])])
        out, cg = gv.run_by_gap(c, pr[[small]], V["f_gap"][[small]])      # the context stays usable
        check_rows(V, out, cg, np.array([small]))
    finally:
        c.close()


def test_a_small_pool_splits_the_call_into_launch_groups(emul_lib, V):
    names = [str(x) for x in V["f_names"]]
    idx = np.array([k for k, n in enumerate(names) if n.startswith(("edge_1025", "edge_2047", "tb_")) and V["f_gap"][k] == 0])
    c = lv.make_context(V["words"], V["offs"], V["lens"], int(V["M"]), int(V["X"]), lib_path=emul_lib, pool_bytes=6 << 20)
    try:
        need = sum(int(V["f_t_len"][k]) * 1024 for k in idx)
        assert need > (3 << 20)      # the traces do not fit the 3 MB main pool together
        out, cg = gv.run_by_gap(c, gv.problems_of(V)[idx], V["f_gap"][idx])
        check_rows(V, out, cg, idx)
    finally:
        c.close()


def _fresh_pair(rng, k):
    n = int(rng.integers(1, 400))
    q = rng.integers(0, 2 if k % 5 == 0 else 4, n).astype(np.uint8)
    if k % 4 == 0:
        t = rng.integers(0, 4, max(1, n + int(rng.integers(-20, 21)))).astype(np.uint8)
    else:
        keep = rng.random(n) > 0.08
        t = q[keep].copy()
        flip = rng.random(t.size) < 0.1
        t[flip] = (t[flip] + 1) % 4
        ins = int(rng.integers(0, 12))
        at = int(rng.integers(0, t.size + 1))
        t = np.concatenate([t[:at], rng.integers(0, 4, ins).astype(np.uint8), t[at:]])
        if t.size == 0:
            t = np.zeros(1, dtype=np.uint8)
    return q, t


@needs_shim
def test_emulation_equals_live_ksw_global2_on_fresh_pairs(emul_lib):
    rng = np.random.default_rng(77)
    pairs = [_fresh_pair(rng, k) for k in range(1000)]
    reads = [s for p in pairs for s in p]
    words, offs, lens = hipabi.pack_reads(reads)
    c = lv.make_context(words, offs, lens, 2, -5, lib_path=emul_lib)
    try:
        pr = lv.whole_read_problems(np.arange(0, 2000, 2), np.arange(1, 2000, 2), lens)
        pr["W"] = [abs(len(q) - len(t)) + int(rng.integers(0, 3)) * int(rng.integers(0, 60)) for q, t in pairs]
        gap = np.arange(1000) % 4
        out, cigs = gv.run_by_gap(c, pr, gap)
        bad = 0
        for k, (q, t) in enumerate(pairs):
            sc, cg = gv.ref_global(q, t, 2, -5, gv.GAPS[gap[k]], int(pr["W"][k]))
            ok = tuple(gv.six(out[k:k + 1])[0]) == (sc,) + gv.fold(q, t, cg) and cigs[k].size == cg.size and (cigs[k] == cg).all()
            bad += not ok
        assert bad == 0
    finally:
        c.close()


@needs_shim
def test_chain_equals_the_live_restatement_on_fresh_pairs(emul_lib):
    rng = np.random.default_rng(78)
    pairs = []
    for k in range(200):
        n = int(rng.integers(60, 500))
        q = rng.integers(0, 4, n).astype(np.uint8)
        keep = rng.random(n) > (0.02, 0.1)[k & 1]
        t = q[keep].copy()
        flip = rng.random(t.size) < (0.03, 0.15)[(k >> 1) & 1]
        t[flip] = (t[flip] + 1) % 4
        t = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 50))).astype(np.uint8), t, rng.integers(0, 4, int(rng.integers(0, 50))).astype(np.uint8)])
        pairs.append((q, t))
    words, offs, lens = hipabi.pack_reads([s for p in pairs for s in p])
    c = lv.make_context(words, offs, lens, 2, -5, lib_path=emul_lib)
    try:
        pr = lv.whole_read_problems(np.arange(0, 400, 2), np.arange(1, 400, 2), lens)
        w = np.array([(50, 200, 30, -60)[k % 4] for k in range(200)])
        T = np.array([0 if w[k] < 0 else (-100, -30, 0)[k % 3] for k in range(200)])
        out, cigs = gv.run_chain_by_group(c, pr, w, T)
        bad = 0
        for k, (q, t) in enumerate(pairs):
            exp, cg, _ = gv.ref_chainx(q, t, 2, -5, int(w[k]), -3, -3, -1, int(T[k]))
            ok = tuple(gv.twelve(out[k:k + 1])[0]) == tuple(exp) and cigs[k].size == cg.size and (cigs[k] == cg).all()
            bad += not ok
        assert bad == 0
    finally:
        c.close()


def test_kglob_problem_stand_alone(tmp_path):
    """tests/emul/check_kglob.cpp: wtz_kglob_problem<C> of all six C, each problem in the form the host picks and every wider one, against a scalar restatement
    of ksw_global2 written in that file, trace and run buffers of exactly the planned size"""
    exe = os.path.join(str(tmp_path), "check_kglob")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DWTZ_EMUL", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "smartdenovo_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "emul", "check_kglob.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 bad" in r.stdout, r.stdout + r.stderr
