"""wtz_kext_batch and wtz_align_batch without a GPU: the DP body of smartdenovo_amd/csrc/wtz_sw_kext.h, compiled into the host emulation of the library
(tests/emul: one lane that holds all 64 * C band slots), is the CPU restatement of the reference's ksw_extend2 (ksw.c:381-478).  It must give the six ints
of the reference
  - for every problem of tests/golden/kext_vectors.npz (dumped from the reference routine by tests/golden/make_kext_vectors.py), and
  - for every problem of tests/golden/kext_wide_vectors.npz (the wide forms, the slot counts at the form edges, views, long problems), and
  - where oracle/_ref/libref_shim.so exists, for 2 000 + 200 fresh seeded pairs against the routine called live: mismatches allowed, 0.
The chain wtz_align_batch (kswx_align_no_stat, kswx.h:1504-1511) is compared with the chain table of the same file and, where the shim exists, with
kextvec.ref_chain run live on 300 fresh pairs (see tests/kextvec.py for what that restatement pins and what the reference's compiled code pins)."""
import os
import subprocess

import numpy as np
import pytest

import kextvec as kv
import localvec as lv
from smartdenovo_amd import hipabi

ROOT = lv.ROOT
needs_shim = pytest.mark.skipif(not kv.have_shim(), reason="needs oracle/_ref/libref_shim.so (the reference's ksw.c compiled where its sources are)")


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


@pytest.fixture(scope="module")
def V():
    return kv.load_vectors()


@pytest.fixture(scope="module")
def vctx(emul_lib, V):
    c = lv.make_context(V["words"], V["offs"], V["lens"], int(V["M"]), int(V["X"]), lib_path=emul_lib)
    yield c
    c.close()


def test_vector_file_holds_the_cases_and_branches_the_feature_names(V):
    names = [str(x) for x in V["f_names"]]
    e = V["f_expect"].astype(np.int64)
    assert 200 <= len(names) <= 600 and len(set(names)) == len(names)
    assert os.path.getsize(kv.VECTORS) < (1 << 19)
    assert int(V["M"]) == 2 and int(V["X"]) == -5
    assert set(kv.QLENS) <= set(int(x) for x in V["f_q_len"])
    assert set(kv.WS) <= set(int(x) for x in V["f_W"])
    for ql in kv.QLENS:
        assert any(n.startswith("qlen_%d_" % ql) for n in names), ql
    for w in kv.WS:
        for kind, above in (("short", False), ("long", True)):
            i = names.index("w_%d_%s" % (w, kind))
            assert (int(V["f_q_len"][i]) > 2 * w + 1) == above, (w, kind)
    assert set(kv.H0S) <= set(int(x) for x in V["f_init_score"])
    assert set(int(x) for x in V["f_zdrop"]) == set(kv.ZDROPS) and set(int(x) for x in V["f_end_bonus"]) == set(kv.END_BONUS)
    assert set(int(x) for x in V["f_gap"]) == {0, 1, 2, 3}
    runoff = [i for i, n in enumerate(names) if n.startswith("runoff_")]
    assert runoff and all(V["f_t_len"][i] > V["f_q_len"][i] + V["f_W"][i] + 50 for i in runoff)
    assert all(V["f_stop"][i] == kv.STOP_M0 for i in runoff)      # they end at the empty band, not at the last row
    rev = [i for i, n in enumerate(names) if n.startswith("rev_")]
    assert rev and all(V["f_q_strand"][i] == -1 and V["f_t_strand"][i] == -1 and V["f_q_from"][i] == V["f_q_len"][i] - 1 for i in rev)
    for prefix in ("copy_", "unrelated_", "two_letter_", "all_A_", "h0_", "clamp_qlen1_"):
        assert any(n.startswith(prefix) for n in names), prefix
    # the branches, recomputed from what the file records
    assert (V["f_stop"] == kv.STOP_M0).sum() > 0 and (V["f_stop"] == kv.STOP_ZDROP).sum() > 0 and (V["f_stop"] == kv.STOP_END).sum() > 0
    assert (e[:, 4] >= 0).sum() > 0 and (e[:, 4] < 0).sum() > 0                     # a row with end == qlen was seen / never seen
    assert (e[:, 4] > e[:, 0] - 100).sum() > 0
    cf, ce = V["c_flags"].astype(np.int64), V["c_expect"].astype(np.int64)
    ran_l, ran_r = (cf & kv.F_LEFT_RAN) != 0, (cf & kv.F_RIGHT_RAN) != 0
    for what, cnt in (("left skipped", (cf & kv.F_LEFT_SKIP) != 0), ("right skipped", (cf & kv.F_RIGHT_SKIP) != 0),
                      ("left role 0", ran_l & ((cf & kv.F_LEFT_ROLE1) == 0)), ("left role 1", (cf & kv.F_LEFT_ROLE1) != 0),
                      ("right role 0", ran_r & ((cf & kv.F_RIGHT_ROLE1) == 0)), ("right role 1", (cf & kv.F_RIGHT_ROLE1) != 0),
                      ("left gscore commit", (cf & kv.F_LEFT_GSCORE) != 0), ("left score commit", ran_l & ((cf & kv.F_LEFT_GSCORE) == 0)),
                      ("right gscore commit", (cf & kv.F_RIGHT_GSCORE) != 0), ("right score commit", ran_r & ((cf & kv.F_RIGHT_GSCORE) == 0)),
                      ("found = 0", ce[:, 0] == 0), ("both ends skipped", ((cf & kv.F_LEFT_SKIP) != 0) & ((cf & kv.F_RIGHT_SKIP) != 0))):
        assert cnt.sum() > 0, what
    # a gscore commit reaches the end of a side, T = 0 never extends
    lens = V["lens"].astype(np.int64)
    ql, tl = lens[V["c_q_read"]], lens[V["c_t_read"]]
    g = (cf & kv.F_RIGHT_GSCORE) != 0
    assert ((ce[g, 5] == ql[g]) | (ce[g, 3] == tl[g])).all()
    t0 = V["c_T"] == 0
    assert t0.sum() > 0 and (cf[t0] == 0).all()
    assert set(int(x) for x in V["c_w"]) == {20, 800} and set(int(x) for x in V["c_T"]) == {-100, -30, 0}
    cn = [str(x) for x in V["c_names"]]
    assert sum(n.startswith("cyc_palindrome_") for n in cn) == 20 and sum(n.startswith("shared_") for n in cn) == 240


def test_restatement_equals_reference_vectors(vctx, V):
    pr = kv.problems_of(V)
    out = kv.run_by_group(vctx, pr, V["f_gap"], V["f_end_bonus"], V["f_zdrop"])
    got, exp = kv.six(out), V["f_expect"].astype(np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(str(V["f_names"][b]), got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    assert (out["rows"] == V["f_rows"]).all() and (out["cells"] == V["f_cells"].astype(np.uint64)).all()
    assert set(int(f) for f in out["form_used"]) == {1, 2, 4, 8, 16, 32}
    assert lv.pool_info(vctx).main_used == 0


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


def _fresh_pairs_narrow(rng, N):
    """lengths 1-300, w in {3, 10, 40, 800}"""
    seqs, par = [], []
    for n in range(N):
        a = rng.integers(0, 4 if n % 3 else 2, int(rng.integers(1, 301))).astype(np.uint8)
        if n % 4 == 0:
            b = rng.integers(0, 4, int(rng.integers(1, 301))).astype(np.uint8)
        else:
            b = _mutate(rng, a, (0.12, 0.25, 0.35)[n % 3])
            if n & 1:
                b = np.concatenate([b, rng.integers(0, 4, int(rng.integers(1, 80))).astype(np.uint8)])
            b = b[:300]
        seqs += [a, b]
        par.append((int(rng.integers(4)), int(rng.choice(kv.END_BONUS)), int(rng.choice(kv.ZDROPS)), int(rng.choice((3, 10, 40, 800))), int(rng.choice(kv.H0S))))
    return seqs, np.array(par)


def _fresh_pairs_wide(rng, N):
    """sides of 300-2 200, w in {300, 512, 800, 1023}, h0 in {0, 1, 30, 400, 5000}; the mutated copies that are cut off go on with unrelated sequence"""
    seqs, par = [], []
    for n in range(N):
        k = 4 if n % 3 else 2
        a = rng.integers(0, k, int(rng.integers(300, 2201))).astype(np.uint8)
        if n % 4 == 0:
            b = rng.integers(0, k, int(rng.integers(300, 2201))).astype(np.uint8)
        else:
            b = _mutate(rng, a, (0.12, 0.25, 0.35)[n % 3]) % k
            if n & 1:
                b = np.concatenate([b[:int(rng.integers(75, b.size + 1))], rng.integers(0, k, int(rng.integers(150, 1100))).astype(np.uint8)])
            b = np.concatenate([b, rng.integers(0, k, max(0, 300 - b.size)).astype(np.uint8)])[:2200]
        seqs += [a, b.astype(np.uint8)]
        par.append((int(rng.integers(4)), int(rng.choice(kv.END_BONUS)), int(rng.choice(kv.ZDROPS)), int(rng.choice((300, 512, 800, 1023))), int(rng.choice((0, 1, 30, 400, 5000)))))
    return seqs, np.array(par)


@needs_shim
def test_restatement_equals_live_ksw_extend2_on_fresh_pairs(emul_lib):
    """narrow: 2 000 pairs, lengths 1-300 (a quarter unrelated, the rest mutated at 12 / 25 / 35 % with deletion runs, half of those followed by unrelated
    sequence, a third over a two-letter alphabet), w, h0, zdrop, end_bonus and the gap costs drawn from the lists of kextvec.
    wide: 200 pairs drawn the same way with sides of 300-2 200 and w up to 1 023; sixteen and thirty-two slots per lane occur at least 40 times each.
    Mismatches allowed: 0."""
    for which in ("narrow", "wide"):
        if which == "narrow":
            N = 2000
            seqs, par = _fresh_pairs_narrow(np.random.default_rng(19), N)
        else:
            N = 200
            seqs, par = _fresh_pairs_wide(np.random.default_rng(29), N)
        words, offs, lens = hipabi.pack_reads(seqs)
        ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=emul_lib)
        try:
            pr = lv.whole_read_problems(np.arange(0, 2 * N, 2), np.arange(1, 2 * N, 2), lens)
            pr["W"], pr["init_score"] = par[:, 3], par[:, 4]
            out = kv.run_by_group(ctx, pr, par[:, 0], par[:, 1], par[:, 2])
            got = kv.six(out)
        finally:
            ctx.close()
        ref = np.array([kv.ref_extend(seqs[2 * n], seqs[2 * n + 1], 2, -5, kv.GAPS[par[n, 0]], int(par[n, 3]), int(par[n, 1]), int(par[n, 2]), int(par[n, 4])) for n in range(N)], dtype=np.int64)
        bad = np.nonzero((got != ref).any(axis=1))[0]
        assert bad.size == 0, [(which, int(b), par[b].tolist(), got[b].tolist(), ref[b].tolist()) for b in bad[:8]]
        if which == "narrow":
            assert (ref[:, 4] > ref[:, 0] - 100).sum() > N // 10 and (ref[:, 2] > 20).sum() > N // 3      # the set is not trivially empty of extensions
        else:
            form = [kv.form_of(kv.slots_of(seqs[2 * n].size, seqs[2 * n + 1].size, 2, -5, kv.GAPS[par[n, 0]], int(par[n, 3]), int(par[n, 1]))) for n in range(N)]
            assert (out["form_used"] == form).all()
            assert form.count(16) >= 40 and form.count(32) >= 40, (form.count(16), form.count(32))
            assert (ref[:, 2] > 200).sum() > N // 3


def test_chain_equals_the_chain_table(vctx, V):
    pr = kv.chain_problems(V["c_q_read"], V["c_t_read"], V["c_t_rev"], V["lens"])
    out = kv.run_chain_by_group(vctx, pr, V["c_w"], V["c_T"])
    got, exp = kv.chain_six(out), V["c_expect"].astype(np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(str(V["c_names"][b]), got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    loc = np.stack([out[f] for f in ("local_score", "local_tb", "local_te", "local_qb", "local_qe")], axis=1).astype(np.int64)
    assert (loc == V["c_local"]).all()
    nf = np.nonzero(exp[:, 0] == 0)[0]
    assert nf.size > 0 and all(not any(out[int(i)].tolist()) for i in nf)      # KSWR_NULL: found = 0 and every other field 0
    assert lv.pool_info(vctx).main_used == 0


def _fresh_chain_pairs(rng, N):
    seqs, trev = [], []
    for n in range(N):
        seg = rng.integers(0, 4, int(rng.integers(30, 200))).astype(np.uint8)
        fl, fr = rng.integers(0, 4, int(rng.integers(0, 120))).astype(np.uint8), rng.integers(0, 4, int(rng.integers(0, 120))).astype(np.uint8)
        a = np.concatenate([fl, seg, fr])
        if n % 4 == 3:
            b = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 120))).astype(np.uint8), _mutate(rng, seg, 0.12), rng.integers(0, 4, int(rng.integers(0, 120))).astype(np.uint8)])
        else:
            b = np.concatenate([_mutate(rng, fl, 0.3), _mutate(rng, seg, 0.12), _mutate(rng, fr, 0.3)])
        seqs += [a, b]
        trev.append(n & 1)
    return seqs, np.array(trev)


@needs_shim
def test_chain_equals_the_restatement_run_live_on_fresh_pairs(emul_lib):
    rng = np.random.default_rng(23)
    N = 300
    seqs, trev = _fresh_chain_pairs(rng, N)
    w = np.array([(20, 800, 5)[n % 3] for n in range(N)])
    T = np.array([(-100, -30, -10, 0)[(n // 3) % 4] for n in range(N)])
    words, offs, lens = hipabi.pack_reads(seqs)
    ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=emul_lib)
    try:
        pr = kv.chain_problems(np.arange(0, 2 * N, 2), np.arange(1, 2 * N, 2), trev, lens)
        got = kv.chain_six(kv.run_chain_by_group(ctx, pr, w, T))
    finally:
        ctx.close()
    ref, flags = [], 0
    for n in range(N):
        t = seqs[2 * n + 1]
        e, fl, _ = kv.ref_chain(seqs[2 * n], (3 - t[::-1]).astype(np.uint8) if trev[n] else t, 2, -5, int(w[n]), -3, -3, -1, int(T[n]))
        ref.append(e)
        flags |= fl
    ref = np.array(ref, dtype=np.int64)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, [(int(b), int(w[b]), int(T[b]), got[b].tolist(), ref[b].tolist()) for b in bad[:8]]
    assert flags & kv.F_LEFT_RAN and flags & kv.F_RIGHT_RAN and flags & (kv.F_LEFT_GSCORE | kv.F_RIGHT_GSCORE)


def test_chain_with_T_0_is_the_local_hit_shifted(vctx, V):
    """no extension without a clip penalty (kswx.h:1388): the rectangle is ksw_align2's with qe and te made exclusive (kswx.h:1508)"""
    sel = np.nonzero(V["c_w"] == 20)[0]
    pr = kv.chain_problems(V["c_q_read"], V["c_t_read"], V["c_t_rev"], V["lens"])[sel]
    a = vctx.align_batch(pr, 20, -3, -3, -1, 0)
    l = vctx.local_batch(pr, 3, 1, 3, 1)
    assert sel.size > 50
    for i in range(sel.size):
        if l["score"][i] <= 0 or min(l["tb"][i], l["qb"][i], l["te"][i], l["qe"][i]) <= -1:
            assert l["te"][i] == -1 and not any(a[i].tolist())
        else:
            assert [a[f][i] for f in kv.CHAIN_FIELDS] == [1, l["score"][i], l["tb"][i], l["te"][i] + 1, l["qb"][i], l["qe"][i] + 1]


def test_limits_and_bad_arguments_are_argument_errors_and_the_context_survives(emul_lib):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, 120).astype(np.uint8)
    b = np.concatenate([a[:80], rng.integers(0, 4, 30).astype(np.uint8)])
    words, offs, lens = hipabi.pack_reads([a, b])
    ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=emul_lib)
    try:
        pr = lv.whole_read_problems([0, 0], [1, 1], lens)
        pr["W"], pr["init_score"] = 40, 30
        good = ctx.kext_batch(pr, 3, 1, 3, 1, 100, -1)
        assert good["score"][0] >= 30 + 2 * 80 and good["qle"][0] >= 80 and good["tle"][0] >= 80
        calls = []
        calls.append(lambda: ctx.kext_batch(pr, 3, 0, 3, 1, 100, -1))                  # e_del = 0: the reference divides by it
        calls.append(lambda: ctx.kext_batch(pr, 3, 1, 3, 0, 100, -1))
        calls.append(lambda: ctx.kext_batch(pr, -1, 1, 3, 1, 100, -1))
        for field, value in (("W", hipabi.KEXT_MAXW + 1), ("W", -1), ("q_len", 0), ("t_len", 0), ("q_len", 121), ("t_strand", 0), ("q_read", 2)):
            bad = pr.copy()
            bad[field][1] = value
            calls.append(lambda bad=bad: ctx.kext_batch(bad, 3, 1, 3, 1, 100, -1))
            if field != "W":
                calls.append(lambda bad=bad: ctx.align_batch(bad, 20, -3, -3, -1, -100))
        calls.append(lambda: ctx.align_batch(pr, hipabi.KEXT_MAXW + 1, -3, -3, -1, -100))
        calls.append(lambda: ctx.align_batch(pr, 20, -3, -3, 0, -100))
        calls.append(lambda: ctx.align_batch(pr, 20, 3, -3, -1, -100))
        for k, call in enumerate(calls):
            with pytest.raises(RuntimeError, match="error -1"):
                call()
            again = ctx.kext_batch(pr, 3, 1, 3, 1, 100, -1)
            assert (again == good).all(), k
            assert lv.pool_info(ctx).main_used == 0
        at = pr.copy()
        at["W"] = hipabi.KEXT_MAXW                                                     # exactly at the limit the call is accepted
        assert (ctx.kext_batch(at, 3, 1, 3, 1, 100, -1)["score"] >= 30 + 2 * 80).all()
        c0 = ctx.counters()
        ctx.align_batch(pr, 20, -3, -3, -1, -100)
        c1 = ctx.counters()
        assert c1.n_kext > c0.n_kext and c1.cells_kext > c0.cells_kext and c1.n_local == c0.n_local + 2
        assert lv.pool_info(ctx).main_used == 0
    finally:
        ctx.close()


# ---- tests/golden/kext_wide_vectors.npz: the wide forms with every exit, the slot counts at the form edges, views, long problems (make_kext_wide_vectors.py) ----
EDGE_S = tuple(64 * c + d for c in (1, 2, 4, 8, 16) for d in (-1, 0, 1)) + (2047,)


@pytest.fixture(scope="module")
def W():
    return kv.load_vectors(kv.WIDE_VECTORS)


@pytest.fixture(scope="module")
def wctx(emul_lib, W):
    c = lv.make_context(W["words"], W["offs"], W["lens"], int(W["M"]), int(W["X"]), lib_path=emul_lib)
    yield c
    c.close()


def test_wide_vector_file_meets_the_conditions_it_was_made_for(W):
    """recomputed from the file: per kernel form at least 3 problems of every exit and branch, at least 4 per slot count at a form edge, the views"""
    names = [str(x) for x in W["f_names"]]
    n = len(names)
    e = W["f_expect"].astype(np.int64)
    assert len(set(names)) == n and os.path.getsize(kv.WIDE_VECTORS) < (1 << 19)
    assert int(W["M"]) == 2 and int(W["X"]) == -5
    assert set(int(x) for x in W["f_init_score"]) <= set(kv.H0S) and set(int(x) for x in W["f_zdrop"]) == set(kv.ZDROPS)
    assert set(int(x) for x in W["f_end_bonus"]) == set(kv.END_BONUS) and set(int(x) for x in W["f_gap"]) == {0, 1, 2, 3}
    slots = np.array([kv.slots_of(int(W["f_q_len"][i]), int(W["f_t_len"][i]), 2, -5, kv.GAPS[W["f_gap"][i]], int(W["f_W"][i]), int(W["f_end_bonus"][i])) for i in range(n)])
    form = np.array([kv.form_of(int(s)) for s in slots])
    assert (slots == W["f_slots"]).all() and (form == W["f_form"]).all()
    stop = W["f_stop"]
    for c in kv.FORMS:
        f = form == c
        for what, sel in (("last row", stop == kv.STOP_END), ("m == 0", stop == kv.STOP_M0), ("z-drop", stop == kv.STOP_ZDROP), ("trim matters", W["f_trim"] != 0),
                          ("gscore == -1", e[:, 4] == -1), ("gscore > score - 100", e[:, 4] > e[:, 0] - 100)):
            assert (f & sel).sum() >= 3, (c, what)
    for S in EDGE_S:
        i = [k for k in range(n) if slots[k] == S]
        assert len(i) >= 4, S
        kinds = set(names[k].split("_", 2)[2] for k in i if names[k].startswith("edge_S%d_" % S))
        assert kinds == {"copy", "unrelated", "prefix", "all_A", "copy_short_t", "copy_short_q"}, S
        w = [kv.clamped_w(int(W["f_q_len"][k]), 2, -5, kv.GAPS[W["f_gap"][k]], int(W["f_W"][k]), int(W["f_end_bonus"][k])) for k in i]
        if S != 2047:      # 2 * 1023 + 1: no side can be shorter than the widest band
            assert any(W["f_t_len"][k] - 1 < ww for k, ww in zip(i, w)) and any(W["f_q_len"][k] - 1 < ww for k, ww in zip(i, w)), S
        else:
            assert any(W["f_t_len"][k] - 1 == ww for k, ww in zip(i, w)) and any(W["f_q_len"][k] - 1 == ww for k, ww in zip(i, w))
    view = np.array([k for k in range(n) if names[k].startswith("view_")])
    assert set(int(x) % 32 for x in W["f_q_from"][view]) == set(range(32)) and set(int(x) % 32 for x in W["f_t_from"][view]) == set(range(32))
    wide_kinds = set((int(W["f_q_strand"][k]), int(W["f_t_strand"][k]), int(W["f_q_rev"][k]), int(W["f_t_rev"][k])) for k in view if form[k] >= 8)
    assert len(wide_kinds) == 16                  # the four strand combinations x (no rev, q_rev, t_rev, both), each in a form with C >= 8
    lens, nreads = W["lens"].astype(np.int64), len(W["lens"])

    def span(k, side):      # first and last base of the view in the read as it was uploaded
        a = int(W["f_%s_from" % side][k])
        b = a + int(W["f_%s_strand" % side][k]) * (int(W["f_%s_len" % side][k]) - 1)
        if W["f_%s_rev" % side][k]:
            a, b = lens[W["f_%s_read" % side][k]] - 1 - a, lens[W["f_%s_read" % side][k]] - 1 - b
        return min(a, b), max(a, b)
    first = [k for k in view if W["f_q_read"][k] == 0 and span(k, "q")[0] == 0]
    last = [k for k in view if W["f_t_read"][k] == nreads - 1 and span(k, "t")[1] == lens[-1] - 1]
    assert set(int(W["f_q_strand"][k]) for k in first) == {1, -1}
    assert set((int(W["f_t_strand"][k]), int(W["f_t_rev"][k])) for k in last) == {(1, 0), (-1, 0), (1, 1)}
    i = names.index("rows_20000_w40")
    assert W["f_rows"][i] == 20000 and stop[i] == kv.STOP_END and W["f_W"][i] == 40
    i = names.index("rows_6000_w1023")
    assert W["f_rows"][i] > 5000 and form[i] == 32
    # the chain rows: both roles on both sides in both wide forms, at least twice
    cf, cs = W["c_flags"].astype(np.int64), W["c_slots"]
    assert 30 <= len(cf) <= 60 and set(int(x) for x in W["c_w"]) == {800, 1023} and set(int(x) for x in W["c_T"]) == {-100, -30}
    assert abs(int(W["c_t_rev"].sum()) * 2 - len(cf)) <= 2
    for side, (ran, role1) in enumerate(((kv.F_LEFT_RAN, kv.F_LEFT_ROLE1), (kv.F_RIGHT_RAN, kv.F_RIGHT_ROLE1))):
        assert (((cf & ran) != 0) == (cs[:, side] > 0)).all()
        for role in (0, 1):
            for c in (16, 32):
                cnt = sum(1 for k in range(len(cf)) if cf[k] & ran and bool(cf[k] & role1) == bool(role) and kv.form_of(int(cs[k, side])) == c)
                assert cnt >= 2, (side, role, c)


def test_restatement_equals_wide_reference_vectors(wctx, W):
    pr = kv.problems_of(W)
    out = kv.run_by_group(wctx, pr, W["f_gap"], W["f_end_bonus"], W["f_zdrop"])
    got, exp = kv.six(out), W["f_expect"].astype(np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(str(W["f_names"][b]), got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    assert (out["rows"] == W["f_rows"]).all() and (out["cells"] == W["f_cells"].astype(np.uint64)).all()
    assert (out["form_used"] == W["f_form"]).all()
    assert lv.pool_info(wctx).main_used == 0


def test_chain_equals_the_wide_chain_table(wctx, W):
    pr = kv.chain_problems(W["c_q_read"], W["c_t_read"], W["c_t_rev"], W["lens"])
    c0 = wctx.counters()
    out = kv.run_chain_by_group(wctx, pr, W["c_w"], W["c_T"])
    got, exp = kv.chain_six(out), W["c_expect"].astype(np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(str(W["c_names"][b]), got[b].tolist(), exp[b].tolist()) for b in bad[:8]]
    loc = np.stack([out[f] for f in ("local_score", "local_tb", "local_te", "local_qb", "local_qe")], axis=1).astype(np.int64)
    assert (loc == W["c_local"]).all()
    assert wctx.counters().n_kext - c0.n_kext == (W["c_slots"] > 0).sum()
    assert lv.pool_info(wctx).main_used == 0


def test_kext_problem_stand_alone(tmp_path):
    """tests/emul/check_kext.cpp: wtz_kext_problem<C> of all six C against a scalar restatement of ksw_extend2 written in that file, on views at both ends of
    an array allocated to the word"""
    exe = os.path.join(str(tmp_path), "check_kext")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DWTZ_EMUL", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "smartdenovo_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "emul", "check_kext.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 bad" in r.stdout, r.stdout + r.stderr
