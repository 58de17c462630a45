#!/usr/bin/env python3
"""Generator of tests/golden/kext_wide_vectors.npz, the second vector file of ksw_extend2 (ksw.c:381-478) and kswx_align_no_stat (kswx.h:1504-1511):
what tests/golden/kext_vectors.npz leaves thin.  Same layout and field names (tests/kextvec.py reads both), plus f_q_rev / f_t_rev, the planned
slot count and kernel form of every problem (f_slots, f_form), whether a fixed band gives other ints (f_trim) and, per chain row and side, the slot
count of the extension stage that ran (c_slots).  Data only: sequences as 2-bit words, arguments, names and recorded ints.  M = 2, X = -5.

  form edges   S = 64 C - 1, 64 C, 64 C + 1 live diagonals for C = 1 ... 16 and S = 2 047 (the most C = 32 holds): at 64 C the last register of lane 63
               is live.  Six problems per S: a mutated copy, an unrelated pair, a shared prefix followed by unrelated sequence, an all-A pair, and a
               copy each with a short target (dlo = t_len - 1 < w) and a short query (q_len - 1 < w).  S = 2 047 = 2 * 1 023 + 1 leaves no room for a
               short side below the widest band: its two "short" problems have t_len - 1 = w and q_len - 1 = w exactly.
  wide / mid   every form with every exit: pairs drawn by draw_pair() (a quarter unrelated, the rest mutated at 12 / 25 / 35 %, half of those cut off
               and followed by unrelated sequence, a third over a two-letter alphabet), h0 in {0, 1, 30, 400, 5000}; for C = 16 and 32 sides of
               300-2 200 and w in {300, 512, 800, 1023}, for the narrower forms sides and bands scaled down to the form.
  views        both sides inside longer reads: every residue of q_from and t_from mod 32, the four strand combinations, q_rev / t_rev / both, and
               views on the first base of the first read and the last base of the last read.
  rows         20 000 x 20 000 at w = 40 and 6 000 x 6 000 at w = 1 023.
  chain        rows of kswx_align_no_stat whose extension stages run in the wide forms.

    python tests/golden/make_kext_wide_vectors.py          (needs oracle/_ref, i.e. a machine that has the reference's sources; a few minutes)

Every expected value is what the reference's own ksw_extend2 returned through oracle/_ref/libref_shim.so; kextvec.py_extend is checked against it on
every problem and gives the stop reason, rows and cells.  The counts the set is meant to reach are asserted and printed before the file is written."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kextvec as kv  # noqa: E402
from smartdenovo_amd import hipabi  # noqa: E402

M, X = 2, -5
MIN_PER_BRANCH, MIN_PER_S = 3, 4
FLANK_RATE = 0.5      # of the chain rows' flanks: at 30 % the local hit of ksw_align2 runs through them and leaves the extension stages a few dozen bases
EDGE_S = tuple(64 * c + d for c in (1, 2, 4, 8, 16) for d in (-1, 0, 1)) + (2047,)
rng = np.random.default_rng(20261020)


def rnd(n, k=4):
    return rng.integers(0, k, int(n)).astype(np.uint8)


def revcomp(s):
    return (3 - s[::-1]).astype(np.uint8)


def pick(xs):
    return xs[int(rng.integers(len(xs)))]


def mutate(s, rate, k=4):
    """substitutions 20 %, insertions 40 %, deletions 40 % of the events; a fifth of the deletions and insertions are runs of 2-8"""
    out = []
    i = 0
    while i < len(s):
        r = rng.random()
        if r < rate * 0.4:
            out.extend(rnd(1 + (rng.integers(1, 8) if rng.random() < 0.2 else 0), k))
        elif r < rate * 0.8:
            i += 1 + (int(rng.integers(1, 8)) if rng.random() < 0.2 else 0)
            continue
        elif r < rate:
            out.append((int(s[i]) + 1 + int(rng.integers(k - 1))) % k)
            i += 1
            continue
        out.append(int(s[i]))
        i += 1
    return np.array(out if out else [0], dtype=np.uint8)


def fit(s, n, k=4):
    """exactly n bases: cut, or continued with unrelated sequence"""
    return s[:n].copy() if s.size >= n else np.concatenate([s, rnd(n - s.size, k)])


reads = []
F = {k: [] for k in ("names", "q_read", "t_read", "q_rev", "t_rev", "q_from", "t_from", "q_strand", "t_strand", "q_len", "t_len", "init_score", "W", "gap", "end_bonus",
                     "zdrop", "seqs")}


def store(d, strand, rev, left, right):
    """a read that holds the bases d, `left` unrelated bases in front of them and `right` behind them in the order the read is addressed, such that the view
    (from, strand, rev) of it walks d: returns (read, from)"""
    logical = np.concatenate([rnd(left), d if strand > 0 else d[::-1], rnd(right)])
    frm = left if strand > 0 else left + d.size - 1
    return (revcomp(logical) if rev else logical), frm


def add_views(name, q, t, w, h0, qv, tv, gap=None, end_bonus=None, zdrop=None):
    """qv / tv: (read index, from, strand, rev) of views that walk q / t"""
    for side, (r, frm, strand, rev), d in (("q", qv, q), ("t", tv, t)):
        F[side + "_read"].append(r)
        F[side + "_from"].append(frm)
        F[side + "_strand"].append(strand)
        F[side + "_rev"].append(rev)
        F[side + "_len"].append(d.size)
        logical = revcomp(reads[r]) if rev else reads[r]
        assert (logical[frm + strand * np.arange(d.size)] == d).all(), name
    F["names"].append(name)
    F["init_score"].append(h0)
    F["W"].append(w)
    F["gap"].append(int(rng.integers(4)) if gap is None else gap)
    F["end_bonus"].append(pick(kv.END_BONUS) if end_bonus is None else end_bonus)
    F["zdrop"].append(pick(kv.ZDROPS) if zdrop is None else zdrop)
    F["seqs"].append((q, t))


def add(name, q, t, w, h0, **kw):
    """two whole reads walked from their first base"""
    q, t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
    reads.append(q)
    reads.append(t)
    add_views(name, q, t, w, h0, (len(reads) - 2, 0, 1, 0), (len(reads) - 1, 0, 1, 0), **kw)


def slots_of_last():
    return kv.slots_of(F["q_len"][-1], F["t_len"][-1], M, X, kv.GAPS[F["gap"][-1]], F["W"][-1], F["end_bonus"][-1])


def draw_pair(n, lo, hi):
    """the recipe of the wide and mid sets: a quarter unrelated; the rest mutated at 12 / 25 / 35 %, half of those cut off and followed by unrelated
    sequence; a third over a two-letter alphabet.  Sides of lo-hi."""
    k = 2 if n % 3 == 0 else 4
    a = rnd(rng.integers(lo, hi + 1), k)
    if n % 4 == 0:
        return a, rnd(rng.integers(lo, hi + 1), k), "unrelated"
    rate = (0.12, 0.25, 0.35)[n % 3]
    b = mutate(a, rate, k)
    kind = "r%d" % int(rate * 100)
    if n & 1:
        b = b[:int(rng.integers(lo // 4, b.size + 1))]
        kind += "_cut"
    return a, fit(b, int(np.clip(b.size + (rng.integers(lo // 2, hi // 2) if n & 1 else 0), lo, hi)), k), kind


# ---- the first base of the first read: a view walked forwards from it, and one walked backwards onto it ----
q = rnd(700)
t = mutate(q, 0.12)
reads.append(np.concatenate([q, rnd(45)]))
reads.append(np.concatenate([t, rnd(13)]))
add_views("view_first_base_fwd", q, t, 300, 400, (0, 0, 1, 0), (1, 0, 1, 0), end_bonus=100)
q2 = reads[0][:250][::-1].copy()
t2 = mutate(q2, 0.12)
r2, f2 = store(t2, -1, 1, 19, 6)
reads.append(r2)
add_views("view_first_base_bwd", q2, t2, 40, 400, (0, 249, -1, 0), (len(reads) - 1, f2, -1, 1), end_bonus=100)

# ---- form edges ----
for S in EDGE_S:
    widest = S == 2047
    for kind, shape in (("copy", "sym" if S & 1 else "short_t"), ("unrelated", "short_t" if S & 1 else "short_q"), ("prefix", "short_q" if S & 1 else "short_t"),
                        ("all_A", "sym" if S & 1 else "short_q"), ("copy_short_t", "short_t"), ("copy_short_q", "short_q")):
        if shape == "sym":
            w = (S - 1) // 2
            ql, tl = w + 1 + int(rng.integers(0, 40)), w + 1 + int(rng.integers(0, 40))
        else:
            w = 1023 if widest else min(1023, S // 2 + 1 + int(rng.integers(0, max(2, S // 8))))
            short, other = S - w, w + 1 + int(rng.integers(0, 40))      # the short side's length - 1 = S - 1 - w < w (S = 2 047: = w)
            ql, tl = (other, short) if shape == "short_t" else (short, other)
        if kind.startswith("copy"):
            q = rnd(ql)
            t = fit(mutate(q, 0.12), tl)
            h0 = pick((30, 400, 5000))
        elif kind == "unrelated":
            q, t, h0 = rnd(ql), rnd(tl), 5000      # a start score under which no cell reaches 0: the whole band stays live
        elif kind == "prefix":
            q = rnd(ql)
            n = min(ql, tl) // 2
            t = np.concatenate([q[:n], rnd(tl - n)])
            h0 = pick((30, 400))
        else:
            q, t, h0 = np.zeros(ql, dtype=np.uint8), np.zeros(tl, dtype=np.uint8), pick((0, 30, 5000))
        add("edge_S%d_%s" % (S, kind), q, t, w, h0, gap=int(rng.integers(3)), end_bonus=100)
        assert slots_of_last() == S, (F["names"][-1], slots_of_last())
        if shape == "short_t":
            assert (tl - 1 < w or widest) and min(w, tl - 1) == tl - 1
        if shape == "short_q":
            assert (ql - 1 < w or widest) and min(w, ql - 1) == ql - 1

# ---- wide forms (C = 16, 32) and the forms below them, every exit ----
n = 0
for form, count, lo, hi, ws in ((32, 44, 300, 2200, (512, 800, 1023)), (16, 40, 300, 2200, (300, 300, 512)), (8, 36, 130, 700, (130, 200, 255)),
                                (4, 36, 70, 400, (70, 100, 127)), (2, 36, 40, 250, (40, 60)), (1, 36, 5, 120, (3, 10, 31))):
    made = 0
    while made < count:
        n += 1
        q, t, kind = draw_pair(n, lo, hi)
        w, gap, eb = pick(ws), int(rng.integers(4)), pick(kv.END_BONUS)
        if kv.form_of(kv.slots_of(q.size, t.size, M, X, kv.GAPS[gap], w, eb)) != form:
            continue
        add("form%d_%d_%s" % (form, made, kind), q, t, w, pick((0, 1, 30, 400, 5000)), gap=gap, end_bonus=eb, zdrop=kv.ZDROPS[made & 1])
        made += 1

# the z-drop exit needs the row maximum to fall by more than zdrop beyond what the gap between the two diagonals costs (ksw.c:458-462); a vertical gap from the
# best cell holds the maximum up until it leaves the band, so the target goes on for more than w rows of unrelated sequence behind a copied prefix, under a start
# score that keeps the row maximum above 0 for that long
for form, ws in ((32, (512, 800)), (16, (300, 400)), (8, (130, 200)), (4, (70, 100)), (2, (40, 60)), (1, (10, 31))):
    for k in range(8):
        w = ws[k & 1]
        p = int(rng.integers(40, 80 + w // 2))          # 2 p, what the prefix gains over a path that never matched, well above zdrop
        q = rnd(p + w + 40 + rng.integers(0, 2 * w))
        t = np.concatenate([mutate(q[:p], 0.12), rnd(w + 60 + rng.integers(0, 100))])
        add("form%d_zdrop_%d" % (form, k), q, t, w, pick((400, 5000)), gap=k % 4, end_bonus=pick(kv.END_BONUS), zdrop=40)
        assert kv.form_of(slots_of_last()) == form, F["names"][-1]

# ---- views inside longer reads ----
for k in range(64):
    cls = k // 16                                      # 16 per size class: the four strand combinations x (no rev, q_rev, t_rev, both)
    qs, ts = (1, -1)[k & 1], (1, -1)[(k >> 1) & 1]
    qr, tr = (k >> 2) & 1, (k >> 3) & 1
    lo, hi, w = ((20, 120, 31), (100, 300, 100), (250, 500, 250), (650, 900, 600))[cls]
    q = rnd(rng.integers(lo, hi + 1))
    t = mutate(q, (0.12, 0.25)[k & 1])
    if k % 3 == 0:
        t = np.concatenate([t[:t.size // 2], rnd(t.size // 2 + 1)])
    t = fit(t, max(t.size, w + 2 if cls >= 2 else 1))
    q = fit(q, max(q.size, w + 2 if cls >= 2 else 1))
    views = []
    for d, strand, rev, res in ((q, qs, qr, k % 32), ((t, ts, tr, (5 * k + 11) % 32))):
        left = int(rng.integers(0, 4)) * 32
        left += (res - (left if strand > 0 else left + d.size - 1)) % 32      # from = res (mod 32)
        r, frm = store(d, strand, rev, left, int(rng.integers(0, 70)))
        assert frm % 32 == res
        reads.append(r)
        views.append((len(reads) - 1, frm, strand, rev))
    add_views("view_%d_q%+d%s_t%+d%s" % (k, qs, "r" if qr else "", ts, "r" if tr else ""), q, t, w, pick((30, 400, 5000)), views[0], views[1], end_bonus=100)

# ---- rows ----
q = rnd(20000)
add("rows_20000_w40", q, fit(mutate(q, 0.05), 20000), 40, 32767, gap=0, end_bonus=100, zdrop=-1)
q = rnd(6000)
add("rows_6000_w1023", q, fit(mutate(q, 0.12), 6000), 1023, 5000, gap=0, end_bonus=100, zdrop=-1)

# ---- the chain set: shared segments with related flanks long enough for the extension stages to run in the wide forms ----
C_ = {k: [] for k in ("names", "q_read", "t_read", "t_rev", "w", "T", "expect", "local", "flags", "slots")}
for k in range(40):
    seg = rnd(rng.integers(80, 401))
    # flanks of 600-1 500 (sixteen and thirty-two slots per lane need a remaining side below / above 512: a third of the rows have one pair of flanks of 280-480);
    # the longer flank of a side alternates between the two reads, so that both roles occur on both sides
    short_side = (None, 0, 1)[k % 3]
    fl = [rnd(rng.integers(280, 481) if short_side == s else rng.integers(600, 1501)) for s in (0, 1)]
    a = np.concatenate([fl[0], seg, fl[1]])
    bl, br = mutate(fl[0], FLANK_RATE), mutate(fl[1], FLANK_RATE)
    if k & 2:
        bl = np.concatenate([rnd(rng.integers(100, 400)), bl])
    else:
        a = np.concatenate([rnd(rng.integers(100, 400)), a])
    if k & 4:
        br = np.concatenate([br, rnd(rng.integers(100, 400))])
    else:
        a = np.concatenate([a, rnd(rng.integers(100, 400))])
    b = np.concatenate([bl, mutate(seg, 0.12), br])
    t_rev = k & 1
    reads.append(a)
    reads.append(revcomp(b) if t_rev else b)
    w, T = (800, 1023)[(k >> 1) & 1], (-100, -30)[(k >> 2) & 1] if k < 32 else (-100, -30)[k & 1]
    rec = []
    e, flg, loc = kv.ref_chain(a, b, M, X, w, -3, -3, -1, T, record=rec)
    sl = [0, 0]
    for side, role, args in rec:
        sl[side] = kv.slots_of(len(args[0]), len(args[1]), M, X, args[4], args[5], args[6])
    for key, v in zip(("names", "q_read", "t_read", "t_rev", "w", "T", "expect", "local", "flags", "slots"),
                      ("wide_%d_w%d_T%d" % (k, w, -T), len(reads) - 2, len(reads) - 1, t_rev, w, T, e, loc, flg, sl)):
        C_[key].append(v)

# ---- the last base of the last read: these reads go last ----
q = rnd(900)
t = fit(mutate(q, 0.12), 880)
rq, fq = store(q, 1, 0, 37, 0)
rt, ft = store(t, 1, 0, 5, 0)
t3 = rt[-200:][::-1].copy()                            # the last read walked backwards from its last base
q3 = mutate(t3, 0.12)
rq3, fq3 = store(q3, -1, 0, 11, 3)
reads.extend([rq, rq3, rt])
iq, iq3, it = len(reads) - 3, len(reads) - 2, len(reads) - 1
add_views("view_last_base_fwd", q, t, 300, 400, (iq, fq, 1, 0), (it, ft, 1, 0), end_bonus=100)
add_views("view_last_base_bwd", q3, t3, 40, 400, (iq3, fq3, -1, 0), (it, rt.size - 1, -1, 0), end_bonus=100)
# the complements of the same two walks: t_rev from the first base of the reversed read is the last base of the stored one
add_views("view_last_base_rev", (3 - q3).astype(np.uint8), (3 - t3).astype(np.uint8), 40, 5000, (iq3, 3, 1, 1), (it, 0, 1, 1), end_bonus=100)


def fixed_band_cells(qlen, w, rows):
    """cells of the first `rows` rows when nothing trims the band"""
    i = np.arange(rows, dtype=np.int64)
    return int(np.maximum(0, np.minimum(qlen, i + w + 1) - np.maximum(0, i - w)).sum())


def work(i):
    q, t = F["seqs"][i]
    args = (q, t, M, X, kv.GAPS[F["gap"][i]], F["W"][i], F["end_bonus"][i], F["zdrop"][i], F["init_score"][i])
    ref = kv.ref_extend(*args)
    six, stop, rows, cells = kv.py_extend(*args)
    assert tuple(int(x) for x in ref) == six, (F["names"][i], ref, six)
    # a band that was never trimmed has the cells of the fixed band: only otherwise can a fixed band give other ints
    w = kv.clamped_w(q.size, M, X, args[4], args[5], args[6])
    trim = cells != fixed_band_cells(q.size, w, rows) and kv.py_extend(*args, trim=False)[0] != six
    return ref, stop, rows, cells, int(trim)


if __name__ == "__main__":
    n = len(F["names"])
    assert len(set(F["names"])) == n
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        done = pool.map(work, range(n), chunksize=1)
    expect = np.array([d[0] for d in done], dtype=np.int32)
    stop = np.array([d[1] for d in done], dtype=np.int32)
    rows = np.array([d[2] for d in done], dtype=np.int64)
    cells = np.array([d[3] for d in done], dtype=np.int64)
    trim = np.array([d[4] for d in done], dtype=np.int32)
    slots = np.array([kv.slots_of(F["q_len"][i], F["t_len"][i], M, X, kv.GAPS[F["gap"][i]], F["W"][i], F["end_bonus"][i]) for i in range(n)], dtype=np.int32)
    form = np.array([kv.form_of(int(s)) for s in slots], dtype=np.int32)
    names = F["names"]
    assert stop[names.index("rows_20000_w40")] == kv.STOP_END and rows[names.index("rows_20000_w40")] == 20000
    assert rows[names.index("rows_6000_w1023")] > 5000 and form[names.index("rows_6000_w1023")] == 32

    branches = (("last row", stop == kv.STOP_END), ("m == 0", stop == kv.STOP_M0), ("z-drop", stop == kv.STOP_ZDROP), ("trim matters", trim != 0),
                ("gscore == -1", expect[:, 4] == -1), ("gscore > score - 100", expect[:, 4] > expect[:, 0] - 100))
    short_of = False
    print("%-4s %8s " % ("C", "problems") + " ".join("%20s" % b[0] for b in branches))
    for c in kv.FORMS:
        cnt = [int((sel & (form == c)).sum()) for _, sel in branches]
        print("%-4d %8d " % (c, int((form == c).sum())) + " ".join("%20d" % x for x in cnt))
        short_of = short_of or min(cnt) < MIN_PER_BRANCH
    assert not short_of
    per_s = {S: int((slots == S).sum()) for S in EDGE_S}
    print("problems per slot count at the form edges: " + ", ".join("%d: %d" % kv_ for kv_ in per_s.items()))
    assert min(per_s.values()) >= MIN_PER_S
    view = [i for i, x in enumerate(names) if x.startswith("view_")]
    assert {F["q_from"][i] % 32 for i in view} == set(range(32)) and {F["t_from"][i] % 32 for i in view} == set(range(32))
    kinds = {(F["q_strand"][i], F["t_strand"][i], F["q_rev"][i], F["t_rev"][i]) for i in view if form[i] >= 8}
    assert len(kinds) == 16, kinds
    print("views: %d, %d of them in forms with C >= 8, every residue of q_from and t_from mod 32" % (len(view), sum(form[i] >= 8 for i in view)))

    cf = np.array(C_["flags"], dtype=np.int64)
    cs = np.array(C_["slots"], dtype=np.int32)
    ran = np.stack([(cf & kv.F_LEFT_RAN) != 0, (cf & kv.F_RIGHT_RAN) != 0], axis=1)
    role1 = np.stack([(cf & kv.F_LEFT_ROLE1) != 0, (cf & kv.F_RIGHT_ROLE1) != 0], axis=1)
    assert ((cs > 0) == ran).all()
    cform = np.array([[kv.form_of(int(s)) if s else 0 for s in r] for r in cs])
    for side in (0, 1):
        for role in (0, 1):
            for c in (16, 32):
                cnt = int((ran[:, side] & (role1[:, side] == bool(role)) & (cform[:, side] == c)).sum())
                print("chain %s stage, %s as the rows, C = %d: %d" % (("left", "right")[side], ("target", "query")[role], c, cnt))
                short_of = short_of or cnt < 2
    assert not short_of
    print("chain gscore commits: left %d, right %d" % (int(((cf & kv.F_LEFT_GSCORE) != 0).sum()), int(((cf & kv.F_RIGHT_GSCORE) != 0).sum())))
    print("function-level problems: %d, chain rows: %d, reads: %d, bases: %d" % (n, len(C_["names"]), len(reads), sum(r.size for r in reads)))

    words, offs, lens = hipabi.pack_reads(reads)
    out = {"words": words, "offs": offs, "lens": lens, "M": np.int32(M), "X": np.int32(X), "f_names": np.array(names), "f_expect": expect, "f_stop": stop,
           "f_rows": rows, "f_cells": cells, "f_trim": trim, "f_slots": slots, "f_form": form}
    for k in ("q_read", "t_read", "q_rev", "t_rev", "q_from", "t_from", "q_strand", "t_strand", "q_len", "t_len", "init_score", "W", "gap", "end_bonus", "zdrop"):
        out["f_" + k] = np.array(F[k], dtype=np.int32)
    out.update({"c_names": np.array(C_["names"]), "c_expect": np.array(C_["expect"], dtype=np.int32), "c_local": np.array(C_["local"], dtype=np.int32),
                "c_flags": cf.astype(np.int32), "c_slots": cs})
    for k in ("q_read", "t_read", "t_rev", "w", "T"):
        out["c_" + k] = np.array(C_[k], dtype=np.int32)
    np.savez_compressed(kv.WIDE_VECTORS, **out)
    print("wrote %s (%d bytes)" % (os.path.relpath(kv.WIDE_VECTORS, kv.ROOT), os.path.getsize(kv.WIDE_VECTORS)))
    assert os.path.getsize(kv.WIDE_VECTORS) < (1 << 19)
