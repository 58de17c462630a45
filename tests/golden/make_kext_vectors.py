#!/usr/bin/env python3
"""Generator of tests/golden/kext_vectors.npz: inputs and outputs of the reference's own ksw_extend2 (ksw.c:381-478), called through
oracle/_ref/libref_shim.so on a seeded problem set, and a second table for the chain kswx_align_no_stat (kswx.h:1504-1511; see tests/kextvec.py for
what pins what there).  The file holds data only: the sequences as 2-bit words (dna.h:78 layout, as wtz_upload_reads takes them); per function-level
problem its wtz_dp_problem_t fields, the index of its gap costs in kextvec.GAPS, end_bonus, zdrop, a name, the six ints the routine returned and,
from the Python restatement checked against them, why it stopped, the rows it entered and their cells; per chain row the two reads, t_rev, w, T, the
six ints (found, score, tb, te, qb, qe), the local hit and the branches taken.  M = 2, X = -5 throughout.

    python tests/golden/make_kext_vectors.py          (needs oracle/_ref, i.e. a machine that has the reference's sources)

The counts of every branch the set is meant to reach are asserted (> 0) and printed before the file is written."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kextvec as kv  # noqa: E402
import localvec as lv  # noqa: E402
from smartdenovo_amd import hipabi  # noqa: E402

M, X = 2, -5
rng = np.random.default_rng(20261019)


def rnd(n, k=4):
    return rng.integers(0, k, int(n)).astype(np.uint8)


def revcomp(s):
    return (3 - s[::-1]).astype(np.uint8)


def mutate(s, rate):
    """substitutions 20 %, insertions 40 %, deletions 40 % of the events; a fifth of the deletions and insertions are runs of 2-8"""
    out = []
    i = 0
    while i < len(s):
        r = rng.random()
        if r < rate * 0.4:
            out.extend(rnd(1 + (rng.integers(1, 8) if rng.random() < 0.2 else 0)))
        elif r < rate * 0.8:
            i += 1 + (int(rng.integers(1, 8)) if rng.random() < 0.2 else 0)
            continue
        elif r < rate:
            out.append((int(s[i]) + 1 + int(rng.integers(3))) % 4)
            i += 1
            continue
        out.append(int(s[i]))
        i += 1
    return np.array(out if out else [0], dtype=np.uint8)


reads = []
F = {k: [] for k in ("names", "q_read", "t_read", "q_from", "t_from", "q_strand", "t_strand", "q_len", "t_len", "init_score", "W", "gap", "end_bonus", "zdrop", "seqs")}


def pick(xs):
    return xs[int(rng.integers(len(xs)))]


def add(name, q, t, w, h0, gap=None, end_bonus=None, zdrop=None, reverse=False):
    """reverse: the problem is the two reads walked backwards from their last base (the views a left extension uses)"""
    q, t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
    reads.append(q[::-1].copy() if reverse else q)
    reads.append(t[::-1].copy() if reverse else t)
    F["names"].append(name)
    F["q_read"].append(len(reads) - 2)
    F["t_read"].append(len(reads) - 1)
    F["q_from"].append(q.size - 1 if reverse else 0)
    F["t_from"].append(t.size - 1 if reverse else 0)
    F["q_strand"].append(-1 if reverse else 1)
    F["t_strand"].append(-1 if reverse else 1)
    F["q_len"].append(q.size)
    F["t_len"].append(t.size)
    F["init_score"].append(h0)
    F["W"].append(w)
    F["gap"].append(int(rng.integers(4)) if gap is None else gap)
    F["end_bonus"].append(pick(kv.END_BONUS) if end_bonus is None else end_bonus)
    F["zdrop"].append(pick(kv.ZDROPS) if zdrop is None else zdrop)
    F["seqs"].append((q, t))


def copy_pair(lq, rate, extra_rows=0, tail=False):
    """a query and a target that is its mutated copy, optionally followed by unrelated sequence / by `extra_rows` more bases"""
    q = rnd(lq)
    t = mutate(q, rate)
    if tail:
        t = np.concatenate([t, rnd(rng.integers(10, 80))])
    if extra_rows:
        t = np.concatenate([t, rnd(extra_rows)])
    return q, t


# query lengths at the lane / per-lane-column edges, each at four band widths
for ql in kv.QLENS:
    for w in (1, 33, 128, 800):
        q, t = copy_pair(ql, 0.12, tail=bool(rng.integers(2)))
        add("qlen_%d_w%d" % (ql, w), q, t, w, pick((30, 400, 5000)))
# band widths at the edges of every kernel instantiation, against a query below and above 2w + 1
for w in kv.WS:
    for kind, ql in (("short", max(1, min(2 * w, w + 5))), ("long", 2 * w + 1 + int(rng.integers(20, 90)))):
        q, t = copy_pair(ql, 0.12, tail=(kind == "short"))
        add("w_%d_%s" % (w, kind), q, t, w, pick((400, 5000, 32767)), end_bonus=100)
# 513-1024 diagonals (sixteen slots per lane): w = 800 against sides of 300-500
for k in range(3):
    q, t = copy_pair(300 + 100 * k, 0.12)
    add("w_800_mid_%d" % k, q, t, 800, 5000, end_bonus=100)
# the band runs off the query: identical start, then far more rows than columns + w
for k, (ql, w) in enumerate(((40, 3), (64, 10), (65, 33), (130, 40), (257, 31), (20, 128))):
    q = rnd(ql)
    t = np.concatenate([q if k % 2 else mutate(q, 0.12), rnd(w + 60 + 20 * k)])
    add("runoff_%d" % k, q, t, w, pick((400, 5000, 32767)))
# mutated copies, half of them followed by unrelated sequence
for k in range(150):
    rate = (0.12, 0.25, 0.35)[k % 3]
    q, t = copy_pair(rng.integers(1, 261), rate, tail=bool(k & 1))
    add("copy_%d_r%d" % (k, int(rate * 100)), q, t, pick((3, 10, 40, 800)), pick(kv.H0S))
# unrelated pairs, two-letter alphabets, all-A pairs: ties
for k in range(40):
    add("unrelated_%d" % k, rnd(rng.integers(1, 200)), rnd(rng.integers(1, 200)), pick((3, 10, 40, 800)), pick(kv.H0S))
for k in range(40):
    q = rnd(rng.integers(1, 200), 2)
    t = mutate(q, 0.25) % 2 if k & 1 else rnd(rng.integers(1, 200), 2)
    add("two_letter_%d" % k, q, t.astype(np.uint8), pick((3, 10, 40, 800)), pick(kv.H0S))
for k, (ql, tl, w) in enumerate(((1, 1, 0), (5, 9, 3), (64, 64, 40), (65, 130, 10), (200, 90, 800), (256, 300, 128), (100, 400, 33))):
    add("all_A_%d" % k, np.zeros(ql, dtype=np.uint8), np.zeros(tl, dtype=np.uint8), w, pick(kv.H0S), zdrop=-1 if k & 1 else 40)
# every start score, z-drop and end bonus against every gap setting at least once
for h0 in kv.H0S:
    for g in range(4):
        q, t = copy_pair(rng.integers(30, 200), 0.25, tail=True)
        add("h0_%d_g%d" % (h0, g), q, t, pick((10, 40)), h0, gap=g)
for eb in kv.END_BONUS:      # the clamp of ksw.c:403-408 bites: one column, no bonus
    add("clamp_qlen1_eb%d" % eb, rnd(1), rnd(30), 40, 30, end_bonus=eb, gap=0)
# both strands of a view: the reads walked backwards from their far end
for k in range(24):
    q, t = copy_pair(rng.integers(1, 261), (0.12, 0.25)[k & 1], tail=bool(k & 2))
    add("rev_%d" % k, q, t, pick((3, 10, 40, 800)), pick(kv.H0S), reverse=True)

n = len(F["names"])
expect = np.zeros((n, 6), dtype=np.int32)
stop = np.zeros(n, dtype=np.int32)
rows = np.zeros(n, dtype=np.int64)
cells = np.zeros(n, dtype=np.int64)
untrimmed_differs = 0
for i in range(n):
    q, t = F["seqs"][i]
    args = (q, t, M, X, kv.GAPS[F["gap"][i]], F["W"][i], F["end_bonus"][i], F["zdrop"][i], F["init_score"][i])
    expect[i] = kv.ref_extend(*args)
    six, stop[i], rows[i], cells[i] = kv.py_extend(*args)
    assert tuple(int(x) for x in expect[i]) == six, (F["names"][i], expect[i].tolist(), six)
    untrimmed_differs += kv.py_extend(*args, trim=False)[0] != six
counts = {
    "m == 0 stop": int((stop == kv.STOP_M0).sum()), "zdrop stop": int((stop == kv.STOP_ZDROP).sum()), "ran to the last row": int((stop == kv.STOP_END).sum()),
    "end == qlen row seen": int((expect[:, 4] >= 0).sum()), "no end == qlen row": int((expect[:, 4] < 0).sum()),
    "gscore > score - 100": int((expect[:, 4] > expect[:, 0] - 100).sum()), "a fixed band gives another result": int(untrimmed_differs),
}

# ---- the chain set ----
C_ = {k: [] for k in ("names", "q_read", "t_read", "t_rev", "w", "T", "expect", "local", "flags")}
COMBOS = [(w, T) for w in (20, 800) for T in (-100, -30, 0)]


def add_chain(name, q, t, t_rev, combos):
    q, t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
    if t is q:
        reads.append(q)
        qi = ti = len(reads) - 1
    else:
        reads.append(q)
        reads.append(t)
        qi, ti = len(reads) - 2, len(reads) - 1
    tt = revcomp(t) if t_rev else t
    for w, T in combos:
        e, fl, loc = kv.ref_chain(q, tt, M, X, w, -3, -3, -1, T)
        for k, v in zip(("names", "q_read", "t_read", "t_rev", "w", "T", "expect", "local", "flags"), ("%s_w%d_T%d" % (name, w, -T), qi, ti, int(t_rev), w, T, e, loc, fl)):
            C_[k].append(v)


# wtcyc's shape: a read against its own reverse complement, with a planted palindrome (cyc_palindrome_* of make_local_vectors.py)
for k in range(10):
    L = int(rng.integers(2000, 8001)) if k < 3 else int(rng.integers(2000, 3001))
    arm = rnd(rng.integers(200, 500))
    mid = rnd(rng.integers(0, 40))
    pal = np.concatenate([arm, mid, mutate(revcomp(arm), 0.12)])
    left = int(rng.integers(100, L - pal.size - 100))
    s = np.concatenate([rnd(left), pal, rnd(L - pal.size - left)])
    add_chain("cyc_palindrome_%d" % k, s, s, 1, [COMBOS[(2 * k) % 6], COMBOS[(2 * k + 1) % 6]])
# pairs sharing a segment; where the flanks go on matching (mutated copies) the extension has something to add
for k in range(40):
    seg = rnd(rng.integers(80, 400))
    fl, fr = rnd(rng.integers(0, 300)), rnd(rng.integers(0, 300))
    related = k % 4 != 3
    a = np.concatenate([fl, seg, fr])
    b = np.concatenate([mutate(fl, 0.3) if related else rnd(rng.integers(0, 300)), mutate(seg, 0.12), mutate(fr, 0.3) if related else rnd(rng.integers(0, 300))])
    if k % 5 == 0:
        b = np.concatenate([rnd(rng.integers(50, 400)), b])      # a longer target side on the left
    if k % 7 == 0:
        a = np.concatenate([a, rnd(rng.integers(50, 400))])      # a longer query side on the right
    opposite = bool(k & 1)
    add_chain("shared_%d" % k, a, revcomp(b) if opposite else b, int(opposite), COMBOS)
add_chain("all_A_all_C", np.zeros(90, dtype=np.uint8), np.ones(70, dtype=np.uint8), 0, COMBOS[:2])
s = rnd(150)
add_chain("hit_touches_both_ends", s, s.copy(), 0, COMBOS[:2])
cf = np.array(C_["flags"], dtype=np.int64)
ce = np.array(C_["expect"], dtype=np.int32)
for name, bit in (("left skipped", kv.F_LEFT_SKIP), ("right skipped", kv.F_RIGHT_SKIP), ("left: target is the rows", None), ("left: query is the rows", kv.F_LEFT_ROLE1),
                  ("right: target is the rows", None), ("right: query is the rows", kv.F_RIGHT_ROLE1), ("left gscore commit", kv.F_LEFT_GSCORE), ("right gscore commit", kv.F_RIGHT_GSCORE)):
    if bit is not None:
        counts["chain " + name] = int(((cf & bit) != 0).sum())
    elif name.startswith("left"):
        counts["chain " + name] = int((((cf & kv.F_LEFT_RAN) != 0) & ((cf & kv.F_LEFT_ROLE1) == 0)).sum())
    else:
        counts["chain " + name] = int((((cf & kv.F_RIGHT_RAN) != 0) & ((cf & kv.F_RIGHT_ROLE1) == 0)).sum())
counts["chain left score commit"] = int((((cf & kv.F_LEFT_RAN) != 0) & ((cf & kv.F_LEFT_GSCORE) == 0)).sum())
counts["chain right score commit"] = int((((cf & kv.F_RIGHT_RAN) != 0) & ((cf & kv.F_RIGHT_GSCORE) == 0)).sum())
counts["chain found = 0"] = int((ce[:, 0] == 0).sum())
counts["chain both ends skipped"] = int((((cf & kv.F_LEFT_SKIP) != 0) & ((cf & kv.F_RIGHT_SKIP) != 0)).sum())
for k, v in counts.items():
    print("%-40s %d" % (k, v))
    assert v > 0, k
print("function-level problems: %d, chain rows: %d, reads: %d" % (n, len(C_["names"]), len(reads)))

words, offs, lens = hipabi.pack_reads(reads)
out = {"words": words, "offs": offs, "lens": lens, "M": np.int32(M), "X": np.int32(X),
       "f_names": np.array(F["names"]), "f_expect": expect, "f_stop": stop, "f_rows": rows, "f_cells": cells}
for k in ("q_read", "t_read", "q_from", "t_from", "q_strand", "t_strand", "q_len", "t_len", "init_score", "W", "gap", "end_bonus", "zdrop"):
    out["f_" + k] = np.array(F[k], dtype=np.int32)
out.update({"c_names": np.array(C_["names"]), "c_expect": ce, "c_local": np.array(C_["local"], dtype=np.int32), "c_flags": cf.astype(np.int32)})
for k in ("q_read", "t_read", "t_rev", "w", "T"):
    out["c_" + k] = np.array(C_[k], dtype=np.int32)
np.savez_compressed(kv.VECTORS, **out)
print("wrote %s (%d bytes)" % (kv.VECTORS, os.path.getsize(kv.VECTORS)))
assert os.path.getsize(kv.VECTORS) < (1 << 19)
