#!/usr/bin/env python3
"""Generator of tests/golden/local_vectors.npz: inputs and outputs of the reference's own ksw_align2(..., KSW_XSTART) (ksw.c:344-366, 16-bit lanes),
called through oracle/_ref/libref_shim.so on a seeded problem set.  The file holds data only: the sequences as 2-bit words (dna.h:78 layout, as
wtz_upload_reads takes them), per problem the two read ids, the index of its gap costs in localvec.GAPS, a name, and the five ints
(score, te, qe, tb, qb) the routine returned; M = 2, X = -5 throughout (the default of wtcyc, pairaln and wtcns).

    python tests/golden/make_local_vectors.py          (needs oracle/_ref, i.e. a machine that has the reference's sources)

The set: unrelated pairs; pairs sharing a segment mutated at 10-15 % (mostly insertions and deletions), same strand and opposite strand; reads
against their own reverse complement with a planted palindrome (wtcyc's shape); query lengths at the lane, stripe and strip edges
(1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049); all-A pairs; gaps of > 64 and > 512 columns and rows inside an alignment; the four
gap-cost settings of localvec.GAPS (unequal opening costs among them); two identical 17 000-base sequences (the score saturates at 32767) and the
same pair with one substitution at base 16 500.

A problem that the reference leaves with tb = -1 (second-pass maximum different from the score, ksw.c:363) was searched for and NOT found:
SEARCH_TB_MINUS1 random small pairs (lengths 1-120, two- and four-letter alphabets, all four gap settings, also M = 1 / X = -1) gave none, and the
set contains none.  None is fabricated.  (With H equal to the plain recurrence the second pass's cells are scores of paths of the first
pass's rectangle read backwards, so its maximum cannot differ while nothing saturates; at saturation both passes stop at 32767.)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import localvec as lv  # noqa: E402
from smartdenovo_amd import hipabi  # noqa: E402

M, X = 2, -5
SEARCH_TB_MINUS1 = 40000
rng = np.random.default_rng(20260117)


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


reads, names, q_read, t_read, gap = [], [], [], [], []


def add(name, q, t, g):
    reads.append(np.asarray(q, dtype=np.uint8))
    reads.append(np.asarray(t, dtype=np.uint8))
    q_read.append(len(reads) - 2)
    t_read.append(len(reads) - 1)
    names.append(name)
    gap.append(g)


def shared_pair(lq, lt, lseg, rate, opposite):
    seg = rnd(lseg)
    a = np.concatenate([rnd(rng.integers(0, max(1, lq - lseg))), seg, rnd(rng.integers(0, max(1, lq - lseg)))])
    m = mutate(seg, rate)
    b = np.concatenate([rnd(rng.integers(0, max(1, lt - lseg))), revcomp(m) if opposite else m, rnd(rng.integers(0, max(1, lt - lseg)))])
    return a, b


def build():
    for n in range(60):
        add("unrelated_%d" % n, rnd(rng.integers(20, 1500)), rnd(rng.integers(20, 1500)), n % 4)
    for n in range(120):
        lq, lt = int(rng.integers(200, 3000)), int(rng.integers(200, 3000))
        a, b = shared_pair(lq, lt, int(min(lq, lt) * rng.uniform(0.3, 0.9)), rng.uniform(0.10, 0.15), n % 3 == 2)
        add("shared_%s_%d" % ("opposite" if n % 3 == 2 else "same", n), a, b, n % 4 if n % 2 else 0)
    for n, L in enumerate((2000, 2500, 3000, 3500, 4000, 4500, 5000, 2200, 3300, 8000)):
        half = mutate(rnd(L // 8), 0.12)
        r = np.concatenate([rnd(L // 3), half, rnd(int(rng.integers(0, 60))), revcomp(mutate(half, 0.12)), rnd(L // 3)])
        add("cyc_palindrome_%d" % n, r, revcomp(r), 0)
    for ql in (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049):
        q = rnd(ql)
        add("qlen_%d_unrelated" % ql, q, rnd(rng.integers(30, 400)), 0)
        add("qlen_%d_inside" % ql, q, np.concatenate([rnd(70), mutate(q, 0.12), rnd(90)]), 0)
        add("qlen_%d_tail" % ql, q, np.concatenate([rnd(130), mutate(q, 0.10)[: max(1, ql - ql // 5)]]), 1)
        add("qlen_%d_exact" % ql, q, q.copy(), 3)
        add("tlen_%d_inside" % ql, np.concatenate([rnd(70), mutate(q, 0.12), rnd(90)]), q, 2)
    for n, (lq, lt) in enumerate(((50, 50), (300, 200), (1100, 700), (64, 1025))):
        add("all_A_%dx%d" % (lt, lq), np.zeros(lq, dtype=np.uint8), np.zeros(lt, dtype=np.uint8), n % 4)
    for n, gl in enumerate((80, 600)):
        for g in (0, 1, 2):
            a, b = rnd(400 + 3 * gl // 2), rnd(400 + 3 * gl // 2)
            add("gap_%d_columns_g%d" % (gl, g), np.concatenate([rnd(30), a, rnd(gl), b, rnd(20)]), np.concatenate([rnd(10), a, b, rnd(40)]), g)
            add("gap_%d_rows_g%d" % (gl, g), np.concatenate([rnd(10), a, b, rnd(40)]), np.concatenate([rnd(30), a, rnd(gl), b, rnd(20)]), g)
    for n in range(40):
        a, b = shared_pair(int(rng.integers(30, 300)), int(rng.integers(30, 300)), int(rng.integers(10, 30)), 0.3, False)
        add("short_lowid_%d" % n, a % (2 if n % 2 else 4), b % (2 if n % 2 else 4), n % 4)
    big = rnd(17000)
    add("identical_17000_saturating", big, big.copy(), 0)
    mut = big.copy()
    mut[16500] = (mut[16500] + 1) % 4
    add("identical_17000_one_substitution_at_16500", big, mut, 0)


def search_tb_minus1():
    found = 0
    for n in range(SEARCH_TB_MINUS1):
        k = 2 if n % 2 else 4
        q, t = rnd(rng.integers(1, 121), k), rnd(rng.integers(1, 121), k)
        if n % 3 == 0:
            t = np.concatenate([rnd(rng.integers(0, 20), k), mutate(q, 0.3) % k])
        m, x = ((2, -5), (1, -1))[(n // 4) % 2]
        r = lv.ref_align(q, t, m, x, lv.GAPS[n % 4])
        if r[3] < 0 or r[4] < 0:
            found += 1
            if (m, x) == (M, X):
                add("tb_minus1_%d" % found, q, t, n % 4)
    return found


def main():
    if not lv.have_shim():
        sys.exit("oracle/_ref/libref_shim.so is missing: build it with `python __graft_entry__.py build` where the reference's sources are")
    build()
    found = search_tb_minus1()
    print("problems with tb = -1 found by the search: %d of %d" % (found, SEARCH_TB_MINUS1))
    expect = np.array([lv.ref_align(reads[q], reads[t], M, X, lv.GAPS[g]) for q, t, g in zip(q_read, t_read, gap)], dtype=np.int32)
    words, offs, lens = hipabi.pack_reads(reads)
    np.savez_compressed(lv.VECTORS, words=words, offs=offs, lens=lens, q_read=np.array(q_read, dtype=np.uint32), t_read=np.array(t_read, dtype=np.uint32),
                        gap=np.array(gap, dtype=np.uint8), expect=expect, names=np.array(names), M=np.int32(M), X=np.int32(X))
    cells = int(sum(int(lens[q]) * int(lens[t]) for q, t in zip(q_read, t_read)))
    print("%d problems, %d reads, %.2f Gcells (first pass), %d bytes" % (len(names), len(reads), cells / 1e9, os.path.getsize(lv.VECTORS)))
    print("saturated: %d, score 0: %d, tb < 0: %d" % (int((expect[:, 0] == 32767).sum()), int((expect[:, 0] == 0).sum()), int((expect[:, 3] < 0).sum())))


if __name__ == "__main__":
    main()
