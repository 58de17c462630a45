"""Shared pieces of the alignment-picture tests (tests/test_pwtext_cpu.py, tests/test_gpu_pwtext.py): a restatement of kswx_cigar2pairwise (kswx.h:1150-1194)
with the marker loop of pairaln.c:115-125, the views of a wtz_dp_problem_t in Python, the case list, and the checks both back ends run."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smartdenovo_amd import hipabi  # noqa: E402
import localvec as lv  # noqa: E402


def picture(q, t, cigar):
    """q, t: 2-bit codes from the alignment's start on; cigar: len << 4 | op words.  The bytes `pairaln -a` prints: query line, marker line, target line."""
    a, b, x, y = [], [], 0, 0
    for w in cigar:
        op, n = int(w) & 15, int(w) >> 4
        assert op in (0, 1, 2)
        a += ["ACGT"[c] for c in q[x:x + n]] if op != 2 else ["-"] * n
        b += ["ACGT"[c] for c in t[y:y + n]] if op != 1 else ["-"] * n
        x, y = x + (n if op != 2 else 0), y + (n if op != 1 else 0)
    m = ["-" if i == "-" else "|" if i == j else "-" if j == "-" else "*" for i, j in zip(a, b)]
    return ("".join(a) + "\n" + "".join(m) + "\n" + "".join(b) + "\n").encode()


def view(reads, p, side):
    """the bases of one side of a DP_PROBLEM record as the library's views define them (reverse complement of the read first, then from / strand / len)"""
    r = reads[int(p[side + "_read"])]
    if p[side + "_rev"]:
        r = (3 - r[::-1]).astype(np.uint8)
    f, s, n = int(p[side + "_from"]), int(p[side + "_strand"]), int(p[side + "_len"])
    return r[f:f + n] if s > 0 else r[np.arange(f, f - n, -1)] if n else r[:0]


def expected(reads, pr, starts, slices, cigar):
    return [picture(view(reads, p, "q")[qb:], view(reads, p, "t")[tb:], cigar[o:o + n]) for p, (qb, tb), (o, n) in zip(pr, starts, slices)]


def split(out, blob):
    return [blob[int(o):int(o) + 3 * (int(c) + 1)] for o, c in zip(out["text_off"], out["cols"])]


def ops(*runs):
    return [n << 4 | op for op, n in runs]


def random_cigar(rng, cols, unit=False, n_ops=None):
    """a CIGAR of exactly `cols` columns; unit: runs of length 1 only (neighbouring operations differ); n_ops: that many operations"""
    if unit:
        o = rng.integers(0, 3, cols)
        for i in range(1, cols):
            if o[i] == o[i - 1]:
                o[i] = (o[i] + 1) % 3
        return [16 | int(x) for x in o]
    if n_ops is None:
        n_ops = max(1, cols // 5)
    n_ops = min(n_ops, cols)
    cuts = np.sort(rng.choice(np.arange(1, cols), n_ops - 1, replace=False)) if n_ops > 1 else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate([[0], cuts, [cols]]))
    return [int(n) << 4 | int(rng.integers(0, 3)) for n in lens]


def consumed(cig):
    return sum(w >> 4 for w in cig if w & 15 != 2), sum(w >> 4 for w in cig if w & 15 != 1)


class Cases:
    """reads, problems, starts, slices and the flat CIGAR of every case the feature names; built once per module"""

    def __init__(self):
        rng = np.random.default_rng(20261019)
        self.reads = [rng.integers(0, 4, n).astype(np.uint8) for n in (21000, 21000, 700, 650, 40, 33)]
        self.words, self.offs, self.lens = hipabi.pack_reads(self.reads)
        self.names, pr, self.starts, self.slices, self.cigar = [], [], [], [], []

        def add(name, cig, q_read=2, t_read=3, q_rev=0, t_rev=0, q_from=0, t_from=0, q_strand=1, t_strand=1, qb=0, tb=0, q_len=None, t_len=None):
            nq, nt = consumed(cig)
            p = np.zeros(1, dtype=hipabi.DP_PROBLEM)[0]
            p["q_read"], p["t_read"], p["q_rev"], p["t_rev"], p["q_from"], p["t_from"], p["q_strand"], p["t_strand"] = q_read, t_read, q_rev, t_rev, q_from, t_from, q_strand, t_strand
            p["q_len"], p["t_len"] = (qb + nq if q_len is None else q_len), (tb + nt if t_len is None else t_len)
            self.names.append(name); pr.append(p); self.starts.append((qb, tb)); self.slices.append((len(self.cigar), len(cig))); self.cigar += cig

        for cols in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024):
            add("cols_%d" % cols, random_cigar(rng, cols), q_read=0, t_read=1, q_from=cols % 7, t_from=cols % 5)
        add("cols_20000", random_cigar(rng, 20011, n_ops=3000), q_read=0, t_read=1)
        add("cols_20000_one_op", ops((0, 20000)), q_read=0, t_read=1, qb=17, tb=400)
        for n in (1, 63, 64, 65, 255, 256, 257):
            add("ops_%d" % n, random_cigar(rng, n, unit=True), q_read=0, t_read=1, q_from=n)
        add("ops_15000_unit", random_cigar(rng, 15003, unit=True), q_read=0, t_read=1)
        add("begins_op1", ops((1, 3), (0, 20), (2, 2), (0, 5)))
        add("ends_op1", ops((0, 20), (2, 2), (0, 5), (1, 4)))
        add("begins_op2", ops((2, 70), (0, 20), (1, 2), (0, 5)))
        add("ends_op2", ops((0, 20), (1, 66), (0, 5), (2, 9)))
        add("zero_start", ops((0, 0), (1, 0), (0, 12), (2, 3)))
        add("zero_middle", ops((0, 12), (2, 0), (0, 0), (1, 0), (0, 7), (1, 3), (2, 0), (2, 2)))
        add("zero_end", ops((0, 12), (1, 3), (0, 0), (2, 0)))
        add("zero_only", ops((0, 0), (1, 0), (2, 0)))
        add("empty_cigar", [])
        add("empty_cigar_inside", [], qb=5, tb=9, q_len=20, t_len=30)
        for k in range(1, 9):      # every text_off mod 4: 3 * (cols + 1) bytes each, one behind the other
            add("tiny_%d" % k, random_cigar(rng, k, unit=k % 2 == 0), q_from=k, t_from=2 * k)
        for k in range(32):        # every q_from / t_from mod 32 (read 2 starts at base 42 000 of the upload: 42 000 mod 32 = 16)
            add("from_%d" % k, ops((0, 40), (1, 3), (0, 37), (2, 5), (0, 11)), q_from=k, t_from=(k * 7 + 3) % 32)
        for qr in (0, 1):
            for tr in (0, 1):
                add("rev_%d%d" % (qr, tr), ops((0, 70), (2, 4), (0, 90), (1, 6), (0, 13)), q_rev=qr, t_rev=tr, q_from=3, t_from=11, qb=2, tb=1)
                add("strand_minus_%d%d" % (qr, tr), ops((0, 70), (2, 4), (0, 90), (1, 6), (0, 13)), q_rev=qr, t_rev=tr, q_from=500, t_from=420, q_strand=-1, t_strand=-1, qb=3, tb=7)
        add("first_base", ops((0, 33), (1, 2)), q_read=0, t_read=0)
        add("last_base", ops((2, 1), (0, 32)), q_read=5, t_read=5, q_len=32, t_len=33)      # read 5 ends the upload
        add("last_base_backwards", ops((0, 33)), q_read=5, t_read=0, q_from=32, q_strand=-1, t_rev=1, t_from=0)
        self.pr = np.array(pr, dtype=hipabi.DP_PROBLEM)
        self.cigar = np.array(self.cigar, dtype=np.uint32)
        self.want = expected(self.reads, self.pr, self.starts, self.slices, self.cigar)

    def sel(self, idx):
        idx = list(idx)
        return self.pr[idx], [self.starts[i] for i in idx], [self.slices[i] for i in idx]


def context(cases, lib_path=None, pool_bytes=1 << 28):
    return lv.make_context(cases.words, cases.offs, cases.lens, 2, -5, lib_path=lib_path, pool_bytes=pool_bytes)


# ---- the checks; ctx is a context over cases' reads on either back end ----
def check_whole_batch(ctx, cases):
    ctx.reset_counters()
    out, blob = ctx.pwtext_batch(cases.pr, cases.starts, cases.slices, cases.cigar)
    got = split(out, blob)
    bad = [n for n, g, w in zip(cases.names, got, cases.want) if g != w]
    assert not bad, bad[:8]
    assert len(blob) == sum(len(w) for w in cases.want) and [int(c) for c in out["cols"]] == [len(w) // 3 - 1 for w in cases.want]
    assert (np.diff(out["text_off"].astype(np.int64)) == 3 * (out["cols"][:-1].astype(np.int64) + 1)).all() and out["text_off"][0] == 0
    k = cases.names.index("tiny_1")
    assert set(int(o) % 4 for o in out["text_off"][k:k + 8]) == {0, 1, 2, 3}
    assert cases.want[cases.names.index("empty_cigar")] == b"\n\n\n" == cases.want[cases.names.index("zero_only")]
    c = ctx.counters()
    assert c.n_pwtext == len(cases.names) and c.bytes_pwtext == len(blob) and c.ms_pwtext > 0
    assert lv.pool_info(ctx).main_used == 0
    sized, none = ctx.pwtext_batch(cases.pr, cases.starts, cases.slices, cases.cigar, sizing_only=True)
    assert none == b"" and (sized == out).all() and ctx.counters().n_pwtext == c.n_pwtext      # the sizing call launches nothing


def check_batching_does_not_matter(ctx, cases):
    n = len(cases.names)
    rev = list(range(n))[::-1]
    out, blob = ctx.pwtext_batch(*cases.sel(rev), cases.cigar)
    assert split(out, blob) == cases.want[::-1]
    for i in range(n):
        out, blob = ctx.pwtext_batch(*cases.sel([i]), cases.cigar)
        assert blob == cases.want[i], cases.names[i]


def check_small_pool(cases, lib_path):
    """a 2 MB main pool: the two 20 000-column pictures and the 15 000-operation table do not fit together, the call is cut into launch groups"""
    ctx = context(cases, lib_path, pool_bytes=4 << 20)
    try:
        big = [cases.names.index(n) for n in ("cols_20000", "ops_15000_unit", "cols_20000_one_op")]
        idx = (big + list(range(0, 40))) * 12
        assert sum(12 * cases.slices[i][1] + len(cases.want[i]) for i in idx) > (2 << 20)
        ctx.reset_counters()
        out, blob = ctx.pwtext_batch(*cases.sel(idx), cases.cigar)
        assert split(out, blob) == [cases.want[i] for i in idx]
        assert ctx.counters().n_pwtext == len(idx) and lv.pool_info(ctx).main_used == 0
    finally:
        ctx.close()


def check_pool_error(cases, lib_path):
    """a 2 MB main pool, and one alignment of 200 000 operations of length 0 needs 2.4 MB of table and CIGAR words"""
    ctx = context(cases, lib_path, pool_bytes=4 << 20)
    try:
        n = 200_000
        cig = np.concatenate([np.zeros(n, dtype=np.uint32), cases.cigar])
        pr, st, sl = cases.sel([0, 1])
        sl = [(0, n), (sl[1][0] + n, sl[1][1])]
        with pytest.raises(RuntimeError, match="error -3"):
            ctx.pwtext_batch(pr, st, sl, cig)
        assert lv.pool_info(ctx).main_cap < 12 * n
        out, blob = ctx.pwtext_batch(pr, st, [(0, 0), sl[1]], cig)      # the context stays usable
        assert split(out, blob) == [b"\n\n\n", cases.want[1]] and lv.pool_info(ctx).main_used == 0
    finally:
        ctx.close()


def check_argument_errors(ctx, cases):
    i, j = cases.names.index("cols_64"), cases.names.index("rev_01")
    pr, st, sl = cases.sel([i, j])
    cig = cases.cigar.copy()

    def refused(pr=pr, st=st, sl=sl, cig=cig, cap=None):
        with pytest.raises(RuntimeError, match="error -1"):
            if cap is None:
                ctx.pwtext_batch(pr, st, sl, cig)
            else:
                import ctypes as C
                p = np.ascontiguousarray(pr, dtype=hipabi.DP_PROBLEM)
                inp = np.zeros(2, dtype=hipabi.PWTEXT_IN)
                inp["qb"], inp["tb"] = [s[0] for s in st], [s[1] for s in st]
                inp["cigar_off"], inp["cigar_len"] = [s[0] for s in sl], [s[1] for s in sl]
                out = np.zeros(2, dtype=hipabi.PWTEXT_RESULT)
                buf = np.zeros(cap + 16, dtype=np.uint8)
                ctx._chk(ctx.lib.wtz_pwtext_batch(ctx.h, p.ctypes.data, inp.ctypes.data, 2, cig.ctypes.data, cig.size, out.ctypes.data, buf.ctypes.data, C.c_uint64(cap)))
        assert lv.pool_info(ctx).main_used == 0

    for op in (3, 7, 15):
        bad = cig.copy()
        bad[sl[1][0] + 2] = (bad[sl[1][0] + 2] & ~np.uint32(15)) | np.uint32(op)
        refused(cig=bad)
    for side in ("q_len", "t_len"):      # the CIGAR walks one base past the view
        short = pr.copy()
        short[side][1] -= 1
        refused(pr=short)
    for s in ((-1, 1), (2, -1), (int(pr["q_len"][1]) + 1, 1), (2, int(pr["t_len"][1]) + 1)):
        refused(st=[st[0], s])
    refused(sl=[sl[0], (cig.size - 1, 2)])
    refused(sl=[sl[0], (cig.size + 1, 0)])
    total = sum(len(cases.want[k]) for k in (i, j))
    refused(cap=total - 1)
    long = pr.copy()
    long["q_len"][1] = 65536
    refused(pr=long)
    out, blob = ctx.pwtext_batch(pr, st, sl, cig)      # the context stays usable
    assert split(out, blob) == [cases.want[i], cases.want[j]]
    assert lv.pool_info(ctx).main_used == 0
