#!/usr/bin/env python3
"""Whole WAVEFRONTS of problems for the lane forms of K-sw1 / K-sw2 (smartdenovo_amd/csrc/wtz_sw_lane.h), recorded from the REFERENCE's own routines.

Needs oracle/_ref/libref_shim.so (`make -C oracle ref`: kswx_extend_align_core kswx.h:234 as ref_extend_fixed, ksw_global2 ksw.c:503 as ref_global).
Output (committed): tests/golden/lane_vectors.npz.  Consumers: tests/test_lane_vectors_cpu.py (host emulation) and tests/test_gpu_lane_waves.py (form 65 of
wtz_test_dp: problems 64k .. 64k+63 of a call share wavefront k, in the caller's order).  `pair`, `Aln` and the scores are make_dp_vectors.py's.

The layout is dp_vectors.npz's (reads 2i / 2i+1 hold the query / target of problem i, `view`), plus per problem
    wave, lane      its place: problem i of a kind sits in lane `lane` of wavefront `wave` of that kind; every wave but the last of a kind has 64 entries
    nc, comp        the wave's instantiation (16 / 32 / 64 / 104 band columns) and its composition (below)
    live            0: a filler with an empty side - the lane forms decline it, so the lane is idle (how a wave in the middle of a call gets idle lanes)
    high            K-sw1: init_score >= 8 (qlen + tlen) + 64, where no absolute test of kswx_extend_align_core can fire (see `check_wave`); 0: init_score in 0 .. 60
and two cost blocks as in dpid_vectors.npz, block b at (I, D) = costs[b]: aln<b>, cig_off<b>, cig<b>, rel_ok<b>.
rel_ok<b> (K-sw1): ref_extend_fixed(init) and ref_extend_fixed(init + 100000) agree in qe, te, the counts and the CIGAR and their scores differ by exactly 100000,
i.e. the answer is translation invariant at this init_score; where it is not, the relative mode's answer is not the reference's and the fold's rule has to decline.

Compositions, one wave of each per class (partial: three):
    sorted        descending (n_col, rows): the product's case
    ragged_rows   rows 1 .. the class's largest, shuffled; the shortest problem in lane 0, the longest in lane 63
    ragged_cols   n_col over the whole range of the class, lanes with n_col <= 8 beside lanes with n_col == the class's largest, the block-skip and store-guard edges
    partial       1, 37 and 63 live lanes; the widest and longest problem is not in lane 0
    clipped       one side cut by the band, targets shorter than the band, rows beyond the band width / beyond 32 and 64 / targets beyond 116 (class 104)
    homo          homopolymer-rich pairs: ties in the last arg-max
K-sw1 at -w 50, plus one wave at -w 5 and one at -w 20 (comp w5 / w20).  K-sw2 with W from {50, 100, 200, 400} mixed inside a wave.

    python tests/golden/make_lane_vectors.py          (writes nothing if a condition on the file fails)"""
import ctypes as C
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_dp_vectors as dp  # noqa: E402

OUT = os.path.join(HERE, "lane_vectors.npz")
S = dp.SCORES
COSTS = ((-3, -3), (-2, -3))
CLASSES = (16, 32, 64, 104)
MAXCOLS, MAXROWS, MAXSPAN, LG_MAXROWS = 104, 511, 1500, 768       # WTZ_LN_MAXCOLS, WTZ_LN_MAXROWS, WTZ_LN_MAXSPAN, WTZ_LG_MAXROWS
SHIFT = 100000
GLOBAL_W = (50, 100, 200, 400)


def lane_class(n_col):
    return 16 if n_col <= 16 else 32 if n_col <= 32 else 64 if n_col <= 64 else 104


def ext_geometry(qlen, tlen, init, w, I, D):
    """wtz_ext_geometry (wtz_sw.h) for a band parameter w > 0: (W, ql, tl, n_col)"""
    mx = min(qlen, tlen) * S["M"] + init - S["T"]
    max_gap = max(1, int((mx + max(I, D)) / -S["E"]) + 1)
    w = min(w, max_gap, max(qlen, tlen))
    if qlen < tlen:
        ql, tl = qlen, min(qlen + w, tlen)
    else:
        tl, ql = tlen, min(tlen + w, qlen)
    return w, ql, tl, min(tl, 2 * w + 1)


def fixed_geo(qlen, tlen, w):
    """geometry of a K-sw1 problem as the planner sees it (init 0), None outside the lane envelope; it is the same at both cost pairs or the problem is not used"""
    gs = set()
    for I, D in COSTS:
        g0, g1 = ext_geometry(qlen, tlen, 0, w, I, D), ext_geometry(qlen, tlen, 1 << 24, w, I, D)
        if g0[0] != g1[0]:
            return None
        gs.add(g0)
    if len(gs) != 1:
        return None
    W, ql, tl, n_col = g0
    if qlen < 1 or tlen < 1 or n_col > MAXCOLS or ql > MAXROWS or ql + tl > MAXSPAN:
        return None
    return W, ql, tl, n_col


def global_geo(qlen, tlen, W):
    n_col = min(qlen, 2 * W + 1)
    if qlen < 1 or tlen < 1 or abs(qlen - tlen) > W or n_col > MAXCOLS or tlen > LG_MAXROWS:
        return None
    return W, tlen, qlen, n_col


K1_TL = {16: (1, 16), 32: (17, 32), 64: (33, 64), 104: (65, 110)}      # target lengths that give the class at -w 50 (n_col = tl up to 101)
K1_QMAX = {16: 66, 32: 82, 64: 114, 104: 511}                           # largest row count of the class: tl + 50, or the envelope
K1_NCMAX = {16: 16, 32: 32, 64: 64, 104: 101}
K2_QL = {16: (1, 16), 32: (17, 32), 64: (33, 64), 104: (65, 104)}
K2_TYP = {16: 30, 32: 40, 64: 70, 104: 100}                           # typical largest row count outside ragged_rows (the file stays small)


def draw_k1(rng, nc, rows=None, ncol=None, qcap=None, w=50, upto=False):
    """(qlen, tlen) of class nc (upto: or a narrower one) at band parameter w with, if asked, exactly `rows` rows / `ncol` band columns"""
    lo, hi = K1_TL[nc]
    if upto:
        lo = 1
    qcap = qcap or min(K1_QMAX[nc], hi + 10)
    for _ in range(10000):
        if ncol is not None and ncol < 2 * w + 1:
            tlen = ncol
        elif ncol is not None:
            tlen = int(rng.integers(ncol, max(ncol, (rows or 120) + w) + 1))
        elif rows is not None and nc == 104:
            tlen = int(rng.integers(max(lo, rows - w), max(lo, min(rows + w, MAXROWS + w)) + 1))
        else:
            tlen = int(rng.integers(lo, hi + 1))
        qlen = rows if rows is not None else int(rng.integers(1, min(qcap, tlen + w) + 1))
        g = fixed_geo(qlen, tlen, w)
        if g and (lane_class(g[3]) == nc or (upto and g[3] <= nc)) and (rows is None or g[1] == rows) and (ncol is None or g[3] == ncol):
            return qlen, tlen
    raise AssertionError("no K-sw1 problem of class %d with rows %s, n_col %s" % (nc, rows, ncol))


def draw_k2(rng, nc, rows=None, ncol=None, rcap=None, W=None):
    """(qlen, tlen, W) of class nc (n_col = min(qlen, 2W + 1)) with, if asked, `rows` target rows / `ncol` band columns"""
    lo, hi = K2_QL[nc]
    rcap = rcap or K2_TYP[nc]
    for _ in range(10000):
        w = W or int(rng.choice(GLOBAL_W))
        if ncol is not None and ncol < 101:
            qlen = ncol
        elif nc == 104 and w == 50 and (ncol == 101 or rng.random() < 0.5):
            qlen = int(rng.integers(101, max(102, (rows or rcap) + w)))          # the band slides: n_col = 2W + 1
        else:
            qlen = int(rng.integers(lo, hi + 1))
        tlen = rows if rows is not None else int(rng.integers(max(1, qlen - w), min(rcap, qlen + w) + 1)) if max(1, qlen - w) <= min(rcap, qlen + w) else 0
        g = global_geo(qlen, tlen, w)
        if g and lane_class(g[3]) == nc and (ncol is None or g[3] == ncol):
            return qlen, tlen, w
    raise AssertionError("no K-sw2 problem of class %d with rows %s, n_col %s" % (nc, rows, ncol))


def ragged(rng, rmax):
    """64 distinct row counts from 1 to rmax, ascending: cubically spaced (many short problems, a few long ones: the file stays small)"""
    rows = set(int(round(1 + (rmax - 1) * (k / 63.0) ** 3)) for k in range(64))
    while len(rows) < 64:
        rows.add(int(rng.integers(2, rmax)))
    return sorted(rows)


class Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.probs = []
        self.nwave = {1: 0, 2: 0}

    def seqs(self, qlen, tlen, style):
        rng = self.rng
        if style == "homo":
            return dp.pair(rng, qlen, tlen, err=0.15, homopolymers=True)
        if style == "far":
            return dp.pair(rng, qlen, tlen, related=False) if rng.random() < 0.5 else dp.pair(rng, qlen, tlen, err=0.4)
        return dp.pair(rng, qlen, tlen, err=float(rng.choice([0.05, 0.15, 0.3])))

    def wave(self, kind, nc, comp, dims, w_param=50, full=True, homo=False):
        """dims: per lane (qlen, tlen[, W]) or None (idle lane: a filler with an empty side).  K-sw1: every fourth live lane gets a low init_score."""
        rng = self.rng
        assert len(dims) == 64 or not full
        k = self.nwave[kind]
        self.nwave[kind] += 1
        nlive = 0
        for lane, d in enumerate(dims):
            p = dict(kind=kind, wave=k, lane=lane, nc=nc, comp=comp, w_param=w_param if kind == 1 else 50, W=0, init=0, live=1, high=0)
            if d is None:
                q, t = dp.pair(rng, 6, 6)
                if lane & 1:
                    q = q[:0]
                else:
                    t = t[:0]
                p.update(live=0, init=int(rng.integers(0, 300)) if kind == 1 else 0, W=50 if kind == 2 else 0)
            else:
                low = kind == 1 and nlive % 4 == 3
                nlive += 1
                q, t = self.seqs(d[0], d[1], "homo" if homo else ("far" if low and rng.random() < 0.6 else "near"))
                if kind == 1:
                    base = 8 * (d[0] + d[1]) + 64
                    p.update(init=int(rng.integers(0, 61)) if low else int(rng.integers(base, min(base + 3000, 1 << 20) + 1)), high=0 if low else 1)
                else:
                    p.update(W=d[2])
            p.update(q=q, t=t)
            self.probs.append(p)

    # ---- the compositions of one class ----
    def k1_class(self, nc):
        rng = self.rng
        geo = lambda d: fixed_geo(d[0], d[1], 50)
        ds = [draw_k1(rng, nc) for _ in range(64)]
        self.wave(1, nc, "sorted", sorted(ds, key=lambda d: (geo(d)[3], geo(d)[1]), reverse=True))
        rows = ragged(rng, K1_QMAX[nc])
        mid = rows[1:-1]
        rng.shuffle(mid)
        self.wave(1, nc, "ragged_rows", [draw_k1(rng, nc, rows=r, ncol=K1_NCMAX[nc] if r == rows[-1] else None, upto=True) for r in [rows[0]] + mid + [rows[-1]]])
        top = K1_NCMAX[nc]
        small = [c for c in (1, 2, 3, 5, 7, 8) if c < K1_TL[nc][0] or nc == 16]
        edges = [c for c in (8, 9, 16, 17, 32, 33, 64, 65, 96, 97) if c <= top]
        cols = []
        for k in range(32):        # pairs: a lane that needs one block of 8 columns or fewer beside a lane with the class's widest band
            cols += [small[k % len(small)], top]
        for k, c in enumerate(edges + [int(x) for x in np.linspace(K1_TL[nc][0], top, 12)]):
            cols[(2 * k + 1) % 64 if k % 3 else (2 * k) % 64] = c
        cols[63], cols[62] = top, small[0]
        self.wave(1, nc, "ragged_cols", [self.any_class_k1(c, nc) for c in cols])
        for nlive in (1, 37, 63):
            lanes = sorted(rng.choice(np.arange(1 if nlive == 1 else 0, 64), size=nlive, replace=False).tolist())
            ds = [draw_k1(rng, nc) for _ in range(nlive)]
            big = draw_k1(rng, nc, rows=min(K1_QMAX[nc], 150), ncol=top)
            ds[int(rng.integers(1, nlive)) if nlive > 1 else 0] = big
            if lanes[0] == 0 and ds[0] == big:
                ds[0], ds[-1] = ds[-1], ds[0]
            dims = [None] * 64
            for lane, d in zip(lanes, ds):
                dims[lane] = d
            self.wave(1, nc, "partial", dims)
        self.wave(1, nc, "clipped", self.k1_clipped(nc))
        self.wave(1, nc, "homo", [draw_k1(rng, nc) for _ in range(64)], homo=True)

    def any_class_k1(self, ncol, nc):
        """a problem with exactly ncol band columns (its own class may be narrower than the wave's)"""
        return draw_k1(self.rng, lane_class(ncol), ncol=ncol, qcap=min(K1_QMAX[nc], ncol + 40))

    def k1_clipped(self, nc):
        rng = self.rng
        lo, hi = K1_TL[nc]
        ds = []
        for k in range(64):
            m = k % 4
            if m == 0:                                      # qlen > tlen + W: the rows are cut
                tlen = int(rng.integers(lo, min(hi, 120) + 1))
                ds.append((tlen + min(50, tlen) + int(rng.integers(1, 40)), tlen) if tlen >= 50 else (tlen + 50 + int(rng.integers(1, 40)), tlen))
            elif m == 1 and nc == 104:                      # tlen > qlen + W: the columns are cut (n_col = tl needs the class's range: 104 only)
                qlen = int(rng.integers(15, 52)) if k % 8 == 1 else int(rng.integers(60, 110))
                ds.append((qlen, qlen + 50 + int(rng.integers(1, 60))))
            elif m == 1:                                    # the target shorter than the band: the je == tlen end candidate
                tlen = int(rng.integers(lo, hi + 1))
                ds.append((int(rng.integers(max(1, tlen - 10), tlen + 30)), tlen))
            elif m == 2 and nc == 104:                      # rows beyond the band width, beyond 64 rows, targets beyond 116: the shift, the refills
                ds.append((int(rng.integers(117, 160)), int(rng.integers(117, 160))))
            elif m == 2:
                tlen = int(rng.integers(lo, hi + 1))
                ds.append((int(rng.integers(tlen, tlen + 50)), tlen))
            else:                                           # rows past 32 (and 64 where the class reaches them)
                ds.append(draw_k1(rng, nc, rows=int(rng.integers(33, K1_QMAX[nc] if nc != 104 else 140))))
        for d in ds:
            g = fixed_geo(d[0], d[1], 50)
            assert g and lane_class(g[3]) == nc, (nc, d, g)
        return ds

    def k1_small_w(self, w):
        rng = self.rng
        ds = []
        for k in range(64):
            for _ in range(1000):
                qlen, tlen = int(rng.integers(1, 6 * w + 30)), int(rng.integers(1, 6 * w + 30))
                if fixed_geo(qlen, tlen, w):
                    break
            ds.append((qlen, tlen))
        nc = max(lane_class(fixed_geo(d[0], d[1], w)[3]) for d in ds)
        self.wave(1, nc, "w%d" % w, ds, w_param=w)

    def k2_class(self, nc, last=False):
        rng = self.rng
        ds = [draw_k2(rng, nc) for _ in range(64)]
        self.wave(2, nc, "sorted", sorted(ds, key=lambda d: (min(d[0], 2 * d[2] + 1), d[1]), reverse=True))
        rmax = LG_MAXROWS if nc == 104 else K2_QL[nc][1] + 200
        rows = ragged(rng, rmax)
        mid = rows[1:-1]
        rng.shuffle(mid)
        top = 101 if nc == 104 else nc
        order = [rows[0]] + mid + [rows[-1]]
        self.wave(2, nc, "ragged_rows", [draw_k2(rng, nc, rows=r, ncol=top if r == rows[-1] else None, W=(50 if nc == 104 else 200) if r == rows[-1] else None) for r in order])
        small = [c for c in (1, 2, 3, 5, 7, 8) if c < K2_QL[nc][0] or nc == 16]
        edges = [c for c in (8, 9, 16, 17, 32, 33, 64, 65, 96, 97) if c <= top]
        cols = []
        for k in range(32):
            cols += [small[k % len(small)], top]
        for k, c in enumerate(edges + [int(x) for x in np.linspace(K2_QL[nc][0], top, 12)]):
            cols[(2 * k + 1) % 64 if k % 3 else (2 * k) % 64] = c
        cols[63], cols[62] = top, small[0]
        self.wave(2, nc, "ragged_cols", [draw_k2(rng, lane_class(c), ncol=c) for c in cols])
        self.wave(2, nc, "clipped", self.k2_clipped(nc))
        self.wave(2, nc, "homo", [draw_k2(rng, nc) for _ in range(64)], homo=True)
        for nlive in (1, 63, 37):
            ds = [draw_k2(rng, nc) for _ in range(nlive)]
            big = draw_k2(rng, nc, rows=K2_TYP[nc] + 20, ncol=top, W=50 if nc == 104 else None)
            ds[int(rng.integers(1, nlive)) if nlive > 1 else 0] = big
            if last and nlive == 37:                        # the last wave of the kind is short: a wavefront with fewer problems than lanes
                self.wave(2, nc, "partial", ds, full=False)
                continue
            lanes = sorted(rng.choice(np.arange(1 if nlive == 1 else 0, 64), size=nlive, replace=False).tolist())
            if lanes[0] == 0 and ds[0] == big:
                ds[0], ds[-1] = ds[-1], ds[0]
            dims = [None] * 64
            for lane, d in zip(lanes, ds):
                dims[lane] = d
            self.wave(2, nc, "partial", dims)

    def k2_clipped(self, nc):
        rng = self.rng
        lo, hi = K2_QL[nc]
        ds = []
        for k in range(64):
            m = k % 4
            w = int(rng.choice(GLOBAL_W))
            qlen = int(rng.integers(lo, hi + 1))
            if m == 0:                                      # |qlen - tlen| == W: the band's edge ends in the corner
                ds.append((qlen, qlen + w, w) if qlen <= w or rng.random() < 0.5 else (qlen, qlen - w, w))
            elif m == 1:                                    # qlen <= W: every row starts at column 0
                ds.append((qlen, max(1, qlen + int(rng.integers(-min(w, qlen - 1), 30))), w) if qlen <= w else (qlen, qlen + int(rng.integers(-20, 20)), 50))
            elif m == 2 and nc == 104:                      # the band slides (n_col = 2W + 1), rows beyond 64 and queries beyond 116: the refills
                q = int(rng.integers(117, 200))
                ds.append((q, q + int(rng.integers(-50, 51)), 50))
            else:                                           # rows past W = 50: the S transition, beside lanes at wider W that never shift
                ds.append((qlen, int(rng.integers(max(1, qlen - 50), qlen + 51)), 50) if m == 2 else (qlen, max(1, qlen + int(rng.integers(40, 51))), w))
        for d in ds:
            g = global_geo(*d)
            assert g and lane_class(g[3]) == nc, (nc, d, g)
        return ds


def fold(q, t, cg):
    mat = mis = ins = dele = x1 = x2 = 0
    for c in cg:
        op, ln = int(c & 0xF), int(c >> 4)
        if op == 0:
            eq = int((q[x1:x1 + ln] == t[x2:x2 + ln]).sum()); mat += eq; mis += ln - eq; x1 += ln; x2 += ln
        elif op == 1:
            x1 += ln; ins += ln
        else:
            x2 += ln; dele += ln
    return mat, mis, ins, dele


def call(ref, p, I, D, init=None):
    """the reference's routine for problem p at the cost pair (I, D): (the ten fields, CIGAR words)"""
    q, t = p["q"], p["t"]
    cg = np.zeros(q.size + t.size + 8, dtype=np.uint32)
    if p["kind"] == 2:
        s = C.c_int()
        qq = np.ascontiguousarray(np.concatenate([q, [0]]).astype(np.uint8))
        tt = np.ascontiguousarray(np.concatenate([t, [0]]).astype(np.uint8))
        n = ref.ref_global(int(q.size), C.c_void_p(qq.ctypes.data), int(t.size), C.c_void_p(tt.ctypes.data), S["M"], S["X"],
                           -I, -S["E"], -D, -S["E"], int(p["W"]), C.byref(s), C.c_void_p(cg.ctypes.data))      # hzm_aln.h:1407
        cg = cg[:n].copy()
        mat, mis, ins, dele = fold(q, t, cg)
        return (s.value, 0, 0, 0, 0, mat + mis + ins + dele, mat, mis, ins, dele), cg
    a = dp.Aln()
    q, t = (x if x.size else np.zeros(1, np.uint8) for x in (q, t))
    n = ref.ref_extend_fixed(int(p["q"].size), C.c_void_p(q.ctypes.data), int(p["t"].size), C.c_void_p(t.ctypes.data), 1, int(p["init"] if init is None else init),
                             int(p["w_param"]), S["M"], S["X"], I, D, S["E"], S["T"], C.byref(a), C.c_void_p(cg.ctypes.data))
    return a.tup(), cg[:n].copy()


def record(ref, p, I, D):
    a, cg = call(ref, p, I, D)
    rel_ok = 1
    if p["kind"] == 1 and p["live"]:
        a2, cg2 = call(ref, p, I, D, init=p["init"] + SHIFT)
        rel_ok = int(a2[0] == a[0] + SHIFT and a2[1:] == a[1:] and np.array_equal(cg, cg2))
    return a, cg, rel_ok


def check_wave(probs):
    """the conditions a wave has to meet whatever the implementation: the envelope, and at least three quarters of the live lanes at a high init_score.
    High: init >= 8 (qlen + tlen) + 64.  A step costs at most 5 and one gap opening at most 3, so every row maximum is >= init - 5 (qlen + tlen) - 8 > 0: no row
    ends the loop, the end candidate is above 0 whenever it is taken, and the fold's rule cannot decline: a high problem inside the envelope MUST be answered."""
    live = [p for p in probs if p["live"]]
    assert live and len(probs) <= 64 and [p["lane"] for p in probs] == list(range(len(probs)))
    for p in probs:
        if not p["live"]:
            assert p["q"].size == 0 or p["t"].size == 0
            continue
        g = fixed_geo(p["q"].size, p["t"].size, p["w_param"]) if p["kind"] == 1 else global_geo(p["q"].size, p["t"].size, p["W"])
        assert g, "outside the envelope: %r" % ({k: p[k] for k in ("kind", "nc", "comp", "wave", "lane")},)
        p["rows"], p["n_col"] = g[1], g[3]
        if p["kind"] == 1:
            assert (p["init"] >= 8 * (p["q"].size + p["t"].size) + 64 and p["init"] <= 1 << 20) if p["high"] else 0 <= p["init"] <= 60
    assert max(p["n_col"] for p in live) <= probs[0]["nc"] and lane_class(max(p["n_col"] for p in live)) == probs[0]["nc"]
    if probs[0]["kind"] == 1:
        assert 4 * sum(p["high"] for p in live) >= 3 * len(live)
        low = [p["lane"] for p in live if not p["high"]]
        assert len(live) < 4 or (low and all(b - a > 1 for a, b in zip(low, low[1:]))), "the low lanes are interleaved with the high ones"
    comp = probs[0]["comp"]
    key = lambda p: (p["n_col"], p["rows"])
    if comp == "sorted":
        assert len(live) == 64 and [key(p) for p in live] == sorted((key(p) for p in live), reverse=True)
    if comp == "ragged_rows":
        r = [p["rows"] for p in probs]
        assert len(live) == 64 and r[0] == min(r) == 1 and r[63] == max(r) and r[63] > max(r[:63]) and r[1:63] != sorted(r[1:63])
    if comp == "ragged_cols":
        c = [p["n_col"] for p in probs]
        top = max(c)
        assert min(c) <= 8 and any(a <= 8 and b == top or b <= 8 and a == top for a, b in zip(c, c[1:]))
        assert all(e in c for e in (8, 9, 16, 17, 32, 33, 64, 65, 96, 97) if e <= top)
    if comp == "partial":
        assert len(live) in (1, 37, 63) and max(live, key=key)["lane"] != 0


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def generate(ref, seed):
    g = Gen(seed)
    for nc in CLASSES:
        g.k1_class(nc)
    g.k1_small_w(5)
    g.k1_small_w(20)
    for nc in (104, 64, 32, 16):
        g.k2_class(nc, last=(nc == 16))
    probs = g.probs
    for kind in (1, 2):
        for k in range(g.nwave[kind]):
            check_wave([p for p in probs if p["kind"] == kind and p["wave"] == k])
    res = [[record(ref, p, I, D) for p in probs] for I, D in COSTS]
    nbad = [sum(1 for p, r in zip(probs, res[b]) if p["kind"] == 1 and p["live"] and not p["high"] and not r[2]) for b in range(2)]
    for b in range(2):      # what the reasoning of check_wave says about the high problems, on the reference itself
        assert all(r[2] for p, r in zip(probs, res[b]) if p["kind"] == 1 and p["live"] and p["high"]), "a high problem is not translation invariant"
    return g, probs, res, nbad


def main():
    if not os.path.exists(dp.SHIM):
        sys.exit("build the reference shim first: make -C oracle ref")
    ref = C.CDLL(dp.SHIM)
    for seed in range(20261021, 20261021 + 20):      # redrawn until both blocks hold 8 low problems whose answer is not translation invariant
        g, probs, res, nbad = generate(ref, seed)
        print("seed %d: low problems with rel_ok false per block: %s" % (seed, nbad))
        if min(nbad) >= 8:
            break
    else:
        sys.exit("the conditions on the committed file are not met: nothing written")
    comps = {}
    for p in probs:
        comps.setdefault((p["kind"], p["nc"]), set()).add(p["comp"])
    for kind in (1, 2):
        for nc in CLASSES:
            assert {"sorted", "ragged_rows", "ragged_cols", "partial", "clipped", "homo"} <= comps[(kind, nc)], (kind, nc)
    assert {"w5", "w20"} <= set().union(*comps.values())
    # ---- views: reverse-complement views and both walking directions, short flanks (the file stays small) ----
    rng = np.random.default_rng(20261022)
    seqs, view = [], []
    for p in probs:
        row = []
        for side in ("q", "t"):
            L = p[side]
            rev, strand = int(rng.integers(0, 2)), int(rng.choice([1, -1]))
            fa, fb = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            seg = L if strand > 0 else L[::-1]
            v = np.concatenate([rng.integers(0, 4, size=fa, dtype=np.uint8), seg, rng.integers(0, 4, size=fb, dtype=np.uint8)]).astype(np.uint8)
            frm = fa if strand > 0 else fa + L.size - 1
            if L.size == 0:
                frm = min(fa, max(0, v.size - 1))
            if v.size == 0:
                v, frm = np.zeros(1, np.uint8), 0
            seqs.append(np.ascontiguousarray(v if not rev else (3 - v)[::-1], dtype=np.uint8))
            row += [rev, frm, strand]
        view.append(row)
    meta = dict(scores=S, costs=COSTS, shift=SHIFT, note="see make_lane_vectors.py; block b = the routines at (I, D) = costs[b]: aln<b>, cig<b>, cig_off<b>, rel_ok<b>")
    arrays = dict(
        kind=np.array([p["kind"] for p in probs], dtype=np.int32), wave=np.array([p["wave"] for p in probs], dtype=np.int32),
        lane=np.array([p["lane"] for p in probs], dtype=np.int32), nc=np.array([p["nc"] for p in probs], dtype=np.int32),
        comp=np.array([p["comp"] for p in probs]), live=np.array([p["live"] for p in probs], dtype=np.uint8), high=np.array([p["high"] for p in probs], dtype=np.uint8),
        init=np.array([p["init"] for p in probs], dtype=np.int32), W=np.array([p["W"] for p in probs], dtype=np.int32),
        w_param=np.array([p["w_param"] for p in probs], dtype=np.int32),
        qlen=np.array([p["q"].size for p in probs], dtype=np.int32), tlen=np.array([p["t"].size for p in probs], dtype=np.int32),
        view=np.array(view, dtype=np.int32), read_off=np.cumsum([0] + [s.size for s in seqs]).astype(np.int64), read_codes=np.concatenate(seqs).astype(np.uint8),
        costs=np.array(COSTS, dtype=np.int32), meta=np.array(json.dumps(meta)),
    )
    for b in range(2):
        arrays["aln%d" % b] = np.array([r[0] for r in res[b]], dtype=np.int32)
        arrays["cig_off%d" % b] = np.cumsum([0] + [r[1].size for r in res[b]]).astype(np.int64)
        arrays["cig%d" % b] = np.concatenate([r[1] for r in res[b]]).astype(np.uint32)
        arrays["rel_ok%d" % b] = np.array([r[2] for r in res[b]], dtype=np.uint8)
    write_npz(OUT, arrays)
    print("%d problems (K-sw1 %d in %d waves, K-sw2 %d in %d waves), %.1f KB" % (len(probs), sum(p["kind"] == 1 for p in probs), g.nwave[1],
                                                                              sum(p["kind"] == 2 for p in probs), g.nwave[2], os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
