"""Loader of tests/golden/lane_vectors.npz (tests/golden/make_lane_vectors.py: whole wavefronts of K-sw1 / K-sw2 problems for the lane forms of wtz_sw_lane.h, recorded
from the reference's own kswx_extend_align_core and ksw_global2 at two cost pairs) and the checks the CPU and the GPU test share.
Block(b) has the interface of dpvec.Vectors for the cost pair b, plus each problem's place (wave, lane), its wave's class and composition, and live / high / rel_ok."""
import json
import os

import numpy as np

import dpvec

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("score", "tb", "te", "qb", "qe", "aln", "mat", "mis", "ins", "del")
CLASSES = (16, 32, 64, 104)
COMPOSITIONS = ("sorted", "ragged_rows", "ragged_cols", "partial", "clipped", "homo")
COSTS = ((-3, -3), (-2, -3))
LN_MAXCOLS, LN_MAXROWS, LN_MAXSPAN, LG_MAXROWS = 104, 511, 1500, 768      # wtz_sw_lane.h, wtz_tasks.h


class Block(dpvec.Vectors):
    def __init__(self, b):
        z = np.load(os.path.join(HERE, "golden", "lane_vectors.npz"))
        self.b = b
        self.kind, self.init, self.W, self.w_param = z["kind"], z["init"], z["W"], z["w_param"]
        self.qlen, self.tlen, self.view = z["qlen"], z["tlen"], z["view"]
        self.read_off, self.read_codes = z["read_off"], z["read_codes"]
        self.wave, self.lane, self.nc, self.comp = z["wave"], z["lane"], z["nc"], z["comp"]
        self.live, self.high = z["live"].astype(bool), z["high"].astype(bool)
        self.aln, self.cig_off, self.cig = z["aln%d" % b], z["cig_off%d" % b], z["cig%d" % b]
        self.rel_ok = z["rel_ok%d" % b].astype(bool)
        self.I, self.D = (int(x) for x in z["costs"][b])
        self.meta = json.loads(str(z["meta"]))
        self.n = self.kind.size

    def where(self, i):
        return "%s class %d composition %s wave %d lane %d, cost block %d (I, D) = (%d, %d)" % (
            "K-sw1" if self.kind[i] == 1 else "K-sw2", self.nc[i], self.comp[i], self.wave[i], self.lane[i], self.b, self.I, self.D)

    def of_kind(self, kind, w=None):
        """the problems of a kind in the file's order: wave after wave, lane after lane (w: K-sw1 problems of that -w only)"""
        return [int(i) for i in np.nonzero((self.kind == kind) & ((self.w_param == w) if w is not None else True))[0]]


def geometry(qlen, tlen, w, I, D, init=0, M=2, E=-1, T=-50):
    """wtz_ext_geometry (wtz_sw.h) for a band parameter w > 0: (W, rows, columns, band columns)"""
    max_gap = max(1, int((min(qlen, tlen) * M + init - T + max(I, D)) / -E) + 1)
    w = min(w, max_gap, max(qlen, tlen))
    if qlen < tlen:
        ql, tl = qlen, min(qlen + w, tlen)
    else:
        tl, ql = tlen, min(tlen + w, qlen)
    return w, ql, tl, min(tl, 2 * w + 1)


def shape(vec, i):
    """(rows, band columns) of live problem i as the lane forms see it; None outside their envelope"""
    q, t = int(vec.qlen[i]), int(vec.tlen[i])
    if q < 1 or t < 1:
        return None
    if vec.kind[i] == 1:
        g0, g1 = geometry(q, t, int(vec.w_param[i]), vec.I, vec.D), geometry(q, t, int(vec.w_param[i]), vec.I, vec.D, init=1 << 24)
        if g0[0] != g1[0] or g0[3] > LN_MAXCOLS or g0[1] > LN_MAXROWS or g0[1] + g0[2] > LN_MAXSPAN:
            return None
        return g0[1], g0[3]
    W = int(vec.W[i])
    n_col = min(q, 2 * W + 1)
    return None if abs(q - t) > W or n_col > LN_MAXCOLS or t > LG_MAXROWS else (t, n_col)


def problems(hipabi, vec, idx, lane_form):
    """wtz_dp_problem_t records; lane_form: W of a K-sw1 problem names its -w (form 65 reads it), else it is 0 as in dp_vectors.npz (band = params.w)"""
    p = np.zeros(len(idx), dtype=hipabi.DP_PROBLEM)
    for k, i in enumerate(idx):
        v = vec.view[i]
        W = vec.W[i] if vec.kind[i] == 2 else (vec.w_param[i] if lane_form else 0)
        p[k] = (2 * i, 2 * i + 1, v[0], v[3], v[1], v[4], v[2], v[5], vec.qlen[i], vec.tlen[i], vec.init[i], W)
    return p


def equals_record(vec, i, out, cigs, k, what):
    """problem i (element k of the call) was answered: the ten fields and every CIGAR word of the record"""
    exp, got = tuple(int(x) for x in vec.aln[i]), tuple(int(out[f][k]) for f in FIELDS)
    if vec.kind[i] == 2:       # ksw_global2 returns the score; the counts are the fold over the CIGAR
        exp, got = (exp[0],) + exp[5:], (got[0],) + got[5:]
    assert got == exp, "%s, %s: %s != %s" % (what, vec.where(i), got, exp)
    ec = vec.expected_cigar(i)
    assert cigs[k].size == ec.size and (cigs[k] == ec).all(), "%s, %s: CIGAR differs: %s != %s" % (what, vec.where(i), cigs[k].tolist(), ec.tolist())


def check_lane_form(vec, idx, out, cigs, what):
    """form 65 against the record: what is answered equals it; every live K-sw2 problem and every high K-sw1 problem is answered (they are inside the envelope, and at
    a high init_score the fold's rule cannot fire); a low problem whose reference answer is not translation invariant is declined; a filler is declined.
    Returns the set of answered problems."""
    answered = set()
    for k, i in enumerate(idx):
        used = int(out["form_used"][k])
        assert used in (0, 65), "%s, %s: form_used %d" % (what, vec.where(i), used)
        if used:
            assert vec.live[i], "%s, %s: a problem with an empty side was answered" % (what, vec.where(i))
            assert vec.kind[i] == 2 or vec.rel_ok[i], "%s, %s: answered, but the reference's answer at init %d is not its answer at init + 100000" % (what, vec.where(i), vec.init[i])
            equals_record(vec, i, out, cigs, k, what)
            answered.add(i)
        else:
            assert not (vec.live[i] and (vec.kind[i] == 2 or vec.high[i])), "%s, %s: declined a problem it must answer (init %d)" % (what, vec.where(i), vec.init[i])
    return answered
