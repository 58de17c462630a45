"""Shared pieces of the ksw_extend2 / kswx_align_no_stat tests (tests/test_kext_cpu.py, tests/test_gpu_kext.py, tests/test_gpu_kext_wide.py) and of the
generators of their vectors (tests/golden/make_kext_vectors.py, tests/golden/make_kext_wide_vectors.py).

Two functions of the reference are called live through oracle/_ref/libref_shim.so: ksw_extend2 (ksw.c:381-478) and, through localvec, ksw_align2
(ksw.c:344-366).  Both are exported from the reference's ksw.c as it is.

kswx_extend_core and kswx_align_no_stat (kswx.h:1386-1441, 1504-1511) are `static inline` and no recipe under oracle/ builds a program that prints
what they return.  ref_chain() below is therefore OUR restatement of those two routines' orchestration (which side is the rows, the cut to other + w,
the exchanged opening costs, the commit rule, the skipped ends), written from the lines cited; every DP value in it comes from the reference's own
compiled ksw_align2 / ksw_extend2.  The chain table of the vector file pins the orchestration to this restatement and every score to the reference.

py_extend() is a plain Python restatement of ksw_extend2 that also reports why the routine stopped, how many rows it entered and the cells of those
rows; the generator checks its six ints against the live routine on every problem it dumps and records the three extra numbers."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import localvec as lv
from smartdenovo_amd import hipabi

ROOT = lv.ROOT
SHIM = lv.SHIM
VECTORS = os.path.join(ROOT, "tests", "golden", "kext_vectors.npz")
WIDE_VECTORS = os.path.join(ROOT, "tests", "golden", "kext_wide_vectors.npz")      # tests/golden/make_kext_wide_vectors.py
FORMS = (1, 2, 4, 8, 16, 32)                                                        # slots per lane of the six kernel instantiations
FIELDS = ("score", "qle", "tle", "gtle", "gscore", "max_off")
CHAIN_FIELDS = ("found", "score", "tb", "te", "qb", "qe")
GAPS = ((3, 1, 3, 1), (2, 1, 3, 1), (3, 1, 2, 1), (4, 2, 4, 2))      # (o_del, e_del, o_ins, e_ins)
QLENS = (1, 2, 63, 64, 65, 255, 256, 257)
WS = (0, 1, 31, 32, 33, 127, 128, 800, 1023)
H0S = (-5, 0, 1, 30, 400, 5000, 32767)
END_BONUS = (0, 30, 100)
ZDROPS = (-1, 40)
STOP_END, STOP_M0, STOP_ZDROP = 0, 1, 2      # py_extend: ran out of rows / row maximum 0 (ksw.c:453) / z-drop (ksw.c:458-462)
# chain flags (one word per chain row)
F_LEFT_SKIP, F_RIGHT_SKIP, F_LEFT_ROLE1, F_RIGHT_ROLE1, F_LEFT_GSCORE, F_RIGHT_GSCORE, F_LEFT_RAN, F_RIGHT_RAN = (1 << k for k in range(8))

have_shim = lv.have_shim
_shim = None


def _mat(M, X):
    mat = np.full((4, 4), X, dtype=np.int8)
    np.fill_diagonal(mat, M)
    return mat


def ref_extend(q, t, M, X, gaps, w, end_bonus, zdrop, h0):
    """live ksw_extend2: (score, qle, tle, gtle, gscore, max_off)"""
    global _shim
    if _shim is None:
        _shim = C.CDLL(SHIM)
        _shim.ksw_extend2.restype = C.c_int
        _shim.ksw_extend2.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_int)] * 5
    mat = _mat(M, X)
    qq = np.array(q, dtype=np.uint8, copy=True)
    tt = np.array(t, dtype=np.uint8, copy=True)
    o = [C.c_int(0) for _ in range(5)]
    sc = _shim.ksw_extend2(qq.size, qq.ctypes.data, tt.size, tt.ctypes.data, 4, mat.ctypes.data, gaps[0], gaps[1], gaps[2], gaps[3], w, end_bonus, zdrop, h0,
                           *[C.byref(x) for x in o])
    return (sc,) + tuple(x.value for x in o)


def py_extend(q, t, M, X, gaps, w, end_bonus, zdrop, h0, trim=True):
    """ksw_extend2 restated: ((score, qle, tle, gtle, gscore, max_off), stop, rows, cells).  trim=False leaves the band at its fixed width."""
    o_del, e_del, o_ins, e_ins = gaps
    oe_del, oe_ins = o_del + e_del, o_ins + e_ins
    qlen, tlen = len(q), len(t)
    q = [int(x) for x in q]
    t = [int(x) for x in t]
    h0 = max(h0, 0)
    eh_h = [0] * (qlen + 1)
    eh_e = [0] * (qlen + 1)
    eh_h[0] = h0
    eh_h[1] = h0 - oe_ins if h0 > oe_ins else 0
    j = 2
    while j <= qlen and eh_h[j - 1] > e_ins:
        eh_h[j] = eh_h[j - 1] - e_ins
        j += 1
    mxs = max(M, X)
    w = min(w, max(1, int((qlen * mxs + end_bonus - o_ins) / e_ins + 1.)))
    w = min(w, max(1, int((qlen * mxs + end_bonus - o_del) / e_del + 1.)))
    mx, max_i, max_j, max_ie, gscore, max_off = h0, -1, -1, -1, -1, 0
    beg, end = 0, qlen
    stop, rows, cells = STOP_END, 0, 0
    for i in range(tlen):
        f, m, mj = 0, 0, -1
        h1 = max(0, h0 - (o_del + e_del * (i + 1)))
        beg = max(beg, i - w)
        end = min(end, i + w + 1, qlen)
        rows += 1
        cells += max(0, end - beg)
        ti = t[i]
        j = beg
        while j < end:
            Mv, e = eh_h[j], eh_e[j]
            eh_h[j] = h1
            Mv += M if q[j] == ti else X
            h = max(Mv, e, f)
            h1 = h
            if not m > h:
                mj = j
            m = max(m, h)
            eh_e[j] = max(e - e_del, max(Mv - oe_del, 0))
            f = max(f - e_ins, max(Mv - oe_ins, 0))
            j += 1
        eh_h[end] = h1
        eh_e[end] = 0
        if j == qlen:
            if not gscore > h1:
                max_ie = i
            gscore = max(gscore, h1)
        if m == 0:
            stop = STOP_M0
            break
        if m > mx:
            mx, max_i, max_j = m, i, mj
            max_off = max(max_off, abs(mj - i))
        elif zdrop > 0:
            if i - max_i > mj - max_j:
                if mx - m - ((i - max_i) - (mj - max_j)) * e_del > zdrop:
                    stop = STOP_ZDROP
                    break
            elif mx - m - ((mj - max_j) - (i - max_i)) * e_ins > zdrop:
                stop = STOP_ZDROP
                break
        if trim:
            j = mj
            while j >= beg and eh_h[j]:
                j -= 1
            beg = j + 1
            j = mj + 2
            while j <= end and eh_h[j]:
                j += 1
            end = j
    return (mx, max_j + 1, max_i + 1, max_ie + 1, gscore, max_off), stop, rows, cells


def clamped_w(qlen, M, X, gaps, w, end_bonus):
    """the band half-width after the clamp of ksw.c:403-408"""
    mxs = max(M, X)
    w = min(w, max(1, int((qlen * mxs + end_bonus - gaps[2]) / gaps[3] + 1.)))
    return min(w, max(1, int((qlen * mxs + end_bonus - gaps[0]) / gaps[1] + 1.)))


def slots_of(qlen, tlen, M, X, gaps, w, end_bonus):
    """live diagonals of a problem as the host plans them (kext_plan / kext_slots of wtz_lib_batch.h): min(w, tlen - 1) + min(w, qlen - 1) + 1 of the clamped w"""
    w = clamped_w(qlen, M, X, gaps, w, end_bonus)
    return min(w, tlen - 1) + min(w, qlen - 1) + 1


def form_of(slots):
    """wtz_kext_form: slots per lane of the instantiation that takes a band of `slots` diagonals"""
    c = 1
    while c < 32 and 64 * c < slots:
        c <<= 1
    return c


def ref_chain(q, t, M, X, w, I, D, E, T, extend=ref_extend, align=lv.ref_align, record=None):
    """kswx_align_no_stat (kswx.h:1504-1511) restated around the live ksw_align2 / ksw_extend2: ((found, score, tb, te, qb, qe), flags, local five).
    record: a list that receives (side, role, arguments handed to `extend`) of every extension stage that ran (side 0 = left, role 1 = query is the rows)"""
    if record is not None:
        inner, stage = extend, [0, 0]

        def extend(*a):
            record.append((stage[0], stage[1], a))
            return inner(*a)
    q = np.asarray(q, dtype=np.uint8)
    t = np.asarray(t, dtype=np.uint8)
    qlen, tlen = q.size, t.size
    score, te, qe, tb, qb = align(q, t, M, X, (-D, -E, -I, -E))
    if qb <= -1 or tb <= -1 or qe <= -1 or te <= -1:
        return (0, 0, 0, 0, 0, 0), 0, (0, 0, 0, 0, 0)
    qe += 1
    te += 1
    local = (score, tb, te, qb, qe)
    flags = 0
    if T < 0:
        g_t, g_q = (-D, -E, -I, -E), (-I, -E, -D, -E)      # the problem's target as rows / the problem's query as rows
        if qb == 0 or tb == 0:
            flags |= F_LEFT_SKIP
        elif tb >= qb:                                                        # kswx.h:1392-1402
            flags |= F_LEFT_RAN
            if record is not None:
                stage[:] = [0, 0]
            y1, y2 = (tb if qb + w > tb else qb + w), qb
            sc, x2, x1, x3, gs, _ = extend(q[qb - y2:qb][::-1], t[tb - y1:tb][::-1], M, X, g_t, w, -T, -1, score)
            if gs <= 0 or gs <= sc + T:
                tb, qb, score = tb - x1, qb - x2, sc
            else:
                tb, qb, score = tb - x3, 0, gs
                flags |= F_LEFT_GSCORE
        else:                                                                 # kswx.h:1403-1413
            flags |= F_LEFT_RAN | F_LEFT_ROLE1
            if record is not None:
                stage[:] = [0, 1]
            y1, y2 = tb, (qb if tb + w > qb else tb + w)
            sc, x1, x2, x3, gs, _ = extend(t[tb - y1:tb][::-1], q[qb - y2:qb][::-1], M, X, g_q, w, -T, -1, score)
            if gs <= 0 or gs <= sc + T:
                tb, qb, score = tb - x1, qb - x2, sc
            else:
                qb, tb, score = qb - x3, 0, gs
                flags |= F_LEFT_GSCORE
        if qe == qlen or te == tlen:
            flags |= F_RIGHT_SKIP
        elif tlen - te >= qlen - qe:                                          # kswx.h:1419-1427
            flags |= F_RIGHT_RAN
            if record is not None:
                stage[:] = [1, 0]
            y1, y2 = ((tlen - te) if qlen - qe + w > tlen - te else qlen - qe + w), qlen - qe
            sc, x2, x1, x3, gs, _ = extend(q[qe:qe + y2], t[te:te + y1], M, X, g_t, w, -T, -1, score)
            if gs <= 0 or gs <= sc + T:
                te, qe, score = te + x1, qe + x2, sc
            else:
                te, qe, score = te + x3, qlen, gs
                flags |= F_RIGHT_GSCORE
        else:                                                                 # kswx.h:1428-1436
            flags |= F_RIGHT_RAN | F_RIGHT_ROLE1
            if record is not None:
                stage[:] = [1, 1]
            y1, y2 = tlen - te, ((qlen - qe) if tlen - te + w > qlen - qe else tlen - te + w)
            sc, x1, x2, x3, gs, _ = extend(t[te:te + y1], q[qe:qe + y2], M, X, g_q, w, -T, -1, score)
            if gs <= 0 or gs <= sc + T:
                te, qe, score = te + x1, qe + x2, sc
            else:
                te, qe, score = tlen, qe + x3, gs
                flags |= F_RIGHT_GSCORE
    return (1, score, tb, te, qb, qe), flags, local


def load_vectors(path=None):
    z = np.load(path or VECTORS)
    return {k: z[k] for k in z.files}


def problems_of(v):
    """the function-level problems of the vector file as wtz_dp_problem_t"""
    pr = np.zeros(len(v["f_q_read"]), dtype=hipabi.DP_PROBLEM)
    for f in ("q_read", "t_read", "q_from", "t_from", "q_strand", "t_strand", "q_len", "t_len", "init_score", "W"):
        pr[f] = v["f_" + f]
    for f in ("q_rev", "t_rev"):      # kext_vectors.npz has neither: whole reads as uploaded
        if "f_" + f in v:
            pr[f] = v["f_" + f]
    return pr


def chain_problems(q_read, t_read, t_rev, lens):
    pr = lv.whole_read_problems(q_read, t_read, lens)
    pr["t_rev"] = t_rev
    return pr


def six(out):
    return np.stack([out[f] for f in FIELDS], axis=1).astype(np.int64)


def chain_six(out):
    return np.stack([out[f] for f in CHAIN_FIELDS], axis=1).astype(np.int64)


def run_by_group(ctx, problems, gap, end_bonus, zdrop):
    """wtz_kext_batch once per (gap costs, end bonus, zdrop) present: they are arguments of the call; results in problem order"""
    out = np.zeros(len(problems), dtype=hipabi.KEXT_RESULT)
    key = np.stack([np.asarray(gap), np.asarray(end_bonus), np.asarray(zdrop)], axis=1).astype(np.int64)
    for g, eb, zd in sorted(set(map(tuple, key.tolist()))):
        sel = np.nonzero((key == (g, eb, zd)).all(axis=1))[0]
        out[sel] = ctx.kext_batch(problems[sel], *GAPS[g], eb, zd)
    return out


def run_chain_by_group(ctx, problems, w, T, I=-3, D=-3, E=-1):
    out = np.zeros(len(problems), dtype=hipabi.ALIGN_RESULT)
    key = np.stack([np.asarray(w), np.asarray(T)], axis=1).astype(np.int64)
    for ww, tt in sorted(set(map(tuple, key.tolist()))):
        sel = np.nonzero((key == (ww, tt)).all(axis=1))[0]
        out[sel] = ctx.align_batch(problems[sel], ww, I, D, E, tt)
    return out
