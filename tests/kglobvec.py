"""Shared pieces of the ksw_global2 / kswx_align tests (tests/test_kglob_cpu.py, tests/test_gpu_kglob.py) and of the generator of their vectors
(tests/golden/make_kglob_vectors.py).

ksw_global2 (ksw.c:503-586) is called live through oracle/_ref/libref_shim.so (ref_global of oracle/ref_shim.c hands it a 4x4 matrix of M / X).
kswx_gen_cigar_core2 and kswx_align (kswx.h:1443-1502) are `static inline` and no recipe under oracle/ builds a program that prints what they return:
ref_chainx() below is OUR restatement of the band rule (kswx.h:1452-1461) and of the fold (kswx.h:1468-1477) around kextvec.ref_chain, which restates
kswx_align_no_stat; every DP value in it comes from the reference's own compiled ksw_align2, ksw_extend2 and ksw_global2."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import kextvec as kv
import localvec as lv
from smartdenovo_amd import hipabi

ROOT = lv.ROOT
SHIM = lv.SHIM
VECTORS = os.path.join(ROOT, "tests", "golden", "kglob_vectors.npz")
FORMS = (1, 2, 4, 8, 16, 32)
FIELDS = ("score", "aln", "mat", "mis", "ins", "del")
CHAIN_FIELDS = ("found", "score", "tb", "te", "qb", "qe", "aln", "mat", "mis", "ins", "del", "band")
# (o_del, e_del, o_ins, e_ins): kswx_align's default, unequal opening costs, unequal extension costs, an opening cost of 0
GAPS = ((3, 1, 3, 1), (2, 1, 4, 1), (3, 1, 3, 2), (0, 1, 0, 1))
B_NONE, B_DIFF, B_W2, B_LIFT, B_EXACT = 0, 1, 2, 3, 4      # which line of kswx.h:1452-1461 decided the band

have_shim = lv.have_shim
_shim = None


def ref_global(q, t, M, X, gaps, w):
    """live ksw_global2: (score, CIGAR words, first operation first)"""
    global _shim
    if _shim is None:
        _shim = C.CDLL(SHIM)
        _shim.ref_global.restype = C.c_int
        _shim.ref_global.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_int), C.c_void_p]
    qq = np.array(q, dtype=np.uint8, copy=True)
    tt = np.array(t, dtype=np.uint8, copy=True)
    cg = np.zeros(qq.size + tt.size + 2, dtype=np.uint32)
    sc = C.c_int(0)
    n = _shim.ref_global(qq.size, qq.ctypes.data, tt.size, tt.ctypes.data, M, X, gaps[0], gaps[1], gaps[2], gaps[3], w, C.byref(sc), cg.ctypes.data)
    return sc.value, cg[:n].copy()


def fold(q, t, cigar):
    """kswx.h:1468-1477: (aln, mat, mis, ins, del); op 1 (query only) counts as del, op 2 (target only) as ins"""
    q = np.asarray(q)
    t = np.asarray(t)
    aln = mat = mis = ins = dele = x1 = x2 = 0
    for wd in cigar:
        op, ln = int(wd) & 0xF, int(wd) >> 4
        aln += ln
        if op == 0:
            eq = int((q[x1:x1 + ln] == t[x2:x2 + ln]).sum())
            mat += eq
            mis += ln - eq
            x1 += ln
            x2 += ln
        elif op == 1:
            x1 += ln
            dele += ln
        else:
            x2 += ln
            ins += ln
    return aln, mat, mis, ins, dele


def cells_of(qlen, tlen, w):
    i = np.arange(tlen, dtype=np.int64)
    return int((np.minimum(i + w + 1, qlen) - np.maximum(i - w, 0)).clip(min=0).sum())


def slots_of(qlen, tlen, w):
    return min(w, tlen - 1) + min(w, qlen - 1) + 1


def form_of(slots, emul=False, qlen=0, w=0):
    """the form wtz_global_batch runs a band of `slots` diagonals in; beyond K-glob the device takes the ring form (33) inside its envelope of 8 190 band
    columns and 1 024 query words, the scalar body (255) outside it, and the emulation always the scalar body"""
    if slots <= hipabi.GLOB_MAXSLOTS:
        return kv.form_of(slots)
    ring = min(qlen, 2 * w + 1) + 2 <= 8192 and (qlen + 63) // 32 + 1 <= 1024
    return 33 if ring and not emul else 255


def forms_of(v, idx, emul=False):
    """form_of for the function-level rows idx of the vector file"""
    return [form_of(int(v["f_slots"][i]), emul, int(v["f_q_len"][i]), int(v["f_W"][i])) for i in idx]


def _cdiv(a, b):
    """C's integer division: truncated towards zero"""
    s = -1 if (a < 0) != (b < 0) else 1
    return s * (abs(a) // abs(b))


def band_rule(w, tb, te, qb, qe, score, M, E):
    """kswx.h:1452-1461: (band, branch)"""
    if w < 0:
        return -w, B_EXACT
    x1 = abs((te - tb) - (qe - qb))
    br = B_NONE
    if w < x1 * 1.5:
        w = int(x1 * 1.5)
        br = B_DIFF
    w2 = _cdiv(min(te - tb, qe - qb) * M - score, -E) + 1
    lifted = False
    if w2 < _cdiv(w, 4) + 1:
        w2 = _cdiv(w, 4) + 1
        lifted = True
    if w > w2:
        w = w2
        br = B_LIFT if lifted else B_W2
    return w, br


def ref_chainx(q, t, M, X, w, I, D, E, T):
    """kswx_align_with_cigar (kswx.h:1513-1520) restated: (the twelve CHAIN_FIELDS, CIGAR words, branch)"""
    q = np.asarray(q, dtype=np.uint8)
    t = np.asarray(t, dtype=np.uint8)
    (found, score, tb, te, qb, qe), _, _ = kv.ref_chain(q, t, M, X, max(w, 0), I, D, E, T)
    if not found:
        return (0,) * 12, np.zeros(0, dtype=np.uint32), B_NONE
    band, br = band_rule(w, tb, te, qb, qe, score, M, E)
    assert band >= abs((te - tb) - (qe - qb))
    sc, cg = ref_global(q[qb:qe], t[tb:te], M, X, (-D, -E, -I, -E), band)
    return (1, sc, tb, te, qb, qe) + fold(q[qb:qe], t[tb:te], cg) + (band,), cg, br


def view(reads, read, rev, frm, strand, n):
    """the n bases of a wtz_dp_problem_t side"""
    r = np.asarray(reads[read], dtype=np.uint8)
    if rev:
        r = (3 - r[::-1]).astype(np.uint8)
    return r[frm:frm + n] if strand > 0 else r[frm - n + 1:frm + 1][::-1]


def encode_cigars(cigs):
    """run lists as one uint16 stream (len << 2 | op, a run of 16 383 or more in pieces of the same op) + offsets"""
    out, offs = [], [0]
    for cg in cigs:
        for wd in cg:
            op, ln = int(wd) & 0xF, int(wd) >> 4
            while ln > 0x3FFE:
                out.append(0x3FFE << 2 | op)
                ln -= 0x3FFE
            out.append(ln << 2 | op)
        offs.append(len(out))
    return np.array(out, dtype=np.uint16), np.array(offs, dtype=np.uint32)


def decode_cigar(stream, offs, i):
    out = []
    for v in stream[int(offs[i]):int(offs[i + 1])]:
        op, ln = int(v) & 3, int(v) >> 2
        if out and (out[-1] & 0xF) == op:
            out[-1] += ln << 4
        else:
            out.append(ln << 4 | op)
    return np.array(out, dtype=np.uint32)


def load_vectors(path=None):
    z = np.load(path or VECTORS)
    return {k: z[k] for k in z.files}


def problems_of(v, prefix="f_"):
    pr = np.zeros(len(v[prefix + "q_read"]), dtype=hipabi.DP_PROBLEM)
    for f in ("q_read", "t_read", "q_rev", "t_rev", "q_from", "t_from", "q_strand", "t_strand", "q_len", "t_len", "W"):
        if prefix + f in v:
            pr[f] = v[prefix + f]
    return pr


def chain_problems(v):
    pr = lv.whole_read_problems(v["c_q_read"], v["c_t_read"], v["lens"])
    pr["q_rev"] = v["c_q_rev"]
    pr["t_rev"] = v["c_t_rev"]
    return pr


def six(out):
    return np.stack([out[f] for f in FIELDS], axis=1).astype(np.int64)


def twelve(out):
    return np.stack([out[f] for f in CHAIN_FIELDS], axis=1).astype(np.int64)


def run_by_gap(ctx, problems, gap_idx, cigar=True):
    """wtz_global_batch once per gap-cost setting present; (results, CIGARs) in problem order"""
    out = np.zeros(len(problems), dtype=hipabi.GLOBAL_RESULT)
    cigs = [None] * len(problems)
    for g in sorted(set(int(x) for x in gap_idx)):
        sel = np.nonzero(np.asarray(gap_idx) == g)[0]
        if cigar:
            o, cg = ctx.global_batch(problems[sel], *GAPS[g])
            for k, i in enumerate(sel):
                cigs[int(i)] = cg[k]
        else:
            o = ctx.global_batch(problems[sel], *GAPS[g], cigar=False)
        o = o.copy()
        o["cigar_off"] = 0      # depends on the call's composition
        out[sel] = o
    return out, cigs


def run_chain_by_group(ctx, problems, w, T, I=-3, D=-3, E=-1):
    out = np.zeros(len(problems), dtype=hipabi.ALIGNX_RESULT)
    cigs = [None] * len(problems)
    key = np.stack([np.asarray(w), np.asarray(T)], axis=1).astype(np.int64)
    for ww, tt in sorted(set(map(tuple, key.tolist()))):
        sel = np.nonzero((key == (ww, tt)).all(axis=1))[0]
        o, cg = ctx.alignx_batch(problems[sel], ww, I, D, E, tt)
        o = o.copy()
        o["cigar_off"] = 0
        out[sel] = o
        for k, i in enumerate(sel):
            cigs[int(i)] = cg[k]
    return out, cigs
