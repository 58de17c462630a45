"""Shared pieces of the local Smith-Waterman tests (tests/test_local_cpu.py, tests/test_gpu_local.py) and of the generator of their vectors
(tests/golden/make_local_vectors.py): the reference's ksw_align2 through oracle/_ref/libref_shim.so, the vector file, and wtz_local_batch over a
list of sequences."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smartdenovo_amd import hipabi  # noqa: E402

SHIM = os.path.join(ROOT, "oracle", "_ref", "libref_shim.so")
VECTORS = os.path.join(ROOT, "tests", "golden", "local_vectors.npz")
KSW_XSTART = 0x80000      # ksw.h:9
FIELDS = ("score", "te", "qe", "tb", "qb")
# (o_del, e_del, o_ins, e_ins): 0 = wtcyc / pairaln default (kswx_align with I = D = -3, E = -1) and wtcns after its first iteration,
# 1 / 2 = unequal opening costs, 3 = wtcns' first iteration (O = -2)
GAPS = ((3, 1, 3, 1), (2, 1, 3, 1), (3, 1, 2, 1), (2, 1, 2, 1))


class KswR(C.Structure):      # kswr_t, ksw.h:14-19
    _fields_ = [(n, C.c_int) for n in ("score", "te", "qe", "score2", "te2", "tb", "qb")]


_shim = None


def have_shim():
    return os.path.exists(SHIM)


def ref_align(q, t, M, X, gaps):
    """ksw_align2(qlen, q, tlen, t, 4, mat, o_del, e_del, o_ins, e_ins, KSW_XSTART, NULL) on writable copies: (score, te, qe, tb, qb)"""
    global _shim
    if _shim is None:
        _shim = C.CDLL(SHIM)
        _shim.ksw_align2.restype = KswR
        _shim.ksw_align2.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    mat = np.full((4, 4), X, dtype=np.int8)
    np.fill_diagonal(mat, M)
    qq = np.array(q, dtype=np.uint8, copy=True)
    tt = np.array(t, dtype=np.uint8, copy=True)
    r = _shim.ksw_align2(qq.size, qq.ctypes.data, tt.size, tt.ctypes.data, 4, mat.ctypes.data, gaps[0], gaps[1], gaps[2], gaps[3], KSW_XSTART, None)
    return (r.score, r.te, r.qe, r.tb, r.qb)


def unpack_reads(words, offs, lens):
    """inverse of hipabi.pack_reads: list of uint8 code arrays"""
    shifts = (np.uint64(62) - np.arange(32, dtype=np.uint64) * np.uint64(2))
    flat = ((words[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.uint8).reshape(-1)
    return [flat[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]


def load_vectors():
    """dict: words / offs / lens (the packed reads), q_read / t_read / gap (index into GAPS) / expect (n x 5) / names, M, X"""
    z = np.load(VECTORS)
    return {k: z[k] for k in z.files}


def whole_read_problems(q_read, t_read, lens):
    pr = np.zeros(len(q_read), dtype=hipabi.DP_PROBLEM)
    pr["q_read"] = q_read
    pr["t_read"] = t_read
    pr["q_strand"] = 1
    pr["t_strand"] = 1
    pr["q_len"] = lens[np.asarray(q_read, dtype=np.int64)]
    pr["t_len"] = lens[np.asarray(t_read, dtype=np.int64)]
    return pr


def five(out):
    return np.stack([out[f] for f in FIELDS], axis=1).astype(np.int64)


def make_context(words, offs, lens, M, X, lib_path=None, pool_bytes=1 << 28):
    ctx = hipabi.Context(hipabi.Params.defaults(M=M, X=X), pool_bytes=pool_bytes, lib_path=lib_path)
    ctx.upload(np.ascontiguousarray(words, dtype=np.uint64), np.ascontiguousarray(offs, dtype=np.uint64), np.ascontiguousarray(lens, dtype=np.uint32))
    return ctx


def run_by_gap(ctx, problems, gap_idx):
    """wtz_local_batch once per gap-cost setting present (the costs are arguments of the call); results in problem order"""
    out = np.zeros(len(problems), dtype=hipabi.LOCAL_RESULT)
    for g in sorted(set(int(x) for x in gap_idx)):
        sel = np.nonzero(np.asarray(gap_idx) == g)[0]
        out[sel] = ctx.local_batch(problems[sel], *GAPS[g])
    return out


def pool_info(ctx):
    class PoolInfo(C.Structure):
        _fields_ = [(n, C.c_uint64) for n in ("main_cap", "main_used", "transient_cap", "transient_peak")]
    p = PoolInfo()
    ctx.lib.wtz_pool_info.argtypes = [C.c_void_p, C.POINTER(PoolInfo)]
    ctx._chk(ctx.lib.wtz_pool_info(ctx.h, C.byref(p)))
    return p
