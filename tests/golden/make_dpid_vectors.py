#!/usr/bin/env python3
"""Function-level vectors of the three banded DPs with SEPARATE gap-open costs, dumped from the REFERENCE's own routines.

The problems are those of make_dp_vectors.py - its committed output dp_vectors.npz is read back: same class labels, same sequences, same views; its generator
functions (`pair`, `ext_geometry`) and its `Aln` are imported - recorded through oracle/_ref/libref_shim.so (`make -C oracle ref`) at
    block 0: I = -2, D = -3 (wtmsa.c:633-634)          block 1: I = -3, D = -2
instead of I = D = O.  kswx_extend_align_shift_core and kswx_extend_align_core take (I, D) as they stand (kswx.h:101, 234); ksw_global2 is called as
global_align_regs_hzmo calls it, hzm_aln.h:1407: (o_del, e_del, o_ins, e_ins) = (-I, -E, -D, -E).
Per block and problem `differs`: the result (the ten fields or the CIGAR) differs from the same routine at (I, I), at (D, D) AND at (D, I) - a device that
had one cost, the other one, or the two the wrong way round misses it.
A class of tests/test_gpu_dp_forms.py::SHIFT_MUST (the classes the K-sw3 register forms must answer) without such a problem in one of the blocks has the
sequences of its problems redrawn (same lengths, init and band; `pair` on a generator of its own; views reset to the plain forward one) until it has one.
The file is written only if, per kind and block, at least a third of the problems have `differs` set and every SHIFT_MUST class has one.

    python tests/golden/make_dpid_vectors.py"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_dp_vectors as dp  # noqa: E402
from dpvec import Vectors  # noqa: E402
from test_gpu_dp_forms import SHIFT_MUST  # noqa: E402

OUT = os.path.join(HERE, "dpid_vectors.npz")
COSTS = ((-2, -3), (-3, -2))
S = dp.SCORES


def call(ref, kind, q, t, init, W, w_param, I, D):
    """the reference's routine of `kind` at the cost pair (I, D): (the ten fields, CIGAR words)"""
    cg = np.zeros(q.size + t.size + 8, dtype=np.uint32)
    if kind == 2:
        s = C.c_int()
        qq = np.ascontiguousarray(np.concatenate([q, [0]]).astype(np.uint8))
        tt = np.ascontiguousarray(np.concatenate([t, [0]]).astype(np.uint8))
        n = ref.ref_global(int(q.size), C.c_void_p(qq.ctypes.data), int(t.size), C.c_void_p(tt.ctypes.data), S["M"], S["X"],
                           -I, -S["E"], -D, -S["E"], int(W), C.byref(s), C.c_void_p(cg.ctypes.data))      # hzm_aln.h:1407
        cg = cg[:n].copy()
        mat = mis = ins = dele = x1 = x2 = 0
        for c in cg:                                    # the fold of make_dp_vectors.call_global
            op, ln = int(c & 0xF), int(c >> 4)
            if op == 0:
                eq = int((q[x1:x1 + ln] == t[x2:x2 + ln]).sum()); mat += eq; mis += ln - eq; x1 += ln; x2 += ln
            elif op == 1:
                x1 += ln; ins += ln
            else:
                x2 += ln; dele += ln
        return (s.value, 0, 0, 0, 0, mat + mis + ins + dele, mat, mis, ins, dele), cg
    a = dp.Aln()
    fn = ref.ref_extend_shift if kind == 0 else ref.ref_extend_fixed
    n = fn(int(q.size), C.c_void_p(q.ctypes.data), int(t.size), C.c_void_p(t.ctypes.data), 1, int(init), int(W if kind == 0 else w_param),
           S["M"], S["X"], I, D, S["E"], S["T"], C.byref(a), C.c_void_p(cg.ctypes.data))
    return a.tup(), cg[:n].copy()


def record(ref, p, I, D):
    """(fields, CIGAR, differs) of problem p at (I, D)"""
    a, cg = call(ref, p["kind"], p["q"], p["t"], p["init"], p["W"], p["w_param"], I, D)
    differs = True
    for I2, D2 in ((I, I), (D, D), (D, I)):
        a2, cg2 = call(ref, p["kind"], p["q"], p["t"], p["init"], p["W"], p["w_param"], I2, D2)
        if a2 == a and np.array_equal(cg2, cg):
            differs = False
    return a, cg, differs


def main():
    if not os.path.exists(dp.SHIM):
        sys.exit("build the reference shim first: make -C oracle ref")
    ref = C.CDLL(dp.SHIM)
    vec = Vectors()
    assert vec.meta["scores"] == S
    probs = [dict(kind=int(vec.kind[i]), cls=str(vec.cls[i]), q=vec.logical(i, "q"), t=vec.logical(i, "t"), init=int(vec.init[i]), W=int(vec.W[i]), w_param=int(vec.w_param[i]),
                  view=[int(x) for x in vec.view[i]], reads=(vec.read(2 * i), vec.read(2 * i + 1)), redrawn=0) for i in range(vec.n)]
    res = [[record(ref, p, I, D) for p in probs] for I, D in COSTS]
    # ---- a class the register forms must answer needs a problem that tells the two costs apart, in both blocks ----
    must = sorted(set().union(*SHIFT_MUST.values()))
    rng = np.random.default_rng(20261101)
    for cls in must:
        idx = [i for i, p in enumerate(probs) if p["cls"] == cls]
        assert idx, cls
        tries = 0
        while not all(any(res[b][i][2] for i in idx) for b in range(2)):
            tries += 1
            assert tries <= 50, "class %s: no redraw differs" % cls
            for i in idx:
                p = probs[i]
                if p["q"].size == 0 or p["t"].size == 0:
                    continue
                q, t = dp.pair(rng, p["q"].size, p["t"].size, err=0.15, homopolymers=(cls == "s_homo"))
                if cls.startswith("s_c"):      # the band class is a property of the lengths and W: unchanged
                    assert dp.ext_geometry(q.size, t.size, p["W"]) == dp.ext_geometry(p["q"].size, p["t"].size, p["W"])
                p.update(q=q, t=t, view=[0, 0, 1, 0, 0, 1], reads=(q, t), redrawn=1)
                for b, (I, D) in enumerate(COSTS):
                    res[b][i] = record(ref, p, I, D)
        if tries:
            print("class %s: sequences redrawn %d time(s)" % (cls, tries))
    # ---- the conditions on the committed file ----
    for b, (I, D) in enumerate(COSTS):
        for kind in (0, 1, 2):
            idx = [i for i, p in enumerate(probs) if p["kind"] == kind]
            nd = sum(res[b][i][2] for i in idx)
            print("(I, D) = (%d, %d) kind %d: %d of %d problems differ from (I, I), (D, D) and (D, I)" % (I, D, kind, nd, len(idx)))
            assert nd * 3 >= len(idx), "the conditions on the committed file are not met: nothing written"
        for cls in must:
            assert any(res[b][i][2] for i, p in enumerate(probs) if p["cls"] == cls), cls
    seqs = [r for p in probs for r in p["reads"]]
    arrays = dict(
        kind=np.array([p["kind"] for p in probs], dtype=np.int32), cls=np.array([p["cls"] for p in probs]),
        init=np.array([p["init"] for p in probs], dtype=np.int32), W=np.array([p["W"] for p in probs], dtype=np.int32),
        w_param=np.array([p["w_param"] for p in probs], dtype=np.int32),
        qlen=np.array([p["q"].size for p in probs], dtype=np.int32), tlen=np.array([p["t"].size for p in probs], dtype=np.int32),
        view=np.array([p["view"] for p in probs], dtype=np.int32), redrawn=np.array([p["redrawn"] for p in probs], dtype=np.uint8),
        read_off=np.cumsum([0] + [s.size for s in seqs]).astype(np.int64), read_codes=np.concatenate(seqs).astype(np.uint8),
        costs=np.array(COSTS, dtype=np.int32),
        meta=np.array(json.dumps(dict(scores=S, costs=COSTS, note="as dp_vectors.npz; block b = the routines at (I, D) = costs[b]: aln<b>, cig<b>, cig_off<b>, differs<b>"))),
    )
    for b in range(2):
        arrays["aln%d" % b] = np.array([r[0] for r in res[b]], dtype=np.int32)
        arrays["cig_off%d" % b] = np.cumsum([0] + [r[1].size for r in res[b]]).astype(np.int64)
        arrays["cig%d" % b] = np.concatenate([r[1] for r in res[b]]).astype(np.uint32)
        arrays["differs%d" % b] = np.array([int(r[2]) for r in res[b]], dtype=np.uint8)
    np.savez_compressed(OUT, **arrays)
    print("%d problems (%d redrawn), %.1f KB" % (len(probs), sum(p["redrawn"] for p in probs), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
