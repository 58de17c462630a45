"""The oracle's three banded DPs against the committed function-level vectors of the reference (tests/golden/dp_vectors.npz:
kswx_extend_align_shift_core kswx.h:101, kswx_extend_align_core kswx.h:234, ksw_global2 ksw.c:503).  Runs anywhere (no reference, no
GPU): this is what pins the oracle's DPs on the GPU box, where /root/reference does not exist."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dpvec import Vectors


class Aln(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("score", "tb", "te", "qb", "qe", "aln", "mat", "mis", "ins", "del_")]

    def tup(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


@pytest.fixture(scope="module")
def ora():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "liboracle.so"], check=True)
    return C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))


@pytest.fixture(scope="module")
def vec():
    return Vectors()


def test_vectors_cover_every_shape_class(vec):
    want = {"s_c1", "s_c4", "s_c8", "s_c12", "s_c16", "s_c20", "s_c24", "s_c28", "s_c32", "s_short", "s_rows", "s_stop", "s_end", "s_homo", "s_wide",
            "s_keyovf", "s_longt", "s_empty", "s_neginit", "s_cw6", "s_cw10", "s_cw14", "s_cw18", "s_cw22", "s_cw28", "s_cw30", "f_w50", "f_w20", "f_w5", "f_w100", "f_w200", "f_long", "f_rows2048", "f_keyovf", "f_stop",
            "f_empty", "f_homo", "g_c1", "g_c2", "g_c4", "g_c8", "g_ring", "g_ringwide", "g_small", "g_long", "g_unrelated", "g_empty", "g_homo"}
    assert want <= set(vec.cls.tolist())
    # the views cover both strands and both walking directions on both sides
    assert {tuple(v) for v in vec.view[:, [0, 2]].tolist()} == {(0, 1), (0, -1), (1, 1), (1, -1)}
    assert {tuple(v) for v in vec.view[:, [3, 5]].tolist()} == {(0, 1), (0, -1), (1, 1), (1, -1)}


def test_band_class_vectors_are_inside_both_frame_forms(vec):
    """The s_cw<n> problems exist to reach the row bodies of n band columns per lane in BOTH one-wave frame forms (DP forms 5 and 7 must answer them,
    tests/test_gpu_dp_forms.py): each has the band it is named for, two problems per class, and lies inside the 32-bit form's 2^20 envelope, its LDS words
    and the packed form's 16-bit window (a) - none of them is declined for its values."""
    from test_packed_window_model import geometry, pk_window
    S = vec.meta["scores"]
    seen = {}
    for i in np.nonzero(np.char.startswith(vec.cls, "s_cw"))[0]:
        w, ql, tl = geometry(int(vec.qlen[i]), int(vec.tlen[i]), int(vec.W[i]))
        n_col = min(tl, 2 * w + 1)
        assert (n_col + 63) // 64 == int(str(vec.cls[i])[4:]), "problem %d (%s)" % (i, vec.cls[i])
        init = max(int(vec.init[i]), 0)
        assert init + abs(S["M"]) * min(ql, tl) + (ql + tl + 4) * abs(S["E"]) + 10000 + abs(S["X"]) + abs(S["O"]) + 16 < (1 << 20)       # wtz_extjob_run_fr
        assert (tl + 63) // 32 + 1 <= 1032 and (tl + 31) // 32 + 3 <= 1032 and (ql + 63) // 64 <= 1024
        assert (S["M"], S["X"], S["O"], S["E"]) == (2, -5, -3, -1)       # the scores pk_window is written for
        win = pk_window(init, ql, tl)
        assert win is not None and win[1] == -10000 and win[2] == -(1 << 30), "problem %d (%s): not in window (a)" % (i, vec.cls[i])
        seen[str(vec.cls[i])] = seen.get(str(vec.cls[i]), 0) + 1
    assert seen == {"s_cw%d" % n: 2 for n in (6, 10, 14, 18, 22, 28, 30)}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_oracle_equals_reference_vectors(kind, vec, ora):
    S = vec.meta["scores"]
    n = 0
    for i in np.nonzero(vec.kind == kind)[0]:
        q, t = vec.logical(i, "q"), vec.logical(i, "t")
        cg = np.zeros(q.size + t.size + 8, dtype=np.uint32)
        if kind == 2:
            s = C.c_int()
            qq = np.ascontiguousarray(np.concatenate([q, [0]]).astype(np.uint8))
            tt = np.ascontiguousarray(np.concatenate([t, [0]]).astype(np.uint8))
            m = ora.ora_global_c(int(q.size), C.c_void_p(qq.ctypes.data), int(t.size), C.c_void_p(tt.ctypes.data), S["M"], S["X"], -S["O"], -S["E"], -S["O"], -S["E"],
                                 int(vec.W[i]), C.byref(s), C.c_void_p(cg.ctypes.data))
            assert s.value == vec.aln[i][0], "problem %d (%s)" % (i, vec.cls[i])
        else:
            a = Aln()
            fn = ora.ora_extend_shift_c if kind == 0 else ora.ora_extend_fixed_c
            W = int(vec.W[i]) if kind == 0 else int(vec.w_param[i])
            m = fn(int(q.size), C.c_void_p(q.ctypes.data), int(t.size), C.c_void_p(t.ctypes.data), 1, int(vec.init[i]), W, S["M"], S["X"], S["O"], S["O"], S["E"], S["T"],
                   C.byref(a), C.c_void_p(cg.ctypes.data))
            assert a.tup() == tuple(vec.aln[i].tolist()), "problem %d (%s)" % (i, vec.cls[i])
        assert (cg[:m] == vec.expected_cigar(i)).all() and m == vec.expected_cigar(i).size, "problem %d (%s): CIGAR" % (i, vec.cls[i])
        n += 1
    assert n > 40


def _ext_geometry(qlen, tlen, init, W, S):
    """wtz_ext_geometry (wtz_sw.h) with one opening cost: (w, ql, tl, n_col)"""
    w = W
    if w > 0:
        w = min(w, max(int((min(qlen, tlen) * S["M"] + init - S["T"] + S["O"]) / -S["E"]) + 1, 1))
    else:
        w = -w
    w = min(w, max(qlen, tlen))
    if qlen < tlen:
        ql, tl = qlen, (qlen + w if qlen + w < tlen else tlen)
    else:
        tl, ql = tlen, (tlen + w if tlen + w < qlen else qlen)
    return w, ql, tl, min(tl, 2 * w + 1)


def test_vectors_reach_the_paths_of_the_register_forms(vec):
    """The K-sw1 and K-sw2 register forms (wtz_sw_fixed.h, wtz_sw_global.h) have paths a short problem never enters; the vectors hold a problem for each, told
    from the lengths, the recorded answers and the recorded CIGARs alone (the forms are the choices of wtz_fixed_problem_wave / wtz_gap_problem_wave; LDS slices of
    12 288 bytes, 1 024 of them sequence words):
      K-sw1, trace in LDS, last computed row even (its nibbles are written by the flush behind the row loop) and odd;
      K-sw1, trace in the pool, a walk of more than one staged block (more than 2 RB rows at the problem's zrow), last computed row even and odd;
      K-sw2, trace in LDS, tlen odd (last row even: the flush) and even;
      K-sw2, trace in the pool, tlen > 2048 and a walk that crosses row 2 048 with columns left (the walk reloads the target words there).
    The last computed row of a K-sw1 problem is known where the answer ends on the last query row and the geometry does not cut the rows: ql - 1."""
    S = vec.meta["scores"]
    ztr_bytes = 12288 - 1024
    seen = set()
    for i in np.nonzero(vec.kind == 1)[0]:
        qlen, tlen, init = int(vec.qlen[i]), int(vec.tlen[i]), max(int(vec.init[i]), 0)
        if qlen <= 0 or tlen <= 0:
            continue
        w, ql, tl, n_col = _ext_geometry(qlen, tlen, init, int(vec.w_param[i]), S)
        if not (int(vec.aln[i][4]) == qlen and ql == qlen):      # qe == qlen: the rows ran to the end
            continue
        run_bytes, zrow, hmax = 4 * (ql + tl + 4), (n_col + 3) & ~3, init + S["M"] * min(ql, tl)
        shape = ql <= 2048 and (tl + 63) // 32 + 1 <= 128
        lds = shape and n_col <= 128 and hmax < (1 << 23) and ((ql + 1) // 2) * zrow + run_bytes <= ztr_bytes
        pool = shape and not lds and n_col <= 512 and hmax < ((1 << 23) if n_col <= 128 else (1 << 21)) and 4096 + run_bytes <= ztr_bytes
        rb = 32 if zrow <= 128 else (16 if zrow <= 256 else 8)
        # the walk starts on (qe - 1, te - 1) and steps while both coordinates are inside (what is left then is appended as one gap, not walked): replay the recorded
        # CIGAR backwards, op 0 moves both, 1 (I) a row, 2 (D) a column; rows walked = the rows between the start and the cell the walk stops on
        r, c = int(vec.aln[i][4]) - 1, int(vec.aln[i][2]) - 1
        r0 = r
        for cw in vec.expected_cigar(i)[::-1]:
            op, ln = int(cw) & 0xF, int(cw) >> 4
            for _ in range(ln):
                if r < 0 or c < 0:
                    break
                r -= op != 2
                c -= op != 1
        rows_walked = r0 - max(r, -1)
        if lds:
            seen.add(("f_lds", (ql - 1) & 1))
        if pool and rows_walked > 2 * rb:
            seen.add(("f_pool_blocks", (ql - 1) & 1))
    for i in np.nonzero(vec.kind == 2)[0]:
        dq, dt, w = int(vec.qlen[i]), int(vec.tlen[i]), int(vec.W[i])
        if dq <= 0 or dt <= 0:
            continue
        n_col = min(dq, 2 * w + 1)
        zrow, run_bytes, qwords = (n_col + 3) & ~3, 4 * (dq + dt + 4), (dq + 63) // 32 + 1
        qbytes = (qwords * 8 + 15) & ~15
        lds = n_col <= 128 and dt <= 2048 and qwords <= 128 and ((dt + 1) // 2) * zrow + run_bytes <= ztr_bytes
        pool = not lds and n_col <= 512 and qbytes + 4096 <= 12288
        if lds:
            seen.add(("g_lds", dt & 1))
        if pool and dt > 2048:
            # rows run over the target: walk the recorded CIGAR backwards from (dt - 1, dq - 1); op 0 moves both, 2 (D) a row, 1 (I) a column
            ii, k = dt - 1, dq - 1
            for c in vec.expected_cigar(i)[::-1]:
                op, ln = int(c) & 0xF, int(c) >> 4
                for _ in range(ln):
                    if ii < 2048:
                        break
                    ii -= op != 1
                    k -= op != 2
                if ii < 2048:
                    break
            if ii == 2047 and k >= 0:
                seen.add(("g_pool_reload", 0))
    assert seen >= {("f_lds", 0), ("f_lds", 1), ("f_pool_blocks", 0), ("f_pool_blocks", 1), ("g_lds", 0), ("g_lds", 1), ("g_pool_reload", 0)}, sorted(seen)
