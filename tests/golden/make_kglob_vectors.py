"""Generator of tests/golden/kglob_vectors.npz: function-level rows for wtz_global_batch (every expected value from the reference's own ksw_global2 in
oracle/_ref/libref_shim.so) and chain rows for wtz_alignx_batch (tests/kglobvec.py:ref_chainx around the reference's ksw_align2, ksw_extend2 and
ksw_global2).  Conventions as in kext_vectors.npz: words / offs / lens, M = 2, X = -5.  Prints and asserts the branch counts it claims.

    python tests/golden/make_kglob_vectors.py        (needs oracle/_ref/libref_shim.so)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kglobvec as gv  # noqa: E402
from smartdenovo_amd import hipabi  # noqa: E402

M, X = 2, -5
rng = np.random.default_rng(20261019)
reads, F, CH = [], [], []


def rseq(n, k=4):
    return rng.integers(0, k, n).astype(np.uint8)


def mutate(s, rate, k=4):
    out, i = [], 0
    while i < len(s):
        r = rng.random()
        if r < rate * 0.3:
            out.extend(rng.integers(0, k, 1 + int(rng.random() < 0.2) * int(rng.integers(1, 6))).tolist())
        elif r < rate * 0.6:
            i += 1 + int(rng.random() < 0.2) * int(rng.integers(1, 6))
            continue
        elif r < rate:
            out.append((int(s[i]) + 1 + int(rng.integers(0, k - 1))) % k)
            i += 1
            continue
        out.append(int(s[i]))
        i += 1
    return np.array(out if out else [0], dtype=np.uint8)


def fit(s, n, k=4):
    s = np.asarray(s, dtype=np.uint8)
    return s[:n] if len(s) >= n else np.concatenate([s, rseq(n - len(s), k)])


def add_read(s):
    reads.append(np.asarray(s, dtype=np.uint8))
    return len(reads) - 1


def add(name, q, t, w, gap=0, **view):
    """a function-level row; without `view` both sides are whole reads of their own"""
    if view:
        p = dict(view)
    else:
        p = dict(q_read=add_read(q), t_read=add_read(t), q_rev=0, t_rev=0, q_from=0, t_from=0, q_strand=1, t_strand=1, q_len=len(q), t_len=len(t))
        if len(q) == len(t) and (np.asarray(q) == np.asarray(t)).all():
            p["t_read"] = p["q_read"]
            reads.pop()
    q = gv.view(reads, p["q_read"], p["q_rev"], p["q_from"], p["q_strand"], p["q_len"])
    t = gv.view(reads, p["t_read"], p["t_rev"], p["t_from"], p["t_strand"], p["t_len"])
    assert abs(len(q) - len(t)) <= w, name
    sc, cg = gv.ref_global(q, t, M, X, gv.GAPS[gap], w)
    p.update(name=name, W=w, gap=gap, expect=(sc,) + gv.fold(q, t, cg), cigar=cg, cells=gv.cells_of(len(q), len(t), w), slots=gv.slots_of(len(q), len(t), w))
    F.append(p)
    return p


# ---------------- form edges ----------------
def shape(S, kind):
    """(qlen, tlen, w) with exactly S band slots: 0 = symmetric (odd S), 1 = q_len - 1 < w (so q_len < 2w + 1), 2 = t_len - 1 < w"""
    if kind == 0:
        w = (S - 1) // 2
        n = w + 1 + int(rng.integers(0, 40))
        return n + int(rng.integers(0, min(w, 9) + 1)), n, w
    short = max(2, S // 3)
    w = S - short
    other = w + 1 + int(rng.integers(0, short))
    return (short, other, w) if kind == 1 else (other, short, w)


EDGES = [64 * c + d for c in (1, 2, 4, 8, 16) for d in (-1, 0, 1)] + [2047, 2049, 2400]
for S in EDGES:
    for vi, var in enumerate(("copy", "unrelated", "all_A", "two_letter", "short_q", "short_t")):
        kind = 1 if var == "short_q" else (2 if var == "short_t" else (0 if S & 1 else 1 + vi % 2))
        ql, tl, w = shape(S, kind)
        k = 2 if var == "two_letter" else 4
        if var == "all_A":
            q, t = np.zeros(ql, dtype=np.uint8), np.zeros(tl, dtype=np.uint8)
        elif var == "unrelated":
            q, t = rseq(ql), rseq(tl)
        else:
            q = rseq(ql, k)
            t = fit(q if var == "copy" else mutate(q, 0.15, k), tl, k)
        p = add("edge_%d_%s" % (S, var), q, t, w, gap=vi % 4 if var in ("two_letter", "all_A") else 0)
        assert p["slots"] == S, (S, var, p["slots"])

# ---------------- small and boundary shapes ----------------
for n in (1, 2, 31, 32, 33, 63, 64, 65):
    q = rseq(n)
    add("w0_%d" % n, q, fit(mutate(q, 0.2), n), 0, gap=n % 4)
add("q1_t1", rseq(1), rseq(1), 0)
add("q1_t1_w3", np.array([2], dtype=np.uint8), np.array([2], dtype=np.uint8), 3)
add("q1_t9", rseq(1), rseq(9), 8)
add("q9_t1", rseq(9), rseq(1), 8, gap=1)
for n in (31, 32, 33, 63, 64, 65):
    for d in (-1, 1):      # |q_len - t_len| = w exactly: the path ends on the band's edge, both tails fire
        w = 7
        q = rseq(n)
        t = mutate(q, 0.1)
        t = fit(t, n + d * w) if n + d * w > 0 else t[:1]
        add("edge_path_%d_%+d" % (n, d), q, t, abs(len(q) - len(t)), gap=(n + d) % 4)
    add("rows_%d" % n, rseq(40), fit(mutate(rseq(40), 0.3), n), max(12, abs(n - 40)), gap=2)
    add("cols_%d" % n, fit(mutate(rseq(40), 0.3), n), rseq(40), max(12, abs(n - 40)), gap=1)
q = rseq(20000)
add("rows_20000_w40", q, fit(mutate(q, 0.06), 20010), 40)
q = rseq(6000)
add("rows_6000_slots_2047", q, fit(mutate(q, 0.12), 6020), 1023)
assert F[-1]["slots"] == 2047
# gap costs: every pattern on the same noisy pair; the impossible CIGAR of ksw.c:541-543 (X = -5 against open 0, extend 1)
q = rseq(300)
t = mutate(q, 0.3)
for g in range(4):
    add("gaps_%d" % g, q, t, abs(len(q) - len(t)) + 20, gap=g)
q = rseq(200)
t = q.copy()
t[50:150:7] = (t[50:150:7] + 1) % 4
add("open0_mismatches", q, t, 10, gap=3)
n_id = sum(1 for w1, w2 in zip(F[-1]["cigar"][:-1], F[-1]["cigar"][1:]) if {int(w1) & 0xF, int(w2) & 0xF} == {1, 2})
print("open0_mismatches: %d runs, %d adjacent I/D pairs (ksw_global2 never opens one gap from the other)" % (len(F[-1]["cigar"]), n_id))
assert n_id == 0

# ---------------- traceback across the staged window (64 row groups x 256 slots at C >= 8) ----------------
a, b, c = rseq(300), rseq(700), rseq(300)
add("tb_vertical_700", np.concatenate([a, c]), np.concatenate([a, b, c]), 720)
add("tb_horizontal_700", np.concatenate([a, b, c]), np.concatenate([a, c]), 720)
assert any((int(x) & 0xF) == 2 and (int(x) >> 4) >= 600 for x in F[-2]["cigar"]) and any((int(x) & 0xF) == 1 and (int(x) >> 4) >= 600 for x in F[-1]["cigar"])
w = 300
core = rseq(1200)
qd = np.concatenate([np.concatenate([core[i:i + 40], rseq(19)]) for i in range(0, 1200, 40)])      # 30 x 19 extra query bases: the path climbs 570 slots
td = np.concatenate([rseq(w - 5), core])                                                         # and starts w - 5 slots below the main diagonal
add("tb_drift", qd, td, w)
print("traceback rows: vertical run %d, horizontal run %d, drift over %d slots" % (max(int(x) >> 4 for x in F[-3]["cigar"] if (int(x) & 0xF) == 2),
      max(int(x) >> 4 for x in F[-2]["cigar"] if (int(x) & 0xF) == 1), F[-1]["slots"]))

# ---------------- views ----------------
big = add_read(rseq(1500))
big2 = add_read(mutate(reads[big], 0.1))
L2 = len(reads[big2])
for o in range(32):
    n = 150 + o
    qs, ts = (1, -1)[o & 1], (1, -1)[(o >> 1) & 1]
    qr, tr_ = (o >> 2) & 1, (o >> 3) & 1
    off_big = sum(len(r) for r in reads[:big])      # base 0 of the query view sits at every offset mod 32 of the uploaded words
    qf = next(f for f in range(200, 400) if ((off_big + (len(reads[big]) - 1 - f if qr else f)) & 31) == o)
    tf = min(L2 - n - 8, o * 3 + 37)
    tf = tf if ts > 0 else tf + n + 5 - 1
    add("view_%d" % o, None, None, 25, gap=o % 4, q_read=big, t_read=big2, q_rev=qr, t_rev=tr_, q_from=qf, t_from=tf, q_strand=qs, t_strand=ts, q_len=n, t_len=n + 5)
add("view_first_base", None, None, 30, q_read=0, t_read=0, q_rev=0, t_rev=0, q_from=0, t_from=0, q_strand=1, t_strand=1, q_len=40, t_len=40)
last = add_read(rseq(333))
add("view_read_end", None, None, 30, q_read=last, t_read=last, q_rev=0, t_rev=1, q_from=332, t_from=0, q_strand=-1, t_strand=1, q_len=100, t_len=110)
arm = rseq(400)
hp = add_read(np.concatenate([arm, rseq(30), mutate((3 - arm[::-1]).astype(np.uint8), 0.12)]))
n = len(reads[hp])
add("view_wtcyc_shape", None, None, 200, q_read=hp, t_read=hp, q_rev=1, t_rev=0, q_from=0, t_from=0, q_strand=1, t_strand=1, q_len=n, t_len=n)
F[-1]["pin_last"] = True

# ---------------- chain rows ----------------
def add_chain(name, q, t, w, T, q_rev=0, t_rev=0, same=False):
    qi = add_read(q)
    ti = qi if same else add_read(t)
    qq = gv.view(reads, qi, q_rev, 0, 1, len(reads[qi]))
    tt = gv.view(reads, ti, t_rev, 0, 1, len(reads[ti]))
    exp, cg, br = gv.ref_chainx(qq, tt, M, X, w, -3, -3, -1, T)
    CH.append(dict(name=name, q_read=qi, t_read=ti, q_rev=q_rev, t_rev=t_rev, w=w, T=T, expect=exp, cigar=cg, branch=br))
    return CH[-1]


add_chain("all_A_all_C", np.zeros(80, dtype=np.uint8), np.ones(90, dtype=np.uint8), 50, -100)
for k in range(14):
    q = rseq(int(rng.integers(200, 700)))
    rate = (0.02, 0.08, 0.15, 0.25)[k % 4]
    t = np.concatenate([rseq(int(rng.integers(0, 60))), mutate(q, rate), rseq(int(rng.integers(0, 60)))])
    add_chain("pair_%d_e%d" % (k, int(rate * 100)), q, t, (50, 200, 800)[k % 3], (-100, -30, 0)[k % 3 if k > 2 else 0], t_rev=k & 1)
for k, (gap_len, w) in enumerate(((60, 50), (150, 60), (90, 100))):      # one long gap: 1.5 * diff raises the band
    a, c = rseq(500), rseq(500)
    add_chain("gap_%d" % gap_len, np.concatenate([a, c]), np.concatenate([mutate(a, 0.03), rseq(gap_len), mutate(c, 0.03)]), w, -200)
for k, w in enumerate((-40, -200)):      # a negative w is the exact band; T >= 0: no extension
    q = rseq(300)
    add_chain("exact_band_%d" % -w, q, mutate(q, 0.1), w, 0)
a, c = rseq(1500), rseq(1500)
add_chain("skew_800", np.concatenate([a, rseq(800), c]), np.concatenate([mutate(a, 0.1), mutate(c, 0.1)]), 1023, -1000)
arm = rseq(900)
add_chain("hairpin", np.concatenate([arm, rseq(40), mutate((3 - arm[::-1]).astype(np.uint8), 0.15)]), None, 800, -100, q_rev=1, same=True)

# ---------------- the last uploaded base ----------------
# the last row ends on the last base that is uploaded: the strand -1 view starts at the final base of the final read
fin = len(reads) - 1
nf = len(reads[fin])
add("view_last_uploaded_base", None, None, 30, q_read=fin, t_read=fin, q_rev=0, t_rev=1, q_from=nf - 1, t_from=0, q_strand=-1, t_strand=1, q_len=100, t_len=110)
assert F[-1]["q_read"] == len(reads) - 1 and F[-1]["q_from"] == len(reads[-1]) - 1

# ---------------- what the file claims ----------------
forms = [gv.form_of(p["slots"], False, p["q_len"], p["W"]) for p in F]
print("function-level rows: %d; by form (device) %s" % (len(F), {f: forms.count(f) for f in sorted(set(forms))}))
assert set(forms) == {1, 2, 4, 8, 16, 32, 33}
ties = sum(1 for p in F if "all_A" in p["name"])
br = [c["branch"] for c in CH]
cnt = {n: br.count(v) for n, v in (("none", gv.B_NONE), ("diff", gv.B_DIFF), ("w2", gv.B_W2), ("lift", gv.B_LIFT), ("exact", gv.B_EXACT))}
wide_chain = sum(1 for c in CH if c["expect"][0] and gv.slots_of(c["expect"][5] - c["expect"][4], c["expect"][3] - c["expect"][2], c["expect"][11]) > hipabi.GLOB_MAXSLOTS)
print("chain rows: %d; found = 0: %d; band decided by %s; T = 0: %d; beyond %d slots: %d; bands %s" % (len(CH), sum(1 for c in CH if not c["expect"][0]), cnt,
      sum(1 for c in CH if c["T"] == 0), hipabi.GLOB_MAXSLOTS, wide_chain, sorted(set(c["expect"][11] for c in CH))))
assert ties >= 18 and cnt["diff"] >= 1 and cnt["w2"] >= 1 and cnt["lift"] >= 1 and cnt["exact"] >= 2 and wide_chain >= 1 and any(not c["expect"][0] for c in CH)
assert max(c["expect"][11] for c in CH) > 1023

words, offs, lens = hipabi.pack_reads(reads)
fc, fo = gv.encode_cigars([p["cigar"] for p in F])
cc, co = gv.encode_cigars([c["cigar"] for c in CH])
out = dict(words=words, offs=offs, lens=lens, M=np.int32(M), X=np.int32(X), f_names=np.array([p["name"] for p in F]), f_gap=np.array([p["gap"] for p in F], dtype=np.int32),
           f_expect=np.array([p["expect"] for p in F], dtype=np.int32), f_cells=np.array([p["cells"] for p in F], dtype=np.uint64), f_slots=np.array([p["slots"] for p in F], dtype=np.int32),
           f_cigar=fc, f_cig_off=fo, c_names=np.array([c["name"] for c in CH]), c_expect=np.array([c["expect"] for c in CH], dtype=np.int32),
           c_branch=np.array(br, dtype=np.int32), c_cigar=cc, c_cig_off=co)
for f in ("q_read", "t_read", "q_rev", "t_rev", "q_from", "t_from", "q_strand", "t_strand", "q_len", "t_len", "W"):
    out["f_" + f] = np.array([p[f] for p in F], dtype=np.int32 if f.endswith(("from", "strand", "len", "W")) else np.uint32)
for f in ("q_read", "t_read", "q_rev", "t_rev"):
    out["c_" + f] = np.array([c[f] for c in CH], dtype=np.uint32)
out["c_w"] = np.array([c["w"] for c in CH], dtype=np.int32)
out["c_T"] = np.array([c["T"] for c in CH], dtype=np.int32)
np.savez_compressed(gv.VECTORS, **out)
size = os.path.getsize(gv.VECTORS)
print("%s: %d bytes" % (os.path.relpath(gv.VECTORS, gv.ROOT), size))
assert size < 256 * 1024
