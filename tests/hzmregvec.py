"""Shared by test_hzmreg_cpu.py and test_gpu_hzmreg.py: the region form of align_hzmaux (wtz_pairs_seed_region, wtz_hzmaux_batch) driven three ways -
the one-call service, the stage-level path, the whole form of test_hzmaux_functions.run_device - and a model of the reference's match walk
(query_single_read_seeds_by_region, hzm_aln.h:117-171, behind the same-strand filter of hzm_aln.h:1193) written from the reference's text, in Python,
sharing nothing with the product."""
import numpy as np

from test_hzmaux_functions import WTGBO, _mutate

FIELDS = ("score", "tb", "te", "qb", "qe", "aln", "mat", "mis", "ins", "del")
MIN_SM = 0.6


def params(prm=WTGBO, min_sm=MIN_SM, refine=0, aux_strand=1):
    from smartdenovo_amd import hipabi
    P = hipabi.Params.defaults(zsize=prm[0], hz=prm[1], kwin=prm[2], ztot=prm[4], zovl=prm[4], max_zmer_freq=prm[5], max_kmer_var=prm[6],
                               w=prm[7], W=prm[8], ew=prm[9], M=prm[11], X=prm[12], O=prm[13], E=prm[15], T=prm[16], min_id=min_sm, refine=refine, aux_strand=aux_strand)
    P.kstep = prm[3]
    return P


def open_ctx(lib_path, seqs, subset=None, pool_bytes=1 << 30, **kw):
    """a context with the reads uploaded and the z-index built (subset: of those reads only)"""
    from smartdenovo_amd import hipabi
    ctx = hipabi.Context(params(**kw), pool_bytes=pool_bytes, lib_path=lib_path)
    ctx.upload(*hipabi.pack_reads(seqs))
    if subset is None:
        ctx.zindex_build()
    else:
        ctx.zindex_build_subset(sorted(subset))
    return ctx


def gates(x, tlen, qlen, min_sm):
    """hzm_aln.h:1715-1718 in float arithmetic"""
    f32 = np.float32
    beg = max(0, x[3] - x[1]); end = min(qlen, x[4] + tlen - x[2])
    return not (x[0] < 0 or f32(x[6]) < f32(x[5]) * f32(min_sm) or f32(x[6]) < f32(end - beg) * f32(min_sm))


def _after_seed(ctx, summ, lens, tid, rid, min_sm, refine):
    n = len(tid)
    items = [i for i in range(n) if summ["gate"][i] and summ["nwin"][i][0]]
    out = [None] * n
    if items:
        res, cig = ctx.pairs_align(items, [0] * len(items))
        off = 0
        for k, i in enumerate(items):
            r = res[k]; c = cig[off:off + int(r["cigar_len"])].copy(); off += int(r["cigar_len"])
            if r["n_regs"] == 0:
                continue
            x = tuple(int(r[f]) for f in FIELDS)
            if not refine and not gates(x, int(lens[tid[i]]), int(lens[rid[i]]), min_sm):
                continue
            out[i] = (x, c)
    return out


def whole_form(ctx, lens, tid, rid, min_sm=MIN_SM, refine=0):
    """wtz_pairs_seed + wtz_pairs_align and the caller's gates, as test_hzmaux_functions.run_device"""
    assert ctx.lib.wtz_batch_begin(ctx.h) == 0
    return _after_seed(ctx, ctx.pairs_seed(tid, rid), lens, tid, rid, min_sm, refine)


def stages(ctx, lens, tid, rid, beg, end, min_sm=MIN_SM, refine=0):
    """wtz_pairs_seed_region + wtz_pairs_align and the caller's gates"""
    assert ctx.lib.wtz_batch_begin(ctx.h) == 0
    return _after_seed(ctx, ctx.pairs_seed_region(tid, rid, beg, end), lens, tid, rid, min_sm, refine)


def service(ctx, tid, rid, beg, end):
    """wtz_hzmaux_batch"""
    res, cig = ctx.hzmaux_batch(tid, rid, beg, end)
    out = []
    for r in res:
        if not r["found"]:
            assert all(int(r[f]) == 0 for f in FIELDS) and r["cigar_len"] == 0
            out.append(None)
        else:
            out.append((tuple(int(r[f]) for f in FIELDS), cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])].copy()))
    return out


def fold_cigar(t, q, x, cigar):
    """the CIGAR walked over the two sequences from (tb, qb): op 0 both, 1 query only, 2 target only (hzm_aln.h:1737-1772); returns (te, qe, mat, mis, ins, del)"""
    ti, qi = x[1], x[3]
    mat = mis = ins = dele = 0
    for w in cigar:
        op, ln = int(w) & 0xF, int(w) >> 4
        if op == 0:
            eq = int((t[ti:ti + ln] == q[qi:qi + ln]).sum()); mat += eq; mis += ln - eq; ti += ln; qi += ln
        elif op == 1:
            ins += ln; qi += ln
        else:
            assert op == 2
            dele += ln; ti += ln
    return ti, qi, mat, mis, ins, dele


# ---- the recorded vectors (tests/golden/make_hzmreg_vectors.py: the reference's own compiled align_hzmaux with beg / end) ----
def load_vectors():
    """the layouts of tests/golden/hzmreg_vectors.npz: dicts of backbone, prm, min_sm, and per case read / beg / end / is_region / differs_from_whole /
    want = None or (the ten kswx_t fields, CIGAR words)"""
    import os
    v = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hzmreg_vectors.npz"))
    lays = [dict(backbone=np.ascontiguousarray(v["backbones"][v["bb_off"][i]:v["bb_off"][i + 1]]), prm=[int(x) for x in v["prm"][i]], min_sm=float(v["min_sm"]), cases=[])
            for i in range(v["prm"].shape[0])]
    for k in range(v["rec"].shape[0]):
        r = v["rec"][k]
        want = (tuple(int(x) for x in r[1:]), v["cigar"][v["cig_off"][k]:v["cig_off"][k + 1]].copy()) if r[0] else None
        lays[int(v["layout"][k])]["cases"].append(dict(read=np.ascontiguousarray(v["reads"][v["rd_off"][k]:v["rd_off"][k + 1]]), beg=int(v["beg"][k]), end=int(v["end"][k]),
                                                       is_region=bool(v["is_region"][k]), differs=bool(v["differs_from_whole"][k]), want=want))
    return lays


def run_vectors(lib_path, lays, how="service"):
    """every layout of load_vectors() in one call (how = "service": wtz_hzmaux_batch, "stages": wtz_pairs_seed_region + wtz_pairs_align, "whole": the interval ignored);
    returns per layout (got, want) in the form of test_hzmaux_functions.same"""
    out = []
    for lay in lays:
        cs = lay["cases"]
        seqs = [lay["backbone"]] + [c["read"] for c in cs]
        lens = [s.size for s in seqs]
        tid, rid = [0] * len(cs), list(range(1, len(cs) + 1))
        beg, end = [c["beg"] for c in cs], [c["end"] for c in cs]
        ctx = open_ctx(lib_path, seqs, prm=lay["prm"], min_sm=lay["min_sm"])
        try:
            if how == "service":
                got = service(ctx, tid, rid, beg, end)
            elif how == "stages":
                got = stages(ctx, lens, tid, rid, beg, end, min_sm=lay["min_sm"])
            else:
                got = whole_form(ctx, lens, tid, rid, min_sm=lay["min_sm"])
        finally:
            ctx.close()
        out.append((got, [c["want"] for c in cs]))
    return out


# ---- the reference's match walk, from its text ----
def zmers(seq, zsize, hz):
    """index_single_read_seeds' walk (hzm_aln.h:83-100): (mer, dir, off, len) in position order"""
    mask = (1 << (2 * zsize)) - 1
    out = []; hzoff = []; kmer = 0; b = 4; i = 0
    for j, c in enumerate(seq):
        c = int(c)
        if hz and c == b:
            continue
        b = c; i += 1; hzoff.append(j)
        kmer = ((kmer << 2) | b) & mask
        if i < zsize:
            continue
        rev = 0; k = kmer
        for _ in range(zsize):
            rev = (rev << 2) | (3 - (k & 3)); k >>= 2
        if rev == kmer:
            continue
        off = hzoff[i - zsize]
        out.append((min(kmer, rev), 0 if rev > kmer else 1, off, min(j + 1 - off, 0xFFFF)))
    return out


def model_matches(t, q, zsize, hz, zmax, zvar, tb, te, cut="break"):
    """the same-strand matches align_hzmaux keeps for the interval [tb, te) of t after the defaults of hzm_aln.h:1690-1691: the walk of hzm_aln.h:133-169 with
    qb = 0, qe = len(q), then hzm_aln.h:1193 with dir 0.  cut = "continue": what a walk WITHOUT the break of hzm_aln.h:161 would keep.  Returns (off1, off2, len1, len2)s."""
    if tb < 0:
        tb = 0
    if te <= 0:
        te = len(t)
    runs = {}
    for m in sorted(zmers(t, zsize, hz), key=lambda z: (z[0], z[2])):      # hzm_aln.h:101
        runs.setdefault(m[0], []).append(m)
    runs = {k: v for k, v in runs.items() if 0 < len(v) < zmax}                # hzm_aln.h:107
    kcnt = {}
    out = []
    for mer, d2, off2, len2 in zmers(q, zsize, hz):
        if mer not in runs:
            continue
        if kcnt.get(mer, 0) >= zmax:                                            # hzm_aln.h:154-157, in front of the interval tests
            continue
        kcnt[mer] = kcnt.get(mer, 0) + 1
        for _, d1, off1, len1 in runs[mer]:
            if off1 < tb:
                continue
            if off1 + len1 > te:
                if cut == "break":
                    break
                continue
            if abs(len1 - len2) > zvar:
                continue
            if d1 ^ d2:
                continue                                                        # hzm_aln.h:1193 with dir 0
            out.append((off1, off2, len1, len2))
    return out


def layout(seed, glen=20000, nreads=10, err=0.12, repeat=None):
    """a backbone and the reads of its layout, each with the interval of the backbone it was drawn from, widened or shifted a little as an estimate from
    pairwise overlaps would be (wtmsa.c:355-369).  repeat = (length, distance): the genome carries an exact duplicate, and reads lie inside or across one copy."""
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 4, size=glen, dtype=np.uint8)
    for _ in range(glen // 300):      # homopolymer runs
        p = int(rng.integers(0, G.size - 20)); G[p:p + int(rng.integers(3, 10))] = G[p]
    if repeat:
        ln, dist = repeat
        a = int(rng.integers(glen // 8, glen // 4))
        G[a + dist:a + dist + ln] = G[a:a + ln]
    reads, iv = [], []
    for k in range(nreads):
        ln = int(rng.integers(1500, 4000))
        if repeat and k % 2 == 0:        # inside or across the second copy
            b = max(0, min(glen - ln, a + dist + int(rng.integers(-ln // 2, repeat[0] // 2))))
        else:
            b = int(rng.integers(0, glen - ln))
        reads.append(np.ascontiguousarray(_mutate(rng, G[b:b + ln], err)))
        iv.append((b + int(rng.integers(-40, 40)), b + ln + int(rng.integers(-40, 40))))
    return G, reads, iv
