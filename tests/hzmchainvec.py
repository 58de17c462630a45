"""Shared by test_hzmchain_cpu.py and test_gpu_hzmchain.py: the vectors of tests/golden/hzmchain_vectors.npz (make_hzmchain_vectors.py: the reference's compiled
align_hzmaux with HZM_FAST_WINDOW_KMER_CHAINING = 0) and the calls that run them with wtz_set_window_chaining.  The runners are hzmregvec's."""
import os

import numpy as np

import hzmregvec as hv


def load_vectors():
    """as hzmregvec.load_vectors, per case also differs (from the flag-1 run), tie, wins = None or the (n, 4) beg[0], beg[1], end[0], end[1] of the chain windows"""
    v = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hzmchain_vectors.npz"))
    lays = [dict(backbone=np.ascontiguousarray(v["backbones"][v["bb_off"][i]:v["bb_off"][i + 1]]), prm=[int(x) for x in v["prm"][i]], min_sm=float(v["min_sm"]), cases=[])
            for i in range(v["prm"].shape[0])]
    for k in range(v["rec"].shape[0]):
        r = v["rec"][k]
        want = (tuple(int(x) for x in r[1:]), v["cigar"][v["cig_off"][k]:v["cig_off"][k + 1]].copy()) if r[0] else None
        wins = v["win"][v["win_off"][k]:v["win_off"][k + 1]].copy() if v["has_win"][k] else None
        lays[int(v["layout"][k])]["cases"].append(dict(read=np.ascontiguousarray(v["reads"][v["rd_off"][k]:v["rd_off"][k + 1]]), beg=int(v["beg"][k]), end=int(v["end"][k]),
                                                       is_region=bool(v["is_region"][k]), differs=bool(v["differs_from_fast"][k]), tie=bool(v["tie"][k]), want=want, wins=wins))
    return lays


def stages_with_windows(ctx, lens, tid, rid, beg, end, min_sm):
    """wtz_pairs_seed_region -> wtz_pairs_windows -> wtz_pairs_align -> wtz_fetch_cigars (hzmregvec.stages with the window boxes fetched in between);
    returns (results, per pair None or the (n, 4) boxes of its chain windows)"""
    assert ctx.lib.wtz_batch_begin(ctx.h) == 0
    summ = ctx.pairs_seed_region(tid, rid, beg, end)
    boxes = ctx.pairs_windows(summ)
    wins, at = [], 0
    for i in range(len(tid)):
        assert summ["nwin"][i][1] == 0
        k = int(summ["nwin"][i][0])
        wins.append(np.array([[b["beg"][0], b["beg"][1], b["end"][0], b["end"][1]] for b in boxes[at:at + k]], dtype=np.int32).reshape(-1, 4) if k else None)
        at += k
    return hv._after_seed(ctx, summ, lens, tid, rid, min_sm, 0), wins


def run_group(lib_path, lays, fast, how, pool_bytes=1 << 30):
    """the layouts `lays` (one parameter set) in ONE context: every backbone and every read uploaded, one call; returns per layout (got, wins or None)"""
    prm, min_sm = lays[0]["prm"], lays[0]["min_sm"]
    assert all(lay["prm"] == prm for lay in lays)
    seqs, tid, rid, beg, end = [], [], [], [], []
    for lay in lays:
        t = len(seqs); seqs.append(lay["backbone"])
        for c in lay["cases"]:
            tid.append(t); rid.append(len(seqs)); seqs.append(c["read"]); beg.append(c["beg"]); end.append(c["end"])
    lens = [s.size for s in seqs]
    ctx = hv.open_ctx(lib_path, seqs, pool_bytes=pool_bytes, prm=prm, min_sm=min_sm)
    try:
        if fast is not None:
            ctx.set_window_chaining(fast)
        if how == "service":
            got, wins = hv.service(ctx, tid, rid, beg, end), None
        else:
            got, wins = stages_with_windows(ctx, lens, tid, rid, beg, end, min_sm)
    finally:
        ctx.close()
    out, at = [], 0
    for lay in lays:
        k = len(lay["cases"])
        out.append((got[at:at + k], wins[at:at + k] if wins is not None else None))
        at += k
    return out


def run_vectors(lib_path, lays, fast, how):
    """every layout, grouped by parameter set (a context has one: two contexts for O = -3 and O = -2); returns per layout (got, wins or None) in the order of lays"""
    out = [None] * len(lays)
    for O in sorted({lay["prm"][13] for lay in lays}):
        idx = [i for i, lay in enumerate(lays) if lay["prm"][13] == O]
        for i, r in zip(idx, run_group(lib_path, [lays[i] for i in idx], fast, how)):
            out[i] = r
    return out


def equal(g, w):
    return (g is None) == (w is None) and (g is None or (g[0] == w[0] and np.array_equal(g[1], w[1])))


def check_vectors(lib_path, lays):
    """the service and the stage-level path with wtz_set_window_chaining(0) equal the record: the ten fields, every CIGAR word, the boxes of the chain windows"""
    from test_hzmaux_functions import same
    nhit = 0
    for how in ("service", "stages"):
        for lay, (got, wins) in zip(lays, run_vectors(lib_path, lays, 0, how)):
            nhit += same([c["want"] for c in lay["cases"]], got, "reference vs " + how)
            for c, g in zip(lay["cases"], got):
                if g is not None:
                    x, cig = g
                    assert hv.fold_cigar(lay["backbone"], c["read"], x, cig) == (x[2], x[4], x[6], x[7], x[8], x[9]) and x[5] == x[6] + x[7] + x[8] + x[9]
            if wins is not None:
                for i, (c, w) in enumerate(zip(lay["cases"], wins)):
                    assert (w is None) == (c["wins"] is None), "case %d: chain windows / none differs" % i
                    assert w is None or np.array_equal(w, c["wins"]), "case %d: window boxes %s != %s" % (i, w.tolist(), c["wins"].tolist())
    return nhit


def dense_window_pair(seed=7, unit=150, copies=6):
    """a backbone with `copies` tandem copies of one `unit`-base stretch (900 bases: little more than one window) and a read drawn across them: every clean z-mer
    of the read's copies matches in every copy of the backbone, so the first scan of the pair - the matches within zwin of the first one, the interval beginning at
    the block - holds several hundred same-strand matches: more than any LDS slice of the pair kernels' size takes (256 matches need 512 + 2 * 256 + 2 words of
    8 bytes, the slice has 1 024), whatever the device.  Returns (backbone, read, beg, end)."""
    from test_hzmaux_functions import _mutate
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 4, size=6000, dtype=np.uint8)
    a = 2000
    G[a:a + unit * copies] = np.tile(G[a:a + unit], copies)
    rd = np.ascontiguousarray(_mutate(rng, G[a - 300:a + 2200], 0.12))
    return G, rd, a - 5, a + 2200


def first_scan_matches(G, rd, prm, beg, end):
    """by the model of the reference's walk: the matches whose off1 lies within zwin of the first match's (the range of the pair's first window scan, hzm_aln.h:606-612)"""
    m = hv.model_matches(G, rd, prm[0], prm[1], prm[5], prm[6], beg, end)
    lo = min(x[0] for x in m)
    return sum(x[0] <= lo + prm[2] for x in m)
