"""Shared by test_gapopen_cpu.py and test_gpu_gapopen.py: the vectors of tests/golden/hzmid_vectors.npz (make_hzmid_vectors.py: the reference's compiled
align_hzmaux as wtmsa runs it - windows by chaining_hzmps, I = -2, D = -3) and the calls that run them with wtz_set_gap_open.  The runners are hzmregvec's."""
import os

import numpy as np

import hzmchainvec as cv
import hzmregvec as hv

I, D = -2, -3


def load_vectors():
    """as hzmregvec.load_vectors; per case also differs_m2 / differs_m3 (the record differs from the same call at (-2, -2) / (-3, -3)) and differs (from both);
    per layout chain_layout = its number in hzmchain_vectors.npz, where the same calls are recorded at (-3, -3)"""
    v = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hzmid_vectors.npz"))
    lays = [dict(backbone=np.ascontiguousarray(v["backbones"][v["bb_off"][i]:v["bb_off"][i + 1]]), prm=[int(x) for x in v["prm"][i]], min_sm=float(v["min_sm"]),
                 chain_layout=int(v["chain_layout"][i]), cases=[]) for i in range(v["prm"].shape[0])]
    for k in range(v["rec"].shape[0]):
        r = v["rec"][k]
        want = (tuple(int(x) for x in r[1:]), v["cigar"][v["cig_off"][k]:v["cig_off"][k + 1]].copy()) if r[0] else None
        lays[int(v["layout"][k])]["cases"].append(dict(read=np.ascontiguousarray(v["reads"][v["rd_off"][k]:v["rd_off"][k + 1]]), beg=int(v["beg"][k]), end=int(v["end"][k]),
                                                       is_region=bool(v["is_region"][k]), differs=bool(v["differs"][k]), differs_m2=bool(v["differs_m2"][k]),
                                                       differs_m3=bool(v["differs_m3"][k]), want=want))
    return lays


def open_all(lib_path, lays, O, pool_bytes=1 << 30):
    """every layout (one parameter set) in ONE context with params.O = O and the windows by chaining_hzmps; returns (ctx, lens, tid, rid, beg, end)"""
    prm = list(lays[0]["prm"])
    assert all(lay["prm"] == lays[0]["prm"] for lay in lays)
    prm[13] = O      # hzmregvec.params reads the context's one params.O from here
    seqs, tid, rid, beg, end = [], [], [], [], []
    for lay in lays:
        t = len(seqs); seqs.append(lay["backbone"])
        for c in lay["cases"]:
            tid.append(t); rid.append(len(seqs)); seqs.append(c["read"]); beg.append(c["beg"]); end.append(c["end"])
    ctx = hv.open_ctx(lib_path, seqs, pool_bytes=pool_bytes, prm=prm, min_sm=lays[0]["min_sm"])
    ctx.set_window_chaining(0)
    return ctx, [s.size for s in seqs], tid, rid, beg, end


def run(ctx, how, lens, tid, rid, beg, end, min_sm):
    return hv.service(ctx, tid, rid, beg, end) if how == "service" else hv.stages(ctx, lens, tid, rid, beg, end, min_sm=min_sm)


def wants(lays):
    return [c["want"] for lay in lays for c in lay["cases"]]


def chain_wants(lays):
    """the committed (-3, -3) records of the same calls: hzmchain_vectors.npz"""
    ch = cv.load_vectors()
    out = []
    for lay in lays:
        twin = ch[lay["chain_layout"]]
        assert np.array_equal(twin["backbone"], lay["backbone"]) and len(twin["cases"]) == len(lay["cases"]) and twin["prm"][13] == -3 and twin["prm"][14] == -3
        for a, b in zip(twin["cases"], lay["cases"]):
            assert np.array_equal(a["read"], b["read"]) and (a["beg"], a["end"]) == (b["beg"], b["end"])
            out.append(a["want"])
    return out
