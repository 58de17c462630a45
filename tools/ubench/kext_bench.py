#!/usr/bin/env python3
"""Time wtz_kext_batch (K-kext, csrc/wtz_sw_kext.h) and the three stages of wtz_align_batch on a seeded wtcyc-shaped set and write
profiles/kext_batch_<date>.json.  Not part of bench.py.

The set: --reads reads of --len bases, each with a planted, 12 %-mutated palindrome, against their own reverse complement (t_rev = 1), w = 800,
I = D = -3, E = -1, T = -100 (wtcyc's call).  A local pass (wtz_local_batch) gives the hits; the ksw_extend2 problems are the RIGHT extensions
kswx_extend_core (kswx.h:1417-1438) would start from them: h0 = the local score, the longer remaining side as rows, cut to the other + w.

Reported: ms_kext (the library's HIP-event time around the K-kext launches: copies and host planning excluded), median of --repeat calls after one
warm-up call; cells_kext per second; where oracle/_ref/libref_shim.so is present, the time of the reference's ksw_extend2 on the same problems on one
host thread (the six ints are compared on the way: a difference ends the run); for wtz_align_batch the share of ms_local and of the left / right
K-kext stages in the device time of the chain.  This process is the only one that opens the device; run it under `timeout -k 10 <seconds>`.

    python tools/ubench/kext_bench.py [--reads 64] [--len 10000] [--repeat 5] [--out FILE] [--no-host]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kextvec as kv  # noqa: E402
import localvec as lv  # noqa: E402
from smartdenovo_amd import hipabi  # noqa: E402

W, I, D, E, T = 800, -3, -3, -1, -100


def revcomp(s):
    return (3 - s[::-1]).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=64)
    ap.add_argument("--len", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of the library (the host emulation: to try the tool without a GPU)")
    a = ap.parse_args()
    rng = np.random.default_rng(20261019)
    seqs = []
    for _ in range(a.reads):
        arm = rng.integers(0, 4, int(rng.integers(1500, 3000))).astype(np.uint8)
        m = revcomp(arm).copy()
        hit = rng.random(m.size) < 0.12
        m[hit] = (m[hit] + 1 + rng.integers(0, 3, int(hit.sum()))) % 4
        pal = np.concatenate([arm, rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.uint8), m])
        left = int(rng.integers(200, a.len - pal.size - 200))
        seqs.append(np.concatenate([rng.integers(0, 4, left).astype(np.uint8), pal, rng.integers(0, 4, a.len - pal.size - left).astype(np.uint8)]))
    words, offs, lens = hipabi.pack_reads(seqs)
    ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=a.lib, pool_bytes=2 << 30)
    ids = np.arange(a.reads)
    pr = kv.chain_problems(ids, ids, np.ones(a.reads, dtype=np.int32), lens)
    loc = ctx.local_batch(pr, -D, -E, -I, -E)
    # the right extensions of those hits, as kswx_extend_core shapes them (target = the reverse complement of the read)
    ext, host = [], []
    for i in range(a.reads):
        qe, te, L = int(loc["qe"][i]) + 1, int(loc["te"][i]) + 1, int(lens[i])
        if loc["score"][i] <= 0 or qe == L or te == L:
            continue
        remq, remt = L - qe, L - te
        e = pr[i].copy()
        e["init_score"], e["W"] = int(loc["score"][i]), W
        rc = revcomp(seqs[i])
        if remt >= remq:
            e["q_from"], e["q_len"], e["t_from"], e["t_len"] = qe, remq, te, min(remt, remq + W)
            host.append((seqs[i][qe:qe + remq], rc[te:te + min(remt, remq + W)], int(loc["score"][i])))
        else:      # the read's own side is the rows: the roles change places (the gap costs are equal here)
            e["q_rev"], e["t_rev"] = 1, 0
            e["q_from"], e["q_len"], e["t_from"], e["t_len"] = te, remt, qe, min(remq, remt + W)
            host.append((rc[te:te + remt], seqs[i][qe:qe + min(remq, remt + W)], int(loc["score"][i])))
        ext.append(e)
    ext = np.array(ext, dtype=hipabi.DP_PROBLEM)
    gaps = (-D, -E, -I, -E)
    out = ctx.kext_batch(ext, *gaps, -T, -1)      # warm-up
    ms = []
    for _ in range(a.repeat):
        ctx.reset_counters()
        ctx.kext_batch(ext, *gaps, -T, -1)
        c = ctx.counters()
        ms.append(c.ms_kext)
        cells = int(c.cells_kext)
    med = statistics.median(ms)
    res = {"what": "wtz_kext_batch: right extensions (w = 800, end_bonus = 100, h0 = local score) of %d reads of %d bases against their reverse complement" % (a.reads, a.len),
           "problems": int(len(ext)), "cells": cells, "rows": int(out["rows"].sum()), "forms": sorted(set(int(f) for f in out["form_used"])), "repeat": a.repeat,
           "ms_kext": [round(x, 3) for x in ms], "ms_kext_median": round(med, 3), "ms_kext_min": round(min(ms), 3),
           "cells_per_s_median": round(cells / (med * 1e-3)) if med > 0 else None}
    if not a.no_host and kv.have_shim():
        t0 = time.perf_counter()
        ref = [kv.ref_extend(q, t, 2, -5, gaps, W, -T, -1, h0) for q, t, h0 in host]
        host_s = time.perf_counter() - t0
        if (np.array(ref, dtype=np.int64) != kv.six(out)).any():
            sys.exit("wtz_kext_batch differs from live ksw_extend2: nothing reported")
        res.update({"host_ksw_extend2_ms_one_thread": round(1e3 * host_s, 3), "host_over_device": round(1e3 * host_s / med, 2) if med > 0 else None})
    # the chain: device time per stage
    ctx.align_batch(pr, W, I, D, E, 0)
    ctx.align_batch(pr, W, I, D, E, T)
    st = []
    for _ in range(a.repeat):
        ctx.reset_counters()
        ctx.align_batch(pr, W, I, D, E, T)
        c = ctx.counters()
        st.append((c.ms_local, c.ms_kext))
    ml, mk = statistics.median(x[0] for x in st), statistics.median(x[1] for x in st)
    res["chain"] = {"what": "wtz_align_batch(w = 800, I = D = -3, E = -1, T = -100) on the same reads", "ms_local_median": round(ml, 3), "ms_kext_left_plus_right_median": round(mk, 3),
                    "share_local": round(ml / (ml + mk), 4), "share_kext": round(mk / (ml + mk), 4)}
    ctx.close()
    print(json.dumps(res))
    path = a.out or os.path.join(ROOT, "profiles", "kext_batch_%s.json" % datetime.date.today().isoformat())
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
