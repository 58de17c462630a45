#!/usr/bin/env python3
"""Time wtz_global_batch (K-glob, csrc/wtz_sw_kglob.h) on a seeded set of wtcyc-shaped rectangles and write profiles/kglob_batch_<date>.json.
Not part of bench.py.

The set: --reads pairs of about --len x --len bases (a read and a 12 %-mutated copy of it, the lengths differing by less than 150), at the band widths
w = 200 / 400 / 800 (401 / 801 / 1 601 band slots: forms 8 / 16 / 32), gap costs (3, 1, 3, 1): what kswx_gen_cigar_core2 hands ksw_global2 from wtcyc.

Reported per width: ms_kglob (the library's HIP-event time around the K-glob launches: copies and host planning excluded) of --repeat calls after one
warm-up call, median and span; cells per second; the DP / traceback split from the wavefronts' own clocks (ticks_kglob_dp / ticks_kglob_tb: the share of
the traceback with its counting in the time a wavefront spends on a problem); the same problems through the parent's own forms of wtz_test_dp
(WTZ_DP_GLOBAL, form 33, and form 32 where its envelope of about 4 000 query bases covers them: wall time of the call, copies included, next to the wall time of the wtz_global_batch call; a form whose envelope does not
cover the problems reports the library's error text); where oracle/_ref/libref_shim.so is present, one host thread of the reference's ksw_global2 on the
same problems (scores and CIGARs are compared on the way: a difference ends the run).  This process is the only one that opens the device; run it under
`timeout -k 10 <seconds>`.

    python tools/ubench/kglob_bench.py [--reads 64] [--len 12000] [--repeat 5] [--out FILE] [--no-host] [--lib FILE]
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
import kglobvec as gv  # noqa: E402
import localvec as lv  # noqa: E402
from smartdenovo_amd import hipabi  # noqa: E402

GAPS = (3, 1, 3, 1)
WIDTHS = (200, 400, 800)


def mutated(rng, s, rate):
    out, i = [], 0
    kinds = rng.random(len(s))
    while i < len(s):
        r = kinds[i]
        if r < rate * 0.3:
            out.append(int(rng.integers(0, 4)))
        elif r < rate * 0.6:
            i += 1
            continue
        elif r < rate:
            out.append((int(s[i]) + 1 + int(rng.integers(0, 3))) % 4)
            i += 1
            continue
        out.append(int(s[i]))
        i += 1
    return np.array(out, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=64)
    ap.add_argument("--len", type=int, default=12000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of the library (the host emulation: to try the tool without a GPU)")
    a = ap.parse_args()
    rng = np.random.default_rng(20261019)
    seqs = []
    for _ in range(a.reads):
        q = rng.integers(0, 4, a.len + int(rng.integers(-300, 300))).astype(np.uint8)
        t = mutated(rng, q, 0.12)
        assert abs(len(q) - len(t)) < 150
        seqs += [q, t]
    words, offs, lens = hipabi.pack_reads(seqs)
    ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=a.lib, pool_bytes=3 << 30)
    base = lv.whole_read_problems(np.arange(0, 2 * a.reads, 2), np.arange(1, 2 * a.reads, 2), lens)
    res = {"what": "wtz_global_batch on %d rectangles of about %d x %d bases (12 %% divergence), gap costs %s" % (a.reads, a.len, a.len, list(GAPS)),
           "repeat": a.repeat, "widths": {}}
    scores = {}
    for w in WIDTHS:
        pr = base.copy()
        pr["W"] = w
        out, cigs = ctx.global_batch(pr, *GAPS)      # warm-up
        ms, wall, dp, tb = [], [], [], []
        for _ in range(a.repeat):
            ctx.reset_counters()
            t0 = time.perf_counter()
            ctx.global_batch(pr, *GAPS)
            wall.append(1e3 * (time.perf_counter() - t0))
            c = ctx.counters()
            ms.append(c.ms_kglob)
            dp.append(int(c.ticks_kglob_dp))
            tb.append(int(c.ticks_kglob_tb))
            cells = int(c.cells_kglob)
        med = statistics.median(ms)
        r = {"slots": 2 * w + 1, "forms": sorted(set(int(f) for f in out["form_used"])), "cells": cells,
             "ms_kglob": [round(x, 3) for x in ms], "ms_kglob_median": round(med, 3), "ms_kglob_span": [round(min(ms), 3), round(max(ms), 3)],
             "gcells_per_s_median": round(cells / (med * 1e-3) / 1e9, 3) if med > 0 else None,
             "wall_ms_call_median": round(statistics.median(wall), 3),
             "ticks_dp_median": int(statistics.median(dp)), "ticks_tb_median": int(statistics.median(tb)),
             "traceback_share_of_wave_time": round(statistics.median(tb) / (statistics.median(tb) + statistics.median(dp)), 4) if dp[0] + tb[0] else None}
        if not a.no_host and gv.have_shim():
            t0 = time.perf_counter()
            ref = [gv.ref_global(seqs[2 * i], seqs[2 * i + 1], 2, -5, GAPS, w) for i in range(a.reads)]
            host_s = time.perf_counter() - t0
            for i, (sc, cg) in enumerate(ref):
                if sc != int(out["score"][i]) or not np.array_equal(cg, cigs[i]):
                    sys.exit("wtz_global_batch differs from live ksw_global2 on problem %d at w = %d: nothing reported" % (i, w))
            r.update({"host_ksw_global2_ms_one_thread": round(1e3 * host_s, 3), "host_over_device": round(1e3 * host_s / med, 2) if med > 0 else None})
        res["widths"][str(w)] = r
        scores[w] = out["score"].copy()
    print(json.dumps(res), flush=True)      # what K-glob itself gave, before the parent's forms run
    for w in WIDTHS:
        pr = base.copy()
        pr["W"] = w
        r, wall_med = res["widths"][str(w)], res["widths"][str(w)]["wall_ms_call_median"]
        # the parent's own forms of ksw_global2 (gap costs from the params: O = 3, E = 1 by default, the same costs)
        # form 32 keeps the query words in the LDS slice of the narrow launch (about 4 000 query bases): rectangles of this size are outside its envelope
        r["test_dp_form_32"] = {"error": "not run: %d query bases are outside the envelope of form 32" % a.len} if a.len > 3900 else None
        for form in ((33,) if a.len > 3900 else (32, 33)):
            try:
                ctx.test_dp(hipabi.DP_GLOBAL, form, pr, cigar_cap=1 << 24)      # warm-up
                tw = []
                for _ in range(a.repeat):
                    t0 = time.perf_counter()
                    o2, _ = ctx.test_dp(hipabi.DP_GLOBAL, form, pr, cigar_cap=1 << 24)
                    tw.append(1e3 * (time.perf_counter() - t0))
                if (o2["score"] != scores[w]).any():
                    sys.exit("form %d of wtz_test_dp differs from wtz_global_batch in the score: nothing reported" % form)
                r["test_dp_form_%d" % form] = {"wall_ms_call": [round(x, 3) for x in tw], "wall_ms_call_median": round(statistics.median(tw), 3),
                                               "over_global_batch_wall": round(statistics.median(tw) / wall_med, 2)}
            except RuntimeError as e:
                r["test_dp_form_%d" % form] = {"error": str(e)[:200]}
    ctx.close()
    print(json.dumps(res))
    path = a.out or os.path.join(ROOT, "profiles", "kglob_batch_%s.json" % datetime.date.today().isoformat())
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
