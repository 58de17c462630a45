#!/usr/bin/env python3
"""Time wtz_local_batch (K-local, csrc/wtz_sw_local.h) on tests/golden/local_vectors.npz and write profiles/local_batch_<date>.json.

Device time = the library's HIP-event time around the kernel (counters.ms_local: copies and host planning excluded), cells = rows x columns of
both passes as executed (counters.cells_local).  Reported: GCUPS (1e9 cell updates per second), the share of the VALU roof of DESIGN.md section 6
(cells x 13 ops / time / 78.6 Tint32op/s, 13 = the VALU instructions of one cell in the kernel's disassembly, 215 per 16-cell row; the packed 16-bit rate is twice that, so the share of it is half), the wall time of the calls, and - where
oracle/_ref/libref_shim.so is present - the reference's ksw_align2 on the same problems on one host thread, with the ratio of the two times.
Not part of bench.py.

With --fill N (default 32) a second figure is taken on the set WITHOUT its two 17 000-base pairs, every problem N times in the call: enough
wavefronts to occupy the device, which the plain set (318 problems, two of them more than half of the cells) does not.

    python tools/local_batch_time.py [--repeat 5] [--fill 32] [--out FILE] [--no-host]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import localvec as lv  # noqa: E402

ROOF_INT32_OPS = 78.6e12
OPS_PER_CELL = 13              # VALU instructions per cell of wtz_kernel_local (215 per 16-cell row by the disassembly; DESIGN.md section 3, K-local)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--fill", type=int, default=32)
    a = ap.parse_args()
    v = lv.load_vectors()
    M, X = int(v["M"]), int(v["X"])
    pr = lv.whole_read_problems(v["q_read"], v["t_read"], v["lens"])
    ctx = lv.make_context(v["words"], v["offs"], v["lens"], M, X, pool_bytes=2 << 30)
    out = lv.run_by_gap(ctx, pr, v["gap"])      # warm-up, and the check that what is timed is right
    if (lv.five(out) != v["expect"]).any():
        sys.exit("wtz_local_batch differs from the reference vectors: nothing timed")
    ms, wall, cells = [], [], 0
    for _ in range(a.repeat):
        ctx.reset_counters()
        t0 = time.perf_counter()
        lv.run_by_gap(ctx, pr, v["gap"])
        wall.append(time.perf_counter() - t0)
        c = ctx.counters()
        ms.append(c.ms_local)
        cells = int(c.cells_local)
    fill = None
    if a.fill > 0:
        keep = np.array([i for i, n in enumerate(v["names"]) if not str(n).startswith("identical_17000")])
        fpr, fgap = np.tile(pr[keep], a.fill), np.tile(v["gap"][keep], a.fill)
        lv.run_by_gap(ctx, fpr, fgap)
        fms = []
        for _ in range(a.repeat):
            ctx.reset_counters()
            lv.run_by_gap(ctx, fpr, fgap)
            c = ctx.counters()
            fms.append(c.ms_local)
            fcells = int(c.cells_local)
        fmed = statistics.median(fms)
        fill = {"what": "the set without the two 17 000-base pairs, every problem %d times per call" % a.fill, "problems": int(len(fpr)), "cells": fcells,
                "kernel_ms": [round(x, 3) for x in fms], "kernel_ms_median": round(fmed, 3), "gcups_median": round(fcells / fmed / 1e6, 2),
                "roof_share_int32_median": round(fcells * OPS_PER_CELL / (fmed * 1e-3) / ROOF_INT32_OPS, 5),
                "roof_share_packed_int16_median": round(fcells * OPS_PER_CELL / (fmed * 1e-3) / (2 * ROOF_INT32_OPS), 5)}
    ctx.close()
    best, med = min(ms), statistics.median(ms)
    res = {
        "what": "wtz_local_batch on tests/golden/local_vectors.npz (one call per gap-cost setting)",
        "problems": int(len(pr)), "cells": cells, "repeat": a.repeat,
        "kernel_ms": [round(x, 3) for x in ms], "kernel_ms_min": round(best, 3), "kernel_ms_median": round(med, 3),
        "wall_ms_median": round(1e3 * statistics.median(wall), 3),
        "gcups_best": round(cells / best / 1e6, 2), "gcups_median": round(cells / med / 1e6, 2),
        "roof": "cells x %d ops / kernel time / %.1f Tint32op/s (DESIGN.md section 6)" % (OPS_PER_CELL, ROOF_INT32_OPS / 1e12),
        "roof_share_int32_median": round(cells * OPS_PER_CELL / (med * 1e-3) / ROOF_INT32_OPS, 5),
        "roof_share_packed_int16_median": round(cells * OPS_PER_CELL / (med * 1e-3) / (2 * ROOF_INT32_OPS), 5),
        "note": "the two 17 000 x 17 000 pairs are 57 % of the cells and each runs on ONE wavefront: the set measures the tail of its largest problems, not a full device",
    }
    if fill:
        res["filled_device"] = fill
    if lv.have_shim() and not a.no_host:
        reads = lv.unpack_reads(v["words"], v["offs"], v["lens"])
        t0 = time.perf_counter()
        for q, t, g in zip(v["q_read"], v["t_read"], v["gap"]):
            lv.ref_align(reads[int(q)], reads[int(t)], M, X, lv.GAPS[int(g)])
        host = time.perf_counter() - t0
        res["host_reference_s"] = round(host, 3)
        res["host_reference"] = "ksw_align2 (SSE2, 16-bit lanes) through oracle/_ref/libref_shim.so, one thread, same problems"
        res["host_over_device_kernel_median"] = round(host / (med * 1e-3), 2)
        res["host_over_device_wall_median"] = round(host / statistics.median(wall), 2)
        if fill:      # the host's rate on the plain set against the device's rate on the filled one (cells per second; the host's cells are the first pass's rows x columns plus the second pass as bounded here)
            res["filled_device"]["gcups_over_host_thread_gcups"] = round(fill["gcups_median"] / (cells / host / 1e9), 1)
    path = a.out or os.path.join(ROOT, "profiles", "local_batch_%s.json" % datetime.date.today().isoformat())
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
