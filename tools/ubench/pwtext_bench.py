#!/usr/bin/env python3
"""Time wtz_pwtext_batch (K-pwtext, csrc/wtz_pwtext.h) on the pictures of a seeded `pairaln -a` block and write profiles/pwtext_<date>.json.
Not part of bench.py.

The set: --pairs pairs of about --len bases, a read and a copy of it mutated at --err (15 %), aligned by ONE wtz_alignx_batch call with pairaln's defaults
(W 800, O -3, E -1, T -100): its ms_local + ms_kext + ms_kglob are the alignment stages of the block.  The pictures are then rendered --repeat times after
one warm-up call, from the CIGARs that call returned and, as the worst case of the search, from CIGARs of the same number of columns made of runs of length 1
only.  Reported per kind: ms_pwtext (the library's HIP-event time around both passes, copies and host planning excluded), median and span; the bytes written;
bytes per second and their ratio to the 6.29 TB/s a streaming copy reaches on the MI355X; the wall time of the call (copies included); the renderer's share of the
block, ms_pwtext / (ms_local + ms_kext + ms_kglob + ms_pwtext).  The pictures are compared with tests/pwtextref.py on the way: a difference ends the run.
This process is the only one that opens the device; run it under `timeout -k 10 <seconds>`.

    python tools/ubench/pwtext_bench.py [--pairs 64] [--len 12000] [--err 0.15] [--repeat 7] [--out FILE] [--lib FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localvec as lv  # noqa: E402
import pwtextref as pw  # noqa: E402
from kglob_bench import mutated  # noqa: E402
from smartdenovo_amd import hipabi  # noqa: E402

HBM_STREAM = 6.29e12      # bytes per second, measured float4 copy on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--len", type=int, default=12000)
    ap.add_argument("--err", type=float, default=0.15)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (the host emulation: to try the tool without a GPU)")
    a = ap.parse_args()
    rng = np.random.default_rng(20261019)
    seqs = []
    for _ in range(a.pairs):
        q = rng.integers(0, 4, a.len + int(rng.integers(-300, 300))).astype(np.uint8)
        seqs += [q, mutated(rng, q, a.err)]
    words, offs, lens = hipabi.pack_reads(seqs)
    ctx = lv.make_context(words, offs, lens, 2, -5, lib_path=a.lib, pool_bytes=3 << 30)
    pr = lv.whole_read_problems(np.arange(0, 2 * a.pairs, 2), np.arange(1, 2 * a.pairs, 2), lens)
    ctx.alignx_batch(pr, 800, -3, -3, -1, -100)      # warm-up
    ctx.reset_counters()
    out, cigs = ctx.alignx_batch(pr, 800, -3, -3, -1, -100)
    c = ctx.counters()
    stages = {"ms_local": round(c.ms_local, 3), "ms_kext": round(c.ms_kext, 3), "ms_kglob": round(c.ms_kglob, 3)}
    ms_align = c.ms_local + c.ms_kext + c.ms_kglob
    assert out["found"].all()
    starts = [(int(o["qb"]), int(o["tb"])) for o in out]
    res = {"what": "wtz_pwtext_batch on the %d pictures of a pairaln -a block: pairs of about %d bases at %.0f %% divergence" % (a.pairs, a.len, 100 * a.err),
           "repeat": a.repeat, "alignment_stages_ms": stages, "hbm_stream_bytes_per_s": HBM_STREAM, "kinds": {}}
    unit = []
    for cg in cigs:      # the same consumption of both sides, runs of length 1 only: no two neighbours alike
        nq, nt = pw.consumed([int(w) for w in cg])
        u = []
        x = y = 0
        while x < nq or y < nt:
            last = u[-1] & 15 if u else 3
            op = 0 if (last != 0 and x < nq and y < nt) else (1 if (x < nq and last != 1) else (2 if (y < nt and last != 2) else (1 if x < nq else 2)))
            u.append(16 | op)
            x += op != 2
            y += op != 1
        unit.append(np.array(u, dtype=np.uint32))
    for kind, lists in (("alignx_cigars", cigs), ("unit_runs", unit)):
        flat = np.concatenate(lists).astype(np.uint32)
        at = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
        slices = [(int(at[i]), len(lists[i])) for i in range(a.pairs)]
        o, blob = ctx.pwtext_batch(pr, starts, slices, flat)      # warm-up
        want = pw.expected(seqs, pr, starts, slices, flat)
        if pw.split(o, blob) != want:
            sys.exit("wtz_pwtext_batch differs from the restatement (%s): nothing reported" % kind)
        ms, wall = [], []
        for _ in range(a.repeat):
            ctx.reset_counters()
            t0 = time.perf_counter()
            ctx.pwtext_batch(pr, starts, slices, flat)
            wall.append(1e3 * (time.perf_counter() - t0))
            cc = ctx.counters()
            ms.append(cc.ms_pwtext)
            nbytes = int(cc.bytes_pwtext)
        med = statistics.median(ms)
        res["kinds"][kind] = {"operations": int(flat.size), "operations_per_alignment_max": int(max(len(x) for x in lists)), "columns_max": int(o["cols"].max()),
                              "bytes_written": nbytes, "ms_pwtext": [round(x, 4) for x in ms], "ms_pwtext_median": round(med, 4),
                              "ms_pwtext_span": [round(min(ms), 4), round(max(ms), 4)],
                              "gbytes_per_s_median": round(nbytes / (med * 1e-3) / 1e9, 2) if med > 0 else None,
                              "share_of_hbm_stream": round(nbytes / (med * 1e-3) / HBM_STREAM, 5) if med > 0 else None,
                              "wall_ms_call_median": round(statistics.median(wall), 3),
                              "share_of_block": round(med / (ms_align + med), 5)}
    ctx.close()
    print(json.dumps(res))
    path = a.out or os.path.join(ROOT, "profiles", "pwtext_%s.json" % datetime.date.today().isoformat())
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
