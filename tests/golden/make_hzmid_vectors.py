"""Generator of tests/golden/hzmid_vectors.npz: align_hzmaux (hzm_aln.h:1684-1775) at wtmsa's REAL defaults - HZM_FAST_WINDOW_KMER_CHAINING = 0 (wtmsa.c:617) and
separate gap-open costs I = -2, D = -3 (wtmsa.c:633-634) - recorded from the reference's own compiled routine.  The device form is
wtz_set_window_chaining(ctx, 0) + wtz_set_gap_open(ctx, -2, -3).

The recorder is the driver text of make_hzmreg_vectors.py with the flag line of make_hzmchain_vectors.py (make_hzmchain_vectors.driver(), imported), run with the
flag at 0.  Compiled into a temporary directory outside the repository with the flags of oracle/Makefile (REFFLAGS, read from that file); nothing of the compile
is kept.

Layouts: the even ones of make_hzmreg_vectors.py (0, 2, 4, 6: two plain backbones, two with an exact duplicate; same seed, so the same backbones, reads and
intervals as in hzmreg_vectors.npz / hzmchain_vectors.npz, where they are recorded at I = D = -3) - interval calls and whole-read (0, -1) calls both.  Every call
is recorded three times by the one compiled driver: at (I, D) = (-2, -3) - the record -, at (-2, -2) and at (-3, -3):
    differs_m2 / differs_m3 = the record or the CIGAR at (-2, -3) differs from the one at (-2, -2) / (-3, -3);   differs = both.
Nothing is written unless: at least 30 calls, at most a quarter of the interval calls without a hit, at least half of the hits with differs.

    python tests/golden/make_hzmid_vectors.py"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_hzmchain_vectors as chain  # noqa: E402
import make_hzmreg_vectors as reg  # noqa: E402

OUT = os.path.join(HERE, "hzmid_vectors.npz")
MIN_SM = reg.MIN_SM
LAYOUTS = (0, 2, 4, 6)          # of make_hzmreg_vectors.make_layouts(): recorded at I = D = -3 in hzmchain_vectors.npz
COSTS = ((-2, -3), (-2, -2), (-3, -3))


def prm(I, D):
    p = reg.prm(I)
    assert p[13] == I and p[14] == I
    p[14] = D
    return p


def parse(raw, n):
    rec = np.zeros((n, 11), dtype=np.int32); cig = []
    at = 0
    for k in range(n):
        r = raw[at:at + 12]; at += 12
        rec[k] = r[:11]
        words = raw[at:at + int(r[11])].astype(np.uint32) if r[0] else np.zeros(0, dtype=np.uint32)
        at += words.size
        cig.append(words)
    assert at == raw.size
    return rec, cig


def main():
    flags = None
    for line in open(os.path.join(ROOT, "oracle", "Makefile")):
        m = re.match(r"REFFLAGS\s*=\s*(.*)", line)
        if m:
            flags = m.group(1).split()
    assert flags, "REFFLAGS not found in oracle/Makefile"
    all_lays = reg.make_layouts()
    lays = [all_lays[i] for i in LAYOUTS]
    assert all(p[13] == -3 and p[14] == -3 for _, p, _ in lays)
    flat = [(li, G, rd, b, e, y) for li, (G, _, cases) in enumerate(lays) for rd, b, e, y in cases]
    # the driver of make_hzmchain_vectors.py also writes the windows a call leaves behind; this file does not record them, so that block is taken out again
    drv = chain.driver()
    assert drv.count(chain.WINDOWS) == 1
    drv = drv.replace(chain.WINDOWS, "")
    td = tempfile.mkdtemp(prefix="hzmid_")
    assert not os.path.abspath(td).startswith(ROOT + os.sep)
    try:
        src, exe = os.path.join(td, "driver.c"), os.path.join(td, "driver")
        open(src, "w").write(drv)
        subprocess.run(["gcc"] + flags + ["-iquote", REF, "-o", exe, src, os.path.join(REF, "ksw.c"), "-lm"], check=True)
        runs = []
        for I, D in COSTS:
            fin, fout = os.path.join(td, "in%d%d.bin" % (I, D)), os.path.join(td, "out%d%d.bin" % (I, D))
            p = np.array(prm(I, D), dtype=np.int32)
            with open(fin, "wb") as f:
                f.write(np.int32(len(flat)).tobytes())
                for _, G, rd, b, e, _ in flat:
                    f.write(p.tobytes() + np.float32(MIN_SM).tobytes() + np.array([G.size, rd.size, b, e], dtype=np.int32).tobytes() + G.tobytes() + rd.tobytes())
            subprocess.run([exe, fin, fout, "0"], check=True)
            runs.append(parse(np.fromfile(fout, dtype=np.int32), len(flat)))
    finally:
        shutil.rmtree(td)
    (rec, cig), (rec2, cig2), (rec3, cig3) = runs
    n = len(flat)
    d2 = np.array([int(not np.array_equal(rec[k], rec2[k]) or not np.array_equal(cig[k], cig2[k])) for k in range(n)], dtype=np.uint8)
    d3 = np.array([int(not np.array_equal(rec[k], rec3[k]) or not np.array_equal(cig[k], cig3[k])) for k in range(n)], dtype=np.uint8)
    differs = d2 & d3
    is_y = np.array([y for *_, y in flat], dtype=np.uint8)
    hit = rec[:, 0] != 0
    nreg, nfail, nhit, ndiff = int(is_y.sum()), int(((is_y == 1) & ~hit).sum()), int(hit.sum()), int((hit & (differs == 1)).sum())
    print("%d calls (%d with an interval, %d of them without a hit), %d hits: %d differ from (-2, -2), %d from (-3, -3), %d from both" %
          (n, nreg, nfail, nhit, int((hit & (d2 == 1)).sum()), int((hit & (d3 == 1)).sum()), ndiff))
    assert n >= 30 and nfail * 4 <= nreg and ndiff * 2 >= nhit, "the conditions on the committed file are not met: nothing written"
    # the (-3, -3) run is what hzmchain_vectors.npz holds for these layouts: the two generators must agree on the calls
    ch = np.load(os.path.join(HERE, "hzmchain_vectors.npz"))
    sel = np.nonzero(np.isin(ch["layout"], LAYOUTS))[0]
    assert sel.size == n and np.array_equal(ch["rec"][sel], rec3), "the (-3, -3) run is not the committed hzmchain record of the same calls"
    rd_off = np.zeros(n + 1, dtype=np.int64); rd_off[1:] = np.cumsum([c[2].size for c in flat])
    bb_off = np.zeros(len(lays) + 1, dtype=np.int64); bb_off[1:] = np.cumsum([G.size for G, _, _ in lays])
    cig_off = np.zeros(n + 1, dtype=np.int64); cig_off[1:] = np.cumsum([c.size for c in cig])
    np.savez_compressed(OUT, backbones=np.concatenate([G for G, _, _ in lays]), bb_off=bb_off, prm=np.array([prm(*COSTS[0]) for _ in lays], dtype=np.int32), min_sm=np.float32(MIN_SM),
                        chain_layout=np.array(LAYOUTS, dtype=np.int32), reads=np.concatenate([c[2] for c in flat]), rd_off=rd_off, layout=np.array([c[0] for c in flat], dtype=np.int32),
                        beg=np.array([c[3] for c in flat], dtype=np.int32), end=np.array([c[4] for c in flat], dtype=np.int32), is_region=is_y,
                        rec=rec, cigar=np.concatenate(cig), cig_off=cig_off, differs=differs, differs_m2=d2, differs_m3=d3)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
