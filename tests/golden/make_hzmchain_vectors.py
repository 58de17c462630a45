"""Generator of tests/golden/hzmchain_vectors.npz: align_hzmaux (hzm_aln.h:1684-1775) with beg / end set AND HZM_FAST_WINDOW_KMER_CHAINING = 0, as the reference's wtmsa
and wtcns run it (wtmsa.c:617, wtcns.c:806): every window of potential_paired_kmers_windows is built by chaining_hzmps (hzm_aln.h:351-408, 544-561).  The device
form is wtz_set_window_chaining(ctx, 0) (K_pair_chain).

The recorder is the driver of make_hzmreg_vectors.py (its text, imported) plus the line that sets the flag - from the command line, so that the one compile also
gives the flag-1 run of the same calls - and the lines that write the windows the call leaves in aux->windows.  Compiled into a temporary directory outside the
repository with the flags of oracle/Makefile (REFFLAGS, read from that file); nothing of the compile is kept.

Layouts: the eight of make_hzmreg_vectors.py (same seed: wtmsa's defaults with I = D = O, O in {-2, -3}) and two with a TANDEM duplicate - 150-300 bases repeated
300-500 bases further on in the backbone, i.e. inside one 800-base window - whose first six Y reads lie across both copies: one z-mer of the read then matches at
two backbone positions and a scan sees equal off2 values, the case in which the order inside a tie group is observable through chaining_hzmps's strict comparisons.

Recorded per call: the return value, the ten kswx_t fields, the CIGAR words; beg[2] / end[2] of the windows that are not `closed` after the call where the
reference got past hzm_aln.h:1699 (has_win; a call that returned 0 got there iff chaining_wtseedv over the windows it left - idempotent - reaches zovl);
differs_from_fast = the flag-1 run of the same driver on the same call gives another record or CIGAR; tie = by hzmregvec.model_matches two matches of the call
have equal off2 and off1 less than zwin apart.
Nothing is written unless: at least 50 calls with an interval, at most a quarter of them without a hit, at least three quarters of them with differs_from_fast,
at least 4 calls with tie.

    python tests/golden/make_hzmchain_vectors.py"""
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
import make_hzmreg_vectors as reg  # noqa: E402
from smartdenovo_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "hzmchain_vectors.npz")
MIN_SM = reg.MIN_SM

SET_FLAG = "\tHZM_FAST_WINDOW_KMER_CHAINING = atoi(argv[3]);\n"
WINDOWS = r"""
		{	/* the windows left behind, where the call got past hzm_aln.h:1699: -1, or their number and beg[2], end[2] of each */
			int32_t nw = -1; uint32_t w;
			if(aux->windows->size && (r[0] || chaining_wtseedv(0, 0, 0, aux->windows, 0, aux->windows->size, aux->mem_cache[0], aux->W) >= (int)aux->zovl)){
				for(nw = 0, w = 0; w < aux->windows->size; w++) if(!aux->windows->buffer[w].closed) nw++;
			}
			fwrite(&nw, 4, 1, out);
			for(w = 0; nw > 0 && w < aux->windows->size; w++) if(!aux->windows->buffer[w].closed){ fwrite(aux->windows->buffer[w].beg, 4, 2, out); fwrite(aux->windows->buffer[w].end, 4, 2, out); }
		}
"""


def driver():
    """make_hzmreg_vectors.DRIVER + the flag + the windows"""
    head = "int main(int argc, char **argv){\n"
    tail = "\t\tif(r[0]) fwrite(aux->cigars->buffer, 4, aux->cigars->size, out);\n"
    assert reg.DRIVER.count(head) == 1 and reg.DRIVER.count(tail) == 1
    return reg.DRIVER.replace(head, head + SET_FLAG).replace(tail, tail + WINDOWS)


def tandem_layouts():
    rng = np.random.default_rng(20261022)
    lays = []
    for k in range(2):
        glen = int(rng.integers(8000, 12001))
        G = synth.random_genome(glen, rng)
        ln, dist = int(rng.integers(150, 301)), int(rng.integers(300, 501))
        a = int(rng.integers(2500, glen - 2500 - dist - ln))
        G[a + dist:a + dist + ln] = G[a:a + ln]
        ny = 8
        cases = []
        for i in range(ny):
            rl = int(rng.integers(1500, 3001))
            if i < 6:                                                      # across both copies
                b = a - int(rng.integers(200, rl - dist - ln - 200))
            else:
                b = int(rng.integers(0, glen - rl + 1))
            b = max(0, min(glen - rl, b))
            rd = np.ascontiguousarray(synth._mutate(G[b:b + rl], 0.15, rng))
            cases.append((rd, b + int(rng.integers(-60, 61)), b + rl + int(rng.integers(-60, 61)), 1))
        for _ in range(2):                                                 # N reads: the whole form
            rl = int(rng.integers(1500, 3001)); b = int(rng.integers(0, glen - rl + 1))
            cases.append((np.ascontiguousarray(synth._mutate(G[b:b + rl], 0.15, rng)), 0, -1, 0))
        lays.append((np.ascontiguousarray(G), reg.prm(-3 if k % 2 == 0 else -2), cases))
    return lays


def parse(raw, n):
    rec = np.zeros((n, 11), dtype=np.int32); cig = []; wins = []; has_win = np.zeros(n, dtype=np.uint8)
    at = 0
    for k in range(n):
        r = raw[at:at + 12]; at += 12
        rec[k] = r[:11]
        words = raw[at:at + int(r[11])].astype(np.uint32) if r[0] else np.zeros(0, dtype=np.uint32)
        at += words.size
        nw = int(raw[at]); at += 1
        has_win[k] = nw >= 0
        w = raw[at:at + 4 * max(nw, 0)].reshape(-1, 4).copy(); at += w.size
        cig.append(words); wins.append(w)
    assert at == raw.size
    return rec, cig, wins, has_win


def main():
    import hzmregvec as hv
    flags = None
    for line in open(os.path.join(ROOT, "oracle", "Makefile")):
        m = re.match(r"REFFLAGS\s*=\s*(.*)", line)
        if m:
            flags = m.group(1).split()
    assert flags, "REFFLAGS not found in oracle/Makefile"
    lays = reg.make_layouts() + tandem_layouts()
    flat = [(li, G, p, rd, b, e, y) for li, (G, p, cases) in enumerate(lays) for rd, b, e, y in cases]
    td = tempfile.mkdtemp(prefix="hzmchain_")
    assert not os.path.abspath(td).startswith(ROOT + os.sep)
    try:
        src, exe, fin = (os.path.join(td, f) for f in ("driver.c", "driver", "in.bin"))
        open(src, "w").write(driver())
        subprocess.run(["gcc"] + flags + ["-iquote", REF, "-o", exe, src, os.path.join(REF, "ksw.c"), "-lm"], check=True)
        with open(fin, "wb") as f:
            f.write(np.int32(len(flat)).tobytes())
            for _, G, p, rd, b, e, _ in flat:
                f.write(np.array(p, dtype=np.int32).tobytes() + np.float32(MIN_SM).tobytes() + np.array([G.size, rd.size, b, e], dtype=np.int32).tobytes() + G.tobytes() + rd.tobytes())
        runs = []
        for flag in ("0", "1"):
            fout = os.path.join(td, "out%s.bin" % flag)
            subprocess.run([exe, fin, fout, flag], check=True)
            runs.append(parse(np.fromfile(fout, dtype=np.int32), len(flat)))
    finally:
        shutil.rmtree(td)
    (rec, cig, wins, has_win), (rec1, cig1, _, _) = runs
    n = len(flat)
    differs = np.array([int(not np.array_equal(rec[k], rec1[k]) or not np.array_equal(cig[k], cig1[k])) for k in range(n)], dtype=np.uint8)
    tie = np.zeros(n, dtype=np.uint8)
    for k, (_, G, p, rd, b, e, _) in enumerate(flat):
        by2 = {}
        for o1, o2, _, _ in hv.model_matches(G, rd, p[0], p[1], p[5], p[6], b, e):
            by2.setdefault(o2, []).append(o1)
        tie[k] = int(any(len(v) > 1 and min(np.diff(sorted(v))) < p[2] for v in by2.values()))
    is_y = np.array([y for *_, y in flat], dtype=np.uint8)
    layout = np.array([c[0] for c in flat], dtype=np.int32)
    for name, sel in (("the eight layouts of make_hzmreg_vectors.py", layout < 8), ("the two tandem layouts", layout >= 8), ("all", layout >= 0)):
        y = sel & (is_y == 1)
        print("%s: %d calls, %d with an interval (%d without a hit, %d differ from the flag-1 run), %d with off2 ties, %d with windows recorded" %
              (name, int(sel.sum()), int(y.sum()), int((y & (rec[:, 0] == 0)).sum()), int((y & (differs == 1)).sum()), int((sel & (tie == 1)).sum()), int((sel & (has_win == 1)).sum())))
    y = is_y == 1
    nreg, nfail, ndiff, ntie = int(y.sum()), int((y & (rec[:, 0] == 0)).sum()), int((y & (differs == 1)).sum()), int(tie.sum())
    assert nreg >= 50 and nfail * 4 <= nreg and ndiff * 4 >= 3 * nreg and ntie >= 4, "the conditions on the committed file are not met: nothing written"
    rd_off = np.zeros(n + 1, dtype=np.int64); rd_off[1:] = np.cumsum([c[3].size for c in flat])
    bb_off = np.zeros(len(lays) + 1, dtype=np.int64); bb_off[1:] = np.cumsum([G.size for G, _, _ in lays])
    cig_off = np.zeros(n + 1, dtype=np.int64); cig_off[1:] = np.cumsum([c.size for c in cig])
    win_off = np.zeros(n + 1, dtype=np.int64); win_off[1:] = np.cumsum([w.shape[0] for w in wins])
    np.savez_compressed(OUT, backbones=np.concatenate([G for G, _, _ in lays]), bb_off=bb_off, prm=np.array([p for _, p, _ in lays], dtype=np.int32), min_sm=np.float32(MIN_SM),
                        reads=np.concatenate([c[3] for c in flat]), rd_off=rd_off, layout=layout,
                        beg=np.array([c[4] for c in flat], dtype=np.int32), end=np.array([c[5] for c in flat], dtype=np.int32), is_region=is_y,
                        rec=rec, cigar=np.concatenate(cig), cig_off=cig_off, has_win=has_win, win=np.concatenate(wins).astype(np.int32), win_off=win_off,
                        differs_from_fast=differs, tie=tie)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
