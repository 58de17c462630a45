"""Generator of tests/golden/hzmreg_vectors.npz: align_hzmaux (hzm_aln.h:1684-1775) with beg / end set, recorded from the reference's own compiled routine.

The recorder is NOT the reference's wtmsa, although that is the program that makes these calls (wtmsa.c:448-477): its main sets
HZM_FAST_WINDOW_KMER_CHAINING = 0 (wtmsa.c:617), which sends every align_hzmaux of that process through the chaining_hzmps branch of
potential_paired_kmers_windows (hzm_aln.h:544-); the device has the branch of the default, 1 (hzm_aln.h:488-543: wtzmo, wtgbo, oracle/ref_shim.c).  So the
recorder is the few lines of DRIVER below: they include hzm_aln.h where it lies (REF, default /root/reference), leave the flag alone and call
align_hzmaux(aux, 0, read, NULL, len, beg, end, 0, min_sm) per case.  Compiled into a temporary directory outside the repository with the flags of
oracle/Makefile (REFFLAGS, read from that file); nothing of the compile is kept.

Layouts (smartdenovo_amd/synth.py: iid genome, PacBio-shape errors at 15 %): a backbone of 8-20 kb, 6-10 Y reads of 1.5-4 kb tiling it, each with the interval
of the backbone it was drawn from moved by up to 60 bases at either end (what wtmsa.c:357-369 derives from pairwise hits is an estimate of just that), and 2 N
reads with the whole form's (0, -1) (wtmsa.c:472-475).  Four of the layouts are drawn from a genome with an exact duplicate of 1.5-2 kb 3-5 kb further on; their
Y reads lie inside one copy (half of them in the first, half in the second) or across an edge of one.  Parameters: wtmsa's defaults (wtmsa.c:618-639, -Z 100 of
init_hzmaux) with I = D = O, O = -3 for the even layouts and -2 for the odd ones (the device has one gap-open cost).
What reaching 4 `differs_from_whole` cases needed: nothing beyond the above - a read inside one copy of the duplicate is enough, the whole form puts it into either
copy or chains across both.

Every case also goes through the whole form live (ref_align_hzmaux of oracle/_ref/libref_shim.so, `make -C oracle ref`): differs_from_whole = the record differs.
Nothing is written unless: at least 40 cases with an interval, at most a quarter of them without a hit, at least 4 that differ from the whole form.

    python tests/golden/make_hzmreg_vectors.py"""
import ctypes as C
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
from smartdenovo_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "hzmreg_vectors.npz")
MIN_SM = 0.5


def prm(O):
    """zsize hz zwin zstep zovl zmax zvar w W ew rw M X I D E T"""
    return [10, 1, 800, 400, 200, 100, 2, 50, 3200, 800, 8, 2, -5, O, O, -1, -10]


DRIVER = r"""
#include "hzm_aln.h"
/* in: n, then per case 17 x int32 prm, float min_sm, int32 tlen, qlen, beg, end, the target's and the read's base codes.  out: per case int32 found, the ten
 * kswx_t fields, the number of CIGAR words and the words */
int main(int argc, char **argv){
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	int32_t n, k, i, h[4], p[17], r[12]; float min_sm;
	if(!in || !out || fread(&n, 4, 1, in) != 1) return 2;
	for(k = 0; k < n; k++){
		HZMAux *aux = init_hzmaux();
		if(fread(p, 4, 17, in) != 17 || fread(&min_sm, 4, 1, in) != 1 || fread(h, 4, 4, in) != 4) return 3;
		uint8_t *t = malloc(h[0] + 1), *q = malloc(h[1] + 1);
		if(fread(t, 1, h[0], in) != (size_t)h[0] || fread(q, 1, h[1], in) != (size_t)h[1]) return 4;
		aux->zsize = p[0]; aux->hz = p[1]; aux->zwin = p[2]; aux->zstep = p[3]; aux->zovl = p[4]; aux->zmax = p[5]; aux->zvar = p[6];
		aux->w = p[7]; aux->W = p[8]; aux->ew = p[9]; aux->rw = p[10]; aux->M = p[11]; aux->X = p[12]; aux->I = p[13]; aux->D = p[14]; aux->E = p[15]; aux->T = p[16];
		aux->has_alignment = 0;
		reset_hzmaux(aux);
		for(i = 0; i < h[0]; i++) add_tseq_hzmaux(aux, t[i]);
		ready_hzmaux(aux);
		memset(r, 0, sizeof r);
		r[0] = align_hzmaux(aux, 0, q, NULL, h[1], h[2], h[3], 0, min_sm);
		if(r[0]){ kswx_t x = aux->hit; r[1] = x.score; r[2] = x.tb; r[3] = x.te; r[4] = x.qb; r[5] = x.qe; r[6] = x.aln; r[7] = x.mat; r[8] = x.mis; r[9] = x.ins; r[10] = x.del; r[11] = aux->cigars->size; }
		fwrite(r, 4, 12, out);
		if(r[0]) fwrite(aux->cigars->buffer, 4, aux->cigars->size, out);
		free(t); free(q); free_hzmaux(aux);
	}
	fclose(out);
	return 0;
}
"""


def make_layouts():
    rng = np.random.default_rng(20261021)
    lays = []
    for k in range(8):
        glen = int(rng.integers(8000, 20001))
        G = synth.random_genome(glen, rng)
        dup = None
        if k >= 4:
            ln, dist = int(rng.integers(1500, 2001)), int(rng.integers(3000, 5001))
            a = int(rng.integers(500, glen - dist - ln - 500))
            G[a + dist:a + dist + ln] = G[a:a + ln]
            dup = (a, a + dist, ln)
        ny = int(rng.integers(6, 11))
        cases = []
        for i in range(ny):
            ln = int(rng.integers(1500, 4001))
            b = int(round(i * (glen - ln) / max(1, ny - 1)))            # tiling
            if dup and i < 6:
                copy = dup[i % 2]
                if i < 4:                                                  # inside one copy
                    ln = int(rng.integers(1500, dup[2] + 1)); b = copy + int(rng.integers(0, dup[2] - ln + 1))
                else:                                                      # across an edge of one
                    b = copy - ln // 2 if i == 4 else copy + dup[2] - ln // 2
            b = max(0, min(glen - ln, b))
            rd = np.ascontiguousarray(synth._mutate(G[b:b + ln], 0.15, rng))
            cases.append((rd, b + int(rng.integers(-60, 61)), b + ln + int(rng.integers(-60, 61)), 1))
        for _ in range(2):                                                 # N reads: the whole form
            ln = int(rng.integers(1500, 4001)); b = int(rng.integers(0, glen - ln + 1))
            cases.append((np.ascontiguousarray(synth._mutate(G[b:b + ln], 0.15, rng)), 0, -1, 0))
        lays.append((np.ascontiguousarray(G), prm(-3 if k % 2 == 0 else -2), cases))
    return lays


def main():
    flags = None
    for line in open(os.path.join(ROOT, "oracle", "Makefile")):
        m = re.match(r"REFFLAGS\s*=\s*(.*)", line)
        if m:
            flags = m.group(1).split()
    assert flags, "REFFLAGS not found in oracle/Makefile"
    shim = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_shim.so"))
    shim.ref_align_hzmaux.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lays = make_layouts()
    td = tempfile.mkdtemp(prefix="hzmreg_")
    assert not os.path.abspath(td).startswith(ROOT + os.sep)
    try:
        src, exe, fin, fout = (os.path.join(td, f) for f in ("driver.c", "driver", "in.bin", "out.bin"))
        open(src, "w").write(DRIVER)
        subprocess.run(["gcc"] + flags + ["-iquote", REF, "-o", exe, src, os.path.join(REF, "ksw.c"), "-lm"], check=True)
        flat = [(li, G, p, rd, b, e, y) for li, (G, p, cases) in enumerate(lays) for rd, b, e, y in cases]
        with open(fin, "wb") as f:
            f.write(np.int32(len(flat)).tobytes())
            for _, G, p, rd, b, e, _ in flat:
                f.write(np.array(p, dtype=np.int32).tobytes() + np.float32(MIN_SM).tobytes() + np.array([G.size, rd.size, b, e], dtype=np.int32).tobytes() + G.tobytes() + rd.tobytes())
        subprocess.run([exe, fin, fout], check=True)
        raw = np.fromfile(fout, dtype=np.int32)
    finally:
        shutil.rmtree(td)
    rec = np.zeros((len(flat), 11), dtype=np.int32); cig = []; cig_off = np.zeros(len(flat) + 1, dtype=np.int64); differs = np.zeros(len(flat), dtype=np.uint8)
    at = 0
    for k, (_, G, p, rd, b, e, y) in enumerate(flat):
        r = raw[at:at + 12]; at += 12
        rec[k] = r[:11]
        words = raw[at:at + int(r[11])].astype(np.uint32) if r[0] else np.zeros(0, dtype=np.uint32)
        at += words.size
        cig.append(words); cig_off[k + 1] = cig_off[k] + words.size
        out = np.zeros(10, dtype=np.int32); buf = np.zeros(G.size + rd.size + 2, dtype=np.uint32); pp = np.array(p, dtype=np.int32)
        n = shim.ref_align_hzmaux(G.ctypes.data, G.size, rd.ctypes.data, rd.size, pp.ctypes.data, MIN_SM, 0, out.ctypes.data, buf.ctypes.data, buf.size)
        assert n >= -1
        whole = np.concatenate([[1], out]) if n >= 0 else np.zeros(11, dtype=np.int32)
        differs[k] = int(not np.array_equal(whole, rec[k]) or (n >= 0 and not np.array_equal(buf[:n], words)))
        if not y:
            assert not differs[k], "the driver's (0, -1) and the shim's whole form disagree: the recorder is wrong"
    assert at == raw.size
    is_y = np.array([y for *_, y in flat], dtype=np.uint8)
    nreg, nfail, ndiff = int(is_y.sum()), int(((rec[:, 0] == 0) & (is_y == 1)).sum()), int(differs.sum())
    print("%d cases with an interval (%d without a hit, %d differ from the whole form), %d whole-form cases" % (nreg, nfail, ndiff, len(flat) - nreg))
    assert nreg >= 40 and nfail * 4 <= nreg and ndiff >= 4, "the conditions on the committed file are not met: nothing written"
    rd_off = np.zeros(len(flat) + 1, dtype=np.int64); rd_off[1:] = np.cumsum([c[3].size for c in flat])
    bb_off = np.zeros(len(lays) + 1, dtype=np.int64); bb_off[1:] = np.cumsum([G.size for G, _, _ in lays])
    np.savez_compressed(OUT, backbones=np.concatenate([G for G, _, _ in lays]), bb_off=bb_off, prm=np.array([p for _, p, _ in lays], dtype=np.int32), min_sm=np.float32(MIN_SM),
                        reads=np.concatenate([c[3] for c in flat]), rd_off=rd_off, layout=np.array([c[0] for c in flat], dtype=np.int32),
                        beg=np.array([c[4] for c in flat], dtype=np.int32), end=np.array([c[5] for c in flat], dtype=np.int32), is_region=is_y,
                        rec=rec, cigar=np.concatenate(cig) if cig else np.zeros(0, dtype=np.uint32), cig_off=cig_off, differs_from_whole=differs)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
