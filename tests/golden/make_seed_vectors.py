#!/usr/bin/env python3
"""Records tests/golden/seed_vectors.npz: the answers of the reference's own index_wtzmo and query_wtzmo (oracle/_ref/libref_seed.so, built by
`make -C oracle ref` where the reference's sources are present) for the cases of tests/seedvec.py.  Per (case, variant): the parameters, the index
statistics, a sha256 of the (k-mer, saturating count) table in k-mer order, and per recorded query every group (key, ol, cnt) in merge order and the
candidate heap array verbatim.  The reads are not stored (sha256 of the packed bank per case).  Every regime a case is there for is asserted on the
reference's data before anything is written, and printed.  Running it twice gives identical bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seedvec as sv  # noqa: E402


def main():
    assert os.path.exists(sv.SHIM), "build the reference shim first: make -C oracle ref"
    ref = sv.SeedLib(sv.SHIM)
    arrays = {}
    recs = {}
    todo = sv.static_variants()
    base = sv.run_seedx(ref, sv.reads_of("plain"), todo[0][2])
    for K in (2, 3, base["max_cnt"], base["max_cnt"] - 1):      # K_edges: cnt > K and cnt <= 1 (wtzmo.c:401-405)
        todo.append(("plain", "K%d" % K, sv.V(K=K)))
    for case, tag, var in todo:
        rec = recs[(case, tag)] = sv.run_seedx(ref, sv.reads_of(case), var)
        sv.pack_record(arrays, "%s/%s" % (case, tag), var, rec)
        arrays["bank/" + case] = sv.bank_sha(sv.reads_of(case))
    for name, cuts in sv.PARTS.items():
        rows = sv.run_seedx_parts(ref, sv.reads_of("plain"), todo[0][2], cuts)
        arrays["parts/%s.r_off" % name] = np.cumsum([0] + [r.size for r in rows]).astype(np.int64)
        arrays["parts/%s.rows" % name] = np.concatenate(rows).astype(np.uint64)
    for line in sv.check_regimes(lambda c, t: (dict(prm=dict(zip(("ksize", "hk", "ksave", "kovl", "ncand", "K"), (int(x) for x in arrays["%s/%s.prm" % (c, t)])))), recs[(c, t)]),
                                 sorted(recs), {k: sv.reads_of(k) for k in sv.READS}):
        print(line)
    sv.write_npz(sv.NPZ, arrays)
    print("%s: %d bytes" % (sv.NPZ, os.path.getsize(sv.NPZ)))


if __name__ == "__main__":
    main()
