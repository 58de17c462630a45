"""Shared by test_seed_cpu.py, test_gpu_seed.py and tests/golden/make_seed_vectors.py: the k-mer index (index_wtzmo, wtzmo.c:349-430) and the seed lookup
(query_wtzmo, wtzmo.c:433-573) function by function.  Three things answer the same questions - the reference's own functions behind oracle/ref_seed_shim.c,
the oracle's restatement behind the same four calls (oracle/oracle_lib.c), and the device library (or its host emulation) through hipabi.Context - and the
recorded answers of the first are in tests/golden/seed_vectors.npz.  Everything compared is an integer and compared for equality.

The read sets are not stored: every case regenerates its reads from a seed with the generator below (SplitMix64, fixed by its definition) and checks the
sha256 of the packed bank against the fixture; a mismatch fails the test."""
import ctypes as C
import hashlib
import io
import os
import re
import subprocess
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(ROOT, "tests", "golden", "seed_vectors.npz")
SHIM = os.path.join(ROOT, "oracle", "_ref", "libref_seed.so")
NONE = 0xFFFFFFFF00000000      # the placeholder row of a query without a candidate (wtzmo.c:499)
PRM = dict(ksize=16, hk=1, ksave=4, kovl=300, ncand=500, K=0)      # wtzmo.c:1543-1588


# ---- the generator ----
class Rng:
    """SplitMix64 (Steele, Lea, Flood 2014): state += 0x9E3779B97F4A7C15, output = the finalizer of the state"""
    def __init__(self, seed):
        self.s = np.array([seed], dtype=np.uint64)

    def u64(self, n):
        with np.errstate(over="ignore"):
            z = self.s[0] + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            if n:
                self.s[0] = z[-1]
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))

    def ints(self, lo, hi, n):
        return (self.u64(n) % np.uint64(hi - lo)).astype(np.int64) + lo

    def int(self, lo, hi):
        return int(self.ints(lo, hi, 1)[0])

    def bases(self, n):
        return (self.u64(n) >> np.uint64(33) & np.uint64(3)).astype(np.uint8)


def rc(s):
    return np.ascontiguousarray((3 - s)[::-1])


def mutate(rng, s, sub, indel=0.0):
    """substitutions at rate sub (always to another base), then deletions and insertions at rate indel each"""
    s = s.copy()
    n = s.size
    r = rng.u64(n)
    hit = (r % np.uint64(1000000)).astype(np.int64) < int(sub * 1000000)
    s[hit] = (s[hit] + 1 + ((r[hit] >> np.uint64(40)) % np.uint64(3)).astype(np.uint8)) & 3
    if indel:
        thr = np.uint64(int(indel * 1000000))
        r = rng.u64(s.size)
        ins = np.flatnonzero(r % np.uint64(1000000) < thr)
        s = np.insert(s, ins, ((r[ins] >> np.uint64(40)) & np.uint64(3)).astype(np.uint8))
        s = s[rng.u64(s.size) % np.uint64(1000000) >= thr]
    return np.ascontiguousarray(s, dtype=np.uint8)


def genome(rng, n):
    G = rng.bases(n)
    for _ in range(n // 300):      # homopolymer runs: -H 1 compresses them
        p = rng.int(0, n - 20)
        G[p:p + rng.int(3, 10)] = G[p]
    return G


def by_length(reads):
    """the order of the reference's main (wtzmo.c:1708): longest first, stable"""
    return [reads[i] for i in sorted(range(len(reads)), key=lambda i: -reads[i].size)]


def sample(rng, G, n, lo, hi, sub, indel, strands=True):
    out = []
    for _ in range(n):
        ln = rng.int(lo, hi)
        b = rng.int(0, G.size - ln)
        r = mutate(rng, G[b:b + ln], sub, indel)
        out.append(rc(r) if strands and rng.int(0, 2) else r)
    return out


def plain_reads(seed=1):
    """about 60 reads of 1.5 - 4 kb at 8x over a 20 kb genome, both strands, in length order"""
    rng = Rng(seed)
    return by_length(sample(rng, genome(rng, 20000), 60, 1500, 4000, 0.03, 0.01))


def strand_reads(seed=2):
    """read 0 holds a segment S; every other long read holds a piece of S and, elsewhere, the reverse complement of another piece of S (of a different
    size, so that either strand may win), between unrelated sequence; the rest are plain reads of the same genome"""
    rng = Rng(seed)
    G = genome(rng, 12000)
    S = G[2000:5000]
    out = [mutate(rng, G[1500:5500], 0.01)]
    for k in range(8):
        a, la = rng.int(0, 1200), rng.int(500, 1500)
        b, lb = rng.int(1300, 1800), rng.int(500, 1200)
        fw, rv = mutate(rng, S[a:a + la], 0.01), rc(mutate(rng, S[b:b + lb], 0.01))
        parts = [rng.bases(rng.int(50, 300)), fw if k % 2 else rv, rng.bases(rng.int(50, 300)), rv if k % 2 else fw, rng.bases(rng.int(50, 300))]
        out.append(np.concatenate(parts))
    return by_length(out + sample(rng, G, 12, 1000, 3000, 0.02, 0.005))


def gate_length():
    """The query length of the length gate.  floor(L * 1.2) in double arithmetic (wtzmo.c:445) equals the integer L * 6 / 5 for every L a read can have (rdlen has
    24 bits; test_seed_cpu.py checks it up to 10 kb), so no length tells the two apart; a multiple of 5 is taken, where L * 1.2 is a whole number and the
    rounding of the double product would show first."""
    return 2005


def gate_reads(seed=3, shuffled=False):
    """one query of length L and candidates that share its sequence, of lengths floor(1.2 L) - 1, floor(1.2 L), floor(1.2 L) + 1, L * 6 / 5 and L / 2"""
    rng = Rng(seed)
    L = gate_length()
    up = int(L * 1.2)
    Q = genome(rng, L)
    out = [Q.copy()]
    for ln in (up - 1, up, up + 1, L * 6 // 5, up + 1, up, L // 2, L - 7):
        out.append(np.concatenate([Q, rng.bases(max(0, ln - L))])[:ln].copy() if ln >= L else Q[:ln].copy())
    out = by_length(out)
    if shuffled:
        p = np.argsort(rng.u64(len(out)), kind="stable")
        out = [out[i] for i in p]
    return out


def short_reads(seed=4, ksize=16):
    """lengths 0, 1, ksize - 1, ksize, ksize + 1, a homopolymer, a read that is one palindromic k-mer, and three reads that overlap, longest first"""
    rng = Rng(seed)
    G = genome(rng, 3000)
    X = np.array([0, 1, 2, 3, 0, 2, 1, 3] * 4, dtype=np.uint8)[:ksize // 2]      # no base repeats: -H 1 leaves it alone
    W = np.array([0, 1, 2, 0, 3, 1, 0, 2, 1, 3, 2, 0, 1, 3, 0, 2, 3, 1, 2, 1], dtype=np.uint8)
    return [G[0:2000].copy(), G[500:2500].copy(), rc(G[900:2700]), np.full(300, 2, dtype=np.uint8), W[:ksize + 1].copy(), W[:ksize].copy(), np.concatenate([X, rc(X)]),
            W[:ksize - 1].copy(), W[:1].copy(), W[:0].copy()]


def saturate_reads(seed=5):
    """16 reads of 10 kb of (AC)n in front of the plain set: two k-mers with more than 65 535 occurrences each"""
    ac = np.tile(np.array([0, 1], dtype=np.uint8), 5000)
    return [ac.copy() for _ in range(16)] + plain_reads(seed)


def many_reads(seed=6):
    """2 300 reads of 560 - 640 bp over a 30 kb genome (46x: the counts stay under the automatic cutoff), in length order: every read is shorter than 1.2 x
    any other, so the keys of a query span all of them"""
    rng = Rng(seed)
    return by_length(sample(rng, genome(rng, 30000), 2300, 560, 640, 0.01, 0.0))


def fat_reads(seed=7):
    """a query of 7 kb (read 0), an exact copy of it, and 30 reads of 2 - 5 kb of the genome it was cut from"""
    rng = Rng(seed)
    G = genome(rng, 30000)
    q = G[10000:17000].copy()
    return by_length([q, q.copy()] + sample(rng, G, 30, 2000, 5000, 0.03, 0.01))


def family_reads(seed=8, n=600):
    """n near-copies (0.5 % substitutions) of one 5 kb read"""
    rng = Rng(seed)
    G = genome(rng, 5000)
    return [mutate(rng, G, 0.005) for _ in range(n)]


def pack_codes(seqs):
    lens = np.array([s.size for s in seqs], dtype=np.uint32)
    offs = np.zeros(len(seqs), dtype=np.uint64)
    if len(seqs) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    codes = np.ascontiguousarray(np.concatenate(seqs) if len(seqs) else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
    return codes, offs, lens


def bank_sha(seqs):
    """sha256 over the packed bank (dna.h:78 layout), the offsets and the lengths"""
    from smartdenovo_amd import hipabi
    w, o, l = hipabi.pack_reads(seqs)
    return np.frombuffer(hashlib.sha256(w.tobytes() + o.tobytes() + l.tobytes()).digest(), dtype=np.uint8).copy()


# ---- the cases: name -> (reads, [variants]); a variant = the parameters, the queries recorded (None = all) ----
def V(queries=None, **kw):
    p = dict(PRM)
    p.update(kw)
    return dict(prm=p, queries=queries)


READS = {
    "plain": plain_reads, "strand_merge": strand_reads, "length_gate": gate_reads, "length_gate_shuffled": lambda: gate_reads(shuffled=True),
    "short": short_reads, "saturate": saturate_reads, "many_reads": many_reads, "fat_group": fat_reads, "second_level_parts": family_reads,
}
_cache = {}


def reads_of(case):
    if case not in _cache:
        _cache[case] = READS[case]()
    return _cache[case]


def static_variants():
    """every (case, tag, variant) that does not depend on the reference's data (K_edges does: the recorder adds it, the tests read it from the fixture)"""
    out = [("plain", "default", V()), ("plain", "S1", V(ksave=1))]
    for k in (5, 32, 15, 17):      # 5 and 32: the bounds of the reference's usage text (wtzmo.c:1453, 1659)
        out.append(("plain", "k%d" % k, V(ksize=k, queries=[0, 7, 30, 59] if k == 5 else None)))      # 5-mers: half a million tuples per query
    out.append(("plain", "H0", V(hk=0)))
    for d in (1, 255, 256, 5000):
        out.append(("plain", "d%d" % d, V(kovl=d)))
    for a in (1, 2, 5):
        out.append(("plain", "A%d" % a, V(ncand=a)))
    out.append(("strand_merge", "S1", V(ksave=1)))
    out.append(("strand_merge", "S1_A3", V(ksave=1, ncand=3)))
    out.append(("length_gate", "S1", V(ksave=1)))
    out.append(("length_gate_shuffled", "S1", V(ksave=1)))
    out.append(("short", "S1", V(ksave=1)))
    out.append(("short", "S1_d20", V(ksave=1, kovl=20)))
    out.append(("saturate", "S1", V(ksave=1, queries=[0, 15, 16, 17, 40, 75])))
    out.append(("many_reads", "default", V(queries=[0, 1, 777, 1500, 2298, 2299])))
    out.append(("fat_group", "S1", V(ksave=1, queries=[0, 1, 2, 31])))
    out.append(("second_level_parts", "K2000", V(K=2000, queries=[0, 299, 599])))
    return out


PARTS = {"halves": (0, 30, 60), "thirds": (0, 20, 40, 60)}      # the plain set cut by read id


# ---- the reference / the oracle behind the four calls ----
class SeedLib:
    def __init__(self, path):
        L = self.lib = C.CDLL(path)
        L.seedx_open.restype = C.c_void_p
        L.seedx_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.seedx_close.argtypes = [C.c_void_p]
        L.seedx_close.restype = None
        L.seedx_index.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.seedx_table.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        L.seedx_table.restype = None
        L.seedx_query.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.seedx_query.restype = C.c_uint32
        L.seedx_groups.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]

    def open(self, seqs, prm):
        return SeedSession(self.lib, seqs, prm)


class SeedSession:
    def __init__(self, lib, seqs, prm):
        self.lib, self.prm, self.n = lib, prm, len(seqs)
        self.keep = pack_codes(seqs)
        p = np.array([prm[k] for k in ("ksize", "hk", "ksave", "kovl", "ncand")], dtype=np.uint32)
        self.h = lib.seedx_open(self.keep[0].ctypes.data, self.keep[1].ctypes.data, self.keep[2].ctypes.data, self.n, p.ctypes.data)

    def close(self):
        self.lib.seedx_close(self.h)
        self.h = None

    def index(self, beg=0, end=None, K=None):
        """returns the stats (as IndexStats names; n_occ = None where saturation hides it) and the table in k-mer order"""
        io_ = np.array([self.prm["K"] if K is None else K, 0, 0, 0], dtype=np.uint64)
        rc_ = self.lib.seedx_index(self.h, beg, self.n if end is None else end, io_.ctypes.data)
        assert rc_ == 0, "seedx_index: the two passes over the reference's index disagree (%d)" % rc_
        nm, ns = int(io_[2]), int(io_[3])
        t = dict(mers=np.zeros(nm, dtype=np.uint64), cnts=np.zeros(nm, dtype=np.uint32), flt=np.zeros(nm, dtype=np.uint8), offs=np.zeros(nm, dtype=np.uint64),
                 runs=np.zeros(nm, dtype=np.uint32), seeds=np.zeros(ns, dtype=np.uint32))
        self.lib.seedx_table(self.h, *[t[k].ctypes.data for k in ("mers", "cnts", "flt", "offs", "runs", "seeds")])
        ktot = int(t["cnts"].sum(dtype=np.uint64))
        st = dict(n_occ=None if (t["cnts"] == 0xFFFF).any() else ktot, n_distinct=nm, ktot=ktot, n_kept=int((t["flt"] == 0).sum()), max_kmer_freq=int(io_[0]), avg_rdlen=int(io_[1]))
        return st, t

    def query(self, pbid, carry=None):
        row = np.zeros(self.prm["ncand"] + 1, dtype=np.uint64)
        n = 0
        if carry is not None:
            row[:] = carry[0]
            n = int(carry[1])
        n = self.lib.seedx_query(self.h, pbid, row.ctypes.data, n)
        return row, n

    def groups(self, pbid):
        """(key, ol, cnt) of every group in merge order"""
        cap = 2 * self.n + 2
        out = np.zeros((cap, 3), dtype=np.uint32)
        n = self.lib.seedx_groups(self.h, pbid, out.ctypes.data, cap)
        assert 0 <= n <= cap
        return out[:n].copy()


def oracle_lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "liboracle.so"], check=True)
    return SeedLib(os.path.join(ROOT, "oracle", "liboracle.so"))


def table_sha(mers, cnts):
    """sha256 of the (k-mer, min(count, 0xFFFF)) list in k-mer order"""
    o = np.argsort(mers, kind="stable")
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(mers[o], dtype="<u8").tobytes() + np.minimum(cnts[o], 0xFFFF).astype("<u4").tobytes()).digest(), dtype=np.uint8).copy()


STAT = ("n_occ", "n_distinct", "ktot", "n_kept", "max_kmer_freq", "avg_rdlen")


def run_seedx(lib, seqs, var):
    """one variant through the four calls: the record that the fixture holds"""
    s = lib.open(seqs, var["prm"])
    try:
        st, t = s.index()
        q = list(range(len(seqs))) if var["queries"] is None else list(var["queries"])
        groups = [s.groups(i) for i in q]
        rows = [s.query(i) for i in q]
    finally:
        s.close()
    return dict(stats=st, tab_sha=table_sha(t["mers"], t["cnts"]), max_cnt=int(t["cnts"].max()) if t["cnts"].size else 0, q=q, groups=groups, rows=[r[:n].copy() for r, n in rows])


def run_seedx_parts(lib, seqs, var, cuts):
    """the reference called part by part as its main does for -G (wtzmo.c:1281-1334): the cutoff resolved by the first part stays, the heaps are carried"""
    s = lib.open(seqs, var["prm"])
    try:
        K = var["prm"]["K"]
        carry = [None] * len(seqs)
        for b, e in zip(cuts[:-1], cuts[1:]):
            st, _ = s.index(b, e, K)
            K = st["max_kmer_freq"]
            carry = [s.query(i, carry[i]) for i in range(len(seqs))]
    finally:
        s.close()
    return [r[:n].copy() for r, n in carry]


# ---- the device library or its host emulation ----
def dev_params(prm):
    from smartdenovo_amd import hipabi
    return hipabi.Params.defaults(ksize=prm["ksize"], hk=prm["hk"], ksave=prm["ksave"], kovl=prm["kovl"], ncand=prm["ncand"])


def dev_open(lib_path, seqs, prm, pool_bytes=1 << 30):
    from smartdenovo_amd import hipabi
    ctx = hipabi.Context(dev_params(prm), pool_bytes=pool_bytes, lib_path=lib_path)
    ctx.upload(*hipabi.pack_reads(seqs))
    return ctx


def dev_stats(st):
    return {k: int(getattr(st, k)) for k in STAT}


def run_device(lib_path, seqs, var, how="all"):
    """the same record from the device: wtz_index_count / _counts_fetch / _finish for the table, wtz_index_build for the stats and the index that answers,
    wtz_candidate_groups_* for the groups (those with ol >= -d only: the device returns no others), wtz_candidates for the rows"""
    ctx = dev_open(lib_path, seqs, var["prm"])
    try:
        q = list(range(len(seqs))) if var["queries"] is None else list(var["queries"])
        st = dev_stats(ctx.index_build(K=var["prm"]["K"]))
        kmers, cnts, n_occ = ctx.index_count()
        assert n_occ == st["n_occ"], "wtz_index_count and wtz_index_build count different occurrences: %d, %d" % (n_occ, st["n_occ"])
        n_kept = ctx.index_finish(cnts, st["max_kmer_freq"])
        groups_f = ctx.candidate_groups(q)          # on the index of wtz_index_finish
        rows_f = ctx.candidates(q)
        ctx.index_build(K=var["prm"]["K"])
        groups = ctx.candidate_groups(q)
        rows, n = ctx.candidates(q)
        for a, b in zip(groups, groups_f):
            assert np.array_equal(a, b), "the index of wtz_index_finish answers other groups than that of wtz_index_build"
        assert np.array_equal(rows, rows_f[0]) and np.array_equal(n, rows_f[1]), "the index of wtz_index_finish answers other rows than that of wtz_index_build"
    finally:
        ctx.close()
    return dict(stats=st, n_kept_finish=n_kept, tab_sha=table_sha(kmers, cnts), kmers=kmers, cnts=cnts, q=q, groups=groups, rows=[rows[i, :n[i]].copy() for i in range(len(q))])


def compare_stats(want, got, where):
    for k in STAT:
        if want[k] is None or want[k] < 0:
            continue       # n_occ where a saturated count hides it
        assert got[k] == want[k], "%s: %s = %d, the reference has %d" % (where, k, got[k], want[k])


def compare_groups(want, got, kovl, q, where, full=False):
    """want: the reference's (key, ol, cnt) of every group; got: (key, ol, cnt) likewise (full) or the device's key << 32 | ol of the groups with ol >= kovl"""
    w = want if full else want[want[:, 1] >= kovl]
    g = got if full else np.stack([(got >> np.uint64(32)).astype(np.uint32), (got & np.uint64(0xFFFFFFFF)).astype(np.uint32)], axis=1)
    cnt = {int(r[0]): int(r[2]) for r in want}
    wd = {int(r[0]): tuple(int(x) for x in r[1:(3 if full else 2)]) for r in w}
    gd = {int(r[0]): tuple(int(x) for x in r[1:(3 if full else 2)]) for r in g}
    for key in sorted(set(wd) | set(gd)):
        assert wd.get(key) == gd.get(key), "%s: query %d, group of read %d strand %d: got %s, the reference has %s (ol[, cnt]; the group has %s tuples)" % (
            where, q, key >> 1, key & 1, gd.get(key), wd.get(key), cnt.get(key))
    assert [int(r[0]) for r in g] == [int(r[0]) for r in w], "%s: query %d: the groups are not in the reference's merge order" % (where, q)


def compare_rows(want, got, q, where):
    assert len(got) == len(want) and all(int(a) == int(b) for a, b in zip(got, want)), "%s: query %d: heap array %s, the reference has %s" % (
        where, q, ["%d:%d" % (int(x) >> 32, int(x) & 0xFFFFFFFF) for x in got], ["%d:%d" % (int(x) >> 32, int(x) & 0xFFFFFFFF) for x in want])


def compare_record(want, got, kovl, where, full=False):
    compare_stats(want["stats"], got["stats"], where)
    assert bytes(got["tab_sha"]) == bytes(want["tab_sha"]), "%s: the (k-mer, count) list differs from the reference's table" % where
    assert list(got["q"]) == list(want["q"])
    for i, q in enumerate(want["q"]):
        compare_groups(want["groups"][i], got["groups"][i], kovl, q, where, full)
        compare_rows(want["rows"][i], got["rows"][i], q, where)


# ---- the regimes, from the reference's groups ----
def constants():
    """the constants of the workgroup form as the DEVICE build has them (smartdenovo_amd/csrc/wtz_seed.h; the #else branch of the emulation's small values)"""
    src = open(os.path.join(ROOT, "smartdenovo_amd", "csrc", "wtz_seed.h")).read()
    env = {}
    for name in ("WTZ_CWG_BINS", "WTZ_CWG_CAP", "WTZ_CWG_SKETCH"):
        env[name] = int(re.search(r"#define %s (\d+)u" % name, src).group(1))
    blk = re.search(r"#if defined\(WTZ_EMUL\).*\n#define WTZ_CWG_L2_MIN .*\n#define WTZ_CWG_L2_PART_UNITS .*\n#else\n#define WTZ_CWG_L2_MIN (.*)\n#define WTZ_CWG_L2_PART_UNITS (.*)\n#endif", src)
    for name, expr in zip(("WTZ_CWG_L2_MIN", "WTZ_CWG_L2_PART_UNITS"), blk.groups()):
        assert re.fullmatch(r"[\dWTZ_CGAPu*() ]+", expr), expr
        env[name] = int(eval(re.sub(r"(\d+)u", r"\1", expr), {"__builtins__": {}}, dict(env)))
    return env


def tuples(groups, kovl):
    """(tuples of the query, tuples of its largest group, tuples of the groups that reach -d = the lower bound of the listed tuples)"""
    c = groups[:, 2].astype(np.int64)
    return int(c.sum()), int(c.max()) if c.size else 0, int(c[groups[:, 1] >= kovl].sum())


# ---- the fixture ----
def write_npz(path, arrays):
    """an .npz whose bytes depend on the arrays alone: fixed member order and time stamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), version=(1, 0))
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue(), compresslevel=9)


def pack_record(arrays, key, var, rec):
    p = var["prm"]
    arrays[key + ".prm"] = np.array([p[k] for k in ("ksize", "hk", "ksave", "kovl", "ncand", "K")], dtype=np.uint32)
    arrays[key + ".stats"] = np.array([-1 if rec["stats"][k] is None else rec["stats"][k] for k in STAT], dtype=np.int64)
    arrays[key + ".tab_sha"] = rec["tab_sha"]
    arrays[key + ".max_cnt"] = np.array([rec["max_cnt"]], dtype=np.uint32)
    arrays[key + ".q"] = np.array(rec["q"], dtype=np.uint32)
    arrays[key + ".g_off"] = np.cumsum([0] + [g.shape[0] for g in rec["groups"]]).astype(np.int64)
    arrays[key + ".g"] = np.concatenate(rec["groups"]).astype(np.uint32) if rec["groups"] else np.zeros((0, 3), dtype=np.uint32)
    arrays[key + ".r_off"] = np.cumsum([0] + [r.size for r in rec["rows"]]).astype(np.int64)
    arrays[key + ".rows"] = np.concatenate(rec["rows"]).astype(np.uint64) if rec["rows"] else np.zeros(0, dtype=np.uint64)


_npz = None


def fixture():
    global _npz
    if _npz is None:
        _npz = dict(np.load(NPZ))
    return _npz


def variants():
    """[(case, tag)] of the fixture, in name order"""
    return sorted(tuple(k[:-4].split("/")) for k in fixture() if k.endswith(".prm"))


def load_record(case, tag):
    v = fixture()
    key = "%s/%s" % (case, tag)
    p = dict(zip(("ksize", "hk", "ksave", "kovl", "ncand", "K"), (int(x) for x in v[key + ".prm"])))
    q = [int(x) for x in v[key + ".q"]]
    go, ro = v[key + ".g_off"], v[key + ".r_off"]
    rec = dict(stats=dict(zip(STAT, (None if x < 0 else int(x) for x in v[key + ".stats"]))), tab_sha=v[key + ".tab_sha"], max_cnt=int(v[key + ".max_cnt"][0]), q=q,
               groups=[v[key + ".g"][go[i]:go[i + 1]] for i in range(len(q))], rows=[v[key + ".rows"][ro[i]:ro[i + 1]] for i in range(len(q))])
    return dict(prm=p, queries=q), rec


def checked_reads(case):
    """the case's reads, regenerated; their packed bank must be the one the fixture was recorded from"""
    seqs = reads_of(case)
    assert bytes(bank_sha(seqs)) == bytes(fixture()["bank/" + case]), "the generator no longer makes the reads of case %s that the fixture was recorded from" % case
    return seqs


def check_regimes(load, keys, reads):
    """Every case states the regime it is there for as an assertion on the REFERENCE's data (load(case, tag) -> (variant, record); reads[case] = its reads), against
    the constants of the device build; returns one line per regime with the measured figures.  Where a regime depends on how many tuples the first sketch level
    lists, the lower bound (the tuples of the groups that reach -d, which the sketch cannot drop) alone crosses the threshold."""
    K = constants()
    out = []

    def tup(case, tag):
        var, rec = load(case, tag)
        return var, rec, [tuples(g, var["prm"]["kovl"]) for g in rec["groups"]]

    var, rec, t = tup("plain", "default")
    g = np.concatenate(rec["groups"])
    reach = g[g[:, 1] >= var["prm"]["kovl"]]
    assert (reach[:, 0] & 1 == 0).sum() > 20 and (reach[:, 0] & 1 == 1).sum() > 20, "plain: groups that reach -d on both strands"
    below = int((g[:, 1] < var["prm"]["kovl"]).sum())
    assert below > 20, "plain: groups below -d"
    out.append("plain: %d groups reach -d (%d on '-'), %d stay below; tuples per query <= %d" % (reach.shape[0], int((reach[:, 0] & 1).sum()), below, max(x[0] for x in t)))
    for tag, unit in (("d255", 1), ("d256", 2)):      # sk_unit = 1 against > 1, sk_thr = 255 (wtz_seed.h: sk_unit = kovl > 255 ? ceil(kovl / 255) : 1)
        kovl = load("plain", tag)[0]["prm"]["kovl"]
        assert (1 if kovl <= 255 else (kovl + 254) // 255) == unit
    assert all(r.size == 1 and int(r[0]) == NONE for r in load("plain", "d5000")[1]["rows"]), "params: a -d nothing reaches leaves the placeholder row"
    for a in (1, 2, 5):
        var, rec, t = tup("plain", "A%d" % a)
        most = max(int((x[:, 1] >= var["prm"]["kovl"]).sum()) for x in rec["groups"])
        assert var["prm"]["ncand"] == a and most > a, "heap: a query with more than -A groups at or above -d"
        out.append("heap A%d: a query has %d groups at or above -d (> %d)" % (a, most, a))
    var, rec, t = tup("strand_merge", "S1")
    both = [0, 0]
    for x in rec["groups"]:
        ol = {int(r[0]): int(r[1]) for r in x if r[1] >= var["prm"]["kovl"]}
        for key in ol:
            if key & 1 == 0 and key + 1 in ol and ol[key] != ol[key + 1]:
                both[ol[key + 1] > ol[key]] += 1
    assert both[0] and both[1], "strand_merge: reads that reach -d on both strands, either strand the larger"
    out.append("strand_merge: %d (query, read) with both strands at or above -d and '+' larger, %d with '-' larger" % tuple(both))
    for case in ("length_gate", "length_gate_shuffled"):
        var, rec = load(case, "S1")
        lens = [s.size for s in reads[case]]
        L = gate_length()
        up = int(L * 1.2)
        assert up == L * 6 // 5 and lens.count(L) == 1 and lens.count(up) >= 2 and lens.count(up + 1) >= 2
        x = rec["groups"][rec["q"].index(lens.index(L))]
        hit = {int(r[0]) >> 1 for r in x}
        assert all((i in hit) == (lens[i] <= up) for i in range(len(lens)) if lens[i] != L), "length_gate: reads of floor(1.2 L) are met, reads of floor(1.2 L) + 1 are not"
        assert (lens == sorted(lens, reverse=True)) == (case == "length_gate")
    out.append("length_gate: L = %d, floor(1.2 L) = %d; the reads of that length are met, those one base longer are not, in length order and shuffled" % (L, up))
    lens = sorted(s.size for s in reads["short"])
    ks = load("short", "S1")[0]["prm"]["ksize"]
    assert lens[:5] == [0, 1, ks - 1, ks, ks] and ks + 1 in lens
    var, rec = load("saturate", "S1")
    assert rec["max_cnt"] == 0xFFFF and rec["stats"]["n_occ"] is None and var["prm"]["K"] == 0, "saturate: a count of 0xFFFF under the automatic cutoff"
    out.append("saturate: largest count 0x%X, ktot %d, automatic K %d" % (rec["max_cnt"], rec["stats"]["ktot"], rec["stats"]["max_kmer_freq"]))
    kept = {}
    for c, tag in keys:
        if c == "plain" and re.fullmatch(r"K\d+", tag):
            kept[int(tag[1:])] = load(c, tag)[1]["stats"]["n_kept"]
    mx = load("plain", "default")[1]["max_cnt"]
    assert sorted(kept) == sorted({2, 3, mx - 1, mx}) and kept[2] < kept[3] < kept[mx - 1] < kept[mx], "K_edges: every cutoff keeps another number of k-mers"
    out.append("K_edges: n_kept %s" % ", ".join("K=%d: %d" % (k, kept[k]) for k in sorted(kept)))
    var, rec, t = tup("many_reads", "default")
    lens = [s.size for s in reads["many_reads"]]
    assert lens == sorted(lens, reverse=True) and max(lens) <= int(min(lens) * 1.2), "many_reads: in length order, no read longer than 1.2 x any query: thr = 0"
    assert 2 * (len(lens) - 0) > K["WTZ_CWG_BINS"] - 1, "many_reads: shift > 0"
    assert min(x[2] for x in t) > 0, "many_reads: every recorded query has groups that reach -d"
    out.append("many_reads: 2 * (idx_end - thr) = %d > WTZ_CWG_BINS - 1 = %d; tuples per query %s" % (2 * len(lens), K["WTZ_CWG_BINS"] - 1, [x[0] for x in t]))
    var, rec, t = tup("fat_group", "S1")
    i = rec["q"].index(0)
    assert t[i][1] > K["WTZ_CWG_CAP"], "fat_group: one group above WTZ_CWG_CAP"
    assert t[i][2] > K["WTZ_CWG_L2_MIN"] and t[i][0] * 12 <= K["WTZ_CWG_L2_PART_UNITS"], "second_level: listed tuples above WTZ_CWG_L2_MIN with parts == 1"
    out.append("fat_group: largest group %d tuples > WTZ_CWG_CAP = %d" % (t[i][1], K["WTZ_CWG_CAP"]))
    out.append("second_level: tuples of the groups that reach -d %d > WTZ_CWG_L2_MIN = %d; all tuples %d x 12 <= WTZ_CWG_L2_PART_UNITS = %d (one part)" % (
        t[i][2], K["WTZ_CWG_L2_MIN"], t[i][0], K["WTZ_CWG_L2_PART_UNITS"]))
    var, rec, t = tup("second_level_parts", "K2000")
    assert var["prm"]["K"] > len(reads["second_level_parts"]) and len(t) == 3
    assert all(x[2] * 12 > K["WTZ_CWG_L2_PART_UNITS"] for x in t), "second_level_parts: listed tuples x 12 above WTZ_CWG_L2_PART_UNITS"
    out.append("second_level_parts: tuples of the groups that reach -d %s, x 12 > WTZ_CWG_L2_PART_UNITS = %d (parts >= %d); largest group %d" % (
        [x[2] for x in t], K["WTZ_CWG_L2_PART_UNITS"], min(-(-x[2] * 12 // K["WTZ_CWG_L2_PART_UNITS"]) for x in t), max(x[1] for x in t)))
    return out


# ---- the host emulation, with its own small second-level thresholds and with the device's ----
HEAVY = {("plain", "k5"), ("second_level_parts", "K2000")}      # half a million listed tuples: thousands of second-level parts under the emulation's own thresholds


def emul_lib(device_thresholds=False):
    emul = os.path.join(ROOT, "tests", "emul")
    if not device_thresholds:
        subprocess.run([os.path.join(emul, "build_emul.sh")], check=True)
        return os.path.join(emul, "libwtz_emul.so")
    out = os.path.join(emul, "libwtz_emul_devthr.so")
    src = [os.path.join(d, f) for d in (os.path.join(ROOT, "smartdenovo_amd", "csrc"), os.path.join(ROOT, "include")) for f in os.listdir(d)]
    if not os.path.exists(out) or any(os.path.isfile(f) and os.path.getmtime(f) > os.path.getmtime(out) for f in src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-DWTZ_EMUL", "-DWTZ_EMUL_DEVICE_THRESHOLDS", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"),
                        "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "smartdenovo_amd", "csrc", "wtz_lib.cpp")], check=True)
    return out


def run_device_parts(lib_path, seqs, var, cuts):
    """-G-style parts on the device: one index per part, the cutoff of the first part kept, rows and ncand_io carried through wtz_candidates"""
    ctx = dev_open(lib_path, seqs, var["prm"])
    try:
        K = var["prm"]["K"]
        q = np.arange(len(seqs), dtype=np.uint32)
        carry = None
        for b, e in zip(cuts[:-1], cuts[1:]):
            K = int(ctx.index_build(b, e, K=K).max_kmer_freq)
            carry = ctx.candidates(q, carry)
    finally:
        ctx.close()
    return [carry[0][i, :carry[1][i]].copy() for i in range(len(seqs))]


def run_device_shards(lib_path, seqs, var, cuts):
    """shards: wtz_index_count per shard, the counts of equal k-mers added, wtz_index_finish, the groups of every shard concatenated, wtz_cand_tail_host;
    returns (stats as wtz_index_build names them, groups per query, rows per query)"""
    ctxs = [dev_open(lib_path, seqs, var["prm"]) for _ in cuts[1:]]
    try:
        counts = [c.index_count(b, e) for c, b, e in zip(ctxs, cuts[:-1], cuts[1:])]
        allk = np.unique(np.concatenate([k for k, _, _ in counts]))
        tot = np.zeros(allk.size, dtype=np.uint64)
        for k, c, _ in counts:
            tot[np.searchsorted(allk, k)] += c
        sat = np.minimum(tot, 0xFFFF)
        ktot = int(sat.sum())
        K = var["prm"]["K"]
        if K < 2:
            K = max(20, ktot // (allk.size + 1)) * 5       # wtzmo.c:380-393
        n_kept = 0
        for ctx, (k, c, _) in zip(ctxs, counts):
            ctx.index_finish(np.minimum(tot[np.searchsorted(allk, k)], 0xFFFFFFFF).astype(np.uint32), K)
        n_kept = int(((sat >= 2) & (sat <= K)).sum())
        q = np.arange(len(seqs), dtype=np.uint32)
        per = [ctx.candidate_groups(q) for ctx in ctxs]
        groups = [np.concatenate([p[i] for p in per]) for i in range(len(seqs))]
        rows = [ctxs[0].cand_tail_host(g) for g in groups]
    finally:
        for c in ctxs:
            c.close()
    st = dict(n_occ=sum(n for _, _, n in counts), n_distinct=int(allk.size), ktot=ktot, n_kept=n_kept, max_kmer_freq=K)
    return st, table_sha(allk, sat.astype(np.uint32)), groups, [r[:n].copy() for r, n in rows]


def load_parts(name):
    v = fixture()
    ro = v["parts/%s.r_off" % name]
    return [v["parts/%s.rows" % name][ro[i]:ro[i + 1]] for i in range(ro.size - 1)]
