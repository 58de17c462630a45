"""ctypes binding of the C ABI in include/wtzmo_hip.h (libwtzmo_hip.so).

Python is test / benchmark orchestration only; the product is the C library + the C host driver.
Loading fails loudly when the HIP library is missing: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwtzmo_hip.so")

SYMBOLS = [
    "wtz_last_error", "wtz_device_count", "wtz_device_memory", "wtz_ctx_create", "wtz_ctx_destroy", "wtz_ctx_clone", "wtz_upload_reads",
    "wtz_index_build", "wtz_zindex_build", "wtz_candidates", "wtz_candidates_begin", "wtz_candidates_end", "wtz_batch_begin", "wtz_pairs_seed",
    "wtz_pairs_windows", "wtz_pairs_align", "wtz_fetch_cigars", "wtz_fetch_cigar_text", "wtz_fetch_cigar_text_begin", "wtz_fetch_cigar_text_end", "wtz_cigar_text_device", "wtz_host_alloc", "wtz_host_free", "wtz_get_counters", "wtz_reset_counters",
    "wtz_test_dp", "wtz_extend_batch", "wtz_local_batch", "wtz_kext_batch", "wtz_align_batch", "wtz_global_batch", "wtz_alignx_batch", "wtz_pwtext_batch", "wtz_pool_info", "wtz_pool_failure_kind",
    "wtz_index_count", "wtz_index_counts_fetch", "wtz_index_finish", "wtz_candidate_groups_begin", "wtz_candidate_groups_end", "wtz_candidate_groups_fetch", "wtz_cand_tail_host", "wtz_zindex_build_subset", "wtz_zindex_build_queries", "wtz_upload_reads_ascii", "wtz_fetch_read_bits", "wtz_append_revcomp_views",
    "wtz_pairs_seed_region", "wtz_hzmaux_batch", "wtz_set_window_chaining", "wtz_set_gap_open",
]


class Params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("ksize", "zsize", "hk", "hz", "ksave", "kovl", "ncand", "nbest",
                                          "kwin", "kstep", "ztot", "zovl", "max_kmer_freq", "max_zmer_freq", "max_kmer_var")] + \
               [("win_rep_norm", C.c_float), ("win_rep_cutoff", C.c_float)] + \
               [(n, C.c_int32) for n in ("w", "ew", "W", "M", "X", "O", "E", "T", "min_score")] + [("min_id", C.c_float)] + \
               [(n, C.c_int32) for n in ("dot_matrix", "xvar", "yvar", "min_block_len", "max_overhang")] + \
               [("deviation_penalty", C.c_float), ("gap_penalty", C.c_float), ("refine", C.c_int32), ("aux_strand", C.c_int32)]

    @classmethod
    def defaults(cls, **kw):
        """wtzmo.c:1543-1588"""
        p = cls(ksize=16, zsize=10, hk=1, hz=1, ksave=4, kovl=300, ncand=500, nbest=100, kwin=800, kstep=400, ztot=300,
                zovl=200, max_kmer_freq=0, max_zmer_freq=64, max_kmer_var=2, win_rep_norm=20.0, win_rep_cutoff=100.0,
                w=50, ew=800, W=3200, M=2, X=-5, O=-3, E=-1, T=-50, min_score=200, min_id=0.5, dot_matrix=0, xvar=128,
                yvar=64, min_block_len=160, max_overhang=256, deviation_penalty=1.0, gap_penalty=0.05, refine=0, aux_strand=0)
        for k, v in kw.items():
            setattr(p, k, v)
        p.kstep = p.kwin // 2
        p.max_overhang = 2 * p.xvar
        return p


class IndexStats(C.Structure):
    _fields_ = [("n_occ", C.c_uint64), ("n_distinct", C.c_uint64), ("ktot", C.c_uint64), ("n_kept", C.c_uint64),
                ("max_kmer_freq", C.c_uint32), ("avg_rdlen", C.c_uint32)]


PAIR_SUMMARY = np.dtype([("n_hits", "<u4"), ("gate", "<u4"), ("ovl", "<u4", 2), ("nwin", "<u4", 2),
                         ("dm_score", "<i4"), ("dm_qb", "<i4"), ("dm_qe", "<i4"), ("dm_tb", "<i4"), ("dm_te", "<i4"), ("dm_dir", "<i4")])
WINBOX = np.dtype([("beg", "<i4", 2), ("end", "<i4", 2)])
ALN_RESULT = np.dtype([("score", "<i4"), ("tb", "<i4"), ("te", "<i4"), ("qb", "<i4"), ("qe", "<i4"), ("aln", "<i4"), ("mat", "<i4"),
                       ("mis", "<i4"), ("ins", "<i4"), ("del", "<i4"), ("n_regs", "<u4"), ("cigar_len", "<u4"), ("cigar_off", "<u8"),
                       ("text_len", "<u4"), ("pad", "<u4"), ("text_off", "<u8")])


DP_PROBLEM = np.dtype([("q_read", "<u4"), ("t_read", "<u4"), ("q_rev", "<u4"), ("t_rev", "<u4"), ("q_from", "<i4"), ("t_from", "<i4"),
                       ("q_strand", "<i4"), ("t_strand", "<i4"), ("q_len", "<i4"), ("t_len", "<i4"), ("init_score", "<i4"), ("W", "<i4")])
DP_RESULT = np.dtype([("score", "<i4"), ("tb", "<i4"), ("te", "<i4"), ("qb", "<i4"), ("qe", "<i4"), ("aln", "<i4"), ("mat", "<i4"),
                      ("mis", "<i4"), ("ins", "<i4"), ("del", "<i4"), ("cigar_len", "<u4"), ("form_used", "<u4"), ("cigar_off", "<u8"), ("cells", "<u8")])
DP_SHIFT, DP_FIXED, DP_GLOBAL = 0, 1, 2
LOCAL_RESULT = np.dtype([("score", "<i4"), ("te", "<i4"), ("qe", "<i4"), ("tb", "<i4"), ("qb", "<i4"), ("form_used", "<u4"), ("cells", "<u8")])
LOCAL_MAXLEN = 65535      # rows / columns of one wtz_local_batch problem (include/wtzmo_hip.h)
KEXT_RESULT = np.dtype([("score", "<i4"), ("qle", "<i4"), ("tle", "<i4"), ("gtle", "<i4"), ("gscore", "<i4"), ("max_off", "<i4"),
                        ("form_used", "<u4"), ("rows", "<u4"), ("cells", "<u8")])
KEXT_MAXW = 1023          # band half-width of one wtz_kext_batch problem (WTZ_KEXT_MAXW)
KEXT_MAXLEN = 0xFFFFF     # its rows / columns (WTZ_KEXT_MAXLEN)
ALIGN_RESULT = np.dtype([(n, "<i4") for n in ("found", "score", "tb", "te", "qb", "qe", "local_score", "local_tb", "local_te", "local_qb", "local_qe")])
GLOBAL_RESULT = np.dtype([(n, "<i4") for n in ("score", "aln", "mat", "mis", "ins", "del")] + [("cigar_len", "<u4"), ("form_used", "<u4"), ("cigar_off", "<u8"), ("cells", "<u8")])
GLOB_MAXSLOTS = 2047      # band slots of one K-glob wavefront (WTZ_GLOB_MAXSLOTS); wider problems run the wide forms 33 / 255
ALIGNX_RESULT = np.dtype([(n, "<i4") for n in ("found", "score", "tb", "te", "qb", "qe", "aln", "mat", "mis", "ins", "del", "band")] +
                         [("form_used", "<u4"), ("cigar_len", "<u4"), ("cigar_off", "<u8")])
HZMAUX_RESULT = np.dtype([(n, "<i4") for n in ("found", "score", "tb", "te", "qb", "qe", "aln", "mat", "mis", "ins", "del")] + [("cigar_len", "<u4"), ("cigar_off", "<u8")])
PWTEXT_IN = np.dtype([("qb", "<i4"), ("tb", "<i4"), ("cigar_len", "<u4"), ("pad", "<u4"), ("cigar_off", "<u8")])
PWTEXT_RESULT = np.dtype([("text_off", "<u8"), ("cols", "<u4"), ("pad", "<u4")])


class Counters(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("ms_index", "ms_zindex", "ms_candidates", "ms_pairs", "ms_winalign", "ms_stitch")] + \
               [(n, C.c_uint64) for n in ("n_candidates_q", "n_pairs", "n_winalign", "n_stitch", "cells_shift", "cells_fixed",
                                          "cells_global", "bytes_seed_algo", "pool_peak")] + \
               [("ms_ext", C.c_double), ("n_extjobs", C.c_uint64), ("ms_gap", C.c_double), ("bytes_zmer_algo", C.c_uint64),
                ("ms_ingest", C.c_double), ("bytes_ingest_algo", C.c_uint64),
                ("ms_local", C.c_double), ("n_local", C.c_uint64), ("cells_local", C.c_uint64),
                ("ms_kext", C.c_double), ("n_kext", C.c_uint64), ("cells_kext", C.c_uint64),
                ("ms_kglob", C.c_double), ("n_kglob", C.c_uint64), ("cells_kglob", C.c_uint64),
                ("ticks_kglob_dp", C.c_uint64), ("ticks_kglob_tb", C.c_uint64),
                ("ms_pwtext", C.c_double), ("n_pwtext", C.c_uint64), ("bytes_pwtext", C.c_uint64)]


def load(path: str | None = None) -> C.CDLL:
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError("libwtzmo_hip.so not found at %s: build it with `python __graft_entry__.py build` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path." % path)
    lib = C.CDLL(path)
    lib.wtz_last_error.restype = C.c_char_p
    lib.wtz_ctx_create.argtypes = [C.c_int, C.POINTER(Params), C.c_uint64, C.POINTER(C.c_void_p)]
    lib.wtz_ctx_destroy.argtypes = [C.c_void_p]
    lib.wtz_ctx_destroy.restype = None
    lib.wtz_upload_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.wtz_index_build.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(IndexStats)]
    lib.wtz_zindex_build.argtypes = [C.c_void_p]
    lib.wtz_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.wtz_batch_begin.argtypes = [C.c_void_p]
    lib.wtz_pairs_seed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.wtz_pairs_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.wtz_pairs_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.wtz_fetch_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.wtz_get_counters.argtypes = [C.c_void_p, C.POINTER(Counters)]
    lib.wtz_reset_counters.argtypes = [C.c_void_p]
    lib.wtz_test_dp.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
    return lib


def check_symbols(path: str | None = None) -> None:
    """Every symbol declared in include/wtzmo_hip.h must be exported (no compute call: works without a GPU)."""
    lib = C.CDLL(path or LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError("libwtzmo_hip.so does not export: " + ", ".join(missing))


def pack_reads(seqs):
    """2-bit pack (dna.h:78 layout) a list of uint8 code arrays given in READ-ID order."""
    lens = np.array([s.size for s in seqs], dtype=np.uint32)
    offs = np.zeros(len(seqs), dtype=np.uint64)
    if len(seqs) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    allb = np.concatenate(seqs).astype(np.uint64) if len(seqs) else np.zeros(0, dtype=np.uint64)
    n = allb.size
    nw = (n + 31) // 32
    pad = np.zeros(nw * 32, dtype=np.uint64)
    pad[:n] = allb
    pad = pad.reshape(nw, 32)
    shifts = (np.uint64(62) - np.arange(32, dtype=np.uint64) * np.uint64(2))
    words = np.bitwise_or.reduce(pad << shifts, axis=1) if nw else np.zeros(0, dtype=np.uint64)
    return np.ascontiguousarray(words, dtype=np.uint64), offs, lens


class Context:
    """Thin RAII wrapper used by tests and bench.py."""

    def __init__(self, params: Params, device: int = 0, pool_bytes: int = 0, lib_path: str | None = None):
        self.lib = load(lib_path)
        self.params = params
        self.h = C.c_void_p()
        self._chk(self.lib.wtz_ctx_create(device, C.byref(params), pool_bytes, C.byref(self.h)))

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError("libwtzmo_hip error %d: %s" % (rc, self.lib.wtz_last_error().decode()))

    def close(self):
        if self.h:
            self.lib.wtz_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def upload(self, words, offs, lens):
        self.n_reads = int(lens.size)
        self._keep = (words, offs, lens)
        self._chk(self.lib.wtz_upload_reads(self.h, words.ctypes.data, words.size, offs.ctypes.data, lens.ctypes.data, lens.size))

    def upload_ascii(self, text: bytes, offs, lens, rand_calls_before=0):
        """f4: the bases as text, packed on the device (wtz_upload_reads_ascii); returns the number of non-ACGT bytes"""
        self.n_reads = int(lens.size)
        self._keep = (text, offs, lens)
        nr = C.c_uint64(0)
        self.lib.wtz_upload_reads_ascii.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
        self._chk(self.lib.wtz_upload_reads_ascii(self.h, text, len(text), offs.ctypes.data, lens.ctypes.data, lens.size, rand_calls_before, C.byref(nr)))
        return int(nr.value)

    def append_revcomp_views(self):
        """reads n .. 2n-1 := reverse complements of reads 0 .. n-1 (wtz_append_revcomp_views)"""
        self.lib.wtz_append_revcomp_views.argtypes = [C.c_void_p]
        self._chk(self.lib.wtz_append_revcomp_views(self.h))
        self.n_reads *= 2

    def fetch_read_bits(self, n_bases):
        nw = (n_bases + 31) // 32
        out = np.zeros(nw, dtype=np.uint64)
        self.lib.wtz_fetch_read_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        self._chk(self.lib.wtz_fetch_read_bits(self.h, out.ctypes.data, nw))
        return out

    def index_build(self, beg=0, end=None, K=0):
        k = C.c_uint32(K)
        st = IndexStats()
        self._chk(self.lib.wtz_index_build(self.h, beg, self.n_reads if end is None else end, C.byref(k), C.byref(st)))
        return st

    def zindex_build(self):
        self._chk(self.lib.wtz_zindex_build(self.h))

    def _cand_rows(self, qids, carry):
        """rows of ncand + 1 words and their entry counts: zero, or the carried-in (rows, n) of an earlier index part copied"""
        stride = self.params.ncand + 1
        rows = np.zeros((qids.size, stride), dtype=np.uint64)
        n = np.zeros(qids.size, dtype=np.uint32)
        if carry is not None:
            rows[:] = np.asarray(carry[0], dtype=np.uint64).reshape(qids.size, stride)
            n[:] = np.asarray(carry[1], dtype=np.uint32)
        return rows, n

    def candidates(self, qids, carry=None):
        """wtz_candidates; carry = the (rows, n) of the same queries from the index parts before this one (-G), so that ncand_io is nonzero on entry"""
        qids = np.ascontiguousarray(qids, dtype=np.uint32)
        rows, n = self._cand_rows(qids, carry)
        self._chk(self.lib.wtz_candidates(self.h, qids.ctypes.data, qids.size, rows.ctypes.data, n.ctypes.data))
        return rows, n

    def candidates_begin(self, qids, carry=None):
        """wtz_candidates_begin: nothing else may be called on the context before candidates_end"""
        qids = np.ascontiguousarray(qids, dtype=np.uint32)
        rows, n = self._cand_rows(qids, carry)
        self._pending = (qids, rows, n)
        self.lib.wtz_candidates_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self._chk(self.lib.wtz_candidates_begin(self.h, qids.ctypes.data, qids.size, rows.ctypes.data, n.ctypes.data))

    def candidates_end(self):
        _, rows, n = self._pending
        self.lib.wtz_candidates_end.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.wtz_candidates_end(self.h, rows.ctypes.data, n.ctypes.data))
        return rows, n

    def index_count(self, beg=0, end=None):
        """wtz_index_count + wtz_index_counts_fetch: the shard's distinct sampled k-mers (ascending), their occurrences in it, and n_occ"""
        nd, no = C.c_uint64(0), C.c_uint64(0)
        self.lib.wtz_index_count.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self._chk(self.lib.wtz_index_count(self.h, beg, self.n_reads if end is None else end, C.byref(nd), C.byref(no)))
        kmers = np.zeros(nd.value, dtype=np.uint64)
        cnts = np.zeros(nd.value, dtype=np.uint32)
        self.lib.wtz_index_counts_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.wtz_index_counts_fetch(self.h, kmers.ctypes.data, cnts.ctypes.data))
        return kmers, cnts, int(no.value)

    def index_finish(self, total_cnt, K):
        """wtz_index_finish: total_cnt[i] = occurrences of the i-th k-mer of index_count over ALL shards; returns n_kept"""
        total_cnt = np.ascontiguousarray(total_cnt, dtype=np.uint32)
        nk = C.c_uint64(0)
        self.lib.wtz_index_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
        self._chk(self.lib.wtz_index_finish(self.h, total_cnt.ctypes.data, K, C.byref(nk)))
        return int(nk.value)

    def candidate_groups(self, qids):
        """wtz_candidate_groups_begin / _end / _fetch: per query the groups with ol >= -d as (read << 1 | strand) << 32 | ol, in key order"""
        qids = np.ascontiguousarray(qids, dtype=np.uint32)
        ng = np.zeros(qids.size, dtype=np.uint32)
        self.lib.wtz_candidate_groups_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        self.lib.wtz_candidate_groups_end.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.wtz_candidate_groups_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        self._chk(self.lib.wtz_candidate_groups_begin(self.h, qids.ctypes.data, qids.size))
        self._chk(self.lib.wtz_candidate_groups_end(self.h, ng.ctypes.data))
        tot = int(ng.sum(dtype=np.uint64))
        g = np.zeros(tot, dtype=np.uint64)
        self._chk(self.lib.wtz_candidate_groups_fetch(self.h, g.ctypes.data, tot))
        return np.split(g, np.cumsum(ng.astype(np.int64))[:-1]) if qids.size else []

    def cand_tail_host(self, groups, carry=None):
        """wtz_cand_tail_host: strand merge + candidate heap (wtzmo.c:516-571) over one query's groups; returns (row, n)"""
        groups = np.ascontiguousarray(groups, dtype=np.uint64)
        row = np.zeros(self.params.ncand + 1, dtype=np.uint64)
        hn = C.c_uint32(0)
        if carry is not None:
            row[:] = carry[0]; hn.value = int(carry[1])
        self.lib.wtz_cand_tail_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        self.lib.wtz_cand_tail_host.restype = None
        self.lib.wtz_cand_tail_host(groups.ctypes.data, groups.size, self.params.kovl, self.params.ncand, row.ctypes.data, C.byref(hn))
        return row, int(hn.value)

    def clone(self, pool_bytes=0):
        """wtz_ctx_clone: a second context on the same device sharing this one's reads and indexes"""
        other = object.__new__(Context)
        other.lib, other.params, other.h = self.lib, self.params, C.c_void_p()
        other.n_reads = self.n_reads
        other._keep = getattr(self, "_keep", None)
        self.lib.wtz_ctx_clone.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        self._chk(self.lib.wtz_ctx_clone(self.h, pool_bytes, C.byref(other.h)))
        return other

    def pairs_seed(self, q, c):
        q = np.ascontiguousarray(q, dtype=np.uint32)
        c = np.ascontiguousarray(c, dtype=np.uint32)
        out = np.zeros(q.size, dtype=PAIR_SUMMARY)
        self._chk(self.lib.wtz_pairs_seed(self.h, q.ctypes.data, c.ctypes.data, q.size, out.ctypes.data))
        return out

    def pairs_seed_region(self, q, c, beg, end):
        """wtz_pairs_seed_region: pairs_seed with one interval [beg, end) of the indexed read q per pair (align_hzmaux's beg / end; needs aux_strand = 1)"""
        q = np.ascontiguousarray(q, dtype=np.uint32)
        c = np.ascontiguousarray(c, dtype=np.uint32)
        beg = np.ascontiguousarray(beg, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        assert q.size == c.size == beg.size == end.size
        out = np.zeros(q.size, dtype=PAIR_SUMMARY)
        self.lib.wtz_pairs_seed_region.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        self._chk(self.lib.wtz_pairs_seed_region(self.h, q.ctypes.data, c.ctypes.data, beg.ctypes.data, end.ctypes.data, q.size, out.ctypes.data))
        return out

    def set_window_chaining(self, fast):
        """wtz_set_window_chaining: 1 (default) = the windows of a scan by their median diagonal, 0 = by chaining_hzmps, as wtmsa and wtcns run align_hzmaux"""
        self.lib.wtz_set_window_chaining.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.wtz_set_window_chaining(self.h, int(fast)))

    def set_gap_open(self, I, D):
        """wtz_set_gap_open: the opening costs of a run of query-only steps (I) and of target-only steps (D) in every device DP, as the reference takes them
        (negative or zero; wtmsa: -2, -3); both are params.O until it is called"""
        self.lib.wtz_set_gap_open.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        self._chk(self.lib.wtz_set_gap_open(self.h, int(I), int(D)))

    def zindex_build_subset(self, ids):
        """the z-index of the listed reads only (ascending ids); every other read gets an empty slice"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self.lib.wtz_zindex_build_subset.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        self._chk(self.lib.wtz_zindex_build_subset(self.h, ids.ctypes.data, ids.size))

    def hzmaux_batch(self, tid, rid, beg, end):
        """align_hzmaux per (target read, query read, beg, end) in one call (wtz_hzmaux_batch): (records, CIGAR words); the CIGAR of record i is
        words[cigar_off : cigar_off + cigar_len].  The buffer holds one word per base of every pair, which no CIGAR exceeds."""
        tid = np.ascontiguousarray(tid, dtype=np.uint32)
        rid = np.ascontiguousarray(rid, dtype=np.uint32)
        beg = np.ascontiguousarray(beg, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        assert tid.size == rid.size == beg.size == end.size
        out = np.zeros(tid.size, dtype=HZMAUX_RESULT)
        lens = self._keep[2].astype(np.int64)
        ok = (tid < lens.size) & (rid < lens.size)
        cap = int(lens[tid[ok]].sum() + lens[rid[ok]].sum()) + 2
        cig = np.zeros(cap, dtype=np.uint32)
        self.lib.wtz_hzmaux_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
        self._chk(self.lib.wtz_hzmaux_batch(self.h, tid.ctypes.data, rid.ctypes.data, beg.ctypes.data, end.ctypes.data, tid.size, out.ctypes.data, cig.ctypes.data, cap))
        return out, cig[:int(out["cigar_len"].sum())].copy()

    def pairs_windows(self, summary):
        n = int(summary["nwin"].sum())
        out = np.zeros(n, dtype=WINBOX)
        self._chk(self.lib.wtz_pairs_windows(self.h, out.ctypes.data, n))
        return out

    def pairs_align(self, pair_idx, dirs):
        pair_idx = np.ascontiguousarray(pair_idx, dtype=np.uint32)
        dirs = np.ascontiguousarray(dirs, dtype=np.uint8)
        out = np.zeros(pair_idx.size, dtype=ALN_RESULT)
        self._chk(self.lib.wtz_pairs_align(self.h, pair_idx.ctypes.data, dirs.ctypes.data, pair_idx.size, out.ctypes.data))
        tot = int(out["cigar_len"].sum())
        cig = np.zeros(tot, dtype=np.uint32)
        self._chk(self.lib.wtz_fetch_cigars(self.h, cig.ctypes.data, tot))
        return out, cig

    def test_dp(self, kind, form, problems, cigar_cap=1 << 22):
        """TEST-ONLY: run DP problems through one device form; returns (results, list of CIGAR arrays)."""
        problems = np.ascontiguousarray(problems, dtype=DP_PROBLEM)
        out = np.zeros(problems.size, dtype=DP_RESULT)
        cig = np.zeros(cigar_cap, dtype=np.uint32)
        self._chk(self.lib.wtz_test_dp(self.h, kind, form, problems.ctypes.data, problems.size, out.ctypes.data, cig.ctypes.data, cig.size))
        return out, [cig[int(o):int(o) + int(n)].copy() for o, n in zip(out["cigar_off"], out["cigar_len"])]

    def local_batch(self, problems, o_del, e_del, o_ins, e_ins):
        """ksw_align2(..., KSW_XSTART) per problem (wtz_local_batch): score, te, qe, tb, qb as the reference returns them."""
        problems = np.ascontiguousarray(problems, dtype=DP_PROBLEM)
        out = np.zeros(problems.size, dtype=LOCAL_RESULT)
        self.lib.wtz_local_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        self._chk(self.lib.wtz_local_batch(self.h, problems.ctypes.data, problems.size, o_del, e_del, o_ins, e_ins, out.ctypes.data))
        return out

    def kext_batch(self, problems, o_del, e_del, o_ins, e_ins, end_bonus, zdrop):
        """ksw_extend2 per problem (wtz_kext_batch): q_* = its query (columns), t_* = its target (rows), init_score = h0, W = w."""
        problems = np.ascontiguousarray(problems, dtype=DP_PROBLEM)
        out = np.zeros(problems.size, dtype=KEXT_RESULT)
        self.lib.wtz_kext_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_int32] * 6 + [C.c_void_p]
        self._chk(self.lib.wtz_kext_batch(self.h, problems.ctypes.data, problems.size, o_del, e_del, o_ins, e_ins, end_bonus, zdrop, out.ctypes.data))
        return out

    def align_batch(self, problems, w, I, D, E, T):
        """kswx_align_no_stat per problem (wtz_align_batch): the local hit extended to both sides; I, D, E, T as negative costs."""
        problems = np.ascontiguousarray(problems, dtype=DP_PROBLEM)
        out = np.zeros(problems.size, dtype=ALIGN_RESULT)
        self.lib.wtz_align_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_int32] * 5 + [C.c_void_p]
        self._chk(self.lib.wtz_align_batch(self.h, problems.ctypes.data, problems.size, w, I, D, E, T, out.ctypes.data))
        return out

    def global_batch(self, problems, o_del, e_del, o_ins, e_ins, cigar=True):
        """ksw_global2 per problem (wtz_global_batch), W = the band: (results, list of CIGAR arrays), or with cigar=False (NULL buffer) the results alone."""
        problems = np.ascontiguousarray(problems, dtype=DP_PROBLEM)
        out = np.zeros(problems.size, dtype=GLOBAL_RESULT)
        cap = int(problems["q_len"].astype(np.int64).sum() + problems["t_len"].astype(np.int64).sum()) + 2 if cigar else 0
        cig = np.zeros(max(cap, 1), dtype=np.uint32)
        self.lib.wtz_global_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_uint64]
        self._chk(self.lib.wtz_global_batch(self.h, problems.ctypes.data, problems.size, o_del, e_del, o_ins, e_ins, out.ctypes.data, cig.ctypes.data if cigar else None, cap))
        if not cigar:
            return out
        return out, [cig[int(o):int(o) + int(n)].copy() for o, n in zip(out["cigar_off"], out["cigar_len"])]

    def alignx_batch(self, problems, w, I, D, E, T, cigar=True):
        """kswx_align / kswx_align_with_cigar per problem (wtz_alignx_batch); I, D, E, T as negative costs; returns as global_batch does."""
        problems = np.ascontiguousarray(problems, dtype=DP_PROBLEM)
        out = np.zeros(problems.size, dtype=ALIGNX_RESULT)
        cap = int(problems["q_len"].astype(np.int64).sum() + problems["t_len"].astype(np.int64).sum()) + 2 if cigar else 0
        cig = np.zeros(max(cap, 1), dtype=np.uint32)
        self.lib.wtz_alignx_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_uint64]
        self._chk(self.lib.wtz_alignx_batch(self.h, problems.ctypes.data, problems.size, w, I, D, E, T, out.ctypes.data, cig.ctypes.data if cigar else None, cap))
        if not cigar:
            return out
        return out, [cig[int(o):int(o) + int(n)].copy() for o, n in zip(out["cigar_off"], out["cigar_len"])]

    def pwtext_batch(self, problems, starts, cigar_slices, cigar, sizing_only=False):
        """the picture of `pairaln -a` per alignment (wtz_pwtext_batch): starts = (qb, tb) pairs, cigar_slices = (offset, length) pairs into `cigar`;
        returns (results, bytes), the picture of alignment i at bytes[text_off : text_off + 3 * (cols + 1)]; sizing_only: the NULL-buffer call, (results, b"")"""
        problems = np.ascontiguousarray(problems, dtype=DP_PROBLEM)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        inp = np.zeros(problems.size, dtype=PWTEXT_IN)
        if problems.size:
            st = np.asarray(starts, dtype=np.int64).reshape(-1, 2)
            sl = np.asarray(cigar_slices, dtype=np.uint64).reshape(-1, 2)
            inp["qb"], inp["tb"], inp["cigar_off"], inp["cigar_len"] = st[:, 0], st[:, 1], sl[:, 0], sl[:, 1]
        out = np.zeros(problems.size, dtype=PWTEXT_RESULT)
        self.lib.wtz_pwtext_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
        args = (self.h, problems.ctypes.data, inp.ctypes.data, problems.size, cigar.ctypes.data if cigar.size else None, cigar.size, out.ctypes.data)
        self._chk(self.lib.wtz_pwtext_batch(*args, None, 0))
        if sizing_only or problems.size == 0:
            return out, b""
        cap = int(out["text_off"][-1]) + 3 * (int(out["cols"][-1]) + 1)
        buf = np.zeros(cap, dtype=np.uint8)
        self._chk(self.lib.wtz_pwtext_batch(*args, buf.ctypes.data, cap))
        return out, buf.tobytes()

    def counters(self) -> Counters:
        c = Counters()
        self._chk(self.lib.wtz_get_counters(self.h, C.byref(c)))
        return c

    def reset_counters(self):
        self._chk(self.lib.wtz_reset_counters(self.h))
