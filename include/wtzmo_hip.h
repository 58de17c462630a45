/*
 * wtzmo_hip.h — C ABI of libwtzmo_hip.so, the MI355X (gfx950) implementation of SMARTdenovo's
 * wtzmo hot path.  Plain C, caller-owned host buffers, opaque device context, no callbacks.
 *
 * The reference has no plugin/FFI boundary: the path's boundary is the `wtzmo` process itself
 * (SURVEY.md §8b).  This ABI therefore mirrors the reference's *function* granularity, so that each
 * entry point can be parity-tested against the reference function it replaces, and is consumed by
 * our own host driver (smartdenovo_amd/csrc/host/, the drop-in `wtzmo` executable):
 *
 *   wtz_upload_reads     <- push_long_read_wtzmo / BaseBank          wtzmo.c:207-215, dna.h:318-410
 *   wtz_index_build      <- index_wtzmo                               wtzmo.c:349-430
 *   wtz_zindex_build     <- index_single_read_seeds (all reads once)  hzm_aln.h:70-115
 *   wtz_candidates       <- query_wtzmo                               wtzmo.c:433-573
 *   wtz_pairs_seed       <- query_single_read_seeds + process_hzmps + merge_paired_kmers_window +
 *                           chaining_wtseedv | dot_matrix_align_hzmps hzm_aln.h:173-224, 580-713, 1134-1186
 *   wtz_pairs_align      <- fast_seeds_align_hzmo + global_align_regs_hzmo (kswx_extend_align_core,
 *                           kswx_extend_align_shift_core, ksw_global2) hzm_aln.h:1247-1486, kswx.h:101-335, ksw.c:503-586;
 *                           with params.refine also kswx_refine_alignment kswx.h:483-659
 *
 *   wtz_local_batch      <- ksw_align2 with KSW_XSTART over ksw_i16         ksw.c:344-366, 233-335 (what kswx_align*, kswx.h:1495-1520, and
 *                           wtcns.c:209, 269 call: the first step of wtcyc, pairaln and wtcns)
 *   wtz_alignx_batch     <- kswx_align / kswx_align_with_cigar              kswx.h:1495-1520 (bin/wtcyc, bin/pairaln)
 *   wtz_pwtext_batch     <- kswx_cigar2pairwise + the marker line           kswx.h:1150-1194, pairaln.c:115-125 (the picture of `pairaln -a`)
 *
 *   wtz_pairs_seed + wtz_pairs_align with params.aux_strand = 1
 *                        <- align_hzmaux, the pair routine of wtgbo   hzm_aln.h:1684-1775 (its caller wtgbo.c:37-56 orients the read first:
 *                           the host uploads every read and its reverse complement, smartdenovo_amd/csrc/host/wtgbo_main.c)
 *   wtz_pairs_seed_region <- the same with beg / end: query_single_read_seeds_by_region   hzm_aln.h:117-171, 1690-1693 (wtmsa.c:448-477, wtjnt)
 *   wtz_hzmaux_batch     <- align_hzmaux as one call per batch of (target, read, beg, end)  hzm_aln.h:1684-1775
 *   wtz_set_window_chaining <- HZM_FAST_WINDOW_KMER_CHAINING: the windows of a scan by the median diagonal or by chaining_hzmps   hzm_aln.h:36, 488, 544 (351-408)
 *   wtz_set_gap_open     <- the I and D arguments of align_hzmaux (separate insertion / deletion opening costs)   hzm_aln.h:1684, wtmsa.c:633-634, wtcns.c:330, 340
 *
 * Everything returned is integer and bit-exact against `wtzmo -t 1`.  The order-dependent state of
 * the reference (closed pairs, contained-read masking, per-read coverage: wtzmo.c:806-822, 1065-1100,
 * 1309-1334) stays with the caller: these functions are pure in (reads, parameters, arguments).
 *
 * Threading: one context per GPU, thread-compatible (not thread-safe per context).
 * Errors: 0 on success, a negative WTZ_E_* otherwise; wtz_last_error() has the message.
 */
#ifndef WTZMO_HIP_H
#define WTZMO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WTZ_OK        0
#define WTZ_E_ARG    -1   /* bad argument */
#define WTZ_E_HIP    -2   /* HIP runtime error (no device, launch failure, ...) */
#define WTZ_E_POOL   -3   /* device scratch pool exhausted: retry with fewer items or a larger pool */
#define WTZ_E_STATE  -4   /* call order violated (e.g. align before seed) */

/* Parameters: one field per reference WTZMO field that the path reads (wtzmo.c:98-132, 1663-1689). */
typedef struct {
	uint32_t ksize, zsize, hk, hz, ksave, kovl, ncand, nbest;
	uint32_t kwin, kstep, ztot, zovl, max_kmer_freq, max_zmer_freq, max_kmer_var;
	float    win_rep_norm, win_rep_cutoff;
	int32_t  w, ew, W, M, X, O, E, T;
	int32_t  min_score; float min_id;
	int32_t  dot_matrix, xvar, yvar, min_block_len, max_overhang;
	float    deviation_penalty, gap_penalty;
	int32_t  refine;         /* -n: kswx_refine_alignment after stitching (wtzmo.c:1031-1034) */
	int32_t  aux_strand;     /* 1 = the pair stages in align_hzmaux's form (hzm_aln.h:1693-1699, wtgbo's caller): only same-strand z-mer matches are kept
	                          * (filter_by_region_hzmps with dir 0, hzm_aln.h:1188-1197, before the window merge), there is no n_hits gate, and the chain
	                          * of strand 0 is kept when its weight is >= ztot (the caller passes -R there: hzm_aln.h:1699 compares with zovl) */
} wtz_params_c;

typedef struct wtz_ctx wtz_ctx_t;

typedef struct {
	uint64_t n_occ;          /* sampled k-mer occurrences in the indexed range */
	uint64_t n_distinct;     /* distinct sampled k-mers (ktyp) */
	uint64_t ktot;           /* sum of saturating counts (wtzmo.c:380-388) */
	uint64_t n_kept;         /* k-mers with 2 <= cnt <= K (the hash table content) */
	uint32_t max_kmer_freq;  /* resolved K */
	uint32_t avg_rdlen;      /* wtzmo.c:361-368 */
} wtz_index_stats_t;

typedef struct {
	uint32_t n_hits;         /* |cache| of the pair */
	uint32_t gate;           /* n_hits*zsize >= ztot (wtzmo.c:857) */
	uint32_t ovl[2];         /* zmo: SEED[dir].ovl after chaining_wtseedv (0 when no window) */
	uint32_t nwin[2];        /* zmo: chain windows kept for strand dir (only when ovl >= ztot) */
	int32_t  dm_score, dm_qb, dm_qe, dm_tb, dm_te, dm_dir;   /* dmo: kswr_t of dot_matrix_align_hzmps */
} wtz_pair_summary_t;

typedef struct { int32_t beg[2], end[2]; } wtz_winbox_t;     /* wt_seed_t.beg/end of a chain window */

typedef struct {
	int32_t  score, tb, te, qb, qe, aln, mat, mis, ins, del;   /* kswx_t of global_align_regs_hzmo */
	uint32_t n_regs;         /* windows that passed wtzmo.c:1026; 0 means "regs->size == 0" (wtzmo.c:1029) */
	uint32_t cigar_len;      /* number of (len<<4|op) words, op M0/I1/D2 */
	uint64_t cigar_off;      /* offset of this item's CIGAR inside the buffer returned by wtz_fetch_cigars */
	uint32_t text_len;       /* length of the CIGAR as text ("%d[MID]"..., kswx_cigar2string kswx.h:1093-1120), no terminator */
	uint32_t pad;
	uint64_t text_off;       /* offset inside the buffer returned by wtz_fetch_cigar_text */
} wtz_aln_result_t;

typedef struct {
	double   ms_index, ms_zindex, ms_candidates, ms_pairs, ms_winalign, ms_stitch;   /* HIP-event kernel time per stage */
	uint64_t n_candidates_q, n_pairs, n_winalign, n_stitch;                           /* work items launched */
	uint64_t cells_shift, cells_fixed, cells_global;                                  /* DP cell updates as the reference loops execute them */
	uint64_t bytes_seed_algo;                                                         /* algorithmic bytes of seed lookup */
	uint64_t pool_peak;
	double   ms_ext;                                                                  /* K-sw3 wave kernel alone (inside ms_stitch) */
	uint64_t n_extjobs;
	double   ms_gap;                                                                  /* K-sw2 gap kernels alone (inside ms_stitch) */
	uint64_t bytes_zmer_algo;                                                         /* algorithmic bytes of z-mer matching: candidate L/4 + 16 B per emitted match (hzm_aln.h:173-224) */
	double   ms_ingest;                                                               /* K_pack_ascii + K_pack_fix of wtz_upload_reads_ascii (kernel time, copies excluded) */
	uint64_t bytes_ingest_algo;                                                       /* 1 byte read + 2 bits written per base */
	double   ms_local;                                                                /* K-local of wtz_local_batch (kernel time, copies excluded) */
	uint64_t n_local, cells_local;                                                    /* its problems and the DP cells (rows x columns of both passes) it executed */
	double   ms_kext;                                                                 /* K-kext of wtz_kext_batch and of the two extension stages of wtz_align_batch (kernel time, copies excluded) */
	uint64_t n_kext, cells_kext;                                                      /* its problems and the DP cells (sum of end - beg over the rows executed) */
	double   ms_kglob;                                                                /* the launch groups of wtz_global_batch and of the last stage of wtz_alignx_batch: K-glob and the wide forms (kernel time, copies excluded) */
	uint64_t n_kglob, cells_kglob;                                                    /* their problems and DP cells (sum of end - beg over the rows) */
	uint64_t ticks_kglob_dp, ticks_kglob_tb;                                          /* DIAGNOSTIC ONLY, K-glob only: ticks of the device's constant 100 MHz wall clock (10 ns each), each wavefront's own, summed over the problems: DP rows / traceback with counting.  Only their ratio is meant to be used (the split of ms_kglob, tools/ubench/kglob_bench.py); no caller should depend on the values */
	double   ms_pwtext;                                                               /* the launch groups of wtz_pwtext_batch: both passes of K-pwtext (kernel time, copies excluded) */
	uint64_t n_pwtext, bytes_pwtext;                                                  /* its alignments and the bytes of picture written */
} wtz_counters_t;

const char *wtz_last_error(void);
int  wtz_device_count(void);
/* free / total bytes of the device's HBM right now.  No reference counterpart: the reference sizes nothing (its indexes live in host RAM, wtzmo.c:249-430,
 * hzm_aln.h:70-115); the host driver sizes the scratch pool and chooses between the all-reads z-mer index and the per-batch one from it. */
int  wtz_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

int  wtz_ctx_create(int device, const wtz_params_c *params, uint64_t pool_bytes, wtz_ctx_t **out);
void wtz_ctx_destroy(wtz_ctx_t *ctx);
/* second context on the same GPU sharing the parent's reads + indexes (read-only), with its own HIP stream, scratch pool and
 * batch state: one per host thread that keeps a batch in flight. pool_bytes 0 = same as the parent. */
int  wtz_ctx_clone(wtz_ctx_t *parent, uint64_t pool_bytes, wtz_ctx_t **out);

/* bits: 2-bit packed bases, 32 per word, base i at bits ((~i)&31)*2 of word i>>5 (dna.h:78);
 * rdoff/rdlen per read in READ-ID order (id = rank by length DESC under the reference's sort, wtzmo.c:1708). */
int  wtz_upload_reads(wtz_ctx_t *ctx, const uint64_t *bits, uint64_t n_words, const uint64_t *rdoff, const uint32_t *rdlen, uint32_t n_reads);

/* f4: the same upload from the bases as TEXT - seq2basebank (dna.h:397-410) on the device.  seq = the sequences of all reads of the
 * input concatenated in FILE order (n_bases bytes; upper or lower case; rdoff / rdlen index into it exactly as they would into the packed bank).
 * Every byte that is not one of ACGTacgt becomes `lrand48() & 3`, drawn in file order like the reference's loader does (dna.h:405) with the state of a
 * glibc process that never called srand48 (X0 = 0); rand_calls_before = lrand48 calls the emulated process made before this input (0 for wtzmo / wtgbo), *n_random (may be NULL) = such
 * bytes found.  The resulting device bank is bit-identical to wtz_upload_reads of the host-packed bank. */
int  wtz_upload_reads_ascii(wtz_ctx_t *ctx, const char *seq, uint64_t n_bases, const uint64_t *rdoff, const uint32_t *rdlen, uint32_t n_reads, uint64_t rand_calls_before, uint64_t *n_random);
/* wtgbo's view of the reads (wtgbo.c:48-49 reverse-complements a '-' candidate BEFORE its z-mers are taken; revbitseq_basebank, dna.h): appends to the n uploaded
 * reads their reverse complements as reads n .. 2n-1 (read n + i = reverse complement of read i over its current [rdoff, rdoff + rdlen) range), packed on the device.
 * Indexes built before the call are dropped. */
int  wtz_append_revcomp_views(wtz_ctx_t *ctx);
/* the packed bank back from the device (n_words = (n_bases + 31) / 32): what a host-side consumer of the 2-bit reads (wtgbo's reverse-complement views, tests) reads */
int  wtz_fetch_read_bits(wtz_ctx_t *ctx, uint64_t *bits, uint64_t n_words);

/* A2 over read ids [id_beg, id_end). *max_kmer_freq: in = -K (0/1 = auto), out = resolved cutoff. */
int  wtz_index_build(wtz_ctx_t *ctx, uint32_t id_beg, uint32_t id_end, uint32_t *max_kmer_freq, wtz_index_stats_t *stats);

/* ---- k-mer index SHARDED by read-id range over several contexts (BASELINE configs[4]; the reference's -G splits the index the
 * same way, wtzmo.c:1281-1285, but filters each part by its own counts).  To equal the UNSHARDED output the frequency filter (cnt > K or
 * cnt <= 1, wtzmo.c:401-405) and the automatic cutoff (wtzmo.c:380-393) must see the counts of all shards:
 *   wtz_index_count        occurrences of the shard's reads [id_beg, id_end), ordered by k-mer; *n_distinct = its distinct sampled k-mers
 *   wtz_index_counts_fetch those k-mers (ascending) with their occurrence counts in this shard
 *   ... the caller adds the counts of equal k-mers over the shards (one exchange), derives K ...
 *   wtz_index_finish       total_cnt[i] = count of the i-th fetched k-mer over ALL shards; builds the shard's table of the k-mers with
 *                          2 <= min(total, 0xFFFF) <= K, each pointing at the shard's own seed run.
 * A query is then answered by every shard (wtz_candidate_groups_*): the (read, strand) groups of a query with ol >= -d, as
 * `(read << 1 | strand) << 32 | ol` in key order.  Shards are contiguous id ranges, so the shards' lists concatenated in shard order are
 * the unsharded list, and wtz_cand_tail_host replays the strand merge and the candidate heap (wtzmo.c:516-571) over it. */
int  wtz_index_count(wtz_ctx_t *ctx, uint32_t id_beg, uint32_t id_end, uint64_t *n_distinct, uint64_t *n_occ);
int  wtz_index_counts_fetch(wtz_ctx_t *ctx, uint64_t *kmers, uint32_t *cnts);
int  wtz_index_finish(wtz_ctx_t *ctx, const uint32_t *total_cnt, uint32_t K, uint64_t *n_kept);
int  wtz_candidate_groups_begin(wtz_ctx_t *ctx, const uint32_t *qids, uint32_t nq);
int  wtz_candidate_groups_end(wtz_ctx_t *ctx, uint32_t *ngroups);                    /* ngroups[i] = groups of query i */
int  wtz_candidate_groups_fetch(wtz_ctx_t *ctx, uint64_t *groups, uint64_t total);   /* packed in query order; total = sum of ngroups */
void wtz_cand_tail_host(const uint64_t *groups, uint32_t ng, uint32_t kovl, uint32_t ncand, uint64_t *heap, uint32_t *hn);

/* A5 for every read + the candidate-side occurrence caps of A6. Call once after wtz_upload_reads. */
int  wtz_zindex_build(wtz_ctx_t *ctx);
/* The same index for the listed reads only (ascending ids); every other read gets an empty slice.  For read sets whose whole z-index
 * (16 B per base) does not fit beside the scratch pool: the caller rebuilds it per batch of queries from the batch's queries + candidates. */
int  wtz_zindex_build_subset(wtz_ctx_t *ctx, const uint32_t *ids, uint32_t n);
/* Several GPUs: the pairs of a batch are dealt by CANDIDATE id, so a device only ever walks the z-mers of its own share of the
 * reads as candidates - the index above then holds that share only (wtz_zindex_build_subset once) - but it needs the table of every QUERY of
 * the batch (hzm_aln.h:70-115 builds exactly that table per query, wtzmo.c:842-845).  This call builds a second, small index of the listed
 * reads (ascending ids) that the pair stages read the query side from; it is rebuilt per batch and dropped by any rebuild of the index above
 * or by ids == NULL, n == 0.  Results are identical to one index holding all reads. */
int  wtz_zindex_build_queries(wtz_ctx_t *ctx, const uint32_t *ids, uint32_t n);

/* A3. cand: nq rows of (ncand+1) u64 `id<<32|ol`; ncand_io[i]: in = entries already in row i
 * (candidate heaps carried across -G index parts, else 0), out = entries after this index part.
 * Rows are the reference's heap arrays verbatim (the caller applies wtzmo.c:813-822). */
int  wtz_candidates(wtz_ctx_t *ctx, const uint32_t *qids, uint32_t nq, uint64_t *cand, uint32_t *ncand_io);
/* the same request split in two, so that the caller's sequential work (the commit of the previous batch) overlaps the kernel:
 * _begin uploads and launches and returns at once; _end waits and fills cand / ncand_out (nq rows as passed to _begin).  No other
 * call on this context may be made in between. */
int  wtz_candidates_begin(wtz_ctx_t *ctx, const uint32_t *qids, uint32_t nq, const uint64_t *cand, const uint32_t *ncand_in);
int  wtz_candidates_end(wtz_ctx_t *ctx, uint64_t *cand, uint32_t *ncand_out);

/* Start a batch: releases all per-batch device results of the previous one. */
int  wtz_batch_begin(wtz_ctx_t *ctx);

/* A5/A6/A7 for n (query, candidate) pairs. Results stay on the device for wtz_pairs_windows / wtz_pairs_align. */
int  wtz_pairs_seed(wtz_ctx_t *ctx, const uint32_t *qid, const uint32_t *cid, uint32_t n, wtz_pair_summary_t *out);

/* wtz_pairs_seed in align_hzmaux's REGION form (hzm_aln.h:1684-1699 with beg / end set, as wtmsa calls it for every read of a layout: wtmsa.c:448-477): pair i
 * matches the z-mers of read cid[i] against the interval [beg[i], end[i]) of the indexed read qid[i] only - query_single_read_seeds_by_region, hzm_aln.h:117-171.
 * Defaults per pair as hzm_aln.h:1690-1691: beg < 0 -> 0, end <= 0 -> the length of read qid[i]; an end behind the read is not clamped (it excludes nothing);
 * beg >= end after the defaults matches nothing (n_hits = 0, gate = 0).  Inside the walk of an indexed z-mer's occurrences (in `off` order, hzm_aln.h:101)
 * an occurrence in front of beg is skipped and the FIRST one that ends behind end ends the walk (hzm_aln.h:160-161: a break - later occurrences of that z-mer are
 * lost even where a shorter homopolymer-expanded length would fit); the length test (hzm_aln.h:162) comes after both.  The second interval test of
 * filter_by_region_hzmps (hzm_aln.h:1194) cannot fail behind that one, and its read-side test cannot fail at all (a z-mer lies inside its read).
 * Everything after the matches is blind to the interval, as in the reference: wtz_pairs_windows / wtz_pairs_align / wtz_fetch_cigars follow unchanged, the end
 * extensions run into the whole indexed read (hzm_aln.h:1714) and tb / te of the alignment may lie outside [beg, end).
 * Needs params.aux_strand = 1 and the zmo engine (params.dot_matrix = 0): WTZ_E_ARG otherwise.  With (0, 0) for every pair it returns what wtz_pairs_seed returns. */
int  wtz_pairs_seed_region(wtz_ctx_t *ctx, const uint32_t *qid, const uint32_t *cid, const int32_t *beg, const int32_t *end, uint32_t n, wtz_pair_summary_t *out);

/* The reference's process-wide HZM_FAST_WINDOW_KMER_CHAINING (hzm_aln.h:36), per context.  fast = 1, the default: every window of a scan
 * (potential_paired_kmers_windows) keeps the members within 50 of its median diagonal, ordered by off1 (hzm_aln.h:488-543) - wtzmo, wtgbo.  fast = 0, what wtmsa
 * and wtcns set at the top of main (wtmsa.c:617, wtcns.c:806): the members of a window are chained by chaining_hzmps (hzm_aln.h:544-561, 351-408) and the chain is
 * the window - its anchors in chain order, its box from the first and the last anchor, its weight the chain's coverage of the read.  The reference hands the
 * window's last member over as an exclusive end (hzm_aln.h:545, 360), so that member is never part of the chain; this is kept.  The setting holds for every later
 * wtz_pairs_seed, wtz_pairs_seed_region and wtz_hzmaux_batch of the context, and wtz_ctx_clone copies it.  fast = 0 needs params.aux_strand = 1 and the zmo engine
 * (the callers that set it are align_hzmaux's): WTZ_E_ARG otherwise, and the setting stays as it was. */
int  wtz_set_window_chaining(wtz_ctx_t *ctx, int fast);

/* The two gap-open costs of the device DPs, per context, as the reference's routines take them (negative or zero): I opens a run of query-only steps (op 1, the E
 * state of kswx_extend_align_shift_core / kswx_extend_align_core: kswx.h:168, column 0 kswx.h:152, the leftover rows of the walk kswx.h:220-223), D a run of
 * target-only steps (op 2, the F state: kswx.h:174, row 0 kswx.h:143, the leftover columns kswx.h:224-227); the band clamp takes max(I, D) (kswx.h:117), the gaps
 * between windows call ksw_global2 with (-I, -E, -D, -E) (hzm_aln.h:1407), kswx_refine_alignment and the z-mer runs carry both.  wtmsa runs align_hzmaux with
 * -2, -3 (wtmsa.c:633-634), wtcns with its -I / -D from the second iteration on (wtcns.c:330, 340).  The default is I = D = params.O - what wtzmo, wtgbo and wtext
 * pass - and wtz_params_c is unchanged.  The setting holds for every later device DP that read params.O before: wtz_pairs_align (windows, gaps, end extensions,
 * the refinement) and through it wtz_hzmaux_batch, wtz_extend_batch, wtz_test_dp, and the planners that size their launches; wtz_ctx_clone copies it.  The services
 * that take their gap costs as arguments (wtz_local_batch, wtz_kext_batch, wtz_align_batch, wtz_alignx_batch, wtz_global_batch) and the dot-matrix engine do not
 * read it.  With I != D the two one-wave register forms of K-sw3 run their split-cost instantiation (wtz_sw_frame.h); with I == D the code that ran before runs.
 * A positive cost or one below -2^20 is WTZ_E_ARG and the setting stays as it was; it waits for the context's stream before it changes the device's block. */
int  wtz_set_gap_open(wtz_ctx_t *ctx, int32_t I, int32_t D);

/* Chain windows of the last wtz_pairs_seed, packed in (pair, strand) order: sum of nwin[] entries. */
int  wtz_pairs_windows(wtz_ctx_t *ctx, wtz_winbox_t *wins, uint64_t n_wins);

/* A9 + A10 for m (pair index into the last wtz_pairs_seed, strand) items. */
int  wtz_pairs_align(wtz_ctx_t *ctx, const uint32_t *pair_idx, const uint8_t *dir, uint32_t m, wtz_aln_result_t *out);
int  wtz_fetch_cigars(wtz_ctx_t *ctx, uint32_t *dst, uint64_t n_ops);
/* the same CIGARs already rendered as text on the device (what the .ovl column 17 holds): sum of text_len bytes */
int  wtz_fetch_cigar_text(wtz_ctx_t *ctx, char *dst, uint64_t n_bytes);
/* wtz_fetch_cigar_text in two halves (kswx_cigar2string kswx.h:1093-1120, as above): _begin renders the text and starts its copy to dst on a stream of its own and
 * returns, _end waits for that copy.  In between the context takes the next range's calls (wtz_batch_begin ... wtz_pairs_align): the copy - 3.4 GB per configs[2]
 * step, 72 ms at the rate of the link - runs beside their kernels.  dst (page-locked: wtz_host_alloc) must not be read before _end returns.  _end may be called
 * from another thread than the one that drives the context. */
int  wtz_fetch_cigar_text_begin(wtz_ctx_t *ctx, char *dst, uint64_t n_bytes);
int  wtz_fetch_cigar_text_end(wtz_ctx_t *ctx);
/* the same text left ON THE DEVICE: *dev_ptr = device address of the n_bytes (valid until the next call on this context).  For a rank that does not write
 * records itself (one process per GPU): the ~6 KB of CIGAR text per record go from this buffer to the committing rank's GPU over xGMI
 * (RCCL send of a tensor that aliases it) without passing through this rank's host memory. */
int  wtz_cigar_text_device(wtz_ctx_t *ctx, uint64_t n_bytes, void **dev_ptr);
/* Page-locked host memory for the buffers the library copies results into (the CIGAR text is ~6 KB per record: a pageable
 * destination halves the copy rate).  Plain malloc semantics otherwise; NULL on failure.  No reference counterpart: the
 * reference formats its records in the worker's own heap (wtzmo.c:1064-1095). */
void *wtz_host_alloc(uint64_t n_bytes);
void  wtz_host_free(void *p);

/* ---- TEST-ONLY entry: function-level parity of every device form of the three banded DPs against vectors dumped from the
 * reference's own routines (tests/golden/dp_vectors.npz, tests/test_gpu_dp_forms.py).  One DP problem per element on sequences taken
 * from the uploaded reads; nothing in the product path calls it.
 *   kind WTZ_DP_SHIFT  <- kswx_extend_align_shift_core kswx.h:101-232   (W as passed to it: negative = exact band)
 *        WTZ_DP_FIXED  <- kswx_extend_align_core       kswx.h:234-335   (band = params.w, as the path always calls it)
 *        WTZ_DP_GLOBAL <- ksw_global2                  ksw.c:503-586    (W = band width of this ONE call; gap costs from params)
 *   form 0 = the form the product would pick (for WTZ_DP_SHIFT: the whole run_extjobs dispatch); otherwise
 *        WTZ_DP_SHIFT : 3 LDS-ring kernel (+ its scalar fallback), 4 scalar body, 5 one-wave kernel in the anti-diagonal frame, 7 the same with two 16-bit cells
 *                       per register; 1, 2 and 6 were kernels that have been removed: their numbers are not reused, the call returns WTZ_E_ARG
 *        WTZ_DP_FIXED / WTZ_DP_GLOBAL : C | 16*pool  (C = 1, 2, 4, 8 band columns per lane; +16 = 4-bit trace in the pool instead of LDS),
 *                       255 scalar body; WTZ_DP_GLOBAL also 32 = LDS-ring wave DP, 33 = the same with the 72 KB slice of the wide launch;
 *                       64 = the lane bodies (one lane per problem, wtz_sw_lane.h) with lane 0 alone in its wavefront: K-sw1 in the ABSOLUTE mode (the reference's
 *                       function for the init_score given; declined beyond 104 band columns, 511 rows, 1500 rows + columns or init_score 2^20), K-sw2 at the band
 *                       width W the problem names (declined for |q_len - t_len| > W, beyond 104 band columns or 768 rows, or an empty side);
 *                       65 = the lane bodies the way the product runs them: problems 64k .. 64k+63 of the call share wavefront k IN THE CALLER'S ORDER (nothing is
 *                       sorted, the last wavefront may be partial; a declined problem leaves its lane idle), the instantiation of a wavefront is the class (16 / 32 /
 *                       64 / 104 band columns) of its widest live problem, and the DP and the traceback are two launches around a lane-interleaved trace block in
 *                       the transient pool (K_ldp / K_ltb, K_gdp / K_gtb).  K-sw1 runs in the RELATIVE mode (init_score 0); the answer is max(init_score, 0) + the
 *                       relative score, unless the fold's rule (wtz_lres_declined) says the shift is not the reference's: then, and for what the planner leaves to
 *                       the chained kernel (a band that depends on init_score, the envelope of form 64, an empty side), form_used = 0.  For form 65 only, W > 0 of
 *                       a WTZ_DP_FIXED problem is the -w of that problem in the place of params.w (one call can hold waves at several -w); K-sw2 as form 64, the
 *                       lanes of a wavefront at their own W, the score reported whether or not the caller would double the band.  The host emulation
 *                       (tests/emul) answers form 65 with the same bodies, one problem per "wavefront"
 *   out[i].form_used = the form that produced the result, 0 = the forced form does not cover this problem (result untouched). */
#define WTZ_DP_SHIFT  0
#define WTZ_DP_FIXED  1
#define WTZ_DP_GLOBAL 2
typedef struct {
	uint32_t q_read, t_read;        /* read ids */
	uint32_t q_rev, t_rev;          /* 1 = reverse-complement view of the read (the candidate's strand '-') */
	int32_t  q_from, t_from;        /* logical position of base 0 of the problem inside the view */
	int32_t  q_strand, t_strand;    /* +1 / -1: walking direction from there (left extensions walk backwards) */
	int32_t  q_len, t_len, init_score, W;
} wtz_dp_problem_t;
typedef struct {
	int32_t  score, tb, te, qb, qe, aln, mat, mis, ins, del;      /* kswx_t; WTZ_DP_GLOBAL: score, aln, mat, mis, ins, del */
	uint32_t cigar_len, form_used;
	uint64_t cigar_off;             /* offset (in words) of this problem's CIGAR inside `cigar` */
	uint64_t cells;                 /* DP cells as the reference loops execute them (extensions) */
} wtz_dp_result_t;
int  wtz_test_dp(wtz_ctx_t *ctx, int32_t kind, int32_t form, const wtz_dp_problem_t *problems, uint32_t n, wtz_dp_result_t *out, uint32_t *cigar, uint64_t cigar_cap);

/* f2: kswx_extend_align (kswx.h:469-481 = kswx_extend_align_shift_core kswx.h:101-232, W as the caller passes it) for n independent problems on
 * views of the uploaded reads - what wtext's worker calls twice per overlap (wtext.c:250, 268) after it clipped the overlap's CIGAR to the retained regions.
 * The jobs go through the same dispatch as the end extensions of wtzmo's stitched alignments.  out[i] = the kswx_t of the call (score, qe, te, aln, mat, mis, ins, del;
 * an empty side returns the start score clamped at 0, like kswx.h:113-118) and cigar_off / cigar_len of its operations (len << 4 | op, first operation first) in `cigar`. */
int  wtz_extend_batch(wtz_ctx_t *ctx, const wtz_dp_problem_t *problems, uint32_t n, wtz_dp_result_t *out, uint32_t *cigar, uint64_t cigar_cap);

/* ksw_align2(qlen, query, tlen, target, 4, mat(M, X), o_del, e_del, o_ins, e_ins, KSW_XSTART, NULL) (ksw.c:344-366) for n independent problems on views of the
 * uploaded reads: the full, unbanded local Smith-Waterman in the reference's 16-bit lanes (ksw_i16, ksw.c:233-335: the kswx callers never set KSW_XBYTE, so
 * H saturates at 32767 like _mm_adds_epi16) and its second pass over the reversed prefixes for the start (ksw.c:358-364).  out[i] = the kswr_t fields as
 * ksw_align2 returns them, inclusive and 0-based, before the callers' ++ (kswx.h:1508-1511): score, te = the smallest target row whose maximum reaches the
 * score (ksw.c:308), qe = the smallest query column holding it (ksw.c:320-322), tb / qb from the second pass (-1 where its maximum differs from the score,
 * ksw.c:363); a score of 0 gives te = -1, qe = 0, tb = qb = 0.  score2 / te2 are not computed (no kswx caller sets KSW_XSUBO).
 * Problems are wtz_dp_problem_t views (q_rev / t_rev, q_from / t_from, q_strand / t_strand, q_len / t_len as for wtz_extend_batch); W and init_score are
 * ignored.  M and X are the context's params (1 <= M <= 127, -128 <= X <= 0: the reference's int8 matrix), the four gap costs are >= 0 with open + extend <= 32767.
 * LIMIT: 1 <= q_len, t_len <= 65535 per problem (one wavefront per problem); anything else is WTZ_E_ARG for the whole call, nothing is truncated and the
 * context stays usable.  form_used = query columns per lane of the first pass (4 up to 256 columns, else 16), cells = rows x columns of both passes as
 * executed.  The call takes 8 * t_len bytes of the main pool per problem whose query exceeds one strip (64 * form_used columns) and leaves the pool empty. */
typedef struct { int32_t score, te, qe, tb, qb; uint32_t form_used; uint64_t cells; } wtz_local_result_t;
int  wtz_local_batch(wtz_ctx_t *ctx, const wtz_dp_problem_t *problems, uint32_t n, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, wtz_local_result_t *out);

/* ksw_extend2(qlen, query, tlen, target, 4, mat(M, X), o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0, &qle, &tle, &gtle, &gscore, &max_off) (ksw.c:381-478)
 * for n independent problems on views of the uploaded reads: the extension with a clip bonus that kswx_extend_core (kswx.h:1386-1441) calls once per end of a
 * local hit.  Rows run over the target, band columns over the query; the band is clamped as ksw.c:403-408 does, follows beg = max(beg, i - w),
 * end = min(end, i + w + 1, qlen) and is trimmed after every row to the zeros around the row's LAST maximum (ksw.c:465-468); a row maximum of 0 (ksw.c:453) or,
 * with zdrop > 0, the z-drop tests (ksw.c:458-462) end the DP.  32-bit arithmetic, no saturation.
 * Problems are wtz_dp_problem_t views as for wtz_extend_batch: q_* is ksw_extend2's query, t_* its target (strand -1 from the far end = the reversed sequences of a
 * left extension, kswx.h:1395), init_score = h0 (clamped at 0, ksw.c:386), W = w.  M and X are the context's params (1 <= M <= 127, -128 <= X <= 0), the gap
 * costs are arguments: o_* >= 0, e_* >= 1 (the reference divides by them, ksw.c:403-406), open + extend <= 32767.
 * out[i] = the return value (score) and the five outputs; rows = DP rows entered before the routine stopped, cells = sum of end - beg over them,
 * form_used = band slots per lane of the kernel instantiation that ran it (1, 2, 4, 8, 16 or 32; chosen from min(w, t_len - 1) + min(w, q_len - 1) + 1 diagonals).
 * LIMIT: 1 <= q_len, t_len <= WTZ_KEXT_MAXLEN (1 048 575), 0 <= W <= WTZ_KEXT_MAXW (1 023: 2 W + 1 diagonals on one wavefront), max(h0, 0) + q_len * M <= 2^30;
 * anything else is WTZ_E_ARG for the whole call before anything is launched, and the context stays usable.  The call takes nothing from the pools and leaves the
 * main pool empty. */
#define WTZ_KEXT_MAXW 1023
#define WTZ_KEXT_MAXLEN 0xFFFFF
typedef struct { int32_t score, qle, tle, gtle, gscore, max_off; uint32_t form_used, rows; uint64_t cells; } wtz_kext_result_t;
int  wtz_kext_batch(wtz_ctx_t *ctx, const wtz_dp_problem_t *problems, uint32_t n, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins,
                    int32_t end_bonus, int32_t zdrop, wtz_kext_result_t *out);

/* kswx_align_no_stat(qlen, query, tlen, target, 4, mat(M, X), w, I, D, E, T) (kswx.h:1504-1511) for n independent problems as three device batches:
 *   1  wtz_local_batch with (-D, -E, -I, -E) (kswx.h:1506); a problem whose qb, tb, qe or te is <= -1 is KSWR_NULL (kswx.h:36, 1507): found = 0, all else 0;
 *      qe and te become exclusive (kswx.h:1508);
 *   2  only when T < 0: every left extension (kswx.h:1390-1415), 3  every right extension (kswx.h:1417-1438), each from the score the step before left.
 *      Per problem the longer remaining side is ksw_extend2's target and is cut to the other side + w; where the problem's target plays ksw_extend2's query the
 *      opening costs change places (kswx.h:1407, 1431).  end_bonus = -T, zdrop = -1.  gscore <= 0 || gscore <= score + T keeps (qle, tle, score), otherwise the
 *      extension runs to the end of the column side with (gtle, gscore).  An end already at 0 / at the sequence end is not extended (kswx.h:1391, 1418).
 *      A stage is at most two K-kext launches groups (one per role), through the launch path of wtz_kext_batch.
 * I, D, E, T as kswx_align receives them (costs as negative numbers, e.g. -3, -3, -1, -100): I, D <= 0, E <= -1; 0 <= w <= WTZ_KEXT_MAXW.  W and init_score of
 * the problems are ignored.  out[i]: found, the extended rectangle [tb, te) x [qb, qe) and its score, and the local hit it grew from (local_te / local_qe
 * exclusive too).  The limits of both underlying calls apply (1 <= q_len, t_len <= 65535) and are checked before anything runs: WTZ_E_ARG for the whole call.
 * What kswx_align (kswx.h:1495-1502) does beyond this - one ksw_global2 over the rectangle with its statistics (kswx.h:1443-1482) - is wtz_alignx_batch below. */
typedef struct { int32_t found, score, tb, te, qb, qe; int32_t local_score, local_tb, local_te, local_qb, local_qe; } wtz_align_result_t;
int  wtz_align_batch(wtz_ctx_t *ctx, const wtz_dp_problem_t *problems, uint32_t n, int32_t w, int32_t I, int32_t D, int32_t E, int32_t T, wtz_align_result_t *out);

/* ksw_global2(qlen, query, tlen, target, 4, mat(M, X), o_del, e_del, o_ins, e_ins, w, &n_cigar, &cigar) (ksw.c:503-586) for n independent problems on views of the
 * uploaded reads: the banded global alignment at ONE band width, W of the problem = w of that call (init_score is ignored).  Rows run over the target, band columns
 * over the query; the tie rules of ksw.c:549-562 and the walk of ksw.c:571-579 with both of its tails are the reference's.  M and X are the context's params
 * (1 <= M <= 127, -128 <= X <= 0), the four gap costs are arguments, >= 0 with open + extend <= 32767.
 * out[i]: score = the return value; aln, mat, mis, ins, del folded from the CIGAR EXACTLY as kswx_gen_cigar_core2 does (kswx.h:1468-1477): op 1 (query only) is
 * counted in del and op 2 (target only) in ins - the other way round than the fold behind wtz_test_dp; cigar_off / cigar_len of the operations (len << 4 | op, first
 * operation first) in `cigar` (cigar = NULL with cigar_cap = 0: statistics only, cigar_off = cigar_len = 0); cells = sum of end - beg over the rows;
 * form_used = the form that ran the problem: 1, 2, 4, 8, 16, 32 = band slots per lane of the K-glob instantiation (up to WTZ_GLOB_MAXSLOTS = 2 047 slots,
 * slots = min(W, t_len - 1) + min(W, q_len - 1) + 1; the narrowest instantiation that holds them), 33 = the LDS-ring wave DP with its 72 KB slice
 * (up to 8 190 band columns and 32 k query bases), 255 = the scalar body on one lane (everything else; in the host emulation every wide problem).
 * LIMITS, all checked before anything is launched (WTZ_E_ARG for the whole call, the context stays usable): 1 <= q_len, t_len <= 65535; W >= 0;
 * |q_len - t_len| <= W (outside the band the reference returns MINUS_INF and walks back through bytes it never wrote);
 * 2 * max(o) + max(e) * (q_len + t_len + 2) + max(M, -X) * (max(q_len, t_len) + 1) <= 2^28 (32-bit cells, sentinel at -2^30).
 * The trace of a launch group comes from the main pool: the library cuts the call into groups that fit it, largest problems first; one problem whose trace does not
 * fit is WTZ_E_POOL (K-glob: 2 bytes per band slot of the instantiation and row, i.e. 32 * C bytes per row, + 4 * (q_len + t_len) of runs).  The call leaves the
 * main pool empty. */
#define WTZ_GLOB_MAXSLOTS 2047
typedef struct { int32_t score, aln, mat, mis, ins, del; uint32_t cigar_len, form_used; uint64_t cigar_off, cells; } wtz_global_result_t;
int  wtz_global_batch(wtz_ctx_t *ctx, const wtz_dp_problem_t *problems, uint32_t n, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins,
                      wtz_global_result_t *out, uint32_t *cigar, uint64_t cigar_cap);

/* kswx_align / kswx_align_with_cigar(qlen, query, tlen, target, 4, mat(M, X), w, I, D, E, T[, &n_cigar, &cigar]) (kswx.h:1495-1502, 1513-1520) for n independent
 * problems: the three stages of wtz_align_batch (the same functions), then kswx_gen_cigar_core2 (kswx.h:1443-1482): the band rule of kswx.h:1452-1461 (the
 * x1 * 1.5 comparison and assignment in double arithmetic truncated to int, w2 from matrix[0] = M and integer division by -E, a negative w = the exact band -w) and
 * one wtz_global_batch stage over [tb, te) x [qb, qe) with (-D, -E, -I, -E).
 * out[i]: found; the kswx_t (score = ksw_global2's, the rectangle, aln / mat / mis / ins / del as above); band = the band the rule gave; form_used;
 * cigar_off / cigar_len as for wtz_global_batch.  found = 0: everything else is 0 (KSWX_NULL).
 * Arguments and limits as for wtz_align_batch; in addition w in [-1023, -1] is accepted together with T >= 0 (with T < 0 the reference hands the negative band to its
 * extensions, where lengths go negative: WTZ_E_ARG).  For path scores the rule always yields a band >= |(te - tb) - (qe - qb)|; the library checks that and
 * fails the call with WTZ_E_STATE instead of running a DP whose corner is outside the band.  With an exact band the caller's input can do that too: a local hit
 * whose rectangle has |(te - tb) - (qe - qb)| > -w.  That is also WTZ_E_STATE, for the WHOLE call (the text names the problem; no result of the call is valid): the
 * reference would return MINUS_INF there and walk back through bytes it never wrote, so there is no per-problem result to report.  A caller that cannot rule such hits
 * out runs wtz_align_batch first and passes only the problems whose rectangle fits its band. */
typedef struct { int32_t found, score, tb, te, qb, qe, aln, mat, mis, ins, del, band; uint32_t form_used, cigar_len; uint64_t cigar_off; } wtz_alignx_result_t;
int  wtz_alignx_batch(wtz_ctx_t *ctx, const wtz_dp_problem_t *problems, uint32_t n, int32_t w, int32_t I, int32_t D, int32_t E, int32_t T,
                      wtz_alignx_result_t *out, uint32_t *cigar, uint64_t cigar_cap);

/* kswx_cigar2pairwise(alns, seqs, n_cigar, cigar) (kswx.h:1150-1194) followed by the marker loop of pairaln.c:115-125 for n alignments: the three-line picture
 * that `pairaln -a` prints.  Alignment i is the view pair problems[i] (q_read / t_read / q_rev / t_rev / q_from / t_from / q_strand / t_strand / q_len / t_len as in
 * wtz_global_batch; init_score and W are ignored; a side of length 0 is allowed), a start (in[i].qb, in[i].tb) inside the views - seqs[0] = query + qb,
 * seqs[1] = target + tb, pairaln.c:114 - and the operations cigar[in[i].cigar_off, + in[i].cigar_len), len << 4 | op as wtz_alignx_batch returns them: op 0 writes both
 * bases, op 1 the query base over '-', op 2 '-' over the target base; operations of length 0 are skipped (kswx.h:1157).  Bases are upper case (bit_base_table).
 * out[i].cols = the sum of the lengths; the picture is 3 * (cols + 1) bytes at text + out[i].text_off, pictures in input order without gaps: the query line, '\n',
 * the marker line, '\n', the target line, '\n' (alns[0], alns[2], alns[1]: pairaln.c:126).  Marker: '-' where the query line has '-', else '|' where the lines are
 * equal, else '-' where the target line has '-', else '*'.  cigar_len = 0 (KSWX_NULL) gives three '\n'.
 * text = NULL with text_cap = 0 is the sizing call: out[i].cols / text_off only, nothing is launched.
 * LIMITS, all checked before anything is launched (WTZ_E_ARG for the whole call, the context stays usable): an op other than 0 / 1 / 2 (the reference exits);
 * a CIGAR that walks past q_len - qb or t_len - tb (the reference reads on); qb / tb outside [0, q_len] / [0, t_len]; a slice outside n_ops; text_cap smaller than
 * the sum; q_len, t_len <= 65535.
 * The device picture, the CIGAR words and one 8-byte table entry per operation come from the main pool: the library cuts the call into launch groups that fit it, in
 * input order (results do not depend on the cut); one alignment that needs more than the main pool (12 bytes per operation + 3 * (cols + 1)) is WTZ_E_POOL.  The
 * call leaves the main pool empty. */
typedef struct { int32_t qb, tb; uint32_t cigar_len, pad; uint64_t cigar_off; } wtz_pwtext_in_t;
typedef struct { uint64_t text_off; uint32_t cols, pad; } wtz_pwtext_result_t;
int  wtz_pwtext_batch(wtz_ctx_t *ctx, const wtz_dp_problem_t *problems, const wtz_pwtext_in_t *in, uint32_t n, const uint32_t *cigar, uint64_t n_ops,
                      wtz_pwtext_result_t *out, char *text, uint64_t text_cap);

/* align_hzmaux(aux, rid, rdseq, NULL, rdlen, beg, end, params.refine, params.min_id) (hzm_aln.h:1684-1775) for n (target read tid[i], query read rid[i]) pairs
 * in one call - what wtmsa runs per read of a layout against a region of the backbone (wtmsa.c:448-477) and, with (0, -1), per N read:
 *   wtz_pairs_seed_region (hzm_aln.h:1690-1699) -> wtz_pairs_align of the pairs with windows and a chain of at least zovl (hzm_aln.h:1700-1714; with
 *   params.refine kswx_refine_alignment, hzm_aln.h:1721-1729, band params.w) -> the gates of hzm_aln.h:1715-1718 in the reference's float arithmetic (with
 *   params.refine the device applied them in front of the refinement) -> the CIGARs of the hits.
 * out[i]: found = align_hzmaux's return value; the kswx_t aux->hit (hzm_aln.h:1730; all 0 without a hit); cigar_off / cigar_len of its operations
 * (len << 4 | op, op 0 both, 1 query only, 2 target only: hzm_aln.h:1737-1772) in `cigar`, hits packed in pair order.  cigar = NULL with cigar_cap = 0: the
 * records alone.  A cigar_cap smaller than the sum of the hits' cigar_len is WTZ_E_ARG, the text names the words needed and out[] is complete (offsets
 * included), so the caller can allocate and call again.
 * Needs params.aux_strand = 1 and the zmo engine (WTZ_E_ARG), and both reads of every pair in the z-index (wtz_zindex_build, or wtz_zindex_build_subset of the
 * targets AND the queries: the device reads a query's position-ordered z-mers from the index too) - WTZ_E_STATE otherwise.  The gap-open costs of every
 * device DP are the context's pair (wtz_set_gap_open: align_hzmaux's I and D, e.g. -2, -3 as wtmsa passes them); until it is called both are params.O.  WTZ_E_POOL: nothing was returned, use fewer pairs per call (the halving loop of the batch tools, ht_halving).
 * The call ends the batch it ran, on success and on failure alike: the main pool goes back empty, wtz_pairs_windows / wtz_pairs_align need a new wtz_pairs_seed. */
typedef struct { int32_t found, score, tb, te, qb, qe, aln, mat, mis, ins, del; uint32_t cigar_len; uint64_t cigar_off; } wtz_hzmaux_result_t;
int  wtz_hzmaux_batch(wtz_ctx_t *ctx, const uint32_t *tid, const uint32_t *rid, const int32_t *beg, const int32_t *end, uint32_t n,
                      wtz_hzmaux_result_t *out, uint32_t *cigar, uint64_t cigar_cap);

/* Scratch accounting, so that the caller can size its batches to the pool instead of discovering the limit by WTZ_E_POOL:
 * the context's scratch is cut into a main pool (everything that lives for the batch: match lists, windows, CIGARs) and a transient
 * pool (K-sw3 trace matrices; the library sizes its own launch groups to it).  main_used = bytes of the main pool in use after the
 * last stage call (wtz_pairs_seed / wtz_pairs_align), transient_peak = high-water mark of the transient pool during it. */
typedef struct { uint64_t main_cap, main_used, transient_cap, transient_peak; } wtz_pool_info_t;
int  wtz_pool_info(wtz_ctx_t *ctx, wtz_pool_info_t *out);
/* which pool the context's last WTZ_E_POOL came from: 0 = none yet, 1 = the main pool (the caller's bytes-per-pair estimate was too low: plan smaller ranges from
 * now on), 2 = the transient trace pool of the K-sw3 launches (the library's own trace budget was too low and has been raised: redo the range, keep the estimate) */
int  wtz_pool_failure_kind(wtz_ctx_t *ctx);

int  wtz_get_counters(wtz_ctx_t *ctx, wtz_counters_t *out);
int  wtz_reset_counters(wtz_ctx_t *ctx);

#ifdef __cplusplus
}
#endif
#endif
