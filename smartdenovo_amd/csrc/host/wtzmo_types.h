/* wtzmo host driver, section 1 of 6: the types every section shares and the process-wide helpers.  wtzmo_main.c includes the sections once each, in this order:
 * wtzmo_types.h, wtzmo_out.h, wtzmo_commit.h, wtzmo_stages.h, wtzmo_ranks.h, wtzmo_ranges.h - one translation unit, everything static. */
static double now_s(void){ struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }
static inline void cpu_relax(void){
#if defined(__x86_64__) || defined(__i386__)
	__builtin_ia32_pause();
#elif defined(__aarch64__) || defined(__arm__)
	__asm__ __volatile__("yield");
#else
	sched_yield();
#endif
}
#define SWAP(T, a, b) do { T t_ = (a); (a) = (b); (b) = t_; } while(0)
typedef struct { uint64_t e; uint32_t pidx; uint32_t pad; } cand_t;
#define GT_CAND(a, b) ((uint32_t)(b)->e > (uint32_t)(a)->e)                  /* wtzmo.c:821 */
HX_DEFINE_SORT_EXACT(sort_cands_exact, cand_t, GT_CAND)
static int gt_read(const void *a, const void *b, void *ctx){ (void)ctx; return ((const hx_read_t*)b)->len > ((const hx_read_t*)a)->len; }               /* wtzmo.c:1708 */

typedef struct { uint32_t pb2, dir, ovl, closed, pidx; } seed_t;
#define GT_SEED(a, b) ((b)->ovl > (a)->ovl)                                 /* wtzmo.c:986 */
HX_DEFINE_SORT_EXACT(sort_seeds_exact, seed_t, GT_SEED)
/* what the order-free part of a query's commit (closed filter, candidate order, window depth, seed weights, seed order) leaves for the sequential part;
 * buffers grow and are kept.  dep: +1 / -1 marks, then the running depth, as 16-bit words (the reference's counters are u2i and wrap the same way): zero between queries */
typedef struct {
	cand_t *cand; size_t capcand; seed_t *seeds; size_t capseeds; uint16_t *dep; size_t capdep;
	uint32_t nc, nseed, ngate; double t[5];      /* t: candidate rows + closed filter + order | window marks | running depth | seed weights | seed order */
} cq_work_t;

typedef struct { uint32_t pb1, pb2, dir2; int qb, qe, tb, te, score, mat, mis, ins, del, aln; char *cigar; } hit_t;

typedef struct {      /* results of the query processed last, not yet merged into the global state */
	uint32_t rd_id;
	hit_t *hits; size_t nhit, caphit;
	uint32_t *masks; size_t nmask, capmask;
	uint64_t *closed; size_t nclosed, capclosed;
	seed_t *seeds; size_t nseed, capseed;
} pending_t;

typedef struct eng_s {
	wtz_params_c P; int do_align; uint32_t n_idx, n_job, i_job;
	hx_store_t st; uint8_t *masked; uint32_t *rdcovs; hx_set_t closed;
	uint32_t *rdlen; uint32_t avg_rdlen;
	uint64_t *closed_order; size_t n_order, cap_order; int keep_order;      /* -9: the pairs in the order they entered closed_alns (the file is a replay of it) */
	wtz_ctx_t *ctx; FILE *out;
	double ing_ms; uint64_t ing_bytes;      /* f4: kernel time / algorithmic bytes of the device ingest at load time (wtz_upload_reads_ascii) */
	int zbatch;                 /* --zindex-batch (automatic above ~2.4 Gbp of reads): the z-mer index is rebuilt per batch of queries for the batch's queries + candidates instead
	                             * of once for all reads (16 B per base: 160 GB at BASELINE configs[3]) */
	int binary_out;             /* --binary-out: 64-byte binary records behind a name table (include/wtz_ovlb.h) instead of the 17 text columns; the CIGAR text is not fetched */
	int zsplit;                 /* several parts (devices or ranks): part d's z-mer index holds the candidate side of the reads = d (mod nparts) only, the queries of a batch get their own small
	                             * index per batch (wtz_zindex_build_queries) - the replicated all-reads build (0.135 s of a 3.2 s configs[2] step, not divided by N) becomes 1 / N of it */
	int shard;                  /* --shard-index: the k-mer index is sharded by read-id range over the devices (reads and z-index stay replicated); output == unsharded */
	uint32_t ndev; int devs[8]; wtz_ctx_t *ctxs[8];      /* --gpus N / --gpu-list: one context per device, reads + both indexes replicated; ctx == ctxs[0] */
	/* candidate rows carried across -G index parts (the reference's rdhits), else NULL */
	uint64_t *rows; uint32_t *nrow; uint32_t stride;
	uint32_t max_batch, first_batch, n_workers; int first_batch_set;
	/* pipeline: batches are planned in query order by whichever worker is free, computed on that worker's context
	 * (own HIP stream + scratch pool) and committed strictly in sequence */
	pthread_mutex_t mu; pthread_cond_t cv;
	/* planned batch sizing: main-pool bytes a pair has needed so far (largest seen, reads are processed longest first), so that the pairs of
	 * a range are cut to fit the pool BEFORE the device stages run; WTZ_E_POOL and the halving below it remain as the safety net */
	double bpp_decay; uint64_t main_cap;
	pending_t pend;
	/* commit_query scratch kept across queries (round 6: the two calloc'ed depth arrays of a query were 60 KB of zeroing + a 10 000-step scalar prefix each -
	 * more than half of the sequential commit): cq_dep = +1 / -1 marks, then the running depth, as 16-bit words (the reference's counters are u2i and wrap the
	 * same way); only the span the query's windows touch is summed, and it is zeroed again behind the query */
	cq_work_t cq;                      /* the commit thread's own */
	struct cq_spec_s *spec;            /* helper threads that prepare the queries ahead of the commit (cq_spec_*) */
	uint32_t *closed_touch;            /* per read: number of closed pairs with this read added so far; a prepared query is valid iff its read's count has not moved */
	char *cig_keep[16]; uint64_t cig_keep_cap[16];      /* page-locked CIGAR text buffer of worker w, kept across steps (pinning is the expensive part) */
	uint64_t cand_main_cap; uint32_t cand_cap0;      /* seed lookup: the pool the requests so far ran in; cand_cap0: batch cap until the first measurement (large inputs) */
	uint8_t *masked0; uint64_t *closed0; size_t nclosed0, n_order0;      /* --repeat: masks, closed pairs and -9 order as loaded (-F, -L): what every step starts from */
	struct {      /* what a step starts from zero: step_reset() is the one place that resets it (whatever must survive a repeat - reads, cig_keep, main_cap, ingest figures - is above) */
		int rows_all; uint32_t cursor, qend, B; uint64_t next_seq, commit_seq; double bytes_per_pair; uint64_t n_split, n_ranges;
		uint64_t pair_bp, n_pairs, nrec, n_spec_hit, n_spec_miss; double t_spec_wait, t_spec_ctl, t_flush;
		double t_cq1[4];            /* section 1 of commit_query in its parts: window marks | running depth | seed weights | seed order */
		double t_cq[4];             /* commit_query sections: candidate rows + closed filter + sort | window depth + seed weights + sort | hits (gates, queueing, masking) | plan_pairs */
		double t_gpu, t_commit, t_zbatch, t_call[6], t_io[2];      /* t_io: waiting for the writer thread before a text buffer is reused / at the end of the run */      /* t_call: wall seconds inside wtz_candidates / pairs_seed / pairs_windows / pairs_align / fetch_cigar_text / planning */
		uint64_t spec_pairs, used_pairs, spec_items, used_items, spec_queries, used_queries, n_batches;
		double pair_row_ratio;       /* planned pairs per candidate row of the ranges before (plan_pairs): the rows bound a range, closed pairs and masked queries thin them out */
		uint64_t n_masked;           /* reads masked by commits of this step (flush_pending) */
		double cand_bpq;             /* seed lookup: main-pool bytes per query of the requests so far (the largest) */
		double last_mask_rate;       /* new masks per used query of the batch that finished last (process_batch: may the next batch be formed in front of the last commit?) */
		double extra_ms[6]; uint64_t extra_u64[7];      /* counters of the cloned contexts */
	} step;
} eng_t;
/* ---- ranks: with one process per GPU (torchrun; bench.py / tests set the exchange hooks through wtzmo_set_dist) the parts of rank 0's
 * batches live in the OTHER PROCESSES: rank 0 plans and commits (the order-dependent part of `wtzmo -t 1` is one sequential
 * stream by definition), every rank runs the pure device stages of its share of the pairs / candidate requests on its own GPU with
 * reads and both indexes replicated, and the results travel to rank 0 (RCCL send / recv when the hooks sit on the nccl backend).
 * One .ovl, written by rank 0, identical to `wtzmo -t 1` for any number of ranks; total work is fixed (strong scaling). ---- */
typedef void (*wtz_dist_bcast_fn)(void *buf, uint64_t nbytes);                   /* from rank 0, same nbytes on every rank */
typedef void (*wtz_dist_send_fn)(const void *buf, uint64_t nbytes, int dst);
typedef void (*wtz_dist_recv_fn)(void *buf, uint64_t nbytes, int src);
typedef void (*wtz_dist_send_dev_fn)(const void *dev_buf, uint64_t nbytes, int dst);      /* like send, but the bytes live in DEVICE memory of this rank's GPU */
static struct { int rank, world; wtz_dist_bcast_fn bcast; wtz_dist_send_fn send; wtz_dist_recv_fn recv; wtz_dist_send_dev_fn send_dev; } g_dist = { 0, 1, NULL, NULL, NULL, NULL };
void wtzmo_set_dist(int rank, int world, wtz_dist_bcast_fn b, wtz_dist_send_fn sd, wtz_dist_recv_fn rv){
	g_dist.rank = rank; g_dist.world = world < 1 ? 1 : world; g_dist.bcast = b; g_dist.send = sd; g_dist.recv = rv; g_dist.send_dev = NULL;
}
/* optional: with this hook a rank > 0 hands its CIGAR text (the bulk of what travels: ~6.4 KB per record, 3.1 GB per configs[2] step) to the exchange straight
 * from the device buffer the library rendered it into (wtz_cigar_text_device) - device to device over xGMI on the nccl backend, no copy through this rank's host */
void wtzmo_set_dist_dev(wtz_dist_send_dev_fn f){ g_dist.send_dev = f; }
#define WTZ_DIST_MAX 16
enum { WTZ_CMD_DONE = 1, WTZ_CMD_PAIRS = 2, WTZ_CMD_CAND_BEGIN = 3, WTZ_CMD_CAND_END = 4, WTZ_CMD_GRP_BEGIN = 5, WTZ_CMD_GRP_END = 6,
       WTZ_CMD_ZIDX = 7,       /* the z-mer index of the batch: arg[0] queries (their ids follow as a broadcast) for the query-side index of every rank; arg[1] != 0: count[r] candidate
                                * reads (ids sent to rank r) for rank r's per-batch candidate-side index (--zindex-batch) */
       WTZ_CMD_ABORT = 8 };    /* rank 0 -> all: some rank failed; every rank leaves with exit code 1 (the reference's convention for every error: list.h:64-67) */
typedef struct { uint64_t cmd, arg[2], count[WTZ_DIST_MAX]; } wtz_dist_hdr_t;
/* Every reply of a rank > 0 starts with a status word: 0 = fine, 1 = scratch pool too small (the range is halved and redone), 2 = this rank failed (its own
 * stderr says why).  On 2, rank 0 finishes the round of the exchange it is in (the other ranks' replies are already on their way), broadcasts WTZ_CMD_ABORT
 * and every process exits 1 - nobody is left blocked in a receive. */
enum { WTZ_ST_OK = 0, WTZ_ST_AGAIN = 1, WTZ_ST_FAILED = 2 };

/* The pairs of a range are dealt to the PARTS of a batch, one part per GPU (--gpus N, or one rank per GPU; one part otherwise): pair
 * (q, c) belongs to part c % nparts.  Every device stage is pure in its pairs, so a part runs pair seeding, windows, alignment and
 * CIGAR rendering of its share on its own context, all parts side by side; the commit reads the results through PART_OF / LOCAL_OF
 * in the plan's order, i.e. the output does not depend on the number of parts.  Dealing by candidate (round 4; it was round-robin)
 * is what lets the z-mer index be split: part d walks only reads = d (mod nparts) as candidates, so its index holds the candidate side
 * of that residue class only (1 / nparts of the build) plus a small query-side index of the batch's queries (wtz_zindex_build_queries). */
typedef struct {
	wtz_ctx_t *ctx; int remote;                 /* remote > 0: the part is computed by that rank (ctx == NULL here) */
	uint8_t *xbuf; uint64_t xcap;              /* ranks: staging of one packed message (round 6: a request is ONE message, a reply a status word + ONE message + the CIGAR text) */
	uint32_t *pq, *pc; uint32_t npair, cappair;
	wtz_pair_summary_t *sum; uint64_t *box_off; wtz_winbox_t *boxes; uint64_t nbox, capbox;
	uint32_t *item_of; uint32_t *it_pair; uint8_t *it_dir; uint32_t nitem; wtz_aln_result_t *aln; char *cig; uint64_t ncig;
	void *cig_dev;               /* rank > 0 with a device-send hook: the text stays on the device (wtz_cigar_text_device) */
	int text_pending;           /* wtz_fetch_cigar_text_begin has been called for this range: part_text_wait() before the text is read */
	char *cigs[2]; uint64_t capcigs[2]; int cig_sel, cig_ext, ext_base;      /* two page-locked CIGAR text buffers, alternating per range; ext ids of the output writer */
	double t_call[6], t_io0;                   /* wall seconds of this part's device calls since the last fold into E (under E->mu) */
	struct eng_s *E; int again;                /* result of the last part_stages run (1 = scratch pool too small) */
	uint32_t *cq_ids, *cq_nr; uint64_t *cq_rows; uint32_t cq_n, cq_cap;      /* this device's share (every nparts-th query) of the candidate request in flight */
} part_t;
#define PIDX(part, local) (((uint32_t)(local) << 4) | (uint32_t)(part))      /* a pair of the plan: part (device / rank) in the low 4 bits, its index inside the part above */
#define PART_OF(b, g) (&(b)->parts[(g) & 15u])
#define CPART_OF(b, g) (&(b)->cparts[(g) & 15u])      /* commit side */
#define LOCAL_OF(b, g) ((g) >> 4)
#define DEAL_PART(np, q, c) ((c) % (np))               /* the part a pair is dealt to: by CANDIDATE id, so that a device only needs the candidate-side z-mers of its own residue class of reads */

typedef struct batch_s {       /* one batch in flight */
	eng_t *E; wtz_ctx_t *ctx; uint64_t seq;    /* ctx: the context of the candidate requests (= parts[0].ctx) */
	uint32_t *bq; uint32_t nbq, capbq;         /* queries in dispatch order */
	uint8_t *want;                              /* slot needs GPU work (not saturated when planned) */
	uint64_t *rows; uint32_t *nrow;             /* candidate heap arrays per slot (stride E->stride) */
	uint32_t *ids;
	part_t *parts; uint32_t nparts;
	part_t *cparts, *spare;                     /* cparts: the result arrays the commit reads (== parts unless ranges are pipelined: then the finished range's
	                                             * arrays are swapped into `spare` and the device stages of the next range fill `parts` meanwhile) */
	uint32_t npair, nitem;                      /* pairs / alignment items of the range over all parts */
	uint32_t *rowpair; size_t caprowpair;       /* pair index (in plan order) per (slot, row entry) */
	uint64_t spec_queries, used_queries;
	int holds_turn;
	/* candidates of the NEXT batch, requested before this batch is committed (single worker, no -G) */
	int pf_inflight; uint32_t *pf_ids; uint32_t pf_n, pf_cap; uint64_t *pf_rows; uint32_t *pf_nr; uint32_t pf_cursor_end;
	/* batches pipelined like ranges (single worker, one process): while the LAST range of this batch is committed, `alt` - a second batch on the same
	 * context(s) - has been formed from the prefetched candidates and runs its first range.  formed: batch_form() has run; started: its first range [0, start_s1) is
	 * already on the device (start_job) */
	struct batch_s *alt; int shares_ctx, formed, started; uint32_t start_s1; void *start_job; uint64_t masked_at_form;
} batch_t;

/* a device-stage failure ends the process at once: other host threads (index builders, parts) may still be inside HIP calls, and running the
 * exit handlers / the HIP runtime's teardown under them ends in a segmentation fault instead of exit code 1 */
#define DIE_NOW() do { fflush(NULL); _exit(1); } while(0)
#define DIE_WTZ(rc, what) do { if((rc) != WTZ_OK){ fprintf(stderr, " -- %s failed: %s --\n", what, wtz_last_error()); DIE_NOW(); } } while(0)
/* a device stage of a part failed: 1 = scratch pool too small (nothing changed, the range is halved), otherwise fatal - at once in a one-process run; between
 * ranks the part reports WTZ_ST_FAILED so that the exchange in flight is finished and rank 0 can end every rank in-band (ranks_abort) */
#define TRY_WTZ(rc, what) do { if((rc) == WTZ_E_POOL) return WTZ_ST_AGAIN; \
	if((rc) != WTZ_OK && g_dist.world > 1){ fprintf(stderr, " -- rank %d: %s failed: %s --\n", g_dist.rank, what, wtz_last_error()); return WTZ_ST_FAILED; } DIE_WTZ(rc, what); } while(0)
static uint32_t nbest_of(const eng_t *E, uint32_t id){
	uint32_t nb = (uint32_t)(((size_t)E->P.nbest) * E->rdlen[id] / E->avg_rdlen);      /* wtzmo.c:806-807 */
	return nb < E->P.nbest ? E->P.nbest : nb;
}
