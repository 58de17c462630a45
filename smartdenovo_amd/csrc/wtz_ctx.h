/*
 * wtz_ctx.h — the context behind wtz_ctx_t: its fields (every one initialised where it is declared), the debugging switches read
 * once per context, the two scratch pools (reset / check), create / clone / destroy and the helpers that park index buffers for the
 * next build.  Included by wtz_lib.cpp after wtz_dev.h.
 */
/* the WTZ_* debugging switches, read once per context (wtz_switches_read), not lazily from worker threads */
struct wtz_switches {
	uint32_t xcd_group = 256;   /* WTZ_XCD_GROUP: consecutive pairs per XCD run in K_pair (0 = identity block -> pair mapping) */
	int zread = 1;           /* WTZ_ZREAD=0: every read's z-mer index by the device-wide form (strided fill + radix sort) instead of one workgroup per read (wtz_task_zread) */
	int ext_fused = 1;       /* WTZ_EXT_FUSED=0: the two end extensions of a stitched overlap in two launches with K_stitch_mid between them instead of on one wavefront (wtz_stitch_fused.h) */
	int ext_pk = 1;          /* WTZ_EXT_PK=0: K-sw3 without the packed 16-bit form (wtz_sw_frame16.h) in front of the 32-bit frame form */
	int heavy_first = -1;    /* WTZ_PAIR_HEAVY_FIRST: the heaviest pairs of a K_pair launch first (-1 = engine default: dmo on, zmo off) */
	int gap_lane = 1;        /* WTZ_GAP_LANE=0: every gap on a wavefront (the form before round 3) */
	int lane = 1;            /* WTZ_WINALIGN_LANE=0: the chained wave-per-window kernel for every window (the form before round 3); 2: run both and compare */
	bool trace = false;      /* WTZ_STAGE_TRACE: name every device stage on stderr before it is launched (locating a device fault) */
	bool fail_once = false;      /* WTZ_POOL_FAIL_ONCE: the injected failure hits one stage call only (the retry must then succeed) */
	unsigned fail_at = 0, tfail_at = 0;      /* WTZ_POOL_FAIL_AT / WTZ_TPOOL_FAIL_AT: fault injection into the main / transient pool (cleared by the first hit under WTZ_POOL_FAIL_ONCE) */
	/* read by the product only: the host emulation has one form of these stages */
	int dm_first_big = 1;    /* WTZ_DM_FIRST_BIG=0: the first K_pair_dm launch without the pool image of a strand (the larger LDS tiers take every such pair) */
	int sw_mode = 0;         /* WTZ_SW_SCALAR=1: K-sw3 by the scalar body (1); WTZ_SW_CHECK=1: both, any difference is fatal (2) */
	int gap_side = 0;        /* WTZ_GAP_SIDESTREAM=1: K-sw2 on a stream of its own beside the left extensions */
	bool profile = false;    /* WTZ_PROFILE_PAIR: per-stage profile lines on stderr */
};
static int env_int(const char *name, int dflt){ const char *e = getenv(name); return e ? atoi(e) : dflt; }
static void wtz_switches_read(wtz_switches *s){
	s->xcd_group = (uint32_t)env_int("WTZ_XCD_GROUP", (int)s->xcd_group);
	s->zread = env_int("WTZ_ZREAD", s->zread);
	s->ext_fused = env_int("WTZ_EXT_FUSED", s->ext_fused);
	s->ext_pk = env_int("WTZ_EXT_PK", s->ext_pk);
	s->heavy_first = env_int("WTZ_PAIR_HEAVY_FIRST", s->heavy_first);
	s->gap_lane = env_int("WTZ_GAP_LANE", s->gap_lane);
	s->lane = env_int("WTZ_WINALIGN_LANE", s->lane);
	s->trace = getenv("WTZ_STAGE_TRACE") != NULL;
	s->fail_once = getenv("WTZ_POOL_FAIL_ONCE") != NULL;
	s->fail_at = (unsigned)env_int("WTZ_POOL_FAIL_AT", 0);
	s->tfail_at = (unsigned)env_int("WTZ_TPOOL_FAIL_AT", 0);
#ifndef WTZ_EMUL
	s->dm_first_big = env_int("WTZ_DM_FIRST_BIG", s->dm_first_big);
	s->sw_mode = env_int("WTZ_SW_CHECK", 0) ? 2 : env_int("WTZ_SW_SCALAR", 0) ? 1 : 0;
	s->gap_side = env_int("WTZ_GAP_SIDESTREAM", 0) ? 1 : 0;
	s->profile = getenv("WTZ_PROFILE_PAIR") != NULL;
#endif
}

struct wtz_ctx {
	int device = 0;
	wtz_switches sw;
	/* z-index arrays of the previous build, kept for the rebuild (same read set -> same sizes): freeing and re-allocating 19 GB per
	 * build cost 0.1 - 0.8 s of hipFree / hipMalloc at configs[2], depending on what else the host's memory manager was doing */
	/* two z-index slots: [0] = the index proper (all reads, or the subset of the batch in flight), [1] = optional second index holding only the
	 * QUERIES of the batch in flight (wtz_zindex_build_queries): with several GPUs every device keeps slot 0 for its own share of the candidate
	 * reads and rebuilds the small slot 1 per batch, instead of all devices building the z-index of all reads */
	struct zslot_t {
		std::vector<std::pair<void*, size_t> > parked, live;
		uint64_t *zoff = NULL; uint64_t n_z = 0; wtz_zindex_t Z; bool have = false; bool sub = false; uint64_t sub_cap = 0;      /* sub: the slot holds a subset of the reads (rebuilt per batch) */
		std::vector<uint32_t> members;      /* sub: the ids of the reads the slot holds, ascending (holds()) */
		zslot_t(){ memset(&Z, 0, sizeof Z); }
		bool holds(uint32_t r) const { return have && (!sub || std::binary_search(members.begin(), members.end(), r)); }
	} zs[2];
#ifndef WTZ_EMUL
	hipStream_t stream = 0;
	hipStream_t stream_side = 0; hipEvent_t ev_side_fork = 0, ev_side_join = 0;      /* side stream of the fused K-sw3 stage: the items dealt to the 32-bit frame form run on it beside the packed launch (run_stitch_fused) */
	hipStream_t stream_gap = 0; hipEvent_t ev_gap_fork = 0, ev_gap_join = 0;   /* side stream of K_gap (runs beside the left extensions) */
#endif
	int window_chaining = 1;          /* wtz_set_window_chaining: HZM_FAST_WINDOW_KMER_CHAINING of the reference (hzm_aln.h:36); 0 = K_pair_chain */
	bool shares_indexes = false;      /* clone: reads / k-mer table / z-index belong to the parent context */
	void *kpark_p[2] = {NULL, NULL}; size_t kpark_b[2] = {0, 0}, klive_b[2] = {0, 0};      /* k-mer table [0] / seed list [1]: buffer parked for the next build, size of the live one (0: not from kalloc) */
	wtz_arena arena;          /* transient device buffers of the API call in progress */
	uint32_t cap_pairs = 0, cap_items = 0;     /* grow-only capacity of the per-batch result arrays */
	wtz_params_t P = wtz_params_t(); wtz_params_t *dP = NULL;
	/* reads */
	uint64_t *bits = NULL; uint64_t n_words = 0; uint64_t *rdoff = NULL; uint32_t *rdlen = NULL; uint32_t n_reads = 0;
	std::vector<uint32_t> h_rdlen;
	/* k-mer index */
	wtz_kslot_t *ktab = NULL; uint64_t kmask = 0; uint32_t *kseeds = NULL; uint64_t n_kocc = 0;
	/* sharded index build in progress (wtz_index_count ... wtz_index_finish): sorted occurrences and the shard's distinct k-mers */
	uint64_t *pend_keys = NULL; uint32_t *pend_vals = NULL; uint64_t pend_tot = 0; uint64_t *pend_dk = NULL, *pend_dstart = NULL; uint32_t *pend_dc = NULL; uint64_t pend_nd = 0; uint32_t pend_beg = 0, pend_end = 0;
	uint64_t *cq_gptr = NULL; uint32_t cq_gcap = 0; bool cq_groups = false; std::vector<uint32_t> cq_ng;
	uint32_t idx_beg = 0, idx_end = 0; bool idx_len_sorted = false;      /* read range of the k-mer index; lengths non-increasing inside it (true unless -b clipped reads after the sort) */
	/* scratch: ONE allocation of pool_bytes, cut in two bump pools: dpool[0] = results and scratch that live for the batch (match lists,
	 * windows, anchors, CIGARs), dpool[1] = the transient pool of the K-sw3 trace matrices, reset after every launch group of extension
	 * jobs (run_extjobs sizes the groups from the jobs' geometry, so its demand is planned, not discovered by exhaustion) */
	wtz_pool_t *dpool = NULL; uint8_t *pool_base = NULL; uint64_t pool_bytes = 0, main_bytes = 0;
	/* per-batch results */
	uint32_t *d_qid = NULL, *d_cid = NULL; wtz_pairres_t *d_pairres = NULL; uint32_t n_pairs = 0; std::vector<wtz_pairres_t> h_pairres;
	wtz_alnres_dev_t *d_alnres = NULL; uint32_t n_items = 0; std::vector<wtz_alnres_dev_t> h_alnres;
	char *d_text = NULL; size_t cap_text = 0;      /* rendered CIGAR text of the last alignment call (wtz_fetch_cigar_text / wtz_cigar_text_device) */
#ifndef WTZ_EMUL
	/* copies are numbered: copy k signals ev_text_done[k & 1].  text_begun = copies started (device-stage thread), text_known_done = copies known to have finished
	 * (a render waits for the latest one before it refills d_text), text_ended = copies whose end has been asked for (the caller's commit thread, in the same order).
	 * Round 5 had ONE event and a plain bool shared by the two threads: _end could wait on the event after _begin had re-recorded it for the next range. */
	hipStream_t stream_copy = 0; hipEvent_t ev_text_ready = 0, ev_text_done[2] = {0, 0}; std::atomic<uint64_t> text_begun{0}, text_known_done{0}, text_ended{0};      /* wtz_fetch_cigar_text_begin / _end: the text's way to the host beside the next range's kernels */
#endif
	bool have_pairs = false, have_items = false;
	/* candidate request in flight (wtz_candidates_begin / _end) */
	uint32_t *cq_thr = NULL;
	uint32_t *cq_q = NULL, *cq_nc = NULL; uint64_t *cq_cand = NULL; unsigned long long *cq_bytes = NULL; uint32_t cq_cap = 0, cq_n = 0; bool cq_pending = false; wtz_timer cq_tm;
	wtz_counters_t cnt = wtz_counters_t();
	uint64_t tpool_peak_call = 0, main_used_call = 0;      /* transient-pool high-water mark / main-pool bytes of the API call in progress */
	int last_pool_fail = 0;      /* which pool the last WTZ_E_POOL came from: 1 = main, 2 = transient (wtz_pool_failure_kind) */
	double ext_use_ratio = 0.4; uint64_t tpool_last_used = 0;      /* run_stitch_fused: share of the trace upper bounds the fused launches have really taken */
	bool fused_ran = false;      /* this stitch stage's fused launch has run: the extension launches behind it only sweep up what it left open */
	unsigned long long ext_fr_total = 0;        /* items dealt to the 32-bit form before the launch (geometry outside the 16-bit window) */
	unsigned long long ext_open_total = 0;      /* items the packed form declined (outside its 16-bit window) and the 32-bit form finished */
};

#ifndef WTZ_EMUL
#define CTX_ENTER(c) (void)hipSetDevice((c)->device); g_stream = (c)->stream; wtz_arena_scope arena_scope_(&(c)->arena)
#else
#define CTX_ENTER(c) wtz_arena_scope arena_scope_(&(c)->arena)
#endif

#define STAGE(c, name) do { if((c)->sw.trace){ (void)dev_sync(); fprintf(stderr, "[stage] %s\n", name); fflush(stderr); } } while(0)

static wtz_reads_t ctx_reads(const wtz_ctx *c){ wtz_reads_t R; R.bits = c->bits; R.rdoff = c->rdoff; R.rdlen = c->rdlen; R.n_reads = c->n_reads; return R; }
static wtz_env_t ctx_env(const wtz_ctx *c){ wtz_env_t V; V.R = ctx_reads(c); V.Z = c->zs[0].Z; V.ZQ = c->zs[1].have ? c->zs[1].Z : c->zs[0].Z; V.P = c->dP; V.pool = c->dpool; V.dm_first_big = (uint32_t)c->sw.dm_first_big; return V; }

static int tpool_reset(wtz_ctx *c){
	wtz_pool_t p; wtz_pool_init(&p, c->pool_base + c->main_bytes, c->pool_bytes - c->main_bytes, c->sw.tfail_at);
	return dev_h2d(c->dpool + 1, &p, sizeof p);
}
static int pool_reset(wtz_ctx *c){
	wtz_pool_t p; wtz_pool_init(&p, c->pool_base, c->main_bytes, c->sw.fail_at);
	CHK(dev_h2d(c->dpool, &p, sizeof p));
	c->tpool_peak_call = 0;
	return tpool_reset(c);
}
/* the transient pool after a launch group: remember its high-water mark, fail on exhaustion */
static int tpool_check(wtz_ctx *c, const char *stage){
	wtz_pool_t p; CHK(dev_d2h(&p, c->dpool + 1, sizeof p));
	const uint64_t u = p.used > p.cap ? p.cap : p.used;
	c->tpool_last_used = u;
	if(u > c->tpool_peak_call) c->tpool_peak_call = u;
	if(p.overflow && c->sw.fail_once) c->sw.tfail_at = 0;
	if(p.overflow) c->last_pool_fail = 2;
	if(p.overflow) return wtz_fail(WTZ_E_POOL, "%s: transient trace pool exhausted (%llu of %llu bytes requested); use a larger pool",
		stage, (unsigned long long)p.used, (unsigned long long)p.cap);
	return WTZ_OK;
}
static int pool_check(wtz_ctx *c, const char *stage){
	wtz_pool_t p; CHK(dev_d2h(&p, c->dpool, sizeof p));
	const uint64_t u = (p.used > p.cap ? p.cap : p.used);
	c->main_used_call = u;
	if(u + c->tpool_peak_call > c->cnt.pool_peak) c->cnt.pool_peak = u + c->tpool_peak_call;
	if(p.overflow && c->sw.fail_once) c->sw.fail_at = 0;       /* injected failure: only the first stage call that gets that far */
	if(p.overflow) c->last_pool_fail = 1;
	if(p.overflow) return wtz_fail(WTZ_E_POOL, "%s: device scratch pool exhausted (%llu of %llu bytes requested); use fewer items per call or a larger pool",
		stage, (unsigned long long)p.used, (unsigned long long)p.cap);
	return WTZ_OK;
}
extern "C" int wtz_device_count(void){
#ifndef WTZ_EMUL
	int n = 0; if(hipGetDeviceCount(&n) != hipSuccess) return 0; return n;
#else
	return 1;
#endif
}

extern "C" int wtz_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes){
	if(!free_bytes || !total_bytes) return wtz_fail(WTZ_E_ARG, "null argument");
#ifndef WTZ_EMUL
	int prev = 0; HIPCHK(hipGetDevice(&prev)); HIPCHK(hipSetDevice(device));
	size_t fr = 0, tot = 0; const hipError_t e = hipMemGetInfo(&fr, &tot); (void)hipSetDevice(prev);
	if(e != hipSuccess) return wtz_fail(WTZ_E_HIP, "hipMemGetInfo: %s", hipGetErrorString(e));
	*free_bytes = fr; *total_bytes = tot;
#else
	(void)device; *free_bytes = *total_bytes = 16ull << 30;
#endif
	return WTZ_OK;
}

extern "C" int wtz_ctx_create(int device, const wtz_params_c *params, uint64_t pool_bytes, wtz_ctx_t **out){
	if(!params || !out) return wtz_fail(WTZ_E_ARG, "null argument");
	if(params->ksize < 5 || params->ksize > 32 || params->zsize < 5 || params->zsize > 16 || params->ksave < 1) return wtz_fail(WTZ_E_ARG, "k/z/S out of range (wtzmo.c:1658-1660)");
#ifndef WTZ_EMUL
	int ndev = 0;
	if(hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return wtz_fail(WTZ_E_HIP, "no HIP device visible: libwtzmo_hip needs an MI355X (gfx950); there is no CPU fallback");
	if(device < 0 || device >= ndev) return wtz_fail(WTZ_E_ARG, "device %d out of range (%d visible)", device, ndev);
	HIPCHK(hipSetDevice(device));
#endif
	wtz_ctx *c = new wtz_ctx();
	c->device = device; c->P = *params; wtz_switches_read(&c->sw);
	c->pool_bytes = pool_bytes ? pool_bytes : (4ull << 30);
#ifndef WTZ_EMUL
	if(!pool_bytes){
		/* default: 45 % of the free HBM, at most 128 GB (288 GB per MI355X; reads + both indexes of a 1.2 Gbp set take ~25 GB).  The host driver
		 * cuts a batch into ranges that fit the pool (wtz_pool_info) and every stage of a range ends in the tail of its slowest tasks:
		 * configs[2] runs in 36 ranges / 5.30 s with 64 GB, 22 ranges / 5.17 s with 128 GB, no further gain at 200 GB.  A second context on
		 * the same device (--workers 2, wtz_ctx_clone) takes 45 % of what is left. */
		size_t fr = 0, tot = 0;
		if(hipMemGetInfo(&fr, &tot) == hipSuccess && fr / 20 * 9 > c->pool_bytes) c->pool_bytes = (uint64_t)(fr / 20 * 9);
		if(c->pool_bytes > (128ull << 30)) c->pool_bytes = 128ull << 30;
		/* WTZ_DEFAULT_POOL_MB: the size a caller gets that did not ask for one (tests: the 128 GB default costs 4.4 s of hipMalloc per process - a hundred
		 * small golden cases spent 400 s of the GPU suite allocating; the pool size never changes a result, only the number of ranges) */
		if(const char *e = getenv("WTZ_DEFAULT_POOL_MB")){ const long long mb = atoll(e); if(mb >= 64 && ((uint64_t)mb << 20) < c->pool_bytes) c->pool_bytes = (uint64_t)mb << 20; }
	}
#endif
	c->pool_bytes &= ~(uint64_t)4095; c->main_bytes = (c->pool_bytes / 2) & ~(uint64_t)4095;
#ifndef WTZ_EMUL
	{ void *ab = NULL; const size_t acap = (size_t)3 << 29;      /* 1.5 GB */
	  if(hipMalloc(&ab, acap) == hipSuccess){ c->arena.base = (uint8_t*)ab; c->arena.cap = acap; } }
	/* every failure from here on unwinds through wtz_ctx_destroy (all fields are initialised; it skips what does not exist yet) */
	if(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess
			|| hipStreamCreateWithFlags(&c->stream_side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_side_fork, hipEventDisableTiming) != hipSuccess
			|| hipEventCreateWithFlags(&c->ev_side_join, hipEventDisableTiming) != hipSuccess
			|| hipStreamCreateWithFlags(&c->stream_gap, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_gap_fork, hipEventDisableTiming) != hipSuccess
			|| hipEventCreateWithFlags(&c->ev_gap_join, hipEventDisableTiming) != hipSuccess){ wtz_ctx_destroy(c); return wtz_fail(WTZ_E_HIP, "hipStreamCreate / hipEventCreate failed"); }
	g_stream = c->stream;
#endif
	int rc;
	if((rc = dev_alloc_persist((void**)&c->dP, sizeof(wtz_params_t))) || (rc = dev_h2d(c->dP, &c->P, sizeof(wtz_params_t))) ||
	   (rc = dev_alloc_persist((void**)&c->dpool, 2 * sizeof(wtz_pool_t)))){
		wtz_ctx_destroy(c); return rc;
	}
	/* a pool of the DEFAULT size is a share of what hipMemGetInfo reported a moment ago: another process on the device (parallel test workers, a second
	 * rank) may have taken it since.  Halve and try again down to 4 GB - the pool size never changes a result (pool exhaustion splits the batch) -;
	 * a size the caller asked for (--pool-gb) fails as it is. */
	for(;;){
#ifndef WTZ_EMUL
		/* a refused attempt that will be retried goes through the raw call: wtz_last_error must not keep the message of a failure that was recovered from */
		if(!pool_bytes && c->pool_bytes > (4ull << 30)){
			if(hipMalloc((void**)&c->pool_base, c->pool_bytes) == hipSuccess){ rc = WTZ_OK; break; }
			(void)hipGetLastError();              /* the refused allocation must not be what a later launch check reads */
			c->pool_base = NULL;
			uint64_t nb = c->pool_bytes / 2; if(nb < (4ull << 30)) nb = 4ull << 30;      /* never below the documented floor */
			c->pool_bytes = nb & ~(uint64_t)4095; c->main_bytes = (c->pool_bytes / 2) & ~(uint64_t)4095;
			continue;
		}
#endif
		rc = dev_alloc_persist((void**)&c->pool_base, c->pool_bytes);      /* the last attempt (or the caller's own size) fails loudly */
		break;
	}
	if(rc || (rc = pool_reset(c))){
		wtz_ctx_destroy(c); return rc;
	}
	*out = c;
	return WTZ_OK;
}

static void free_pending_index(wtz_ctx *c);
/* the table and the seed list of the previous build are kept for the next one of about the same size (a repeat of the step, the next shard of the same job) */
static void kpark(wtz_ctx *c, int w, void *p, size_t bytes){ if(!p) return; if(c->kpark_p[w]) dev_free_persist(c->kpark_p[w]); c->kpark_p[w] = p; c->kpark_b[w] = bytes; }
static void kflush(wtz_ctx *c){ for(int w = 0; w < 2; w++){ if(c->kpark_p[w]) dev_free_persist(c->kpark_p[w]); c->kpark_p[w] = NULL; c->kpark_b[w] = 0; } }
static int kalloc(wtz_ctx *c, int w, void **p, size_t n){
	if(c->kpark_p[w] && c->kpark_b[w] >= n && c->kpark_b[w] <= n + n / 8 + ((size_t)1 << 20)){ *p = c->kpark_p[w]; c->klive_b[w] = c->kpark_b[w]; c->kpark_p[w] = NULL; c->kpark_b[w] = 0; return WTZ_OK; }
	if(c->kpark_p[w]){ dev_free_persist(c->kpark_p[w]); c->kpark_p[w] = NULL; c->kpark_b[w] = 0; }
	int rc = dev_alloc_persist(p, n); if(rc == WTZ_OK) c->klive_b[w] = n; return rc;
}
static void free_kindex(wtz_ctx *c){
	if(!c->shares_indexes){
		if(c->klive_b[0]) kpark(c, 0, c->ktab, c->klive_b[0]); else dev_free_persist(c->ktab);
		if(c->klive_b[1]) kpark(c, 1, c->kseeds, c->klive_b[1]); else dev_free_persist(c->kseeds);
		c->klive_b[0] = c->klive_b[1] = 0;
	}
	c->ktab = NULL; c->kseeds = NULL; c->kmask = 0;
}
/* z-index allocation with recycling: a parked buffer of (nearly) the wanted size is taken instead of a fresh hipMalloc */
static int zalloc(wtz_ctx::zslot_t *z, void **p, size_t n){
	if(n == 0) n = 16;
	for(size_t i = 0; i < z->parked.size(); i++){
		if(z->parked[i].second >= n && z->parked[i].second <= n + n / 8 + 4096){
			*p = z->parked[i].first; z->live.push_back(z->parked[i]); z->parked.erase(z->parked.begin() + (long)i); return WTZ_OK;
		}
	}
	int rc = dev_alloc_persist(p, n); if(rc) return rc;
	z->live.push_back(std::make_pair(*p, n)); return WTZ_OK;
}
static void zpark_all(wtz_ctx::zslot_t *z){ for(size_t i = 0; i < z->live.size(); i++) z->parked.push_back(z->live[i]); z->live.clear(); }
static void zflush_parked(wtz_ctx::zslot_t *z){ for(size_t i = 0; i < z->parked.size(); i++) dev_free_persist(z->parked[i].first); z->parked.clear(); }
static void free_zindex(wtz_ctx *c){
	for(int k = 0; k < 2; k++){
		wtz_ctx::zslot_t *z = &c->zs[k];
		if(!c->shares_indexes){ zpark_all(z); zflush_parked(z); }      /* every z-index array comes from zalloc */
		z->zoff = NULL; memset(&z->Z, 0, sizeof z->Z); z->have = false; z->sub = false; z->sub_cap = 0; z->n_z = 0; z->members.clear();
	}
}
static void free_batch(wtz_ctx *c){ c->n_pairs = 0; c->n_items = 0; c->have_pairs = false; c->have_items = false; }
static void free_batch_storage(wtz_ctx *c){
	dev_free_persist(c->d_qid); dev_free_persist(c->d_cid); dev_free_persist(c->d_pairres); dev_free_persist(c->d_alnres);
	c->d_qid = c->d_cid = NULL; c->d_pairres = NULL; c->d_alnres = NULL; c->cap_pairs = c->cap_items = 0; free_batch(c);
}
static int reserve_pairs(wtz_ctx *c, uint32_t n){
	if(n <= c->cap_pairs && c->d_pairres) return WTZ_OK;
	uint32_t cap = c->cap_pairs ? c->cap_pairs : 4096; while(cap < n) cap *= 2;
	(void)dev_sync();
	dev_free_persist(c->d_qid); dev_free_persist(c->d_cid); dev_free_persist(c->d_pairres); c->d_qid = c->d_cid = NULL; c->d_pairres = NULL; c->cap_pairs = 0;
	CHK(dev_alloc_persist((void**)&c->d_qid, (size_t)cap * 4)); CHK(dev_alloc_persist((void**)&c->d_cid, (size_t)cap * 4));
	CHK(dev_alloc_persist((void**)&c->d_pairres, (size_t)cap * sizeof(wtz_pairres_t)));
	c->cap_pairs = cap; return WTZ_OK;
}
static int reserve_items(wtz_ctx *c, uint32_t m){
	if(m <= c->cap_items && c->d_alnres) return WTZ_OK;
	uint32_t cap = c->cap_items ? c->cap_items : 4096; while(cap < m) cap *= 2;
	(void)dev_sync();
	dev_free_persist(c->d_alnres); c->d_alnres = NULL; c->cap_items = 0;
	CHK(dev_alloc_persist((void**)&c->d_alnres, (size_t)cap * sizeof(wtz_alnres_dev_t)));
	c->cap_items = cap; return WTZ_OK;
}

extern "C" void wtz_ctx_destroy(wtz_ctx_t *c){
	if(!c) return;
	{ CTX_ENTER(c); (void)dev_sync(); }
	free_batch_storage(c); free_kindex(c); if(!c->shares_indexes) kflush(c); free_zindex(c);
	dev_free_persist(c->d_text);
	dev_free_persist(c->cq_q); dev_free_persist(c->cq_nc); dev_free_persist(c->cq_cand); dev_free_persist(c->cq_bytes); dev_free_persist(c->cq_thr); dev_free_persist(c->cq_gptr);
	free_pending_index(c);
#ifndef WTZ_EMUL
	arena_cache_flush(&c->arena);
	if(c->arena.base) (void)hipFree(c->arena.base);
#endif
	if(!c->shares_indexes){ dev_free_persist(c->bits); dev_free_persist(c->rdoff); dev_free_persist(c->rdlen); }
	dev_free_persist(c->dP); dev_free_persist(c->dpool); dev_free_persist(c->pool_base);
#ifndef WTZ_EMUL
	if(c->stream_side) (void)hipStreamDestroy(c->stream_side);
	if(c->stream_gap) (void)hipStreamDestroy(c->stream_gap);
	if(c->stream_copy){ (void)hipStreamSynchronize(c->stream_copy); (void)hipStreamDestroy(c->stream_copy); if(c->ev_text_ready) (void)hipEventDestroy(c->ev_text_ready); for(int k = 0; k < 2; k++) if(c->ev_text_done[k]) (void)hipEventDestroy(c->ev_text_done[k]); }
	{ hipEvent_t evs[4] = { c->ev_side_fork, c->ev_side_join, c->ev_gap_fork, c->ev_gap_join }; for(int k = 0; k < 4; k++) if(evs[k]) (void)hipEventDestroy(evs[k]); }
	if(c->stream) (void)hipStreamDestroy(c->stream);
#endif
	delete c;
}

/* A second context on the same GPU that SHARES the parent's read-only device data (reads, k-mer table, z-index) and has its
 * own stream, scratch pool and per-batch state: lets a host thread keep another batch in flight.  The parent must outlive the
 * clone and must not rebuild its indexes while clones are in use (re-clone after wtz_index_build / wtz_zindex_build). */
extern "C" int wtz_ctx_clone(wtz_ctx_t *p, uint64_t pool_bytes, wtz_ctx_t **out){
	if(!p || !out) return wtz_fail(WTZ_E_ARG, "null argument");
	wtz_ctx_t *c = NULL;
	int rc = wtz_ctx_create(p->device, &p->P, pool_bytes ? pool_bytes : p->pool_bytes, &c);
	if(rc) return rc;
	c->shares_indexes = true; c->window_chaining = p->window_chaining;
	if(c->P.I != p->P.I || c->P.D != p->P.D){ rc = wtz_set_gap_open(c, p->P.I, p->P.D); if(rc){ wtz_ctx_destroy(c); return rc; } }
	c->bits = p->bits; c->n_words = p->n_words; c->rdoff = p->rdoff; c->rdlen = p->rdlen; c->n_reads = p->n_reads; c->h_rdlen = p->h_rdlen;
	c->ktab = p->ktab; c->kmask = p->kmask; c->kseeds = p->kseeds; c->n_kocc = p->n_kocc;
	c->idx_beg = p->idx_beg; c->idx_end = p->idx_end; c->idx_len_sorted = p->idx_len_sorted;
	for(int k = 0; k < 2; k++){ c->zs[k].zoff = p->zs[k].zoff; c->zs[k].n_z = p->zs[k].n_z; c->zs[k].Z = p->zs[k].Z; c->zs[k].have = p->zs[k].have; c->zs[k].sub = p->zs[k].sub; c->zs[k].members = p->zs[k].members; }
	*out = c;
	return WTZ_OK;
}

/* The gap-open costs of the device DPs, per context: I opens a run of query-only steps (the E state, kswx.h:168), D a run of target-only steps (the F state,
 * kswx.h:174), as the reference's callers pass them (wtmsa.c:633-634: -2, -3).  Until it is called both are params.O. */
extern "C" int wtz_set_gap_open(wtz_ctx_t *c, int32_t I, int32_t D){
	if(!c) return wtz_fail(WTZ_E_ARG, "null context");
	if(I > 0 || D > 0 || I < WTZ_GAP_OPEN_MIN || D < WTZ_GAP_OPEN_MIN) return wtz_fail(WTZ_E_ARG, "wtz_set_gap_open: I = %d, D = %d: costs are passed as the reference takes them, in [%d, 0]", I, D, WTZ_GAP_OPEN_MIN);
	if(c->P.I == I && c->P.D == D) return WTZ_OK;
	CTX_ENTER(c);
	CHK(dev_sync());      /* nothing in flight reads the block while it changes */
	wtz_params_t P = c->P; P.I = I; P.D = D;
	CHK(dev_h2d(c->dP, &P, sizeof(wtz_params_t)));
	c->P = P;
	return WTZ_OK;
}
