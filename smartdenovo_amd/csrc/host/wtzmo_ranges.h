/* wtzmo host driver, section 6 of 6: batches of queries, their ranges (plan -> device stages -> commit), serial or pipelined, and the worker loop */
/* a range came back with "scratch pool too small": was it the library's transient trace pool alone (its own budget, raised by now) on every local part that failed?
 * Then the bytes-per-pair estimate of the MAIN pool is not what was wrong and stays as it is (one under-estimated trace budget used to halve every later
 * range).  Parts on other ranks cannot be asked: they count as a main-pool failure. */
static int range_failed_on_traces_only(const batch_t *b){
	if(g_dist.world > 1) return 0;
	int seen = 0;
	for(uint32_t d = 0; d < b->nparts; d++){
		const part_t *pt = &b->parts[d];
		if(!pt->ctx || pt->npair == 0) continue;
		const int k = wtz_pool_failure_kind(pt->ctx);
		if(k == 1) return 0;
		if(k == 2) seen = 1;
	}
	return seen;
}
/* end of the range that starts at slot s0: as many slots as fit the main scratch pool at the measured bytes per pair */
static uint32_t range_end(eng_t *E, batch_t *b, uint32_t s0){
	pthread_mutex_lock(&E->mu);
	/* before the first measurement: a small probe range (about 2000 pairs, never more than 1 MB per pair allows) - repeat-rich reads
	 * need tens of MB per pair where iid reads need a few hundred KB, and the longest reads come first */
	const double cap = E->main_cap ? (double)E->main_cap : 0.0;
	const double prior = cap / 2048.0 > 1048576.0 ? cap / 2048.0 : 1048576.0;
	const double bpp = E->step.bytes_per_pair > 0 ? E->step.bytes_per_pair : prior;
	const double row_ratio = E->step.pair_row_ratio;
	pthread_mutex_unlock(&E->mu);
	static double fill = -1.0;      /* WTZ_RANGE_FILL: the share of the main pool a range is planned to (candidate rows are an upper bound of its pairs) */
	/* measured at configs[2] (round 5, gpurun_out/r05r, r05s; every stage of a range ends in the tail of its slowest tasks, so fewer and larger ranges win until the
	 * pool overflows and a range is redone in halves): 0.7 -> 28 ranges 2.10 s, 1.0 -> 21 ranges 1.98 s, 1.4 -> 16 ranges 1.97 s (pool peak 96 of 128 GB),
	 * 1.8 -> one overflow, 2.11 s; with batches of 8 192 queries 1.4 -> 14 ranges 1.94 s */
	if(fill < 0){ const char *e = getenv("WTZ_RANGE_FILL"); fill = e ? atof(e) : 1.2; if(fill <= 0) fill = 1.2; }
	/* the budget is in PAIRS, the slots are cut by candidate ROWS: closed pairs (the other read of the pair came first), masked and saturated queries thin the rows out -
	 * to 0.9 at configs[2], to less than a tenth at the configs[3] shape (70x: every pair is found from both sides), where ranges held 17 000 pairs for a pool that holds
	 * 40 000.  The share measured on the ranges before (+ 25 %) scales the budget; an estimate that was too low ends in the split of the range like any other */
	double ratio = row_ratio * 1.25; if(ratio > 1.0 || ratio <= 0) ratio = 1.0;
	uint64_t budget = cap > 0 ? (uint64_t)(fill * cap / bpp / ratio) : ~0ull;
	if(budget < 16) budget = 16;
	uint32_t s1 = s0; uint64_t acc = 0;
	while(s1 < b->nbq && (s1 == s0 || acc + (b->want[s1] ? b->nrow[s1] : 0) <= budget)){ acc += b->want[s1] ? b->nrow[s1] : 0; s1++; }
	return s1;
}
/* Candidate search (A3) depends on the read and the index only, so the next batch's request can be in flight while this
 * batch is committed on the host.  The next queries are chosen with the masks as they are NOW; whoever the commit masks or
 * saturates meanwhile is dropped / demoted when the batch is formed - the batch composition is free (any batch size gives
 * the same output), only the query ORDER and the one-query masking lag are part of the contract. */
static void prefetch_begin(eng_t *E, batch_t *b){
	if(E->n_workers != 1 || E->step.rows_all || E->step.cursor >= E->step.qend) return;
	const uint32_t B = E->step.B;
	if(B > b->pf_cap){ b->pf_cap = B; b->pf_ids = (uint32_t*)hx_realloc(b->pf_ids, 4 * (size_t)B); b->pf_rows = (uint64_t*)hx_realloc(b->pf_rows, (size_t)B * E->stride * 8); b->pf_nr = (uint32_t*)hx_realloc(b->pf_nr, 4 * (size_t)B); }
	uint32_t j = E->step.cursor, n = 0;
	for(; j < E->step.qend && n < B; j++){
		if((j % E->n_job) != E->i_job) continue;
		if(E->masked[j]) continue;
		if(E->rdcovs[j] >= nbest_of(E, j)) continue;        /* already saturated: needs no candidates; it is re-examined when the batch is formed */
		b->pf_ids[n] = j; b->pf_nr[n] = 0; n++;
	}
	b->pf_n = n; b->pf_cursor_end = j;
	if(n == 0) return;
	memset(b->pf_rows, 0, (size_t)n * E->stride * 8);
	if(E->shard) shard_candidates_begin(E, b->pf_ids, n);
	else if(b->nparts == 1){
		int rc = wtz_candidates_begin(b->ctx, b->pf_ids, n, b->pf_rows, b->pf_nr); DIE_WTZ(rc, "wtz_candidates_begin");
	} else {
		/* the seed lookup is pure per query: query k of the request goes to device / rank k % nparts (the launches return at once) */
		int local_failed = 0;
		if(g_dist.world > 1){
			wtz_dist_hdr_t h; memset(&h, 0, sizeof h); h.cmd = WTZ_CMD_CAND_BEGIN;
			for(uint32_t d = 0; d < b->nparts; d++) h.count[d] = (n + b->nparts - 1 - d) / b->nparts;
			g_dist.bcast(&h, sizeof h);
		}
		for(uint32_t d = 0; d < b->nparts; d++){
			part_t *pt = &b->parts[d];
			const uint32_t m = (n + b->nparts - 1 - d) / b->nparts;
			if(m > pt->cq_cap){ pt->cq_cap = m; pt->cq_ids = (uint32_t*)hx_realloc(pt->cq_ids, 4 * (size_t)m); pt->cq_nr = (uint32_t*)hx_realloc(pt->cq_nr, 4 * (size_t)m); pt->cq_rows = (uint64_t*)hx_realloc(pt->cq_rows, (size_t)m * E->stride * 8); }
			pt->cq_n = m;
			for(uint32_t k = 0; k < m; k++){ pt->cq_ids[k] = b->pf_ids[(size_t)k * b->nparts + d]; pt->cq_nr[k] = 0; }
			if(m) memset(pt->cq_rows, 0, (size_t)m * E->stride * 8);
			if(pt->remote){ if(m) g_dist.send(pt->cq_ids, 4 * (uint64_t)m, pt->remote); continue; }
			int rc = wtz_candidates_begin(pt->ctx, pt->cq_ids, m, pt->cq_rows, pt->cq_nr);
			if(rc != WTZ_OK && g_dist.world > 1){ fprintf(stderr, " -- rank 0: wtz_candidates_begin failed: %s --\n", wtz_last_error()); local_failed = 1; continue; }
			DIE_WTZ(rc, "wtz_candidates_begin");
		}
		if(local_failed) ranks_abort("rank 0 failed in the seed lookup");      /* every rank has its ids: the request is complete, the next thing they read is a header */
	}
	b->pf_inflight = 1;
}
/* the seed lookup allocates its scratch per query from the main pool as it goes (tuples of the query: coverage x length) and an exhausted pool ends the run: the
 * batches are capped at what 0.6 of the pool holds at the bytes per query of the requests before (the longest reads come first, so the estimate errs on the safe side) */
static void cand_scratch_seen(eng_t *E, batch_t *b, uint32_t n_lookup){
	wtz_pool_info_t pi;
	if(n_lookup < 32 || b->nparts != 1 || E->shard || b->ctx == NULL || wtz_pool_info(b->ctx, &pi) != WTZ_OK || pi.main_used == 0) return;
	const double bpq = (double)pi.main_used / (double)n_lookup;
	pthread_mutex_lock(&E->mu);
	{ const double keep = E->step.cand_bpq * 0.7; E->step.cand_bpq = bpq > keep ? bpq : keep; }      /* follows the measurements down by at most 30 % per request (reads get shorter) */
	E->cand_main_cap = pi.main_cap;
	pthread_mutex_unlock(&E->mu);
}
static uint32_t cand_batch_cap(const eng_t *E){
	uint32_t cap = E->max_batch;
	if(E->step.cand_bpq > 0 && E->cand_main_cap){ const double c = 0.6 * (double)E->cand_main_cap / E->step.cand_bpq; if(c < (double)cap) cap = c < 256.0 ? 256u : (uint32_t)c; }
	else if(E->cand_cap0 && cap > E->cand_cap0) cap = E->cand_cap0;
	return cap;
}
/* The z-mer index of a batch (after its candidate rows are known, before its first range).
 *   --zindex-batch (read sets whose all-reads index does not fit: 16 B per base): part d's index is rebuilt from the batch's candidate reads
 *     = d (mod nparts) - with one part: from the batch's queries + all their candidates, one index;
 *   several parts: the batch's queries go into the second, query-side index of EVERY part (wtz_zindex_build_queries).
 * Parts of this process build side by side on their own threads; between ranks the lists travel with WTZ_CMD_ZIDX and every rank builds its own
 * (no reply: a failure shows in the status word of the rank's next reply). */
typedef struct { wtz_ctx_t *ctx; int have_c, have_q; const uint32_t *cl, *ql; uint32_t ncl, nql; int rc; char err[256]; } zjob_t;
static void *zjob_main(void *arg){
	zjob_t *j = (zjob_t*)arg;
	j->rc = zbuild_part(j->ctx, j->have_c, j->cl, j->ncl, j->have_q, j->ql, j->nql);
	if(j->rc != WTZ_OK) snprintf(j->err, sizeof j->err, "%s", wtz_last_error());
	return NULL;
}
static void batch_zindex(eng_t *E, batch_t *b){
	const uint32_t n_all = (uint32_t)(E->st.n_rd + E->st.n_qr), np = b->nparts; const int ranks = g_dist.world > 1;
	const int have_c = E->zbatch > 0, have_q = E->zsplit;
	uint32_t *ql = (uint32_t*)hx_realloc(NULL, 4 * ((size_t)b->nbq + 1)), nql = 0;
	uint32_t *cl[WTZ_DIST_MAX], ncl[WTZ_DIST_MAX]; memset(cl, 0, sizeof cl); memset(ncl, 0, sizeof ncl);
	for(uint32_t s = 0; s < b->nbq; s++) if(b->want[s]) ql[nql++] = b->bq[s];       /* ascending: a batch takes its queries in id order */
	if(have_c){
		uint8_t *mark = (uint8_t*)calloc((size_t)n_all + 1, 1);
		for(uint32_t s = 0; s < b->nbq; s++){
			if(!b->want[s]) continue;
			if(!have_q) mark[b->bq[s]] = 1;          /* one part: queries and candidates share the one index */
			for(uint32_t k = 0; k < b->nrow[s]; k++){ const uint32_t id2 = (uint32_t)(b->rows[(size_t)s * E->stride + k] >> 32); if(id2 < n_all) mark[id2] = 1; }
		}
		for(uint32_t d = 0; d < np; d++) cl[d] = (uint32_t*)hx_realloc(NULL, 4 * ((size_t)n_all / np + 2));
		for(uint32_t r = 0; r < n_all; r++) if(mark[r]){ const uint32_t d = have_q ? DEAL_PART(np, 0, r) : 0; cl[d][ncl[d]++] = r; }
		free(mark);
	}
	const double tz0 = now_s();
	if(ranks){
		wtz_dist_hdr_t h; memset(&h, 0, sizeof h); h.cmd = WTZ_CMD_ZIDX; h.arg[0] = nql; h.arg[1] = (uint64_t)have_c;
		for(uint32_t d = 0; d < np; d++) h.count[d] = ncl[d];
		g_dist.bcast(&h, sizeof h);
		if(nql) g_dist.bcast(ql, 4 * (uint64_t)nql);
		if(have_c) for(uint32_t d = 1; d < np; d++) if(ncl[d]) g_dist.send(cl[d], 4 * (uint64_t)ncl[d], (int)d);
		const int rc = zbuild_part(E->ctx, have_c, cl[0], ncl[0], have_q, ql, nql);
		if(rc != WTZ_OK){ fprintf(stderr, " -- rank 0: the z-mer index of the batch failed: %s --\n", wtz_last_error()); ranks_abort("rank 0 failed"); }
	} else {
		zjob_t zj[8]; pthread_t th[8];
		for(uint32_t d = 0; d < np && d < 8; d++){ zj[d].ctx = b->parts[d].ctx; zj[d].have_c = have_c; zj[d].have_q = have_q; zj[d].cl = cl[d]; zj[d].ncl = ncl[d]; zj[d].ql = ql; zj[d].nql = nql; zj[d].rc = WTZ_OK; }
		for(uint32_t d = 1; d < np; d++) if(pthread_create(&th[d], NULL, zjob_main, &zj[d]) != 0){ fprintf(stderr, " -- cannot start a device thread --\n"); DIE_NOW(); }
		zjob_main(&zj[0]);
		for(uint32_t d = 1; d < np; d++) pthread_join(th[d], NULL);
		for(uint32_t d = 0; d < np; d++) if(zj[d].rc != WTZ_OK){ fprintf(stderr, " -- the z-mer index of the batch failed on device %d: %s --\n", E->devs[d], zj[d].err); DIE_NOW(); }
	}
	pthread_mutex_lock(&E->mu); E->step.t_gpu += now_s() - tz0; E->step.t_zbatch += now_s() - tz0; pthread_mutex_unlock(&E->mu);
	for(uint32_t d = 0; d < np; d++) free(cl[d]);
	free(ql);
}
/* the next batch of queries (id order) with their candidate heaps (A3) and - where the z-mer index is per batch - its index; 0: no queries left */
static int batch_form(batch_t *b){
	eng_t *E = b->E;
	/* ---- take the next batch of queries (id order) ---- */
	pthread_mutex_lock(&E->mu);
	if(E->step.cursor >= E->step.qend){ pthread_mutex_unlock(&E->mu); return 0; }
	const uint32_t B = E->step.B;
	const int use_pf = b->pf_inflight;
	const uint32_t jend = use_pf ? b->pf_cursor_end : E->step.qend;      /* a prefetched batch covers exactly the reads the prefetch looked at */
	const uint32_t need = use_pf ? (jend - E->step.cursor) + 1 : B + 1;  /* saturated reads of the range ride along without candidates */
	if(need > b->capbq){ b->capbq = need; b->bq = (uint32_t*)hx_realloc(b->bq, 4 * (size_t)b->capbq); b->want = (uint8_t*)hx_realloc(b->want, b->capbq); b->ids = (uint32_t*)hx_realloc(b->ids, 4 * (size_t)b->capbq);
		b->rows = (uint64_t*)hx_realloc(b->rows, (size_t)b->capbq * E->stride * 8); b->nrow = (uint32_t*)hx_realloc(b->nrow, 4 * (size_t)b->capbq); }
	b->nbq = 0;
	uint32_t j = E->step.cursor, nwant = 0;
	for(; j < jend && (use_pf || b->nbq < B); j++){
		if((j % E->n_job) != E->i_job) continue;
		if(E->masked[j]) continue;
		/* reads whose coverage is already saturated (wtzmo.c:808) need no GPU work but stay in the dispatch sequence:
		 * their dispatch is what merges the previous query's masks (one-query masking lag) */
		const int sat = E->rdcovs[j] >= nbest_of(E, j);
		b->want[b->nbq] = (uint8_t)!sat; b->nrow[b->nbq] = 0;
		if(!sat){
			if(E->step.rows_all){ memcpy(b->rows + (size_t)b->nbq * E->stride, E->rows + (size_t)j * E->stride, (size_t)E->stride * 8); b->nrow[b->nbq] = E->nrow[j]; }
			nwant++;
		}
		b->bq[b->nbq++] = j;
	}
	E->step.cursor = j;
	b->seq = E->step.next_seq++; b->holds_turn = 0; b->spec_queries = b->nbq; b->used_queries = 0; b->masked_at_form = E->step.n_masked;
	E->step.spec_queries += b->nbq; E->step.n_batches++;
	{ const uint32_t mb = cand_batch_cap(E); if(E->step.B < mb) E->step.B = E->step.B * 4 > mb ? mb : E->step.B * 4; else if(E->step.B > mb) E->step.B = mb; }      /* ramp-up; corrected at commit */
	pthread_mutex_unlock(&E->mu);
	/* ---- candidate heaps of the batch's queries (A3) ---- */
	if(use_pf){
		const double tg0 = now_s();
		int rc = WTZ_OK, cand_failed = -1;
		if(E->shard) shard_candidates_end(E, b->pf_n, b->pf_rows, b->pf_nr);
		else if(b->nparts == 1){ rc = wtz_candidates_end(b->ctx, b->pf_rows, b->pf_nr); DIE_WTZ(rc, "wtz_candidates_end"); cand_scratch_seen(E, b, b->pf_n); }
		else for(uint32_t d = 0; d < b->nparts; d++){
			part_t *pt = &b->parts[d];
			if(d == 0 && g_dist.world > 1){ wtz_dist_hdr_t h; memset(&h, 0, sizeof h); h.cmd = WTZ_CMD_CAND_END; g_dist.bcast(&h, sizeof h); }
			if(pt->remote){
				const uint64_t sz_rows = (uint64_t)pt->cq_n * E->stride * 8, sz_nr = 4 * (uint64_t)pt->cq_n;
				uint8_t *x = part_xbuf(pt, 8 + sz_rows + sz_nr);
				g_dist.recv(x, 8 + sz_rows + sz_nr, pt->remote);
				uint64_t st = 0; memcpy(&st, x, 8);
				if(st != WTZ_ST_OK){ if(cand_failed < 0) cand_failed = pt->remote; continue; }
				if(pt->cq_n){ memcpy(pt->cq_rows, x + 8, sz_rows); memcpy(pt->cq_nr, x + 8 + sz_rows, sz_nr); }
			} else {
				rc = wtz_candidates_end(pt->ctx, pt->cq_rows, pt->cq_nr);
				if(rc != WTZ_OK && g_dist.world > 1){ fprintf(stderr, " -- rank 0: wtz_candidates_end failed: %s --\n", wtz_last_error()); if(cand_failed < 0) cand_failed = 0; continue; }
				DIE_WTZ(rc, "wtz_candidates_end");
			}
			for(uint32_t k = 0; k < pt->cq_n; k++){ const size_t g = (size_t)k * b->nparts + d; memcpy(b->pf_rows + g * E->stride, pt->cq_rows + (size_t)k * E->stride, (size_t)E->stride * 8); b->pf_nr[g] = pt->cq_nr[k]; }
		}
		if(cand_failed >= 0){ char why[64]; snprintf(why, sizeof why, "rank %d failed in the seed lookup", cand_failed); ranks_abort(why); }
		const double tg1 = now_s();
		b->pf_inflight = 0;
		uint32_t k = 0;
		for(uint32_t s = 0; s < b->nbq; s++){
			if(!b->want[s]) continue;
			while(k < b->pf_n && b->pf_ids[k] < b->bq[s]) k++;
			if(k >= b->pf_n || b->pf_ids[k] != b->bq[s]){ fprintf(stderr, " -- internal error: read %u has no prefetched candidates --\n", b->bq[s]); DIE_NOW(); }
			memcpy(b->rows + (size_t)s * E->stride, b->pf_rows + (size_t)k * E->stride, (size_t)E->stride * 8); b->nrow[s] = b->pf_nr[k];
		}
		pthread_mutex_lock(&E->mu); E->step.t_gpu += tg1 - tg0; E->step.t_call[0] += tg1 - tg0; pthread_mutex_unlock(&E->mu);
	} else if(nwant){
		uint32_t n = 0;
		for(uint32_t s = 0; s < b->nbq; s++) if(b->want[s]) b->ids[n++] = b->bq[s];
		uint64_t *rows = (uint64_t*)hx_realloc(NULL, (size_t)n * E->stride * 8); uint32_t *nr = (uint32_t*)hx_realloc(NULL, 4 * (size_t)n);
		n = 0;
		for(uint32_t s = 0; s < b->nbq; s++) if(b->want[s]){ memcpy(rows + (size_t)n * E->stride, b->rows + (size_t)s * E->stride, (size_t)b->nrow[s] * 8); nr[n] = b->nrow[s]; n++; }
		const double tg0 = now_s();
		if(E->shard){ shard_candidates_begin(E, b->ids, n); shard_candidates_end(E, n, rows, nr); }
		else { int rc = wtz_candidates(b->ctx, b->ids, n, rows, nr); DIE_WTZ(rc, "wtz_candidates"); cand_scratch_seen(E, b, n); }
		const double tg1 = now_s();
		n = 0;
		for(uint32_t s = 0; s < b->nbq; s++) if(b->want[s]){ memcpy(b->rows + (size_t)s * E->stride, rows + (size_t)n * E->stride, (size_t)E->stride * 8); b->nrow[s] = nr[n]; n++; }
		free(rows); free(nr);
		pthread_mutex_lock(&E->mu); E->step.t_gpu += tg1 - tg0; E->step.t_call[0] += tg1 - tg0; pthread_mutex_unlock(&E->mu);
	}
	if(b->nbq && (E->zbatch > 0 || E->zsplit)) batch_zindex(E, b);
	return 1;
}
/* after a range that fit: the capacity of the main pool and the bytes a pair needed (range_end plans the next ranges with them).  A part that another rank computes has no
 * context here and is not measured */
static void range_measure_pool(eng_t *E, const batch_t *b){
	for(uint32_t d = 0; b->npair && d < b->nparts; d++){
		wtz_pool_info_t pi; const part_t *pt = &b->parts[d];
		if(pt->npair == 0 || pt->ctx == NULL || wtz_pool_info(pt->ctx, &pi) != WTZ_OK) continue;
		pthread_mutex_lock(&E->mu);
		E->main_cap = pi.main_cap * b->nparts;                  /* the range is dealt over nparts pools */
		const double bpp = (double)pi.main_used / (double)pt->npair;
		if(pt->npair >= 8 && bpp > E->step.bytes_per_pair) E->step.bytes_per_pair = bpp;
		else if(pt->npair >= 256 && E->bpp_decay > 0 && bpp < E->step.bytes_per_pair){      /* the longest reads come first: let the estimate follow the measurements down, 15 % per range at most */
			const double floor_ = E->step.bytes_per_pair * E->bpp_decay; E->step.bytes_per_pair = bpp > floor_ ? bpp : floor_; }
		pthread_mutex_unlock(&E->mu);
	}
}
/* the wall seconds of the parts' device calls since the last fold (parallel devices: part 0 counts), and their waits for the writer */
static void parts_fold_times(batch_t *b, double t_call[5], double *t_io0){
	for(uint32_t d = 0; d < b->nparts; d++){ part_t *pt = &b->parts[d]; for(int k = 0; k < 5; k++){ if(d == 0) t_call[k] += pt->t_call[k]; pt->t_call[k] = 0; } *t_io0 += pt->t_io0; pt->t_io0 = 0; }
}
static void ranges_count_one(eng_t *E){ pthread_mutex_lock(&E->mu); E->step.n_ranges++; pthread_mutex_unlock(&E->mu); }
/* The commit of slots [s0, s1) over the results in b->cparts when it is this batch's turn.  t_gpu, t_call, t_io0: the seconds of the range's device stages, added to the
 * step's under the same lock; the range's commit time runs from t_commit_from */
static void range_commit(eng_t *E, batch_t *b, uint32_t s0, uint32_t s1, uint32_t npair, uint32_t nitem, double t_gpu, const double t_call[5], double t_io0, double t_commit_from){
	pthread_mutex_lock(&E->mu);
	E->step.t_gpu += t_gpu; E->step.t_io[0] += t_io0; for(int k = 0; k < 5; k++) E->step.t_call[k] += t_call[k];
	while(!b->holds_turn && E->step.commit_seq != b->seq) pthread_cond_wait(&E->cv, &E->mu);
	b->holds_turn = 1;
	E->step.spec_pairs += npair; E->step.spec_items += nitem;
	/* commit in query order with the reference's one-query masking lag (wtzmo.c:1315-1333) */
	{ const double tc = now_s(); cq_spec_start(E, b, s0, s1, npair); E->step.t_spec_ctl += now_s() - tc; }
	for(uint32_t s = s0; s < s1; s++){
		if(s + 1 < s1) commit_prefetch(E, b, s + 1);
		if(!E->masked[b->bq[s]]){ const double tf = now_s(); flush_pending(E); E->step.t_flush += now_s() - tf; commit_query(E, b, s); }
		cq_spec_done(E, s);
	}
	{ const double tc = now_s(); cq_spec_stop(E); E->step.t_spec_ctl += now_s() - tc; }
	out_submit(&g_ow);      /* nothing of this batch stays in the chunk under construction (see out_wait_ext) */
	E->step.t_commit += now_s() - t_commit_from;
	pthread_mutex_unlock(&E->mu);
}
/* slots [s0,s1): plan pairs, run the device stages, commit in query order when it is this batch's turn. A range whose
 * scratch demand exceeds the pool is split in two (the second half is planned after the first half is committed). */
static void process_range(eng_t *E, batch_t *b, uint32_t s0, uint32_t s1);
/* [s0, s1) came back with "scratch pool too small" (nothing of it is committed): account for the split, then the two halves one after the other */
static void range_overflowed(eng_t *E, batch_t *b, uint32_t s0, uint32_t s1, const char *errtext){
	pthread_mutex_lock(&E->mu); E->step.n_split++; if(!range_failed_on_traces_only(b)) E->step.bytes_per_pair = (E->step.bytes_per_pair > 0 ? E->step.bytes_per_pair : 1048576.0) * 2.0; pthread_mutex_unlock(&E->mu);
	if(s1 - s0 <= 1){ fprintf(stderr, " -- device scratch pool too small even for one query: %s (use --pool-gb) --\n", errtext); DIE_NOW(); }
	fprintf(stderr, "[wtzmo-mi355x] scratch pool exhausted with %u queries in flight; splitting the batch\n", s1 - s0);
	const uint32_t mid = s0 + (s1 - s0) / 2;
	process_range(E, b, s0, mid);
	process_range(E, b, mid, s1);
}
static void process_range(eng_t *E, batch_t *b, uint32_t s0, uint32_t s1){
	pthread_mutex_lock(&E->mu);
	plan_pairs(E, b, s0, s1);
	pthread_mutex_unlock(&E->mu);
	const double tg0 = now_s();
	const int again = gpu_stages(E, b);
	for(uint32_t d = 0; d < b->nparts; d++) part_text_wait(&b->parts[d], &b->parts[d].t_call[4]);      /* this path commits at once */
	const double tg1 = now_s();
	if(again){ range_overflowed(E, b, s0, s1, wtz_last_error()); return; }
	range_measure_pool(E, b);
	if(s1 == b->nbq && !b->pf_inflight){ pthread_mutex_lock(&E->mu); prefetch_begin(E, b); pthread_mutex_unlock(&E->mu); }
	double t_call[5] = {0, 0, 0, 0, 0}, t_io0 = 0; parts_fold_times(b, t_call, &t_io0);
	range_commit(E, b, s0, s1, b->npair, b->nitem, tg1 - tg0, t_call, t_io0, tg1);
}
/* the slots of a batch in ranges whose pairs (candidate rows are their upper bound) fit the main scratch pool at the measured bytes per pair */
static void process_batch_serial(eng_t *E, batch_t *b, uint32_t s0){
	while(s0 < b->nbq){
		const uint32_t s1 = range_end(E, b, s0);
		process_range(E, b, s0, s1);
		ranges_count_one(E);
		s0 = s1;
	}
}
/* Ranges PIPELINED: while the host commits range r (sequential by definition: 0.36 s of a 3.7 s configs[2] step) the device stages of range
 * r + 1 run on a helper thread.  Range r + 1 is therefore planned BEFORE range r is committed, i.e. against masks / closed pairs / coverage
 * one range older: every piece of order-dependent state only removes work, so the plan is a superset of what the commit will
 * ask for and the output cannot change - a few more speculative pairs are computed.  The finished range's result arrays are swapped into
 * the batch's spare set (cparts) so that the next range can fill `parts`.  A range that overflows the scratch pool is redone by the serial
 * path (halving), then the pipeline starts again behind it. */
typedef struct { eng_t *E; batch_t *b; int again; double t0, t1; pthread_t th; int running; char err[256]; } gpujob_t;
static void *gpujob_main(void *arg){ gpujob_t *j = (gpujob_t*)arg; j->t0 = now_s(); j->again = gpu_stages(j->E, j->b); j->t1 = now_s();
	if(j->again) snprintf(j->err, sizeof j->err, "%s", wtz_last_error());      /* wtz_last_error is thread-local: the text is this helper thread's */
	return NULL; }
static void gpujob_start(gpujob_t *j, eng_t *E, batch_t *b){ j->E = E; j->b = b; j->again = 0; if(pthread_create(&j->th, NULL, gpujob_main, j) != 0){ fprintf(stderr, " -- cannot start the device-stage thread --\n"); DIE_NOW(); } j->running = 1; }
static int gpujob_wait(gpujob_t *j){ if(j->running){ pthread_join(j->th, NULL); j->running = 0; } return j->again; }
/* "plan this range and start it on the helper thread": its end by the pool budget, its pairs against the state as it is now, its device stages */
static void range_launch(eng_t *E, batch_t *b, gpujob_t *job, uint32_t s0, uint32_t *s1){
	*s1 = range_end(E, b, s0);
	pthread_mutex_lock(&E->mu); plan_pairs(E, b, s0, *s1); pthread_mutex_unlock(&E->mu); gpujob_start(job, E, b);
}
/* the finished range's results move to the commit view (b->spare): the device stages of the next range fill b->parts meanwhile */
static void parts_results_to_spare(batch_t *b){
	for(uint32_t d = 0; d < b->nparts; d++){
		part_t *p = &b->parts[d], *c = &b->spare[d];
		SWAP(wtz_pair_summary_t*, p->sum, c->sum); SWAP(uint64_t*, p->box_off, c->box_off); SWAP(wtz_winbox_t*, p->boxes, c->boxes);
		SWAP(uint64_t, p->capbox, c->capbox); SWAP(uint64_t, p->nbox, c->nbox);
		SWAP(uint32_t*, p->item_of, c->item_of); SWAP(uint32_t*, p->it_pair, c->it_pair); SWAP(uint8_t*, p->it_dir, c->it_dir); SWAP(wtz_aln_result_t*, p->aln, c->aln);
		c->cig = p->cig; c->cig_ext = p->cig_ext; c->ncig = p->ncig; c->nitem = p->nitem; c->npair = p->npair;
		c->ctx = p->ctx; c->text_pending = p->text_pending; p->text_pending = 0;
	}
	b->cparts = b->spare;
}
/* the candidate request in flight moves to the batch that will be formed from it; several parts: the request's per-part arrays travel with it */
static void prefetch_move(batch_t *b, batch_t *nb){
	SWAP(int, b->pf_inflight, nb->pf_inflight); SWAP(uint32_t*, b->pf_ids, nb->pf_ids); SWAP(uint32_t, b->pf_n, nb->pf_n); SWAP(uint32_t, b->pf_cap, nb->pf_cap);
	SWAP(uint64_t*, b->pf_rows, nb->pf_rows); SWAP(uint32_t*, b->pf_nr, nb->pf_nr); SWAP(uint32_t, b->pf_cursor_end, nb->pf_cursor_end);
	for(uint32_t d = 0; d < b->nparts; d++){ part_t *pa = &b->parts[d], *pn = &nb->parts[d];
		SWAP(uint32_t*, pa->cq_ids, pn->cq_ids); SWAP(uint32_t*, pa->cq_nr, pn->cq_nr); SWAP(uint64_t*, pa->cq_rows, pn->cq_rows); SWAP(uint32_t, pa->cq_cap, pn->cq_cap); SWAP(uint32_t, pa->cq_n, pn->cq_n); }
}
/* In front of the commit of b's last range [s0, s1): the next batch is formed from the prefetched candidates, and its first range is started on the device ... */
static void next_batch_early(eng_t *E, batch_t *b, uint32_t s0, uint32_t s1){
	batch_t *nb = b->alt;
	/* ... where that pays.  The commit about to run masks reads (the longest reads come first and contain many of the reads behind them), and whatever it masks
	 * inside the range started early was computed for nothing: E. coli shape with every boundary overlapped 6 790 queries planned for 3 017 used, 0.274 s per step
	 * against 0.242; configs[2] 1.81 s against 1.85.  So the next batch is FORMED here (its candidates are known: that is what the estimate needs; a slot masked
	 * later is skipped when its range is planned) and its first range is STARTED here only if
	 *     expected waste = share of the reads to come that the commit will mask (new masks per used query of this batch so far x the queries of its last range /
	 *                      the unmasked reads to come, at most 1) x the pairs of that first range x the step's device time per planned pair
	 *  <= what is hidden  = the queries of the last range x the step's commit time per used query (+ 3 ms of forming and planning).
	 * WTZ_BATCH_OVERLAP_GAIN scales the right side (default 1; 0 = never start early, 1e9 = always) */
	static double gain = -1.0; if(gain < 0){ const char *e = getenv("WTZ_BATCH_OVERLAP_GAIN"); gain = e ? atof(e) : 1.0; }
	if(!nb || !b->pf_inflight || nb->formed || gain <= 0) return;
	const double rate = (s0 >= 64 && b->used_queries >= 32) ? (double)(E->step.n_masked - b->masked_at_form) / (double)b->used_queries : E->step.last_mask_rate;
	uint64_t left = 0; for(uint32_t j = E->step.cursor; j < E->step.qend; j++) left += !E->masked[j];
	uint32_t n_last = 0; for(uint32_t s = s0; s < s1; s++) n_last += (b->want[s] && !E->masked[b->bq[s]]);
	double waste = rate < 0 ? 1.0 : rate * (double)n_last / (double)(left ? left : 1); if(waste > 1.0) waste = 1.0;
	prefetch_move(b, nb);
	if(!batch_form(nb)) return; else nb->formed = 1;
	if(!nb->nbq) return;
	const uint32_t s1n = range_end(E, nb, 0);
	uint64_t rows = 0; for(uint32_t s = 0; s < s1n; s++) rows += nb->want[s] ? nb->nrow[s] : 0;
	pthread_mutex_lock(&E->mu);
	const double per_pair = E->step.spec_pairs ? E->step.t_gpu / (double)E->step.spec_pairs : -1.0, per_commit = E->step.used_queries ? E->step.t_commit / (double)E->step.used_queries : 0.0;
	pthread_mutex_unlock(&E->mu);
	const double cost = per_pair < 0 ? 1e30 : waste * (double)rows * per_pair, hidden = (double)n_last * per_commit + 0.003;
	const int early = gain >= 1e8 || cost <= gain * hidden;
	if(getenv("WTZ_BATCH_OVERLAP_TRACE")) fprintf(stderr, "[batch-overlap] batch %llu: %.2f new masks per used query, last range %u queries, %llu unmasked reads to come: share masked %.3f; first range of the next batch %llu pairs: expected waste %.1f ms against %.1f ms hidden -> %s\n",
		(unsigned long long)b->seq, rate, n_last, (unsigned long long)left, waste, (unsigned long long)rows, cost < 1e29 ? cost * 1e3 : -1.0, hidden * 1e3, early ? "started early" : "formed only");
	if(!early) return; else if(nb->start_job == NULL) nb->start_job = calloc(1, sizeof(gpujob_t));
	range_launch(E, nb, (gpujob_t*)nb->start_job, 0, &nb->start_s1);      /* the same end as s1n: nothing that range_end reads has moved */
	nb->started = 1;
}
static void process_batch(eng_t *E, batch_t *b){
	static int overlap = -1;
	if(overlap < 0){ const char *e = getenv("WTZ_RANGE_OVERLAP"); overlap = e ? atoi(e) : 1; }
	if(!overlap || E->n_workers != 1 || b->nbq == 0){ b->cparts = b->parts; process_batch_serial(E, b, 0); return; }
	if(b->start_job == NULL) b->start_job = calloc(1, sizeof(gpujob_t));
	gpujob_t *job = (gpujob_t*)b->start_job;      /* lives in the batch: the batch before may have started our first range already */
	uint32_t s0 = 0, s1;
	if(b->started){ s1 = b->start_s1; b->started = 0; }      /* the batch before this one started our first range in front of its last commit */
	else range_launch(E, b, job, s0, &s1);
	for(;;){
		if(gpujob_wait(job)){
			/* scratch pool exhausted: nothing of [s0, s1) is committed and nothing else is in flight: the serial path splits it */
			for(uint32_t d = 0; d < b->nparts; d++) part_text_wait(&b->parts[d], NULL);
			b->cparts = b->parts;
			range_overflowed(E, b, s0, s1, job->err); ranges_count_one(E);
			s0 = s1;
			if(s0 >= b->nbq) break;
			range_launch(E, b, job, s0, &s1);
			continue;
		}
		const double t_gpu = job->t1 - job->t0;
		const uint32_t r_npair = b->npair, r_nitem = b->nitem;
		range_measure_pool(E, b); parts_results_to_spare(b);
		double t_call[5] = {0, 0, 0, 0, 0}, t_io0 = 0; parts_fold_times(b, t_call, &t_io0);
		/* next range: planned now (one range of staleness), computed while this one is committed */
		const uint32_t n0 = s1;
		uint32_t n1 = n0;
		if(n0 < b->nbq) range_launch(E, b, job, n0, &n1);
		else {
			if(!b->pf_inflight){ pthread_mutex_lock(&E->mu); prefetch_begin(E, b); pthread_mutex_unlock(&E->mu); }
			next_batch_early(E, b, s0, s1);
		}
		for(uint32_t d = 0; d < b->nparts; d++) part_text_wait(&b->spare[d], &t_call[4]);      /* the finished range's text: its copy ran beside the planning above and the first kernels of the next range */
		range_commit(E, b, s0, s1, r_npair, r_nitem, t_gpu, t_call, t_io0, now_s());
		ranges_count_one(E);
		if(n0 >= b->nbq) break;
		s0 = n0; s1 = n1;
	}
	b->cparts = b->parts;
}
static void *worker_main(void *arg){
	batch_t *b = (batch_t*)arg; eng_t *E = b->E;
	for(;;){
		if(!b->formed && !batch_form(b)) break;       /* formed already: by the batch before it, in front of its last commit */
		b->formed = 0;
		if(b->nbq) process_batch(E, b);
		/* ---- hand the turn to the next batch ---- */
		pthread_mutex_lock(&E->mu);
		while(!b->holds_turn && E->step.commit_seq != b->seq) pthread_cond_wait(&E->cv, &E->mu);
		E->step.commit_seq = b->seq + 1;
		if(b->used_queries * 2 < b->spec_queries && E->step.B > E->first_batch){ E->step.B /= 2; if(E->step.B < 8) E->step.B = 8; }   /* too much discarded work */
		E->step.last_mask_rate = b->used_queries ? (double)(E->step.n_masked - b->masked_at_form) / (double)b->used_queries : -1.0;
		pthread_cond_broadcast(&E->cv);
		pthread_mutex_unlock(&E->mu);
		if(b->alt && b->alt->formed) b = b->alt;      /* formed (and started) in front of this batch's last commit */
	}
	return NULL;
}
