/* wtzmo host driver, section 5 of 6: one process per GPU (the protocol of wtzmo_types.h) and the k-mer index sharded by read id */
/* rank 0, at a boundary of the protocol (every other rank is waiting for the next request): end all ranks */
static void ranks_abort(const char *why){
	fprintf(stderr, " -- %s: ending all %d ranks --\n", why, g_dist.world);
	wtz_dist_hdr_t h; memset(&h, 0, sizeof h); h.cmd = WTZ_CMD_ABORT;
	g_dist.bcast(&h, sizeof h);
	DIE_NOW();
}
/* test hook: WTZ_RANK_FAIL_AT="<rank>:<n>" makes that rank's n-th device-stage request fail (the in-band abort path must end every rank with exit code 1) */
static int rank_fail_injected(void){
	static int rank = -2, at = 0, seen = 0;
	if(rank == -2){ const char *e = getenv("WTZ_RANK_FAIL_AT"); rank = -1; if(e && sscanf(e, "%d:%d", &rank, &at) != 2) rank = -1; }
	if(rank != g_dist.rank) return 0;
	if(++seen != at) return 0;
	fprintf(stderr, " -- rank %d: injected failure of request %d (WTZ_RANK_FAIL_AT) --\n", g_dist.rank, at);
	return 1;
}

static uint8_t *part_xbuf(part_t *pt, uint64_t n){
	if(n > pt->xcap){ pt->xcap = n + n / 4 + 4096; pt->xbuf = (uint8_t*)hx_realloc(pt->xbuf, pt->xcap); }
	return pt->xbuf;
}
/* rank 0: part r of the range is computed by rank r (part 0 here, meanwhile) */
static int gpu_stages_ranks(eng_t *E, batch_t *b){
	const int dm = E->P.dot_matrix;
	wtz_dist_hdr_t h; memset(&h, 0, sizeof h); h.cmd = WTZ_CMD_PAIRS;
	for(uint32_t r = 0; r < b->nparts; r++) h.count[r] = b->parts[r].npair;
	g_dist.bcast(&h, sizeof h);
	for(uint32_t r = 1; r < b->nparts; r++){
		part_t *pt = &b->parts[r];
		if(pt->npair){      /* queries | candidates in one message */
			uint8_t *x = part_xbuf(pt, 8 * (uint64_t)pt->npair);
			memcpy(x, pt->pq, 4 * (size_t)pt->npair); memcpy(x + 4 * (size_t)pt->npair, pt->pc, 4 * (size_t)pt->npair);
			g_dist.send(x, 8 * (uint64_t)pt->npair, (int)r);
		}
	}
	b->parts[0].E = E;
	int st = b->parts[0].again = rank_fail_injected() ? WTZ_ST_FAILED : part_stages(E, &b->parts[0]);
	int failed = st == WTZ_ST_FAILED ? 0 : -1;      /* the rank that failed (its replies still complete the round) */
	for(uint32_t r = 1; r < b->nparts; r++){
		part_t *pt = &b->parts[r];
		uint64_t rh[4]; g_dist.recv(rh, sizeof rh, (int)r);
		pt->nitem = 0; pt->ncig = 0; pt->again = (int)rh[0];
		if(rh[0] == WTZ_ST_FAILED){ if(failed < 0) failed = (int)r; continue; }
		if(rh[0]){ if(st == WTZ_ST_OK) st = WTZ_ST_AGAIN; continue; }
		if(pt->npair == 0) continue;
		/* the reply proper: summaries | window boxes | alignment results in ONE message whose size the status word's counts give (round 5: three messages);
		 * the CIGAR text follows as a message of its own - it comes straight out of the peer's device memory */
		const uint64_t nb_r = dm ? 0 : rh[1], ni_r = dm ? 0 : rh[2];
		const uint64_t sz_sum = sizeof(wtz_pair_summary_t) * (uint64_t)pt->npair, sz_box = sizeof(wtz_winbox_t) * nb_r, sz_aln = sizeof(wtz_aln_result_t) * ni_r;
		uint8_t *x = part_xbuf(pt, sz_sum + sz_box + sz_aln);
		g_dist.recv(x, sz_sum + sz_box + sz_aln, (int)r);
		pt->sum = (wtz_pair_summary_t*)hx_realloc(pt->sum, sizeof(wtz_pair_summary_t) * (pt->npair + 1));
		memcpy(pt->sum, x, sz_sum);
		if(dm) continue;
		pt->box_off = (uint64_t*)hx_realloc(pt->box_off, 8 * ((size_t)pt->npair * 2 + 1));
		uint64_t nb = 0;
		for(uint32_t i = 0; i < pt->npair; i++) for(int d = 0; d < 2; d++){ pt->box_off[(size_t)i * 2 + d] = nb; nb += pt->sum[i].nwin[d]; }
		pt->box_off[(size_t)pt->npair * 2] = nb; pt->nbox = nb;
		if(nb != rh[1]){ fprintf(stderr, " -- rank %u reports %llu windows, its summaries say %llu --\n", r, (unsigned long long)rh[1], (unsigned long long)nb); DIE_NOW(); }
		if(nb > pt->capbox){ pt->capbox = nb; pt->boxes = (wtz_winbox_t*)hx_realloc(pt->boxes, sizeof(wtz_winbox_t) * nb); }
		if(nb) memcpy(pt->boxes, x + sz_sum, sz_box);
		part_plan_items(E, pt);
		if(pt->nitem != rh[2]){ fprintf(stderr, " -- rank %u aligned %llu items, the plan has %u --\n", r, (unsigned long long)rh[2], pt->nitem); DIE_NOW(); }
		if(pt->nitem){
			pt->aln = (wtz_aln_result_t*)hx_realloc(pt->aln, sizeof(wtz_aln_result_t) * pt->nitem);
			memcpy(pt->aln, x + sz_sum + sz_box, sz_aln);
			if(!part_text_buffer(pt, rh[3])) DIE_NOW();
			if(rh[3]) g_dist.recv(pt->cig, rh[3], (int)r);
			pt->ncig = rh[3];
		}
	}
	if(failed >= 0){ char why[64]; snprintf(why, sizeof why, "rank %d failed in the device stages of a range", failed); ranks_abort(why); }
	b->nitem = 0; for(uint32_t d = 0; d < b->nparts; d++) b->nitem += b->parts[d].nitem;
	return st;
}
/* all parts of the range side by side (one host thread per extra part); 1 = some part's scratch pool was too small */
static int gpu_stages(eng_t *E, batch_t *b){
	if(g_dist.world > 1) return gpu_stages_ranks(E, b);
	pthread_t th[16];
	for(uint32_t d = 1; d < b->nparts; d++){ b->parts[d].E = E; if(pthread_create(&th[d], NULL, part_main, &b->parts[d]) != 0){ fprintf(stderr, " -- cannot start a device thread --\n"); DIE_NOW(); } }
	b->parts[0].E = E; b->parts[0].again = part_stages(E, &b->parts[0]);
	int again = b->parts[0].again;
	for(uint32_t d = 1; d < b->nparts; d++){ pthread_join(th[d], NULL); again |= b->parts[d].again; }
	b->nitem = 0; for(uint32_t d = 0; d < b->nparts; d++) b->nitem += b->parts[d].nitem;
	return again;
}
/* ranks > 0: serve rank 0's requests with this GPU until the overlap phase is over.  A failure here never ends the process on the spot: it is reported in the
 * status word of the next reply (the requests in between are answered with empty payloads), and rank 0 ends all ranks with WTZ_CMD_ABORT. */
static void remote_loop(eng_t *E, part_t *pt){
	const int dm = E->P.dot_matrix; const int me = g_dist.rank;
	int failed = 0;
#define REMOTE_TRY(rc, what) do { if((rc) != WTZ_OK && !failed){ failed = 1; fprintf(stderr, " -- rank %d: %s failed: %s --\n", me, what, wtz_last_error()); } } while(0)
	pt->E = E;
	for(;;){
		wtz_dist_hdr_t h; g_dist.bcast(&h, sizeof h);
		if(h.cmd == WTZ_CMD_DONE) break;
		if(h.cmd == WTZ_CMD_ABORT){ fprintf(stderr, " -- rank %d: abort requested by rank 0 --\n", me); DIE_NOW(); }
		const uint32_t n = (uint32_t)h.count[me];
		if(h.cmd == WTZ_CMD_PAIRS){
			if(n > pt->cappair){ pt->cappair = n; pt->pq = (uint32_t*)hx_realloc(pt->pq, 4 * (size_t)n); pt->pc = (uint32_t*)hx_realloc(pt->pc, 4 * (size_t)n); }
			if(n){ uint8_t *x = part_xbuf(pt, 8 * (uint64_t)n); g_dist.recv(x, 8 * (uint64_t)n, 0); memcpy(pt->pq, x, 4 * (size_t)n); memcpy(pt->pc, x + 4 * (size_t)n, 4 * (size_t)n); }
			pt->npair = n;
			if(rank_fail_injected()) failed = 1;
			const int again = failed ? WTZ_ST_FAILED : part_stages(E, pt);
			if(again == WTZ_ST_FAILED) failed = 1;
			uint64_t rh[4] = { (uint64_t)again, pt->nbox, pt->nitem, pt->ncig };
			if(n == 0 || dm || again){ rh[1] = 0; rh[2] = 0; rh[3] = 0; }
			g_dist.send(rh, sizeof rh, 0);
			if(again || n == 0) continue;
			{
				const uint64_t sz_sum = sizeof(wtz_pair_summary_t) * (uint64_t)n, sz_box = dm ? 0 : sizeof(wtz_winbox_t) * pt->nbox, sz_aln = dm ? 0 : sizeof(wtz_aln_result_t) * (uint64_t)pt->nitem;
				uint8_t *x = part_xbuf(pt, sz_sum + sz_box + sz_aln);
				memcpy(x, pt->sum, sz_sum); if(sz_box) memcpy(x + sz_sum, pt->boxes, sz_box); if(sz_aln) memcpy(x + sz_sum + sz_box, pt->aln, sz_aln);
				g_dist.send(x, sz_sum + sz_box + sz_aln, 0);
			}
			if(!dm && pt->nitem && pt->ncig){ if(g_dist.send_dev) g_dist.send_dev(pt->cig_dev, pt->ncig, 0); else g_dist.send(pt->cig, pt->ncig, 0); }
		} else if(h.cmd == WTZ_CMD_ZIDX){
			const uint32_t nql = (uint32_t)h.arg[0]; const int have_c = h.arg[1] != 0;
			uint32_t *ql = (uint32_t*)hx_realloc(NULL, 4 * ((size_t)nql + 1)), *cl = (uint32_t*)hx_realloc(NULL, 4 * ((size_t)n + 1));
			if(nql) g_dist.bcast(ql, 4 * (uint64_t)nql);
			if(have_c && n) g_dist.recv(cl, 4 * (uint64_t)n, 0);
			if(!failed){ int rc = zbuild_part(pt->ctx, have_c, cl, n, 1, ql, nql); REMOTE_TRY(rc, "the z-mer index of the batch"); }
			free(ql); free(cl);
		} else if(h.cmd == WTZ_CMD_CAND_BEGIN){
			if(n > pt->cq_cap){ pt->cq_cap = n; pt->cq_ids = (uint32_t*)hx_realloc(pt->cq_ids, 4 * (size_t)n); pt->cq_nr = (uint32_t*)hx_realloc(pt->cq_nr, 4 * (size_t)n); pt->cq_rows = (uint64_t*)hx_realloc(pt->cq_rows, (size_t)n * E->stride * 8); }
			pt->cq_n = n;
			if(n){ g_dist.recv(pt->cq_ids, 4 * (uint64_t)n, 0); memset(pt->cq_rows, 0, (size_t)n * E->stride * 8); memset(pt->cq_nr, 0, 4 * (size_t)n); }
			if(!failed){ int rc = wtz_candidates_begin(pt->ctx, pt->cq_ids, n, pt->cq_rows, pt->cq_nr); REMOTE_TRY(rc, "wtz_candidates_begin"); }
		} else if(h.cmd == WTZ_CMD_CAND_END){
			if(!failed){ int rc = wtz_candidates_end(pt->ctx, pt->cq_rows, pt->cq_nr); REMOTE_TRY(rc, "wtz_candidates_end"); }
			{   /* status | rows | counts in one message of a size rank 0 knows (a failed rank sends the same size with the status set) */
				const uint64_t sz_rows = (uint64_t)pt->cq_n * E->stride * 8, sz_nr = 4 * (uint64_t)pt->cq_n;
				uint8_t *x = part_xbuf(pt, 8 + sz_rows + sz_nr);
				const uint64_t st = failed ? WTZ_ST_FAILED : WTZ_ST_OK; memcpy(x, &st, 8);
				if(pt->cq_n){ memcpy(x + 8, pt->cq_rows, sz_rows); memcpy(x + 8 + sz_rows, pt->cq_nr, sz_nr); }
				g_dist.send(x, 8 + sz_rows + sz_nr, 0);
			}
		} else if(h.cmd == WTZ_CMD_GRP_BEGIN){
			/* sharded index: every rank answers every query of the request with the groups of its shard */
			const uint32_t nq = (uint32_t)h.count[0];
			if(nq > pt->cq_cap){ pt->cq_cap = nq; pt->cq_ids = (uint32_t*)hx_realloc(pt->cq_ids, 4 * (size_t)nq); pt->cq_nr = (uint32_t*)hx_realloc(pt->cq_nr, 4 * (size_t)nq); pt->cq_rows = (uint64_t*)hx_realloc(pt->cq_rows, (size_t)nq * E->stride * 8); }
			pt->cq_n = nq;
			if(nq) g_dist.bcast(pt->cq_ids, 4 * (uint64_t)nq);
			if(!failed){ int rc = wtz_candidate_groups_begin(pt->ctx, pt->cq_ids, nq); REMOTE_TRY(rc, "wtz_candidate_groups_begin"); }
		} else if(h.cmd == WTZ_CMD_GRP_END){
			uint64_t tot = 0; uint64_t *gr = NULL;
			if(!failed){ int rc = wtz_candidate_groups_end(pt->ctx, pt->cq_nr); REMOTE_TRY(rc, "wtz_candidate_groups_end"); }
			if(!failed){
				for(uint32_t k = 0; k < pt->cq_n; k++) tot += pt->cq_nr[k];
				gr = (uint64_t*)hx_realloc(NULL, 8 * (tot + 1));
				int rc = wtz_candidate_groups_fetch(pt->ctx, gr, tot); REMOTE_TRY(rc, "wtz_candidate_groups_fetch");
			}
			{   /* status | group counts in one message of a known size, then the groups */
				uint8_t *x = part_xbuf(pt, 8 + 4 * (uint64_t)pt->cq_n);
				const uint64_t st = failed ? WTZ_ST_FAILED : WTZ_ST_OK; memcpy(x, &st, 8);
				if(pt->cq_n){ if(failed) memset(x + 8, 0, 4 * (size_t)pt->cq_n); else memcpy(x + 8, pt->cq_nr, 4 * (size_t)pt->cq_n); }
				g_dist.send(x, 8 + 4 * (uint64_t)pt->cq_n, 0);
				if(!failed && tot) g_dist.send(gr, 8 * tot, 0);
			}
			free(gr);
		} else { fprintf(stderr, " -- rank %d: unknown request %llu --\n", me, (unsigned long long)h.cmd); DIE_NOW(); }
	}
#undef REMOTE_TRY
}
/* ---- k-mer index sharded by read-id range over the devices (--shard-index; include/wtzmo_hip.h).  One exchange: the shards' distinct k-mers
 * with their counts are merged on the host, the frequency filter and the automatic cutoff (wtzmo.c:380-405) use the TOTAL counts, so the
 * tables together hold exactly the k-mers of the unsharded index and every seed run is the unsharded run cut at the shard borders. ---- */
#define SHARD_N(E) (g_dist.world > 1 ? (uint32_t)g_dist.world : (E)->ndev)      /* one shard per device of this process, or per rank (one process per GPU) */
static void shard_range(const eng_t *E, uint32_t n_rd, uint32_t d, uint32_t *b, uint32_t *e){
	const uint32_t N = SHARD_N(E), per = (n_rd + N - 1) / N;      /* contiguous id ranges like the reference's -G parts (wtzmo.c:1281-1285) */
	*b = d * per < n_rd ? d * per : n_rd; *e = (d + 1) * per < n_rd ? (d + 1) * per : n_rd;
}
static void shard_index_build(eng_t *E, uint32_t n_rd, uint32_t *K_io){
	const uint32_t N = SHARD_N(E); const int ranks = g_dist.world > 1, me = g_dist.rank;
	uint64_t nd[WTZ_DIST_MAX], nocc[WTZ_DIST_MAX], *km[WTZ_DIST_MAX]; uint32_t *lc[WTZ_DIST_MAX], *tc[WTZ_DIST_MAX];
	memset(km, 0, sizeof km); memset(lc, 0, sizeof lc); memset(tc, 0, sizeof tc);
	for(uint32_t d = 0; d < N; d++){
		if(ranks && (int)d != me) continue;                         /* the other ranks count their own shards */
		wtz_ctx_t *cx = ranks ? E->ctx : E->ctxs[d];
		uint32_t b, e; shard_range(E, n_rd, d, &b, &e);
		int rc = wtz_index_count(cx, b, e, &nd[d], &nocc[d]); DIE_WTZ(rc, "wtz_index_count");
		km[d] = (uint64_t*)hx_realloc(NULL, 8 * (nd[d] + 1)); lc[d] = (uint32_t*)hx_realloc(NULL, 4 * (nd[d] + 1)); tc[d] = (uint32_t*)hx_realloc(NULL, 4 * (nd[d] + 1));
		rc = wtz_index_counts_fetch(cx, km[d], lc[d]); DIE_WTZ(rc, "wtz_index_counts_fetch");
	}
	uint64_t kbuf[4] = {0, 0, 0, 0};      /* K, occurrences, distinct, table entries: rank 0 -> all */
	if(ranks && me != 0){
		/* the one exchange of the build: this shard's (k-mer, count) list to rank 0, the total counts of the same k-mers back */
		uint64_t hd[2] = { nd[me], nocc[me] };
		g_dist.send(hd, sizeof hd, 0);
		if(nd[me]){ g_dist.send(km[me], 8 * nd[me], 0); g_dist.send(lc[me], 4 * nd[me], 0); g_dist.recv(tc[me], 4 * nd[me], 0); }
		g_dist.bcast(kbuf, sizeof kbuf);
		uint64_t kept = 0; int rc = wtz_index_finish(E->ctx, tc[me], (uint32_t)kbuf[0], &kept); DIE_WTZ(rc, "wtz_index_finish");
		*K_io = (uint32_t)kbuf[0];
		free(km[me]); free(lc[me]); free(tc[me]);
		return;
	}
	if(ranks) for(uint32_t r = 1; r < N; r++){
		uint64_t hd[2]; g_dist.recv(hd, sizeof hd, (int)r); nd[r] = hd[0]; nocc[r] = hd[1];
		km[r] = (uint64_t*)hx_realloc(NULL, 8 * (nd[r] + 1)); lc[r] = (uint32_t*)hx_realloc(NULL, 4 * (nd[r] + 1)); tc[r] = (uint32_t*)hx_realloc(NULL, 4 * (nd[r] + 1));
		if(nd[r]){ g_dist.recv(km[r], 8 * nd[r], (int)r); g_dist.recv(lc[r], 4 * nd[r], (int)r); }
	}
	/* N-way merge of the ascending lists: total count per k-mer, ktyp = distinct k-mers, ktot = sum of the saturating counts (wtzmo.c:276, 380-388) */
	uint64_t pos[WTZ_DIST_MAX], ktyp = 0, ktot = 0; memset(pos, 0, sizeof pos);
	for(;;){
		uint64_t m = ~0ull; int any = 0;
		for(uint32_t d = 0; d < N; d++) if(pos[d] < nd[d]){ if(!any || km[d][pos[d]] < m) m = km[d][pos[d]]; any = 1; }
		if(!any) break;
		uint64_t tot = 0;
		for(uint32_t d = 0; d < N; d++) if(pos[d] < nd[d] && km[d][pos[d]] == m) tot += lc[d][pos[d]];
		const uint32_t t32 = tot > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)tot;
		for(uint32_t d = 0; d < N; d++) if(pos[d] < nd[d] && km[d][pos[d]] == m){ tc[d][pos[d]] = t32; pos[d]++; }
		ktyp++; ktot += tot > 0xFFFFu ? 0xFFFFu : tot;
	}
	uint32_t K = *K_io;
	if(K < 2){ uint32_t kavg = (uint32_t)(ktot / (ktyp + 1)); if(kavg < 20) kavg = 20; K = kavg * 5; }       /* wtzmo.c:380-393 */
	*K_io = K;
	uint64_t occ = 0, kept_all = 0;
	for(uint32_t d = 0; d < N; d++){
		occ += nocc[d];
		if(ranks && d){ if(nd[d]) g_dist.send(tc[d], 4 * nd[d], (int)d); }
		else { uint64_t kept = 0; int rc = wtz_index_finish(ranks ? E->ctx : E->ctxs[d], tc[d], K, &kept); DIE_WTZ(rc, "wtz_index_finish"); kept_all += kept; }
		free(km[d]); free(lc[d]); free(tc[d]);
	}
	if(ranks){ kbuf[0] = K; kbuf[1] = occ; kbuf[2] = ktyp; g_dist.bcast(kbuf, sizeof kbuf); }
	fprintf(stderr, "[wtzmo-mi355x] index in %u shards by read id%s: %llu k-mer occurrences, %llu distinct, %llu table entries%s, cutoff %u\n", N, ranks ? " (one per rank)" : "",
		(unsigned long long)occ, (unsigned long long)ktyp, (unsigned long long)kept_all, ranks ? " in shard 0" : " over the shards", K);
}
/* candidate heaps of n queries against the sharded index: every shard answers every query with its (read, strand) groups (key order); the
 * shards are ascending id ranges, so their lists in shard order are the unsharded group list, and the heap replay runs over that */
static void shard_candidates_begin(eng_t *E, const uint32_t *ids, uint32_t n){
	if(g_dist.world > 1){
		wtz_dist_hdr_t h; memset(&h, 0, sizeof h); h.cmd = WTZ_CMD_GRP_BEGIN; h.count[0] = n;
		g_dist.bcast(&h, sizeof h);
		if(n) g_dist.bcast((void*)ids, 4 * (uint64_t)n);
		int rc = wtz_candidate_groups_begin(E->ctx, ids, n); DIE_WTZ(rc, "wtz_candidate_groups_begin");
		return;
	}
	for(uint32_t d = 0; d < E->ndev; d++){ int rc = wtz_candidate_groups_begin(E->ctxs[d], ids, n); DIE_WTZ(rc, "wtz_candidate_groups_begin"); }
}
static void shard_candidates_end(eng_t *E, uint32_t n, uint64_t *rows, uint32_t *nr){
	const uint32_t N = SHARD_N(E); const int ranks = g_dist.world > 1;
	uint32_t *ng[WTZ_DIST_MAX]; uint64_t *gr[WTZ_DIST_MAX], tot[WTZ_DIST_MAX]; int failed = -1;
	if(ranks){ wtz_dist_hdr_t h; memset(&h, 0, sizeof h); h.cmd = WTZ_CMD_GRP_END; g_dist.bcast(&h, sizeof h); }
	for(uint32_t d = 0; d < N; d++){
		ng[d] = (uint32_t*)hx_realloc(NULL, 4 * ((size_t)n + 1));
		if(ranks && d){
			uint64_t st = 0;
			{ uint8_t *x = (uint8_t*)hx_realloc(NULL, 8 + 4 * (size_t)n); g_dist.recv(x, 8 + 4 * (uint64_t)n, (int)d); memcpy(&st, x, 8); if(n) memcpy(ng[d], x + 8, 4 * (size_t)n); free(x); }
			tot[d] = 0; gr[d] = NULL;
			if(st != WTZ_ST_OK){ if(failed < 0) failed = (int)d; memset(ng[d], 0, 4 * ((size_t)n + 1)); continue; }
			for(uint32_t k = 0; k < n; k++) tot[d] += ng[d][k];
			gr[d] = (uint64_t*)hx_realloc(NULL, 8 * (tot[d] + 1));
			if(tot[d]) g_dist.recv(gr[d], 8 * tot[d], (int)d);
			continue;
		}
		wtz_ctx_t *cx = ranks ? E->ctx : E->ctxs[d];
		int rc = wtz_candidate_groups_end(cx, ng[d]);
		tot[d] = 0; gr[d] = NULL;
		if(rc == WTZ_OK){
			for(uint32_t k = 0; k < n; k++) tot[d] += ng[d][k];
			gr[d] = (uint64_t*)hx_realloc(NULL, 8 * (tot[d] + 1));
			rc = wtz_candidate_groups_fetch(cx, gr[d], tot[d]);
		}
		if(rc != WTZ_OK && ranks){ fprintf(stderr, " -- rank 0: the candidate groups of its shard failed: %s --\n", wtz_last_error()); if(failed < 0) failed = 0; memset(ng[d], 0, 4 * ((size_t)n + 1)); tot[d] = 0; continue; }
		DIE_WTZ(rc, "wtz_candidate_groups_end / _fetch");
	}
	if(failed >= 0){ char why[64]; snprintf(why, sizeof why, "rank %d failed in the sharded seed lookup", failed); ranks_abort(why); }
	uint64_t off[WTZ_DIST_MAX], *join = NULL; size_t capj = 0; memset(off, 0, sizeof off);
	for(uint32_t k = 0; k < n; k++){
		size_t m = 0; for(uint32_t d = 0; d < N; d++) m += ng[d][k];
		if(m + 1 > capj){ capj = (m + 1) * 2; join = (uint64_t*)hx_realloc(join, 8 * capj); }
		m = 0; for(uint32_t d = 0; d < N; d++){ memcpy(join + m, gr[d] + off[d], 8 * (size_t)ng[d][k]); m += ng[d][k]; off[d] += ng[d][k]; }
		uint32_t hn = nr[k];
		wtz_cand_tail_host(join, (uint32_t)m, E->P.kovl, E->P.ncand, rows + (size_t)k * E->stride, &hn);
		nr[k] = hn;
	}
	free(join);
	for(uint32_t d = 0; d < N; d++){ free(ng[d]); free(gr[d]); }
}
