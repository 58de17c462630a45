/* wtzmo host driver, section 3 of 6: the order-dependent commit - pending state, records, the prepared part of a query (also by helper threads), commit_query */
/* ---------------- record writer + state merge (wtzmo.c:1170-1249, 1319-1329) ---------------- */
static void order_push(eng_t *E, uint64_t v){
	if(!E->keep_order) return;
	if(E->n_order == E->cap_order){ E->cap_order = E->cap_order ? E->cap_order * 2 : 4096; E->closed_order = (uint64_t*)hx_realloc(E->closed_order, 8 * E->cap_order); }
	E->closed_order[E->n_order++] = v;
}
static void flush_pending(eng_t *E){
	pending_t *p = &E->pend;
	const hx_read_t *reads = E->st.reads;
	if(p->rd_id != 0xFFFFFFFFu){
		if(!E->do_align){
			for(size_t i = 0; i < p->nseed; i++){
				const seed_t *s = &p->seeds[i];
				if(s->closed) continue;
				char *o = (char*)hx_realloc(NULL, strlen(reads[p->rd_id].name) + strlen(reads[s->pb2].name) + 96);
				out_raw(o, (size_t)sprintf(o, "# %s\t%c\t%d\t%s\t%c\t%d\t%d\n", reads[p->rd_id].name, '+', reads[p->rd_id].len,
					reads[s->pb2].name, "+-"[s->dir], reads[s->pb2].len, s->ovl));
			}
		} else {
			for(size_t j = 0; j < p->nhit; j++){
				hit_t *h = &p->hits[j];
				E->step.nrec++;
				if(h->aln == 0) h->aln = 1;
				uint32_t x1 = (uint32_t)(h->tb < h->qb ? h->tb : h->qb);
				int r1 = (int)reads[h->pb1].len - h->te, r2 = (int)reads[h->pb2].len - h->qe;
				uint32_t x2 = (uint32_t)(r1 < r2 ? r1 : r2);
				if(x1 + x2 <= 200u){ E->rdcovs[h->pb1]++; E->rdcovs[h->pb2]++; }          /* max_unalign_in_dovetail, wtzmo.c:175 */
				/* the record itself was queued for the writer thread when the hit was committed (emit_record): same order, same bytes */
			}
		}
	}
	p->nhit = 0; p->nseed = 0;
	for(size_t i = 0; i < p->nmask; i++){ if(!E->masked[p->masks[i]]) E->step.n_masked++; E->masked[p->masks[i]] = 1; }
	p->nmask = 0;
	for(size_t i = 0; i < p->nclosed; i++){
		if(hx_set_put(&E->closed, p->closed[i])){
			order_push(E, p->closed[i]);
			uint32_t a = (uint32_t)(p->closed[i] >> 33), b = (uint32_t)((p->closed[i] & 0xFFFFFFFFu) >> 1);
			E->step.pair_bp += (uint64_t)E->rdlen[a] + E->rdlen[b]; E->step.n_pairs++;
			/* behind the insertion: a helper that sees the new count sees the pair (cq_spec_*) */
			__atomic_store_n(&E->closed_touch[a], E->closed_touch[a] + 1u, __ATOMIC_RELEASE); __atomic_store_n(&E->closed_touch[b], E->closed_touch[b] + 1u, __ATOMIC_RELEASE);      /* one writer: a release store, not a locked read-modify-write */
		}
	}
	p->nclosed = 0;
}

static void pend_mask(pending_t *p, uint32_t id){
	for(size_t i = 0; i < p->nmask; i++) if(p->masks[i] == id) return;
	if(p->nmask == p->capmask){ p->capmask = p->capmask ? p->capmask * 2 : 16; p->masks = (uint32_t*)hx_realloc(p->masks, p->capmask * 4); }
	p->masks[p->nmask++] = id;
}
/* what flush_pending will touch for this pair, requested now (one query early): its slot of the closed-pair table (a random line of a table of tens of MB: the merge of
 * a configs[2] step's 487 000 pairs was 0.07 s of misses) and the two reads' counters */
static eng_t *g_pend_eng = NULL;
static inline void pend_prefetch_pair(uint64_t v){
	const eng_t *E = g_pend_eng;
	if(!E || !E->closed.cap) return;
	__builtin_prefetch(&E->closed.tab[hx_mix(v) & (E->closed.cap - 1)], 1, 1);
	const uint32_t a = (uint32_t)(v >> 33), b = (uint32_t)((v & 0xFFFFFFFFu) >> 1);
	__builtin_prefetch(&E->closed_touch[a], 1, 1); __builtin_prefetch(&E->closed_touch[b], 1, 1);
}
static void pend_closed(pending_t *p, uint64_t v){
	pend_prefetch_pair(v);
	if(p->nclosed == p->capclosed){ p->capclosed = p->capclosed ? p->capclosed * 2 : 64; p->closed = (uint64_t*)hx_realloc(p->closed, p->capclosed * 8); }
	p->closed[p->nclosed++] = v;
}
static void pend_hit(pending_t *p, const hit_t *h){
	if(g_pend_eng){ __builtin_prefetch(&g_pend_eng->rdcovs[h->pb2], 1, 1); }
	if(p->nhit == p->caphit){ p->caphit = p->caphit ? p->caphit * 2 : 64; p->hits = (hit_t*)hx_realloc(p->hits, p->caphit * sizeof(hit_t)); }
	p->hits[p->nhit++] = *h;
}

/* one .ovl line (print_hits_wtzmo, wtzmo.c:1170-1249) queued for the writer thread; cigar == NULL prints "0M" */
static void emit_record(eng_t *E, const hit_t *h, const char *cigar, size_t cigar_len, int ext){
	(void)E;
	orec_t *r = out_slot(cigar_len + 128);
	r->pb1 = h->pb1; r->pb2 = h->pb2; r->tb = h->tb; r->te = h->te; r->qb = h->qb; r->qe = h->qe; r->score = h->score;
	r->mat = h->mat; r->mis = h->mis; r->ins = h->ins; r->del = h->del; r->aln = h->aln; r->dir2 = (uint8_t)h->dir2; r->kind = 0;
	r->cigar = cigar; r->cigar_len = (uint32_t)cigar_len; r->ext = (int8_t)ext;
	/* The text is read LATER, on a writer thread - the short ones too (they are copied into the formatted run there) - so every record that points into a
	 * text buffer holds that buffer (ext_busy) until its chunk is on the stream, whatever its length: a chunk of short records only used to leave the
	 * buffer unprotected, and the part refilled (or freed) it two ranges later under a writer that lagged behind a slow consumer. */
	if(cigar && cigar_len > 0 && !(ext >= 0 && ext < OW_MAX_EXT)){      /* a text buffer the writer does not track (parts beyond OW_MAX_EXT / 2): the record takes a copy */
		char *cp = (char*)hx_realloc(NULL, cigar_len); memcpy(cp, cigar, cigar_len); r->cigar = cp; r->kind = 2;
	} else if(cigar && cigar_len > 0){
		owriter_t *w = &g_ow; ochunk_t *c = w->cur;
		if(!(c->ext_mask & (1u << ext))){ c->ext_mask |= 1u << ext; pthread_mutex_lock(&w->mu); w->ext_busy[ext]++; pthread_mutex_unlock(&w->mu); }
	}
}

__attribute__((unused)) static char *cigar_text(const uint32_t *c, uint32_t n){        /* kswx.h:1093-1120 */
	size_t cap = (size_t)n * 11 + 2, k = 0; char *s = (char*)hx_realloc(NULL, cap);
	for(uint32_t i = 0; i < n; i++){
		uint32_t op = c[i] & 0xF, len = c[i] >> 4;
		if(len == 0) continue;
		if(op > 2){ fprintf(stderr, " -- CIGAR only support M(0),I(1),D(2) cigar, but met ?(%u) --\n", op); DIE_NOW(); }
		char d[12]; int nd = 0;
		while(len){ d[nd++] = (char)('0' + len % 10); len /= 10; }
		while(nd) s[k++] = d[--nd];
		s[k++] = "MID"[op];
	}
	s[k] = 0; return s;
}

/* a[i] <- a[lo] + ... + a[i] for i in [lo, hi), 16-bit wrap-around; lo is a multiple of 8 */
#ifdef __SSE2__
#include <emmintrin.h>
#endif
static void depth_prefix_u16(uint16_t *a, size_t lo, size_t hi){
	size_t i = lo; uint16_t run = 0;
#ifdef __SSE2__
	__m128i carry = _mm_setzero_si128();
	for(; i + 8 <= hi; i += 8){
		__m128i x = _mm_loadu_si128((const __m128i*)(a + i));
		x = _mm_add_epi16(x, _mm_slli_si128(x, 2)); x = _mm_add_epi16(x, _mm_slli_si128(x, 4)); x = _mm_add_epi16(x, _mm_slli_si128(x, 8));
		x = _mm_add_epi16(x, carry);
		_mm_storeu_si128((__m128i*)(a + i), x);
		carry = _mm_shuffle_epi32(_mm_shufflehi_epi16(x, 0xFF), 0xFF);      /* the last sum in every word */
	}
	if(i > lo) run = a[i - 1];
#endif
	for(; i < hi; i++){ run = (uint16_t)(run + a[i]); a[i] = run; }
}

/* weights[i] of wtzmo.c:933-936: float = (depth rule); then float = float * (double positional factor) */
static inline float rep_weight(const uint16_t *windeps, const wtz_params_c *P, int alen, int i){
	float w = (windeps[i] <= P->win_rep_norm) ? 1.0 : ((windeps[i] >= P->win_rep_cutoff) ? 0.0 : P->win_rep_norm / (float)windeps[i]);
	int df = i < alen / 2 ? alen / 2 - i : i - alen / 2;
	w = w * (0.3 + 0.7 * (df / (alen / 2.0)));
	return w;
}

/* The commit of a query walks its pairs' summaries and window boxes - results that arrived from the device a moment ago and are in no cache - in candidate order:
 * 72 of the commit's 240 ms per configs[2] step were those misses (round 6, timers in parts).  The lines of the NEXT query's pairs are requested while this one is committed. */
static void commit_prefetch(const eng_t *E, const batch_t *b, uint32_t slot){
	if(!b->want[slot] || E->masked[b->bq[slot]]) return;
	const uint32_t n = b->nrow[slot]; const int dm = E->P.dot_matrix;
	for(uint32_t k = 0; k < n; k++){
		const uint32_t g = b->rowpair[(size_t)slot * E->stride + k];
		if(g == 0xFFFFFFFFu) continue;
		const part_t *pt = CPART_OF(b, g); const uint32_t li = LOCAL_OF(b, g);
		__builtin_prefetch(&pt->sum[li], 0, 1);
		if(!dm){ __builtin_prefetch(&pt->box_off[(size_t)li * 2], 0, 1); if(pt->item_of) __builtin_prefetch(&pt->item_of[li], 0, 1); }
	}
}
/* ---------------- commit of one query over the batch results (wtzmo.c:806-1130) ---------------- */
/* The part that does not depend on the ORDER of the commits, only on the set of closed pairs: candidates filtered by that set, in the reference's order, trimmed
 * (wtzmo.c:813-822); window depth, repeat-weighted seeds, seed order (wtzmo.c:905-986).  `racy`: called by a helper thread beside the committing thread (cq_spec_*). */
static void cq_prepare(const eng_t *E, const batch_t *b, uint32_t slot, cq_work_t *w, int racy){
	const wtz_params_c *P = &E->P;
	const uint32_t pbid = b->bq[slot];
	const int alen = (int)E->rdlen[pbid];
	const double tq0 = now_s();
	uint32_t nc = b->nrow[slot];
	if(w->capcand < (size_t)nc + 1){ w->capcand = ((size_t)nc + 1) * 2; w->cand = (cand_t*)hx_realloc(w->cand, sizeof(cand_t) * w->capcand); }
	cand_t *cand = w->cand;
	for(uint32_t i = 0; i < nc; i++){
		cand[i].e = b->rows[(size_t)slot * E->stride + i]; cand[i].pidx = b->rowpair[(size_t)slot * E->stride + i]; cand[i].pad = 0;
		const uint64_t key = hx_pair_key(pbid, cand[i].e >> 32);
		if(racy ? hx_set_has_racy(&E->closed, key) : hx_set_has(&E->closed, key)) cand[i].e &= 0xFFFFFFFF00000000ULL;
	}
	sort_cands_exact(cand, nc);
	while(nc && (uint32_t)cand[nc - 1].e == 0) nc--;
	w->nc = nc; w->nseed = 0; w->ngate = 0;
	const double tq1 = now_s(); w->t[0] = tq1 - tq0; w->t[1] = w->t[2] = w->t[3] = w->t[4] = 0;
	if(P->dot_matrix) return;
	for(uint32_t i = 0; i < nc; i++){       /* the window boxes of the pairs that are walked below (their summaries were requested one query ago: commit_prefetch) */
		if(cand[i].pidx == 0xFFFFFFFFu) continue;
		const part_t *pt = CPART_OF(b, cand[i].pidx); const uint32_t li = LOCAL_OF(b, cand[i].pidx);
		const wtz_pair_summary_t *S = &pt->sum[li];
		if(!S->gate) continue;
		const wtz_winbox_t *bx = pt->boxes + pt->box_off[(size_t)li * 2];
		const uint32_t nb = S->nwin[0] + S->nwin[1];
		for(uint32_t k = 0; k < nb; k += 4) __builtin_prefetch(bx + k, 0, 1);      /* 16-byte boxes: four per line */
	}
	if(w->capdep < (size_t)alen + 24){      /* zero from the start and after every query */
		w->capdep = ((size_t)alen + 24) * 2; free(w->dep);
		w->dep = (uint16_t*)calloc(w->capdep, 2); if(!w->dep){ fprintf(stderr, " -- Out of memory --\n"); DIE_NOW(); }
	}
	uint16_t *windeps = w->dep;
	int dep_lo = alen, dep_hi = 0;             /* span of the marks */
	if(w->capseeds < (size_t)nc + 1){ w->capseeds = ((size_t)nc + 1) * 2; w->seeds = (seed_t*)hx_realloc(w->seeds, sizeof(seed_t) * w->capseeds); }
	seed_t *seeds = w->seeds; uint32_t nseed = 0, ngate = 0;
	for(uint32_t i = 0; i < nc; i++){
		const uint32_t id2 = (uint32_t)(cand[i].e >> 32);
		if(cand[i].pidx == 0xFFFFFFFFu){ fprintf(stderr, " -- internal error: pair (%u,%u) missing from the batch plan --\n", pbid, id2); DIE_NOW(); }
		const part_t *pt = CPART_OF(b, cand[i].pidx); const uint32_t li = LOCAL_OF(b, cand[i].pidx);
		const wtz_pair_summary_t *S = &pt->sum[li];
		if(!S->gate) continue;
		ngate++;
		for(uint32_t dir = 0; dir < 2; dir++){
			const wtz_winbox_t *bx = pt->boxes + pt->box_off[(size_t)li * 2 + dir];
			for(uint32_t k = 0; k < S->nwin[dir]; k++){       /* wtzmo.c:908 increments windeps over [beg,end): kept as +1/-1 marks, summed below */
				const int wb = bx[k].beg[0], we = bx[k].end[0];
				if(wb < we){ windeps[wb]++; windeps[we]--; if(wb < dep_lo) dep_lo = wb; if(we > dep_hi) dep_hi = we; }
			}
		}
		const uint32_t dir = (S->ovl[0] < S->ovl[1]);
		if(S->ovl[dir] >= P->ztot){ seed_t sd; sd.pb2 = id2; sd.dir = dir; sd.ovl = S->ovl[dir]; sd.closed = 0; sd.pidx = cand[i].pidx; seeds[nseed++] = sd; }
	}
	const double tqa = now_s(); w->t[1] = tqa - tq1;
	/* running depth over the span of the marks (it is zero outside: every interval is closed); arithmetic modulo 2^16 like the reference's u2i counters */
	if(dep_lo < dep_hi) depth_prefix_u16(windeps, (size_t)(dep_lo & ~7), (size_t)dep_hi + 1);
	const double tqb = now_s(); w->t[2] = tqb - tqa;
	/* repeat weighting: the reference fills weights[0..alen) (wtzmo.c:933-936) but only reads the entry at the middle of each
	 * window (954): evaluated on demand by rep_weight() with the same float/double mix */
	for(uint32_t i = 0; i < nseed; i++){
		seed_t *sd = &seeds[i];
		const int blen = (int)E->rdlen[sd->pb2];
		const part_t *pt = CPART_OF(b, sd->pidx); const uint32_t li = LOCAL_OF(b, sd->pidx);
		const wtz_pair_summary_t *S = &pt->sum[li];
		const wtz_winbox_t *bx = pt->boxes + pt->box_off[(size_t)li * 2 + sd->dir];
		uint32_t ol = 0; double avg;
		for(uint32_t k = 0; k < S->nwin[sd->dir]; k++){
			avg = (bx[k].end[0] - bx[k].beg[0]) * rep_weight(windeps, P, alen, (bx[k].beg[0] + bx[k].end[0]) / 2);
			int mid = (int)((bx[k].beg[1] + bx[k].end[1]) / 2);
			int df = mid < blen / 2 ? blen / 2 - mid : mid - blen / 2;
			avg = avg * (0.3 + 0.7 * (df / (blen / 2.0)));
			ol += avg;
		}
		sd->ovl = ol & 0x1FFFFFFFu;
		if(ol * P->win_rep_cutoff < P->ztot * P->win_rep_norm) sd->closed = 1;                 /* wtzmo.c:964 */
	}
	const double tqc = now_s(); w->t[3] = tqc - tqb;
	sort_seeds_exact(seeds, nseed);
	if(dep_lo < dep_hi) memset(windeps + (dep_lo & ~7), 0, 2 * (size_t)(dep_hi + 1 - (dep_lo & ~7)));
	w->nseed = nseed; w->ngate = ngate; w->t[4] = now_s() - tqc;
}

/* ---- queries prepared ahead of the commit by helper threads (round 6).  The prepared part of a query depends on the closed-pair set only through the pairs that
 * hold the query's own read, so: every pair that enters the set bumps a counter of both its reads (flush_pending, AFTER the insertion); a helper notes the
 * query's counter BEFORE it reads the set; the committing thread takes a prepared query iff the counter has not moved since - otherwise it prepares the query
 * again itself, as before.  The set is read while the committing thread inserts into it: no growth happens meanwhile (hx_set_reserve in front of the range),
 * and a slot goes from empty to a key in one aligned store.  WTZ_COMMIT_HELPERS=<n> (default 4, 0 = none). ---- */
#define CQ_RING 64u
typedef struct { cq_work_t w; uint32_t v0; int skipped; uint64_t ready_for; } cq_ent_t;      /* ready_for == slot + 1: filled for that slot */
typedef struct cq_spec_s {
	eng_t *E; const batch_t *b; uint32_t s0, s1;
	uint64_t next, done; int stop, active, nth;        /* next: the slot a helper takes next; done: slots below it are consumed (a ring entry is free again) */
	pthread_t th[16]; cq_ent_t ring[CQ_RING];
} cq_spec_t;
static void *cq_spec_main(void *arg){
	cq_spec_t *sp = (cq_spec_t*)arg; eng_t *E = sp->E; const batch_t *b = sp->b;
	for(;;){
		uint64_t s = __atomic_load_n(&sp->next, __ATOMIC_RELAXED);
		if(s >= sp->s1 || __atomic_load_n(&sp->stop, __ATOMIC_RELAXED)) break;
		if(s >= __atomic_load_n(&sp->done, __ATOMIC_ACQUIRE) + CQ_RING){ cpu_relax(); continue; }      /* the ring is full: the commit has to catch up */
		if(!__atomic_compare_exchange_n(&sp->next, &s, s + 1, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) continue;
		cq_ent_t *en = &sp->ring[s % CQ_RING];
		/* the entry's previous occupant (slot s - CQ_RING) may have been passed by the commit without being waited for (a masked or saturated query) while its helper is
		 * still at work: it has been taken before this slot and will finish */
		if(s >= (uint64_t)sp->s0 + CQ_RING) while(__atomic_load_n(&en->ready_for, __ATOMIC_ACQUIRE) != s - CQ_RING + 1) cpu_relax();
		const uint32_t pbid = b->bq[s];
		en->skipped = (!b->want[s] || __atomic_load_n(&E->masked[pbid], __ATOMIC_RELAXED)) ? 1 : 0;
		if(!en->skipped){
			en->v0 = __atomic_load_n(&E->closed_touch[pbid], __ATOMIC_ACQUIRE);
			cq_prepare(E, b, (uint32_t)s, &en->w, 1);
		}
		__atomic_store_n(&en->ready_for, s + 1, __ATOMIC_RELEASE);
	}
	return NULL;
}
/* Room the closed-pair table needs in front of a range so that it does not grow (hx_set_reserve: EXTRA keys without a growth step; a growth frees the table the helpers read)
 * while the helpers run.  What the commit of the range can insert: a planned pair closes at most once (npair); the first flush_pending of the range merges what the query
 * before it left pending (pend.nclosed); one query's rows (stride) on top, so that the bound does not hang on where in a query the range begins. */
static size_t cq_closed_room(const eng_t *E, uint64_t npair){ return (size_t)npair + E->pend.nclosed + E->stride; }
static void cq_spec_start(eng_t *E, const batch_t *b, uint32_t s0, uint32_t s1, uint64_t npair){
	static int nth = -1;
	if(nth < 0){ const char *e = getenv("WTZ_COMMIT_HELPERS"); nth = e ? atoi(e) : 4; if(nth < 0) nth = 0; if(nth > 16) nth = 16; }
	if(!E->spec){ E->spec = (cq_spec_t*)calloc(1, sizeof(cq_spec_t)); if(!E->spec) DIE_NOW(); }
	cq_spec_t *sp = E->spec;
	sp->active = 0;
	if(nth == 0 || E->step.rows_all || s1 < s0 + 2) return;
	hx_set_reserve(&E->closed, cq_closed_room(E, npair));
	sp->E = E; sp->b = b; sp->s0 = s0; sp->s1 = s1; sp->next = s0; sp->done = s0; sp->stop = 0; sp->nth = 0;
	for(uint32_t k = 0; k < CQ_RING; k++) sp->ring[k].ready_for = 0;
	for(int k = 0; k < nth; k++){ if(pthread_create(&sp->th[sp->nth], NULL, cq_spec_main, sp) == 0) sp->nth++; }
	sp->active = sp->nth > 0;
}
static inline void cq_spec_done(eng_t *E, uint32_t slot){ if(E->spec && E->spec->active) __atomic_store_n(&E->spec->done, (uint64_t)slot + 1, __ATOMIC_RELEASE); }
static void cq_spec_stop(eng_t *E){
	cq_spec_t *sp = E->spec;
	if(!sp || !sp->active) return;
	__atomic_store_n(&sp->stop, 1, __ATOMIC_RELAXED);
	for(int k = 0; k < sp->nth; k++) pthread_join(sp->th[k], NULL);
	sp->active = 0;
}
/* the prepared part of query `slot`: a helper's if it is still valid, else made here */
static cq_work_t *cq_take(eng_t *E, batch_t *b, uint32_t slot){
	cq_spec_t *sp = E->spec;
	if(sp && sp->active){
		cq_ent_t *en = &sp->ring[slot % CQ_RING];
		const double t0 = now_s();
		while(__atomic_load_n(&en->ready_for, __ATOMIC_ACQUIRE) != (uint64_t)slot + 1) cpu_relax();      /* slots are taken in order: some helper has this one */
		E->step.t_spec_wait += now_s() - t0;
		if(!en->skipped && __atomic_load_n(&E->closed_touch[b->bq[slot]], __ATOMIC_ACQUIRE) == en->v0){ E->step.n_spec_hit++; return &en->w; }
		E->step.n_spec_miss++;
	}
	cq_prepare(E, b, slot, &E->cq, 0);
	E->step.t_cq[0] += E->cq.t[0]; E->step.t_cq[1] += E->cq.t[1] + E->cq.t[2] + E->cq.t[3] + E->cq.t[4];
	for(int k = 0; k < 4; k++) E->step.t_cq1[k] += E->cq.t[k + 1];
	return &E->cq;
}

static void commit_query(eng_t *E, batch_t *b, uint32_t slot){
	const wtz_params_c *P = &E->P;
	pending_t *pd = &E->pend;
	const uint32_t pbid = b->bq[slot];
	pd->rd_id = pbid;
	const uint32_t nbest = nbest_of(E, pbid);
	uint32_t bcov = E->rdcovs[pbid];
	if(bcov >= nbest) return;
	E->step.used_queries++; b->used_queries++;
	if(!b->want[slot]){ fprintf(stderr, " -- internal error: no candidate row for read %u --\n", pbid); DIE_NOW(); }
	cq_work_t *w = cq_take(E, b, slot);
	const double tq2 = now_s();
	cand_t *cand = w->cand; const uint32_t nc = w->nc;
	if(E->step.rows_all){       /* -G: the trimmed, sorted list persists as the reference's rdhits entry */
		for(uint32_t i = 0; i < nc; i++) E->rows[(size_t)pbid * E->stride + i] = cand[i].e;
		E->nrow[pbid] = nc;
	}
	if(P->dot_matrix){
		for(uint32_t i = 0; i < nc; i++){
			const uint32_t id2 = (uint32_t)(cand[i].e >> 32);
			if(cand[i].pidx == 0xFFFFFFFFu){ fprintf(stderr, " -- internal error: pair (%u,%u) missing from the batch plan --\n", pbid, id2); DIE_NOW(); }
			const wtz_pair_summary_t *S = &CPART_OF(b, cand[i].pidx)->sum[LOCAL_OF(b, cand[i].pidx)];
			if(!S->gate) continue;
			E->step.used_pairs++;
			pend_closed(pd, hx_pair_key(id2, pbid));
			int d1 = S->dm_qe - S->dm_qb, d2 = S->dm_te - S->dm_tb;
			uint32_t ol = (uint32_t)(d1 > d2 ? d1 : d2);
			/* -N: print_hits_wtzmo gets the (empty) seed list and drops the dot-matrix hits unprinted and uncounted (wtzmo.c:1175-1210, 1319) */
			if(E->do_align && S->dm_score >= P->min_score && S->dm_score >= (int)(P->min_id * ol)){
				hit_t H; memset(&H, 0, sizeof H);
				H.pb1 = pbid; H.pb2 = id2; H.dir2 = (uint32_t)S->dm_dir; H.score = S->dm_score;
				H.tb = S->dm_tb; H.te = S->dm_te; H.qb = S->dm_qb; H.qe = S->dm_qe; H.mat = S->dm_score; H.aln = (int)ol;
				pend_hit(pd, &H);
				emit_record(E, &H, NULL, 0, -1);
			}
		}
		E->step.t_cq[2] += now_s() - tq2;
		return;
	}
	E->step.used_pairs += w->ngate;
	seed_t *seeds = w->seeds; const uint32_t nseed = w->nseed;
	if(!E->do_align){
		if(pd->capseed < nseed){ pd->capseed = nseed; pd->seeds = (seed_t*)hx_realloc(pd->seeds, sizeof(seed_t) * nseed); }
		memcpy(pd->seeds, seeds, sizeof(seed_t) * nseed); pd->nseed = nseed;
	} else {
		uint32_t ncand = P->ncand;
		for(uint32_t i = 0; i < nseed && i < ncand; i++){      /* the alignment results the loop below reads */
			const part_t *pt = CPART_OF(b, seeds[i].pidx); const uint32_t item = pt->item_of[LOCAL_OF(b, seeds[i].pidx)];
			if(item != 0xFFFFFFFFu) __builtin_prefetch(&pt->aln[item], 0, 1);
		}
		for(uint32_t i = 0; i < nseed && i < ncand; i++){
			seed_t *s = &seeds[i];
			if(s->closed){ ncand++; continue; }
			pend_closed(pd, hx_pair_key(s->pb2, pbid));
			const part_t *pt = CPART_OF(b, s->pidx);
			const uint32_t item = pt->item_of[LOCAL_OF(b, s->pidx)];
			if(item == 0xFFFFFFFFu || pt->it_dir[item] != s->dir){ fprintf(stderr, " -- internal error: alignment of (%u,%u) missing from the batch plan --\n", pbid, s->pb2); DIE_NOW(); }
			E->step.used_items++;
			const wtz_aln_result_t *x = &pt->aln[item];
			if(x->n_regs == 0){ s->closed = 1; ncand++; continue; }
			if(x->score < P->min_score || x->mat < x->aln * P->min_id) continue;
			hit_t H; memset(&H, 0, sizeof H);
			H.pb1 = pbid; H.pb2 = s->pb2; H.dir2 = s->dir; H.score = x->score;
			H.tb = x->tb; H.te = x->te; H.qb = x->qb; H.qe = x->qe; H.mat = x->mat; H.mis = x->mis; H.ins = x->ins; H.del = x->del; H.aln = x->aln;
			pend_hit(pd, &H);
			if(E->binary_out) emit_record(E, &H, NULL, 0, -1); else emit_record(E, &H, pt->cig + x->text_off, x->text_len, pt->cig_ext);
			{   /* dovetail / containment bookkeeping (wtzmo.c:1065-1100) */
				const uint32_t len1 = E->rdlen[H.pb1], len2 = E->rdlen[H.pb2];
				uint32_t x1 = (uint32_t)(H.tb < H.qb ? H.tb : H.qb);
				int r1 = (int)len1 - H.te, r2 = (int)len2 - H.qe;
				uint32_t x2 = (uint32_t)(r1 < r2 ? r1 : r2);
				if(x1 + x2 <= 200u){
					uint32_t x3 = ((H.tb == 0 && H.qb) || (H.te == (int)len1 && H.qe < (int)len2));
					uint32_t x4 = ((H.qb == 0 && H.tb) || (H.qe == (int)len2 && H.te < (int)len1));
					x1 = len2 + (uint32_t)H.qb - (uint32_t)H.qe;
					x2 = len1 + (uint32_t)H.tb - (uint32_t)H.te;
					if(x1 <= 0u && x3 == 0){               /* max_unalign_in_contained = 0, wtzmo.c:174 */
						if(x2 <= 0u && x4 == 0){
							if(len1 > len2){ pend_mask(pd, H.pb2); }
							else if(len1 < len2){ pend_mask(pd, H.pb1); break; }
							else if(H.pb2 > H.pb1){ pend_mask(pd, H.pb2); continue; }
							else { pend_mask(pd, H.pb1); break; }
						} else { pend_mask(pd, H.pb2); continue; }
						ncand++;
					} else if(x2 <= 0u && x4 == 0){ pend_mask(pd, H.pb1); break; }
					bcov++;
					if(bcov >= nbest) break;
				}
			}
		}
	}
	E->step.t_cq[2] += now_s() - tq2;
}
