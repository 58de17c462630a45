/* wtzmo host driver, section 4 of 6: the pairs of a range and the device stages of one part */
/* under E->mu: pairs of slots [s0,s1) whose candidate pair is not closed right now */
static void plan_pairs(eng_t *E, batch_t *b, uint32_t s0, uint32_t s1){
	const double tp0 = now_s();
	b->npair = 0;
	for(uint32_t d = 0; d < b->nparts; d++) b->parts[d].npair = 0;
	if((size_t)b->nbq * E->stride > b->caprowpair){ b->caprowpair = (size_t)b->nbq * E->stride; b->rowpair = (uint32_t*)hx_realloc(b->rowpair, b->caprowpair * 4); }
	uint64_t rows_seen = 0;
	for(uint32_t s = s0; s < s1; s++){
		const uint32_t q = b->bq[s];
		rows_seen += b->want[s] ? b->nrow[s] : 0;              /* what range_end counted */
		if(!b->want[s] || E->masked[q] || E->rdcovs[q] >= nbest_of(E, q)) continue;
		for(uint32_t k = 0; k < b->nrow[s]; k++){
			const uint64_t e = b->rows[(size_t)s * E->stride + k];
			const uint32_t id2 = (uint32_t)(e >> 32);
			b->rowpair[(size_t)s * E->stride + k] = 0xFFFFFFFFu;
			if((uint32_t)e == 0 || id2 == 0xFFFFFFFFu) continue;
			if(hx_set_has(&E->closed, hx_pair_key(q, id2))) continue;
			const uint32_t dpart = DEAL_PART(b->nparts, q, id2);
			part_t *pt = &b->parts[dpart];
			if(pt->npair == pt->cappair){ pt->cappair = pt->cappair ? pt->cappair * 2 : 4096; pt->pq = (uint32_t*)hx_realloc(pt->pq, pt->cappair * 4); pt->pc = (uint32_t*)hx_realloc(pt->pc, pt->cappair * 4); }
			if(pt->npair >= (1u << 28)){ fprintf(stderr, " -- more than 2^28 pairs of one range on one device --\n"); DIE_NOW(); }
			pt->pq[pt->npair] = q; pt->pc[pt->npair] = id2; pt->npair++;
			b->rowpair[(size_t)s * E->stride + k] = PIDX(dpart, pt->npair - 1); b->npair++;
		}
	}
	if(rows_seen >= 256){      /* the share of the rows that became pairs: follows the ranges down by a tenth per range at most, up at once */
		const double r = (double)b->npair / (double)rows_seen, keep = E->step.pair_row_ratio * 0.9;
		E->step.pair_row_ratio = r > keep ? r : keep;
	}
	E->step.t_cq[3] += now_s() - tp0;
}

/* the alignment items of a part: the best strand of every pair whose chain passes -r (wtzmo.c:913-914); a pure function of the summaries */
static void part_plan_items(eng_t *E, part_t *b){
	const wtz_params_c *P = &E->P;
	b->item_of = (uint32_t*)hx_realloc(b->item_of, 4 * ((size_t)b->npair + 1));
	b->it_pair = (uint32_t*)hx_realloc(b->it_pair, 4 * ((size_t)b->npair + 1));
	b->it_dir = (uint8_t*)hx_realloc(b->it_dir, (size_t)b->npair + 1);
	b->nitem = 0;
	for(uint32_t i = 0; i < b->npair; i++){
		b->item_of[i] = 0xFFFFFFFFu;
		if(!E->do_align || !b->sum[i].gate) continue;
		const uint32_t dir = (b->sum[i].ovl[0] < b->sum[i].ovl[1]);
		if(b->sum[i].ovl[dir] < P->ztot) continue;
		b->item_of[i] = b->nitem; b->it_pair[b->nitem] = i; b->it_dir[b->nitem] = (uint8_t)dir; b->nitem++;
	}
}
/* the page-locked CIGAR text buffer of the part for this range (two alternate: the records of the previous range may still be
 * waiting for the writer thread inside the other one); 0 = cannot allocate */
static int part_text_buffer(part_t *b, uint64_t tot){
	const int sel = (b->cig_sel ^= 1);
	b->cig_ext = b->ext_base >= 0 ? b->ext_base + sel : -1;
	{ const double tw0 = now_s(); out_wait_ext(b->cig_ext); b->t_io0 += now_s() - tw0; }
	if(tot > b->capcigs[sel]){
		uint64_t cap = b->capcigs[sel] ? b->capcigs[sel] : ((uint64_t)16 << 20); while(cap < tot) cap += cap / 2;
		wtz_host_free(b->cigs[sel]); b->cigs[sel] = (char*)wtz_host_alloc(cap + 1); b->capcigs[sel] = cap;
		if(!b->cigs[sel]){ fprintf(stderr, "[wtzmo-mi355x] cannot allocate %llu bytes of page-locked memory for the CIGAR text\n", (unsigned long long)cap); return 0; }
	}
	b->cig = b->cigs[sel];
	return 1;
}
/* the CIGAR text of the part's last range is on its way to the host (wtz_fetch_cigar_text_begin): wait for it */
static void part_text_wait(part_t *pt, double *t_acc){
	if(!pt->text_pending || pt->ctx == NULL) return;
	const double t0 = now_s();
	const int rc = wtz_fetch_cigar_text_end(pt->ctx);
	if(t_acc) *t_acc += now_s() - t0;
	pt->text_pending = 0;
	if(rc != WTZ_OK){ fprintf(stderr, " -- wtz_fetch_cigar_text_end failed: %s --\n", wtz_last_error()); DIE_NOW(); }
}
/* no lock held: the speculative device stages of ONE part's pairs on its context. 1 = scratch pool too small, nothing changed */
static int part_stages(eng_t *E, part_t *b){
	const wtz_params_c *P = &E->P;
	int rc;
	b->nitem = 0; b->ncig = 0;
	if(b->npair == 0) return 0;
	b->sum = (wtz_pair_summary_t*)hx_realloc(b->sum, sizeof(wtz_pair_summary_t) * (b->npair + 1));
	{ const double tc0 = now_s(); rc = wtz_pairs_seed(b->ctx, b->pq, b->pc, b->npair, b->sum); b->t_call[1] += now_s() - tc0; } TRY_WTZ(rc, "wtz_pairs_seed");
	if(!P->dot_matrix){
		b->box_off = (uint64_t*)hx_realloc(b->box_off, 8 * ((size_t)b->npair * 2 + 1));
		uint64_t nb = 0;
		for(uint32_t i = 0; i < b->npair; i++) for(int d = 0; d < 2; d++){ b->box_off[(size_t)i * 2 + d] = nb; nb += b->sum[i].nwin[d]; }
		b->box_off[(size_t)b->npair * 2] = nb; b->nbox = nb;
		if(nb > b->capbox){ b->capbox = nb; b->boxes = (wtz_winbox_t*)hx_realloc(b->boxes, sizeof(wtz_winbox_t) * nb); }
		{ const double tc0 = now_s(); rc = wtz_pairs_windows(b->ctx, b->boxes, nb); b->t_call[2] += now_s() - tc0; } TRY_WTZ(rc, "wtz_pairs_windows");
		part_plan_items(E, b);
		if(b->nitem){
			b->aln = (wtz_aln_result_t*)hx_realloc(b->aln, sizeof(wtz_aln_result_t) * b->nitem);
			{ const double tc0 = now_s(); rc = wtz_pairs_align(b->ctx, b->it_pair, b->it_dir, b->nitem, b->aln); b->t_call[3] += now_s() - tc0; } TRY_WTZ(rc, "wtz_pairs_align");
			uint64_t tot = 0; for(uint32_t i = 0; i < b->nitem; i++) tot += b->aln[i].text_len;
			if(E->binary_out) tot = 0;              /* binary records carry no CIGAR column (what `cut -f1-16` drops in the zmo pipeline): 3 GB per configs[2] step stay on the device */
			else if(g_dist.rank > 0 && g_dist.send_dev){      /* this rank only forwards the text: it never leaves the device on this side */
				const double tc0 = now_s(); b->cig_dev = NULL; rc = wtz_cigar_text_device(b->ctx, tot, &b->cig_dev); b->t_call[4] += now_s() - tc0; TRY_WTZ(rc, "wtz_cigar_text_device");
			} else {
				if(!part_text_buffer(b, tot)) return WTZ_ST_AGAIN;
				if(g_dist.world == 1){      /* the copy runs beside what the context does next: part_text_wait() before anybody reads the text */
					const double tc0 = now_s(); rc = wtz_fetch_cigar_text_begin(b->ctx, b->cig, tot); b->t_call[4] += now_s() - tc0; TRY_WTZ(rc, "wtz_fetch_cigar_text_begin"); b->text_pending = 1;
				} else
				{ const double tc0 = now_s(); rc = wtz_fetch_cigar_text(b->ctx, b->cig, tot); b->t_call[4] += now_s() - tc0; } TRY_WTZ(rc, "wtz_fetch_cigar_text");     /* rendered on the device */
			}
			b->ncig = tot;
		}
	}
	return 0;
}

static void *part_main(void *arg){ part_t *pt = (part_t*)arg; pt->again = part_stages(pt->E, pt); return NULL; }
/* the z-mer index of a batch on one context: `cl` (zbatch) = the candidate-side reads of this device for the batch, `ql` (several parts) = the batch's queries */
static int zbuild_part(wtz_ctx_t *ctx, int have_c, const uint32_t *cl, uint32_t ncl, int have_q, const uint32_t *ql, uint32_t nql){
	int rc = WTZ_OK;
	if(have_c) rc = wtz_zindex_build_subset(ctx, cl, ncl);
	if(rc == WTZ_OK && have_q) rc = wtz_zindex_build_queries(ctx, ql, nql);
	return rc;
}
