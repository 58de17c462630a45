/*
 * wtz_lib_hzmaux.h — align_hzmaux with beg / end (hzm_aln.h:1684-1775) as a batch service: wtz_hzmaux_batch, the pair stages in aux form behind one call.
 * Included by wtz_lib_batch.h.
 */
/* the gates behind the stitched alignment (hzm_aln.h:1715-1718) in the reference's float arithmetic, as gbo_hit_passes (host/wtgbo_core.h) applies them for wtgbo */
static bool hzmaux_gates(const wtz_aln_result_t &a, int32_t tlen, int32_t qlen, float min_sm){
	int32_t beg = a.qb - a.tb; if(beg < 0) beg = 0;
	int32_t end = a.qe + tlen - a.te; if(end > qlen) end = qlen;
	const int32_t ovl = end - beg;
	return !(a.score < 0 || (float)a.mat < (float)a.aln * min_sm || (float)a.mat < (float)ovl * min_sm);
}

/* the device stages of wtz_hzmaux_batch: itp = the pairs that went on to the alignment (hzm_aln.h:1698-1699: windows, and a chain of at least zovl), aln = their
 * results, words = their CIGARs in that order */
static int hzmaux_stages(wtz_ctx_t *c, const uint32_t *tid, const uint32_t *rid, const int32_t *beg, const int32_t *end, uint32_t n,
		std::vector<uint32_t> &itp, std::vector<wtz_aln_result_t> &aln, std::vector<uint32_t> &words){
	std::vector<wtz_pair_summary_t> sum(n);
	CHK(wtz_pairs_seed_region(c, tid, rid, beg, end, n, sum.data()));      /* starts the batch like wtz_batch_begin: the results of the one before are dropped, the pools go back empty */
	for(uint32_t i = 0; i < n; i++) if(sum[i].gate && sum[i].nwin[0]) itp.push_back(i);
	const uint32_t m = (uint32_t)itp.size();
	if(m == 0) return WTZ_OK;
	const std::vector<uint8_t> itd(m, 0);
	aln.resize(m);
	CHK(wtz_pairs_align(c, itp.data(), itd.data(), m, aln.data()));
	uint64_t tot = 0; for(uint32_t k = 0; k < m; k++) tot += aln[k].cigar_len;
	words.resize((size_t)tot + 1);
	return wtz_fetch_cigars(c, words.data(), tot);
}

/* align_hzmaux(aux, rid, rdseq, NULL, rdlen, beg, end, refine, min_sm) for n (target read, query read) pairs, the target's index being what ready_hzmaux
 * (hzm_aln.h:1676-1678) builds: wtz_batch_begin, wtz_pairs_seed_region (hzm_aln.h:1690-1699), wtz_pairs_align of the pairs with windows and a chain
 * (hzm_aln.h:1700-1714, with params.refine also 1721-1729), the gates of hzm_aln.h:1715-1718 and the CIGARs of the hits, packed in pair order.  Nothing of the
 * call lives on: the main pool goes back empty and there is no batch for wtz_pairs_windows / wtz_pairs_align to continue. */
extern "C" int wtz_hzmaux_batch(wtz_ctx_t *c, const uint32_t *tid, const uint32_t *rid, const int32_t *beg, const int32_t *end, uint32_t n,
		wtz_hzmaux_result_t *out, uint32_t *cigar, uint64_t cigar_cap){
	BATCH_ARGS(c, n, tid && rid && beg && end && out && (cigar || !cigar_cap), "wtz_hzmaux_batch", "pairs");
	CHK(region_args(c, "wtz_hzmaux_batch"));
	if(!c->zs[0].have) return wtz_fail(WTZ_E_STATE, "wtz_hzmaux_batch before wtz_zindex_build / wtz_zindex_build_subset");
	const wtz_ctx::zslot_t &zt = c->zs[1].have ? c->zs[1] : c->zs[0];      /* where the pair stages read the indexed side from (ctx_env) */
	for(uint32_t i = 0; i < n; i++){
		if(tid[i] >= c->n_reads || rid[i] >= c->n_reads) return wtz_fail(WTZ_E_ARG, "pair %u: read id out of range", i);
		if(!zt.holds(tid[i])) return wtz_fail(WTZ_E_STATE, "wtz_hzmaux_batch: pair %u: target read %u is not in the z-index", i, tid[i]);
		if(!c->zs[0].holds(rid[i])) return wtz_fail(WTZ_E_STATE, "wtz_hzmaux_batch: pair %u: query read %u is not in the z-index (its z-mers are read from there)", i, rid[i]);
	}
	CTX_ENTER(c);
	std::vector<uint32_t> itp; std::vector<wtz_aln_result_t> aln; std::vector<uint32_t> words;
	const int rc = hzmaux_stages(c, tid, rid, beg, end, n, itp, aln, words);
	if(rc != WTZ_OK){      /* WTZ_E_POOL above all: nothing was returned and nothing stays - no batch to continue, an empty main pool; the error and its text are the stage's */
		free_batch(c);
		(void)batch_leave(c);
		return rc;
	}
	const uint32_t m = (uint32_t)itp.size();
	memset(out, 0, (size_t)n * sizeof(wtz_hzmaux_result_t));
	uint64_t src = 0, dst = 0;
	for(uint32_t k = 0; k < m; k++){
		const wtz_aln_result_t &a = aln[k]; const uint32_t i = itp[k];
		/* hzm_aln.h:1712, then 1715-1718: with params.refine the device applied them in front of the refinement (wtz_task_refine) and says so through n_regs */
		const bool hit = a.n_regs > 0 && (c->P.refine || hzmaux_gates(a, (int32_t)c->h_rdlen[tid[i]], (int32_t)c->h_rdlen[rid[i]], c->P.min_id));
		if(hit){
			wtz_hzmaux_result_t o; memset(&o, 0, sizeof o);
			o.found = 1; o.score = a.score; o.tb = a.tb; o.te = a.te; o.qb = a.qb; o.qe = a.qe; o.aln = a.aln; o.mat = a.mat; o.mis = a.mis; o.ins = a.ins; o.del = a.del;
			o.cigar_len = a.cigar_len; o.cigar_off = dst;
			if(cigar && dst + a.cigar_len <= cigar_cap) memcpy(cigar + dst, words.data() + src, (size_t)a.cigar_len * 4);
			dst += a.cigar_len;
			out[i] = o;
		}
		src += a.cigar_len;
	}
	free_batch(c);
	CHK(batch_leave(c));
	if(cigar && dst > cigar_cap) return wtz_fail(WTZ_E_ARG, "wtz_hzmaux_batch: CIGAR buffer too small (%llu words needed)", (unsigned long long)dst);
	return WTZ_OK;
}
