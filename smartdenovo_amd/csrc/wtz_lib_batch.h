/*
 * wtz_lib_batch.h — the DP routines as batch services for callers that hold their own problems: wtz_extend_batch (K-sw3), wtz_local_batch (K-local)
 * and, through wtz_testdp.h, the test-only wtz_test_dp.  Included by wtz_lib.cpp.
 */
/* the two sides of problem i as views of the uploaded reads (h_off: the reads' offsets, fetched by the caller), or WTZ_E_ARG.  allow_empty: a side of
 * length 0 is a problem like any other (its start is not looked at); max_len > 0: the longest side the caller's kernel takes */
static int dp_problem_views(const wtz_ctx *c, const std::vector<uint64_t> &h_off, const wtz_dp_problem_t &p, uint32_t i, bool allow_empty, int32_t max_len, wtz_seq_packed *q, wtz_seq_packed *t){
	if(p.q_read >= c->n_reads || p.t_read >= c->n_reads) return wtz_fail(WTZ_E_ARG, "problem %u: read id out of range", i);
	if((p.q_strand != 1 && p.q_strand != -1) || (p.t_strand != 1 && p.t_strand != -1)) return wtz_fail(WTZ_E_ARG, "problem %u: strand must be +1 or -1", i);
	if(!allow_empty && (p.q_len < 1 || p.t_len < 1)) return wtz_fail(WTZ_E_ARG, "problem %u: empty sequence", i);
	if(max_len > 0 && (p.q_len > max_len || p.t_len > max_len)) return wtz_fail(WTZ_E_ARG, "problem %u: %d x %d is beyond the %d x %d of one wavefront", i, p.t_len, p.q_len, max_len, max_len);
	wtz_readview vq, vt;
	vq.bits = c->bits; vq.off = h_off[p.q_read]; vq.len = c->h_rdlen[p.q_read]; vq.rev = p.q_rev ? 1u : 0u;
	vt.bits = c->bits; vt.off = h_off[p.t_read]; vt.len = c->h_rdlen[p.t_read]; vt.rev = p.t_rev ? 1u : 0u;
	const int64_t qlast = (int64_t)p.q_from + (int64_t)p.q_strand * (p.q_len > 0 ? p.q_len - 1 : 0), tlast = (int64_t)p.t_from + (int64_t)p.t_strand * (p.t_len > 0 ? p.t_len - 1 : 0);
	if(p.q_len < 0 || p.t_len < 0 || (p.q_len > 0 && (p.q_from < 0 || p.q_from >= (int64_t)vq.len || qlast < 0 || qlast >= (int64_t)vq.len))
			|| (p.t_len > 0 && (p.t_from < 0 || p.t_from >= (int64_t)vt.len || tlast < 0 || tlast >= (int64_t)vt.len)))
		return wtz_fail(WTZ_E_ARG, "problem %u: region outside its read", i);
	*q = vq.sub(p.q_from, p.q_strand); *t = vt.sub(p.t_from, p.t_strand);
	return WTZ_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* f2: end extensions for a caller that holds its own overlaps (wtext)                                */
/* ------------------------------------------------------------------------------------------------ */
/* kswx_extend_align (kswx.h:469-481) = kswx_extend_align_shift_core (kswx.h:101-232) for n independent problems on views of the uploaded reads: the SAME job
 * dispatch as the ends of wtzmo's stitched alignments (run_extjobs: register DP on one wavefront per job, LDS-ring and scalar forms for what is
 * outside their envelope).  out[i]: the kswx_t of the call + where its CIGAR words (traceback order reversed: first operation first) start in `cigar`. */
extern "C" int wtz_extend_batch(wtz_ctx_t *c, const wtz_dp_problem_t *pr, uint32_t n, wtz_dp_result_t *out, uint32_t *cigar, uint64_t cigar_cap){
	if(!c || !c->bits) return wtz_fail(WTZ_E_ARG, "reads not uploaded");
	if(n == 0) return WTZ_OK;
	if(!pr || !out || (!cigar && cigar_cap)) return wtz_fail(WTZ_E_ARG, "null argument");
	CTX_ENTER(c);
	CHK(pool_reset(c));
	std::vector<uint64_t> h_off(c->n_reads);
	CHK(dev_d2h(h_off.data(), c->rdoff, (size_t)c->n_reads * 8));
	std::vector<wtz_extjob_t> jobs(n);
	for(uint32_t i = 0; i < n; i++){
		const wtz_dp_problem_t &p = pr[i];
		wtz_extjob_t j; memset(&j, 0, sizeof j);
		CHK(dp_problem_views(c, h_off, p, i, true, 0, &j.q, &j.t));
		j.qlen = p.q_len; j.tlen = p.t_len; j.init_score = p.init_score; j.W = p.W; j.item = i; j.valid = 1;
		jobs[i] = j;
	}
	const wtz_env_t V = ctx_env(c);
	wtz_extjob_t *d_jobs = NULL; CHK(dev_alloc((void**)&d_jobs, (size_t)n * sizeof(wtz_extjob_t))); CHK(dev_h2d(d_jobs, jobs.data(), (size_t)n * sizeof(wtz_extjob_t)));
	wtz_timer tm; tm.start();
	CHK(run_extjobs(c, V, d_jobs, n));
	CHK(dev_sync());
	c->cnt.ms_stitch += tm.stop();
	CHK(tpool_check(c, "wtz_extend_batch"));
	CHK(dev_d2h(jobs.data(), d_jobs, (size_t)n * sizeof(wtz_extjob_t)));
	std::vector<uint64_t> off((size_t)n + 1); uint64_t tot = 0;
	for(uint32_t i = 0; i < n; i++){
		if(jobs[i].bad) return wtz_fail(WTZ_E_POOL, "wtz_extend_batch: problem %u ran out of scratch", i);
		const bool empty = jobs[i].qlen <= 0 || jobs[i].tlen <= 0;
		off[i] = tot; tot += empty ? 0 : jobs[i].cigar_len;
		c->cnt.cells_shift += jobs[i].cells;
	}
	off[n] = tot;
	if(tot > cigar_cap) return wtz_fail(WTZ_E_ARG, "wtz_extend_batch: CIGAR buffer too small (%llu words needed)", (unsigned long long)tot);
	if(tot){
		uint64_t *d_off = NULL; uint32_t *d_flat = NULL;
		CHK(dev_alloc((void**)&d_off, ((size_t)n + 1) * 8)); CHK(dev_h2d(d_off, off.data(), ((size_t)n + 1) * 8));
		CHK(dev_alloc((void**)&d_flat, (size_t)tot * 4));
		CHK(wtz_launch<K_extcopy>(n, [=] WTZ_LAMBDA (uint64_t t){ const uint64_t o = d_off[t], e = d_off[t + 1]; const uint32_t *src = d_jobs[t].cigar; for(uint64_t k = o; k < e; k++) d_flat[k] = src[k - o]; }));
		CHK(dev_sync());
		CHK(dev_d2h(cigar, d_flat, (size_t)tot * 4));
	}
	for(uint32_t i = 0; i < n; i++){
		wtz_dp_result_t o; memset(&o, 0, sizeof o);
		const wtz_extjob_t &j = jobs[i];
		const bool empty = j.qlen <= 0 || j.tlen <= 0;
		if(empty){ o.score = j.init_score < 0 ? 0 : j.init_score; }      /* kswx.h:113-118: an empty side returns the (clamped) start score and no operations */
		else { o.score = j.x.score; o.tb = j.x.tb; o.te = j.x.te; o.qb = j.x.qb; o.qe = j.x.qe; o.aln = j.x.aln; o.mat = j.x.mat; o.mis = j.x.mis; o.ins = j.x.ins; o.del = j.x.del; o.cigar_len = j.cigar_len; }
		o.cigar_off = off[i]; o.cells = j.cells; o.form_used = j.done ? j.done : 3;
		out[i] = o;
	}
	CHK(pool_check(c, "wtz_extend_batch"));
	return WTZ_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* local Smith-Waterman with start coordinates (the routine wtcyc, pairaln and wtcns start from)      */
/* ------------------------------------------------------------------------------------------------ */
/* ksw_align2(..., KSW_XSTART) with 16-bit lanes (ksw.c:344-366 over ksw_i16, ksw.c:233-335) for n independent problems on views of the uploaded reads:
 * K-local (wtz_sw_local.h), one wavefront per problem, both passes on the same wavefront, largest problem first.  The strip-boundary column of a
 * problem (two buffers of t_len words, only for queries of more than one strip) is planned on the host and taken from the main pool in one block. */
extern "C" int wtz_local_batch(wtz_ctx_t *c, const wtz_dp_problem_t *pr, uint32_t n, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, wtz_local_result_t *out){
	if(!c || !c->bits) return wtz_fail(WTZ_E_ARG, "reads not uploaded");
	if(n == 0) return WTZ_OK;
	if(!pr || !out) return wtz_fail(WTZ_E_ARG, "null argument");
	if(n > 0x7FFFFFFFu) return wtz_fail(WTZ_E_ARG, "wtz_local_batch: more than 2^31 - 1 problems in one call");      /* one block per problem */
	/* the value range of the 16-bit routine: scores as the reference's int8 matrix holds them (kswx.h:1495-1520 fills it from M / X), gap costs >= 0 (ksw.c:253-256) */
	if(c->P.M < 1 || c->P.M > 127 || c->P.X > 0 || c->P.X < -128) return wtz_fail(WTZ_E_ARG, "wtz_local_batch: M must be in [1, 127] and X in [-128, 0]");
	if(o_del < 0 || e_del < 0 || o_ins < 0 || e_ins < 0 || (int64_t)o_del + e_del > 32767 || (int64_t)o_ins + e_ins > 32767) return wtz_fail(WTZ_E_ARG, "wtz_local_batch: gap costs must be >= 0 and open + extend <= 32767");
	CTX_ENTER(c);
	CHK(pool_reset(c));
	std::vector<uint64_t> h_off(c->n_reads);
	CHK(dev_d2h(h_off.data(), c->rdoff, (size_t)c->n_reads * 8));
	std::vector<wtz_locprob_t> hp(n);
	unsigned long long bnd_words = 0;
	for(uint32_t i = 0; i < n; i++){
		const wtz_dp_problem_t &p = pr[i];
		wtz_locprob_t d; CHK(dp_problem_views(c, h_off, p, i, false, WTZ_LOC_MAXLEN, &d.q, &d.t)); d.qlen = p.q_len; d.tlen = p.t_len; d.bnd_off = bnd_words;
		if(p.q_len > wtz_loc_strip_cols(p.q_len)) bnd_words += 2ull * (unsigned long long)p.t_len;      /* more than one strip: on the device, more than 1 024 columns */
		hp[i] = d;
	}
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b){ return (uint64_t)hp[a].qlen * (uint64_t)hp[a].tlen > (uint64_t)hp[b].qlen * (uint64_t)hp[b].tlen; });
	wtz_locprob_t *d_pr = NULL; uint32_t *d_order = NULL; wtz_locres_t *d_res = NULL; uint32_t *d_bnd = NULL;
	CHK(dev_alloc((void**)&d_pr, (size_t)n * sizeof(wtz_locprob_t))); CHK(dev_h2d(d_pr, hp.data(), (size_t)n * sizeof(wtz_locprob_t)));
	CHK(dev_alloc((void**)&d_order, (size_t)n * 4)); CHK(dev_h2d(d_order, order.data(), (size_t)n * 4));
	CHK(dev_alloc((void**)&d_res, (size_t)n * sizeof(wtz_locres_t))); CHK(dev_set(d_res, 0, (size_t)n * sizeof(wtz_locres_t)));
	if(bnd_words){
		if(bnd_words * 4ull > c->main_bytes){ c->last_pool_fail = 1; return wtz_fail(WTZ_E_POOL, "wtz_local_batch: %llu bytes of strip boundaries in a main pool of %llu; use fewer problems per call or a larger pool", bnd_words * 4ull, (unsigned long long)c->main_bytes); }
		if(pool_alloc_host(c, 0, (size_t)bnd_words * 4, (void**)&d_bnd) != WTZ_OK){      /* the pool's own rounding on top of a request that just fitted */
			c->last_pool_fail = 1;
			return wtz_fail(WTZ_E_POOL, "wtz_local_batch: no room for %llu bytes of strip boundaries in the main pool; use fewer problems per call or a larger pool", bnd_words * 4ull);
		}
	}
	wtz_locsc_t S; S.M = c->P.M; S.X = c->P.X; S.oe_del = o_del + e_del; S.e_del = e_del; S.oe_ins = o_ins + e_ins; S.e_ins = e_ins;
	wtz_timer tm; tm.start();
#ifndef WTZ_EMUL
	WTZ_LAUNCH(wtz_kernel_local, n, 64, 0, g_stream, (const wtz_locprob_t*)d_pr, (const uint32_t*)d_order, n, S, d_bnd, d_res);
#else
	for(uint32_t b = 0; b < n; b++){ const uint32_t id = d_order[b]; wtz_local_problem(d_pr[id], S, d_bnd, d_res[id]); }
#endif
	CHK(dev_sync());
	c->cnt.ms_local += tm.stop();
	std::vector<wtz_locres_t> hr(n);
	CHK(dev_d2h(hr.data(), d_res, (size_t)n * sizeof(wtz_locres_t)));
	for(uint32_t i = 0; i < n; i++){
		wtz_local_result_t o; memset(&o, 0, sizeof o);
		o.score = hr[i].score; o.te = hr[i].te; o.qe = hr[i].qe; o.tb = hr[i].tb; o.qb = hr[i].qb; o.form_used = hr[i].form; o.cells = hr[i].cells;
		c->cnt.cells_local += hr[i].cells;
		out[i] = o;
	}
	c->cnt.n_local += n;
	CHK(pool_check(c, "wtz_local_batch"));
	/* nothing of the call lives on: the main pool goes back empty (wtz_pool_info shows main_used = 0; the bytes taken are in counters.pool_peak) */
	CHK(pool_reset(c));
	c->main_used_call = 0;
	return WTZ_OK;
}

#include "wtz_testdp.h"
