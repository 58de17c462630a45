/*
 * wtz_lib_batch.h — the DP routines as batch services for callers that hold their own problems: wtz_extend_batch (K-sw3), wtz_local_batch (K-local),
 * wtz_kext_batch (K-kext), wtz_align_batch (K-local + K-kext), through wtz_lib_glob.h wtz_global_batch (K-glob) and wtz_alignx_batch (all three), through
 * wtz_lib_pwtext.h wtz_pwtext_batch (K-pwtext), through wtz_lib_hzmaux.h wtz_hzmaux_batch (the pair stages behind one call) and, through wtz_testdp.h, the test-only
 * wtz_test_dp.  Included by wtz_lib.cpp.
 *
 * The skeleton they are written against stands first, each step once: BATCH_ARGS / batch_count / batch_begin (a call before it looks at a problem), batch_scores,
 * batch_order, batch_upload / batch_fetch (the two ends of a launch group), form_dispatch / for_each_form, pack_runs, pool_fail, batch_leave.
 */
/* WTZ_E_POOL from a request the host planned itself; kind as wtz_pool_failure_kind reports it (1 = main pool) */
static int pool_fail(wtz_ctx *c, int kind, const char *fmt, ...){
	va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
	c->last_pool_fail = kind; return WTZ_E_POOL;
}
/* nothing of a call lives on: the main pool goes back empty (wtz_pool_info shows main_used = 0; the bytes taken are in counters.pool_peak) */
static int batch_leave(wtz_ctx *c){ CHK(pool_reset(c)); c->main_used_call = 0; return WTZ_OK; }
/* one block per item */
static int batch_count(uint32_t n, const char *who, const char *items){ return n > 0x7FFFFFFFu ? wtz_fail(WTZ_E_ARG, "%s: more than 2^31 - 1 %s in one call", who, items) : WTZ_OK; }
/* the checks every entry point starts with, in the order a caller sees them; n == 0 is WTZ_OK whatever the other arguments are (BATCH_ARGS returns on it too).
 * args_ok: no argument of the call is a null pointer that must not be one; who: NULL for the entry points without a limit on n */
#define BATCH_ARGS(c, n, args_ok, who, items) do { const int rc_ = batch_args(c, n, args_ok, who, items); if(rc_ != WTZ_OK || (n) == 0) return rc_; } while(0)
static int batch_args(const wtz_ctx *c, uint32_t n, bool args_ok, const char *who, const char *items){
	if(!c || !c->bits) return wtz_fail(WTZ_E_ARG, "reads not uploaded");
	if(n == 0) return WTZ_OK;
	if(!args_ok) return wtz_fail(WTZ_E_ARG, "null argument");
	return who ? batch_count(n, who, items) : WTZ_OK;
}
/* behind CTX_ENTER, once all arguments that are not problems are checked: empty pools and THE fetch of the reads' offsets of the call */
static int batch_begin(wtz_ctx *c, std::vector<uint64_t> &h_off){
	CHK(pool_reset(c)); h_off.resize(c->n_reads);
	return dev_d2h(h_off.data(), c->rdoff, (size_t)c->n_reads * 8);
}
/* the value range of the 16-bit routines, or WTZ_E_ARG: scores as the reference's int8 matrix holds them (kswx.h:1495-1520 fills it from M / X), gap opening costs >= 0
 * (ksw.c:253-256; an opening cost of 0 is a setting like any other), gap extension costs >= min_ext: 1 where the routine divides by them (ksw.c:403-406), else 0 */
static int batch_scores(const wtz_ctx *c, const char *who, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, int32_t min_ext){
	if(c->P.M < 1 || c->P.M > 127 || c->P.X > 0 || c->P.X < -128) return wtz_fail(WTZ_E_ARG, "%s: M must be in [1, 127] and X in [-128, 0]", who);
	if(o_del < 0 || o_ins < 0 || e_del < min_ext || e_ins < min_ext || (int64_t)o_del + e_del > 32767 || (int64_t)o_ins + e_ins > 32767)
		return wtz_fail(WTZ_E_ARG, min_ext ? "%s: gap opening costs must be >= 0, gap extension costs >= 1 and open + extend <= 32767" : "%s: gap costs must be >= 0 and open + extend <= 32767", who);
	return WTZ_OK;
}
/* the order of a launch: by form (NULL: one form), widest first, and inside a form by weight, largest first; equal problems keep their order */
static std::vector<uint32_t> batch_order(uint32_t n, const uint32_t *form, const std::vector<uint64_t> &weight){
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b){ if(form && form[a] != form[b]) return form[a] > form[b]; return weight[a] > weight[b]; });
	return order;
}
/* the problems, their order (d_order == NULL: none) and zeroed results on the device, from the arena scope of the caller */
template<typename P, typename R> static int batch_upload(const std::vector<P> &hp, const std::vector<uint32_t> &order, P **d_pr, uint32_t **d_order, R **d_res){
	const size_t n = hp.size();
	CHK(dev_alloc((void**)d_pr, n * sizeof(P))); CHK(dev_h2d(*d_pr, hp.data(), n * sizeof(P)));
	if(d_order){ CHK(dev_alloc((void**)d_order, n * 4)); CHK(dev_h2d(*d_order, order.data(), n * 4)); }
	CHK(dev_alloc((void**)d_res, n * sizeof(R))); CHK(dev_set(*d_res, 0, n * sizeof(R)));
	return WTZ_OK;
}
/* the end of a launch group that began with batch_upload and tm.start(): one synchronisation, the kernel time to ms, the results back into hr */
template<typename R> static int batch_fetch(wtz_timer &tm, double &ms, size_t n, const R *d_res, std::vector<R> &hr){
	CHK(dev_sync()); ms += tm.stop(); hr.resize(n);
	return dev_d2h(hr.data(), d_res, n * sizeof(R));
}
/* the run-time form (slots per lane: 1, 2, 4, 8, 16, 32) as a compile-time constant: f(std::integral_constant<int, C>()) */
template<typename F> static int form_dispatch(uint32_t C, F f){
	switch(C){
		case 1: return f(std::integral_constant<int, 1>());
		case 2: return f(std::integral_constant<int, 2>());
		case 4: return f(std::integral_constant<int, 4>());
		case 8: return f(std::integral_constant<int, 8>());
		case 16: return f(std::integral_constant<int, 16>());
		default: return f(std::integral_constant<int, 32>());
	}
}
/* one call per form present among the n problems form_of(0 .. n - 1) (sorted by form): f(form constant, b0, b1) for the stretch [b0, b1) */
template<typename FORM, typename F> static int for_each_form(uint32_t n, FORM form_of, F f){
	for(uint32_t b0 = 0, b1; b0 < n; b0 = b1){
		const uint32_t C = form_of(b0);
		for(b1 = b0 + 1; b1 < n && form_of(b1) == C; b1++){}
		CHK(form_dispatch(C, [&](auto K){ return f(K, b0, b1); }));
	}
	return WTZ_OK;
}
/* the run lists of off.size() - 1 problems (off[t]: the words in front of list t, off.back(): all; src(t): where list t lies on the device) packed on the device and fetched in one copy to dst[0, off.back()) */
template<typename TAG, typename SRC> static int pack_runs(const std::vector<uint64_t> &off, SRC src, uint32_t *dst){
	const size_t n = off.size() - 1; const uint64_t tot = off[n];
	if(tot == 0) return WTZ_OK;
	uint64_t *d_off = NULL; uint32_t *d_flat = NULL;
	CHK(dev_alloc((void**)&d_off, (n + 1) * 8)); CHK(dev_h2d(d_off, off.data(), (n + 1) * 8));
	CHK(dev_alloc((void**)&d_flat, (size_t)tot * 4));
	CHK(wtz_launch<TAG>(n, [=] WTZ_LAMBDA (uint64_t t){ const uint64_t o = d_off[t], e = d_off[t + 1]; const uint32_t *s = src(t); for(uint64_t k = o; k < e; k++) d_flat[k] = s[k - o]; }));
	CHK(dev_sync());
	return dev_d2h(dst, d_flat, (size_t)tot * 4);
}

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
	BATCH_ARGS(c, n, pr && out && (cigar || !cigar_cap), NULL, NULL);
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
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
	std::vector<uint64_t> off((size_t)n + 1, 0);
	for(uint32_t i = 0; i < n; i++){
		if(jobs[i].bad) return wtz_fail(WTZ_E_POOL, "wtz_extend_batch: problem %u ran out of scratch", i);      /* the kind stays what the call before left */
		off[i + 1] = off[i] + ((jobs[i].qlen <= 0 || jobs[i].tlen <= 0) ? 0 : jobs[i].cigar_len);
		c->cnt.cells_shift += jobs[i].cells;
	}
	const uint64_t tot = off[n];
	if(tot > cigar_cap) return wtz_fail(WTZ_E_ARG, "wtz_extend_batch: CIGAR buffer too small (%llu words needed)", (unsigned long long)tot);
	CHK(pack_runs<K_extcopy>(off, [=] WTZ_LAMBDA (uint64_t t) -> const uint32_t* { return d_jobs[t].cigar; }, cigar));
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
static int local_run(wtz_ctx *c, const std::vector<uint64_t> &h_off, const wtz_dp_problem_t *pr, uint32_t n, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, wtz_local_result_t *out){
	wtz_arena_scope launch_scope(&c->arena);      /* the buffers of the launch go back when it returns (scopes nest) */
	std::vector<wtz_locprob_t> hp(n); std::vector<uint64_t> area(n);
	unsigned long long bnd_words = 0;
	for(uint32_t i = 0; i < n; i++){
		const wtz_dp_problem_t &p = pr[i];
		wtz_locprob_t d; CHK(dp_problem_views(c, h_off, p, i, false, WTZ_LOC_MAXLEN, &d.q, &d.t)); d.qlen = p.q_len; d.tlen = p.t_len; d.bnd_off = bnd_words;
		if(p.q_len > wtz_loc_strip_cols(p.q_len)) bnd_words += 2ull * (unsigned long long)p.t_len;      /* more than one strip: on the device, more than 1 024 columns */
		hp[i] = d; area[i] = (uint64_t)p.q_len * (uint64_t)p.t_len;
	}
	wtz_locprob_t *d_pr = NULL; uint32_t *d_order = NULL; wtz_locres_t *d_res = NULL;
	CHK(batch_upload(hp, batch_order(n, NULL, area), &d_pr, &d_order, &d_res));
	uint32_t *d_bnd = NULL;
	if(bnd_words){
		if(bnd_words * 4ull > c->main_bytes) return pool_fail(c, 1, "wtz_local_batch: %llu bytes of strip boundaries in a main pool of %llu; use fewer problems per call or a larger pool", bnd_words * 4ull, (unsigned long long)c->main_bytes);
		if(pool_alloc_host(c, 0, (size_t)bnd_words * 4, (void**)&d_bnd) != WTZ_OK)      /* the pool's own rounding on top of a request that just fitted */
			return pool_fail(c, 1, "wtz_local_batch: no room for %llu bytes of strip boundaries in the main pool; use fewer problems per call or a larger pool", bnd_words * 4ull);
	}
	wtz_locsc_t S; S.M = c->P.M; S.X = c->P.X; S.oe_del = o_del + e_del; S.e_del = e_del; S.oe_ins = o_ins + e_ins; S.e_ins = e_ins;
	wtz_timer tm; tm.start();
#ifndef WTZ_EMUL
	WTZ_LAUNCH(wtz_kernel_local, n, 64, 0, g_stream, (const wtz_locprob_t*)d_pr, (const uint32_t*)d_order, n, S, d_bnd, d_res);
#else
	for(uint32_t b = 0; b < n; b++){ const uint32_t id = d_order[b]; wtz_local_problem(d_pr[id], S, d_bnd, d_res[id]); }
#endif
	std::vector<wtz_locres_t> hr;
	CHK(batch_fetch(tm, c->cnt.ms_local, n, d_res, hr));
	for(uint32_t i = 0; i < n; i++){
		wtz_local_result_t o; memset(&o, 0, sizeof o);
		o.score = hr[i].score; o.te = hr[i].te; o.qe = hr[i].qe; o.tb = hr[i].tb; o.qb = hr[i].qb; o.form_used = hr[i].form; o.cells = hr[i].cells;
		c->cnt.cells_local += hr[i].cells;
		out[i] = o;
	}
	c->cnt.n_local += n;
	CHK(pool_check(c, "wtz_local_batch"));
	return batch_leave(c);
}
extern "C" int wtz_local_batch(wtz_ctx_t *c, const wtz_dp_problem_t *pr, uint32_t n, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, wtz_local_result_t *out){
	BATCH_ARGS(c, n, pr && out, "wtz_local_batch", "problems");
	CHK(batch_scores(c, "wtz_local_batch", o_del, e_del, o_ins, e_ins, 0));
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	return local_run(c, h_off, pr, n, o_del, e_del, o_ins, e_ins, out);
}

/* ------------------------------------------------------------------------------------------------ */
/* ksw_extend2 as a batch service, and kswx_align_no_stat on top of it and of wtz_local_batch           */
/* ------------------------------------------------------------------------------------------------ */
/* the arguments every problem of a K-kext launch shares, or WTZ_E_ARG */
static int kext_scores(const wtz_ctx *c, const char *who, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, int32_t zdrop, wtz_kextsc_t *S){
	CHK(batch_scores(c, who, o_del, e_del, o_ins, e_ins, 1));
	S->M = c->P.M; S->X = c->P.X; S->o_del = o_del; S->e_del = e_del; S->o_ins = o_ins; S->e_ins = e_ins; S->zdrop = zdrop;
	return WTZ_OK;
}
/* problem i of a K-kext launch from its two views, or WTZ_E_ARG (the LIMIT of include/wtzmo_hip.h): the band width after the clamp of ksw.c:403-408 and the
 * diagonals the band can reach, which decide the kernel instantiation */
static int kext_plan(const wtz_ctx *c, const std::vector<uint64_t> &h_off, const wtz_dp_problem_t &p, uint32_t i, const wtz_kextsc_t &S, int32_t end_bonus, wtz_kextprob_t *d){
	CHK(dp_problem_views(c, h_off, p, i, false, WTZ_KEXT_MAXLEN, &d->q, &d->t));
	if(p.W < 0 || p.W > WTZ_KEXT_MAXW) return wtz_fail(WTZ_E_ARG, "problem %u: band width %d outside [0, %d]", i, p.W, WTZ_KEXT_MAXW);
	const int32_t h0 = p.init_score < 0 ? 0 : p.init_score;
	if((int64_t)h0 + (int64_t)p.q_len * S.M > (1 << 30)) return wtz_fail(WTZ_E_ARG, "problem %u: start score + q_len * M beyond 2^30", i);
	if(end_bonus < -(1 << 30) || end_bonus > (1 << 30)) return wtz_fail(WTZ_E_ARG, "problem %u: end bonus beyond 2^30 in magnitude", i);
	int32_t w = p.W;
	int32_t max_ins = (int32_t)((double)((int64_t)p.q_len * S.M + end_bonus - S.o_ins) / S.e_ins + 1.); max_ins = max_ins > 1 ? max_ins : 1; w = w < max_ins ? w : max_ins;
	int32_t max_del = (int32_t)((double)((int64_t)p.q_len * S.M + end_bonus - S.o_del) / S.e_del + 1.); max_del = max_del > 1 ? max_del : 1; w = w < max_del ? w : max_del;
	d->qlen = p.q_len; d->tlen = p.t_len; d->h0 = h0; d->w = w; d->dlo = w < p.t_len - 1 ? w : p.t_len - 1;
	return WTZ_OK;
}
static int32_t kext_slots(const wtz_kextprob_t &d){ return d.dlo + (d.w < d.qlen - 1 ? d.w : d.qlen - 1) + 1; }

template<int C> static int kext_launch(const wtz_kextprob_t *pr, const uint32_t *order, uint32_t n, const wtz_kextsc_t &S, wtz_kextres_t *res){
#ifdef WTZ_EMUL
	for(uint32_t b = 0; b < n; b++) wtz_kext_problem<C>(pr[order[b]], S, res[order[b]]);
#else
	WTZ_LAUNCH(wtz_kernel_kext<C>, n, 64, 0, g_stream, pr, order, n, S, res);
#endif
	return WTZ_OK;
}
/* THE launch path of K-kext: the problems of one score setting, one launch per kernel instantiation present, one wavefront per problem, largest first.
 * hr[i], form[i]: result and slots per lane of problem i.  Counts into ms_kext / n_kext / cells_kext. */
static int kext_run(wtz_ctx *c, const std::vector<wtz_kextprob_t> &hp, const wtz_kextsc_t &S, std::vector<wtz_kextres_t> &hr, std::vector<uint32_t> &form){
	const uint32_t n = (uint32_t)hp.size();
	hr.resize(n); form.resize(n);
	if(n == 0) return WTZ_OK;
	wtz_arena_scope launch_scope(&c->arena);      /* the buffers of this launch group go back when it returns (scopes nest) */
	std::vector<uint64_t> weight(n);
	for(uint32_t i = 0; i < n; i++){ form[i] = (uint32_t)wtz_kext_form(kext_slots(hp[i])); weight[i] = (uint64_t)hp[i].tlen * (uint64_t)kext_slots(hp[i]); }
	const std::vector<uint32_t> order = batch_order(n, form.data(), weight);
	wtz_kextprob_t *d_pr = NULL; uint32_t *d_order = NULL; wtz_kextres_t *d_res = NULL;
	CHK(batch_upload(hp, order, &d_pr, &d_order, &d_res));
	wtz_timer tm; tm.start();
	CHK(for_each_form(n, [&](uint32_t b){ return form[order[b]]; }, [&](auto K, uint32_t b0, uint32_t b1){ return kext_launch<decltype(K)::value>(d_pr, d_order + b0, b1 - b0, S, d_res); }));
	CHK(batch_fetch(tm, c->cnt.ms_kext, n, d_res, hr));
	for(uint32_t i = 0; i < n; i++) c->cnt.cells_kext += hr[i].cells;
	c->cnt.n_kext += n;
	return WTZ_OK;
}

/* ksw_extend2 (ksw.c:381-478) for n independent problems on views of the uploaded reads: K-kext (wtz_sw_kext.h) */
extern "C" int wtz_kext_batch(wtz_ctx_t *c, const wtz_dp_problem_t *pr, uint32_t n, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, int32_t end_bonus, int32_t zdrop, wtz_kext_result_t *out){
	BATCH_ARGS(c, n, pr && out, "wtz_kext_batch", "problems");
	wtz_kextsc_t S; CHK(kext_scores(c, "wtz_kext_batch", o_del, e_del, o_ins, e_ins, zdrop, &S));
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	std::vector<wtz_kextprob_t> hp(n);
	for(uint32_t i = 0; i < n; i++) CHK(kext_plan(c, h_off, pr[i], i, S, end_bonus, &hp[i]));
	std::vector<wtz_kextres_t> hr; std::vector<uint32_t> form;
	CHK(kext_run(c, hp, S, hr, form));
	for(uint32_t i = 0; i < n; i++){
		wtz_kext_result_t o; memset(&o, 0, sizeof o);
		o.score = hr[i].score; o.qle = hr[i].qle; o.tle = hr[i].tle; o.gtle = hr[i].gtle; o.gscore = hr[i].gscore; o.max_off = hr[i].max_off;
		o.form_used = form[i]; o.rows = hr[i].rows; o.cells = hr[i].cells;
		out[i] = o;
	}
	CHK(pool_check(c, "wtz_kext_batch"));
	return batch_leave(c);
}

/* kswx_align_no_stat (kswx.h:1504-1511): the local hit of wtz_local_batch, then kswx_extend_core (kswx.h:1386-1441) as two stages of K-kext launches.
 * side 0 = left (the reversed prefixes in front of the hit), 1 = right; role 0 = the problem's target is ksw_extend2's target (rows), 1 = its query is. */
/* the argument checks of wtz_align_batch, under the name of the entry point that makes them */
static int align_args(const wtz_ctx *c, const char *who, const wtz_dp_problem_t *pr, uint32_t n, const void *out, int32_t w, int32_t I, int32_t D, int32_t E, int32_t T, wtz_kextsc_t *SR){
	BATCH_ARGS(c, n, pr && out, NULL, NULL);
	if(I > 0 || D > 0 || E > -1 || I < -32767 || D < -32767 || E < -32767 || T < -(1 << 30)) return wtz_fail(WTZ_E_ARG, "%s: I and D must be <= 0 and E <= -1 (costs as negative numbers)", who);
	if(w < 0 || w > WTZ_KEXT_MAXW) return wtz_fail(WTZ_E_ARG, "%s: band width %d outside [0, %d]", who, w, WTZ_KEXT_MAXW);
	/* by role: kswx.h:1396 / 1422 and, with the opening costs exchanged, kswx.h:1407 / 1431 */
	CHK(kext_scores(c, who, -D, -E, -I, -E, -1, &SR[0]));
	CHK(kext_scores(c, who, -I, -E, -D, -E, -1, &SR[1]));
	return WTZ_OK;
}
static int align_stages(wtz_ctx *c, const char *entry, const std::vector<uint64_t> &h_off, const wtz_dp_problem_t *pr, uint32_t n, int32_t w, int32_t I, int32_t D, int32_t E, int32_t T, const wtz_kextsc_t *SR, wtz_align_result_t *out);
extern "C" int wtz_align_batch(wtz_ctx_t *c, const wtz_dp_problem_t *pr, uint32_t n, int32_t w, int32_t I, int32_t D, int32_t E, int32_t T, wtz_align_result_t *out){
	wtz_kextsc_t SR[2];
	CHK(align_args(c, "wtz_align_batch", pr, n, out, w, I, D, E, T, SR));
	if(n == 0) return WTZ_OK;
	CHK(batch_count(n, "wtz_local_batch", "problems"));      /* stage 1's limit, under its name */
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	return align_stages(c, "wtz_align_batch", h_off, pr, n, w, I, D, E, T, SR, out);
}
/* the three stages of kswx_align_no_stat, shared by wtz_align_batch and wtz_alignx_batch (behind the caller's batch_begin); leaves the main pool empty */
static int align_stages(wtz_ctx *c, const char *entry, const std::vector<uint64_t> &h_off, const wtz_dp_problem_t *pr, uint32_t n, int32_t w, int32_t I, int32_t D, int32_t E, int32_t T, const wtz_kextsc_t *SR, wtz_align_result_t *out){
	/* stage 1; its own checks (1 <= q_len, t_len <= 65535, the views) come before its launch, and nothing else has run by then */
	std::vector<wtz_local_result_t> loc(n);
	CHK(local_run(c, h_off, pr, n, -D, -E, -I, -E, loc.data()));
	for(uint32_t i = 0; i < n; i++){
		wtz_align_result_t o; memset(&o, 0, sizeof o);
		const wtz_local_result_t &l = loc[i];
		if(!(l.qb <= -1 || l.tb <= -1 || l.qe <= -1 || l.te <= -1)){
			o.found = 1; o.score = o.local_score = l.score; o.tb = o.local_tb = l.tb; o.qb = o.local_qb = l.qb; o.te = o.local_te = l.te + 1; o.qe = o.local_qe = l.qe + 1;
		}
		out[i] = o;
	}
	if(T >= 0) return WTZ_OK;
	for(int side = 0; side < 2; side++){
		std::vector<wtz_kextprob_t> hp[2]; std::vector<uint32_t> who[2];
		for(uint32_t i = 0; i < n; i++){
			const wtz_align_result_t &o = out[i];
			if(!o.found) continue;
			const wtz_dp_problem_t &p = pr[i];
			const int32_t remq = side == 0 ? o.qb : p.q_len - o.qe, remt = side == 0 ? o.tb : p.t_len - o.te;
			if(remq == 0 || remt == 0) continue;                                   /* kswx.h:1391, 1418 */
			const int role = remt >= remq ? 0 : 1;
			const int32_t cols = role == 0 ? remq : remt, other = role == 0 ? remt : remq;
			const int32_t nrow = cols + w > other ? other : cols + w;              /* the row side is cut to the column side + w */
			/* the two remaining sides as views of the problem's views: from the hit outwards */
			wtz_dp_problem_t e = p;
			const int32_t qat = side == 0 ? o.qb - 1 : o.qe, tat = side == 0 ? o.tb - 1 : o.te, dir = side == 0 ? -1 : 1;
			const int32_t qf = p.q_from + p.q_strand * qat, tf = p.t_from + p.t_strand * tat, qs = p.q_strand * dir, ts = p.t_strand * dir;
			if(role == 0){ e.q_from = qf; e.q_strand = qs; e.q_len = cols; e.t_from = tf; e.t_strand = ts; e.t_len = nrow; }
			else { e.q_read = p.t_read; e.q_rev = p.t_rev; e.q_from = tf; e.q_strand = ts; e.q_len = cols; e.t_read = p.q_read; e.t_rev = p.q_rev; e.t_from = qf; e.t_strand = qs; e.t_len = nrow; }
			e.init_score = o.score; e.W = w;
			wtz_kextprob_t d; CHK(kext_plan(c, h_off, e, i, SR[role], -T, &d));
			hp[role].push_back(d); who[role].push_back(i);
		}
		for(int role = 0; role < 2; role++){
			std::vector<wtz_kextres_t> hr; std::vector<uint32_t> form;
			CHK(kext_run(c, hp[role], SR[role], hr, form));
			for(size_t k = 0; k < hr.size(); k++){
				wtz_align_result_t &o = out[who[role][k]];
				const wtz_dp_problem_t &p = pr[who[role][k]];
				const wtz_kextres_t &x = hr[k];
				const bool clip = x.gscore <= 0 || x.gscore <= x.score + T;        /* kswx.h:1398: the best cell, not the end of the column side */
				/* columns / rows taken: (qle, tle), or everything that was left of the column side and gtle rows */
				const int32_t dcol = clip ? x.qle : -1, drow = clip ? x.tle : x.gtle;
				int32_t &qend = side == 0 ? o.qb : o.qe, &tend = side == 0 ? o.tb : o.te;
				const int32_t qlim = side == 0 ? 0 : p.q_len, tlim = side == 0 ? 0 : p.t_len, sg = side == 0 ? -1 : 1;
				if(role == 0){ qend = dcol < 0 ? qlim : qend + sg * dcol; tend += sg * drow; }
				else { tend = dcol < 0 ? tlim : tend + sg * dcol; qend += sg * drow; }
				o.score = clip ? x.score : x.gscore;
			}
		}
	}
	CHK(pool_check(c, entry));
	return batch_leave(c);
}

#include "wtz_lib_glob.h"
#include "wtz_lib_pwtext.h"
#include "wtz_lib_hzmaux.h"
#include "wtz_testdp.h"
