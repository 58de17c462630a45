/*
 * wtz_lib_align.h — wtz_pairs_align and the stage runners under it: K-sw1 (lane pipeline, chained wave kernel), K-sw2 (lane pipeline,
 * wavefront kernel), K-sw3 (extension jobs, both ends fused on one wavefront), stitching.  Included by wtz_lib.cpp.
 */
/* the context's two gap-open costs differ (wtz_set_gap_open): the K-sw3 register forms are launched in their split-cost instantiation (wtz_sw_frame.h), the
 * lane DPs and the gap kernels in the instantiation that reads both costs; otherwise each runs the instantiation in which the two are one value, as before */
static bool ext_split(const wtz_ctx *c){ return c->P.I != c->P.D; }
#ifndef WTZ_EMUL
/* upper bound of the transient-pool bytes one K-sw3 job takes (trace rows come 64 at a time; a row is the widest of the wave forms), its row bound and its band class */
WTZ_HD uint64_t wtz_ext_trace_need(int32_t qlen, int32_t tlen, int32_t init, int32_t W, int32_t M, int32_t I, int32_t D, int32_t E, int32_t T, int32_t *ql_out, int32_t *ncol_out){
	if(ql_out) *ql_out = 0;
	if(ncol_out) *ncol_out = 0;
	if(qlen <= 0 || tlen <= 0) return 0;
	if(init < 0) init = 0;
	int32_t ql, tl, n_col;
	wtz_ext_geometry(qlen, tlen, init, W, M, I, D, E, T, ql, tl, n_col);
	if(ql_out) *ql_out = ql;
	if(ncol_out) *ncol_out = n_col;
	/* row bytes: the widest of the one-wave register forms (4-column steps), a 256-lane row (the layout of the removed four-wave kernels) and the LDS-ring kernel
	 * (odd columns per lane).  The 256-lane term stays: the launch groups and ext_use_ratio are calibrated against this bound, and it changes no result */
	const uint64_t c_reg = ((uint64_t)(n_col + 63) / 64 + 3) / 4, c_mw = ((uint64_t)(n_col + 255) / 256 + 3) / 4 * 4, c_gen = ((((uint64_t)(n_col + 63) / 64) | 1) + 3) / 4;
	uint64_t zrow = (c_reg > c_gen ? c_reg : c_gen) * 256; if(c_mw * 256 > zrow) zrow = c_mw * 256;
	uint64_t nb = ((uint64_t)(ql + 63) / 64) * 64 * zrow + (uint64_t)WTZ_TRACE_MAXCHUNK * 8 + (uint64_t)(ql + 2) * 4 + 256;
	if((n_col + 63) / 64 > 32 || (tl + 63) / 32 + 1 > 1032){      /* outside the wave forms: the scalar body's row arrays and byte matrix, grown in powers of two */
		uint64_t z = 1024; while(z < (uint64_t)ql * (uint64_t)n_col) z <<= 1;
		uint64_t r = 64; while(r < (uint64_t)tl + 3) r <<= 1;
		uint64_t zb = 64; while(zb < (uint64_t)ql + 2) zb <<= 1;
		nb = z + 8 * r + 4 * zb + 256;
	}
	return nb;
}
static uint64_t ext_trace_need(const wtz_ctx *c, int32_t qlen, int32_t tlen, int32_t init, int32_t W, int32_t *ql_out, int32_t *ncol_out){
	return wtz_ext_trace_need(qlen, tlen, init, W, c->P.M, c->P.I, c->P.D, c->P.E, c->P.T, ql_out, ncol_out);
}
#define WTZ_LAUNCH_SP(c, kernel, tw, ...) do { if(ext_split(c)) WTZ_LAUNCH((kernel<tw, true>), __VA_ARGS__); else WTZ_LAUNCH((kernel<tw, false>), __VA_ARGS__); } while(0)

/* Both end extensions of every item of the stage on one wavefront per item (wtz_stitch_fused.h).  The items are ordered by the rows their two extensions can
 * run at most (longest first) and the launch is made only if the traces of ALL jobs fit the transient pool together (their geometry is known before any
 * extension has run: wtz_task_stitch_left's rgeo); otherwise c->fused_ran stays false and the stage runs its launches one after the other as before. */
static int run_stitch_fused(wtz_ctx *c, const wtz_env_t &V, const wtz_alnitem_t *d_items, wtz_stitch_state_t *d_st, wtz_extjob_t *d_jl, wtz_extjob_t *d_jr, const wtz_gapres_t *d_gaps, const int32_t *d_rgeo, uint32_t m){
	c->fused_ran = false;
	if(m == 0) return WTZ_OK;
	/* order and budget on the device (the host form - fetch the geometry, order 31 000 items, send the order back - was 2.7 ms of an idle device per range):
	 * key = the rows both jobs can run at most, inverted (ascending stable radix sort = longest first, ties in item order); the trace bounds are summed with an atomic */
	uint64_t *d_k = NULL; uint32_t *d_order = NULL; unsigned long long *d_acc = NULL;
	uint32_t *d_open = NULL;
	CHK(dev_alloc((void**)&d_k, (size_t)m * 8)); CHK(dev_alloc((void**)&d_order, (size_t)m * 4)); CHK(dev_alloc((void**)&d_acc, 24)); CHK(dev_set(d_acc, 0, 24));
	if(c->sw.ext_pk) CHK(dev_alloc((void**)&d_open, ((size_t)m + 1) * 4));
	{
		const int32_t pM = c->P.M, pI = c->P.I, pD = c->P.D, pE = c->P.E, pT = c->P.T, pW = -c->P.ew;
		const bool use_pk = c->sw.ext_pk != 0; const wtz_params_t *dP = V.P;
		CHK(wtz_launch<K_misc>(m, [=] WTZ_LAMBDA (uint64_t t){
			const wtz_extjob_t &j = d_jl[t];
			int32_t qa = 0, qb = 0;
			unsigned long long nb = wtz_ext_trace_need(j.valid ? j.qlen : -1, j.tlen, 0, pW, pM, pI, pD, pE, pT, &qa, (int32_t*)NULL);
			nb += wtz_ext_trace_need(d_rgeo[2 * t], d_rgeo[2 * t + 1], 0, pW, pM, pI, pD, pE, pT, &qb, (int32_t*)NULL);
			const uint32_t rows = (uint32_t)qa + (uint32_t)qb;
			/* which form takes the item (bit 32 of the key: the items of the 32-bit form end up behind those of the packed form, both longest-first): the packed
			 * form needs both extensions inside its 16-bit window - the left one's init_score is known, the right one's is not (wtz_pk_window_range) */
			uint32_t to_fr = 0;
			if(use_pk){
				if(j.valid && j.qlen > 0 && j.tlen > 0){
					int32_t W = pW, ql = 0, tl = 0, nc = 0, bias, ng, sh; const int32_t in0 = j.init_score < 0 ? 0 : j.init_score;
					wtz_ext_geometry(j.qlen, j.tlen, in0, W, pM, pI, pD, pE, pT, ql, tl, nc);
					if(!wtz_pk_window(dP, in0, ql, tl, &bias, &ng, &sh)) to_fr = 1;
				}
				if(d_rgeo[2 * t] > 0 && d_rgeo[2 * t + 1] > 0){
					/* the right extension's init_score (wtz_task_stitch_mid) = the left extension's score - 100 M + the windows and gaps behind the first window: all of it
					 * known here but the left extension's gain, which lies in [0, M * min(its two sides)] */
					const wtz_stitch_state_t &st = d_st[t]; const wtz_alnitem_t &it = d_items[t];
					long long i_lo = st.x.score, gain = 0;
					if(j.valid && j.qlen > 0 && j.tlen > 0) gain = (long long)pM * (j.qlen < j.tlen ? j.qlen : j.tlen);
					const wtz_gapres_t *gp = d_gaps + (it.regs - d_items[0].regs);
					for(uint32_t k = st.first + 1; k < it.nwin; k++) if(it.regs[k].pass == 1) i_lo += (long long)gp[k].score + it.regs[k].x.score;
					int32_t W = pW, ql = 0, tl = 0, nc = 0;
					wtz_ext_geometry(d_rgeo[2 * t], d_rgeo[2 * t + 1], 0, W, pM, pI, pD, pE, pT, ql, tl, nc);
					if(!wtz_pk_window_range(dP, ql, tl, i_lo, i_lo + gain)) to_fr = 1;
				}
			}
			d_k[t] = ((uint64_t)to_fr << 32) | (uint64_t)(0xFFFFFFFFu - rows); d_order[t] = (uint32_t)t;
			if(to_fr) WTZ_ATOMIC_ADD64(&d_acc[2], 1ull);
			if(nb) WTZ_ATOMIC_ADD64(&d_acc[0], nb);
			if(rows) WTZ_ATOMIC_ADD64(&d_acc[1], (unsigned long long)rows);
		}));
	}
	CHK(dev_sort_pairs_u64_u32(d_k, d_order, m, 33));
	unsigned long long h_acc[3] = {0, 0, 0}; CHK(dev_d2h(h_acc, d_acc, 24));
	const uint64_t acc = h_acc[0]; const unsigned long long ext_sum = h_acc[1];
	const uint64_t budget = (c->pool_bytes - c->main_bytes) / 16 * 15;
	/* acc sums UPPER bounds (every job run to its last row); the traces are allocated 64 rows at a time as a job runs, and most jobs end early: what the launches
	 * before this one took of their bounds (x 1.3, never below a fifth) is what this one is expected to take.  An estimate that was too low ends in WTZ_E_POOL like
	 * any other exhausted pool: the host redoes the range in halves. */
	/* what does not fit at once runs in up to four groups (every ng-th item of the order each: all groups are ordered longest-first), the transient pool reset between them */
	uint32_t ng = 1; while(ng < 4 && (double)acc * c->ext_use_ratio / ng > (double)budget) ng++;
	if((double)acc * c->ext_use_ratio / ng > (double)budget){ if(c->sw.profile) fprintf(stderr, "[ext-profile] fused launch declined: %u items, trace bounds %.1f GB x %.2f against %.1f GB\n", m, acc / 1e9, c->ext_use_ratio, budget / 1e9); return WTZ_OK; }          /* the two launches cut their jobs into groups that fit */
	double ms_l = 0; uint64_t used_sum = 0;
	for(uint32_t g = 0; g < ng; g++){
		const uint32_t mg = (m - g + ng - 1) / ng;
		if(mg == 0) continue;
		CHK(tpool_reset(c));
		wtz_timer te; te.start();
		if(c->sw.ext_pk){
			/* the packed 16-bit form; the items dealt to the 32-bit form beforehand (the tail of the order: a handful of the longest extensions per step) run beside
			 * it on the side stream; what the packed form declines after all is listed and finished by the 32-bit form behind it */
			uint32_t n_fr = ng == 1 ? (uint32_t)h_acc[2] : 0u;
			if(n_fr > mg) n_fr = mg;
			CHK(dev_set(d_open, 0, 4));
			if(n_fr){
				HIPCHK(hipEventRecord(c->ev_side_fork, g_stream)); HIPCHK(hipStreamWaitEvent(c->stream_side, c->ev_side_fork, 0));
				WTZ_LAUNCH_SP(c, wtz_kernel_stitch_ext_fr, 1032, n_fr, 64, WTZ_WAVE_LDS_BYTES, c->stream_side, V, d_items, d_st, d_jl, d_jr, d_gaps, (const uint32_t*)d_order + (mg - n_fr), n_fr, 1u, 0u);
				HIPCHK(hipEventRecord(c->ev_side_join, c->stream_side));
			}
			const uint32_t n_pk = mg - n_fr;
			if(n_pk){
				WTZ_LAUNCH_SP(c, wtz_kernel_stitch_ext_pk, 1032, n_pk, 64, WTZ_PK_LDS_BYTES(1032), g_stream, V, d_items, d_st, d_jl, d_jr, d_gaps, (const uint32_t*)d_order, n_pk, ng, g, d_open);
			}
			if(n_fr) HIPCHK(hipStreamWaitEvent(g_stream, c->ev_side_join, 0));
			uint32_t n_open = 0; CHK(dev_d2h(&n_open, d_open, 4));
			c->ext_open_total += n_open; c->ext_fr_total += n_fr;
			if(n_open){ WTZ_LAUNCH_SP(c, wtz_kernel_stitch_ext_fr, 1032, n_open, 64, WTZ_WAVE_LDS_BYTES, g_stream, V, d_items, d_st, d_jl, d_jr, d_gaps, (const uint32_t*)d_open + 1, n_open, 1u, 0u); }
		} else WTZ_LAUNCH_SP(c, wtz_kernel_stitch_ext_fr, 1032, mg, 64, WTZ_WAVE_LDS_BYTES, g_stream, V, d_items, d_st, d_jl, d_jr, d_gaps, (const uint32_t*)d_order, mg, ng, g);
		ms_l += te.stop();
		{
			const int rc_t = tpool_check(c, "K-sw3 extension jobs (both ends on one wavefront)");
			if(rc_t != WTZ_OK){
				/* the budget under-estimated what the traces take: the next launch is planned with twice the share (the host redoes this range in halves and is told
				 * that it was the transient pool, so that its bytes-per-pair estimate of the MAIN pool is left alone: wtz_pool_failure_kind) */
				c->ext_use_ratio = c->ext_use_ratio * 2.0 > 1.0 ? 1.0 : c->ext_use_ratio * 2.0;
				return rc_t;
			}
		}
		used_sum += c->tpool_last_used;
	}
	c->cnt.ms_ext += ms_l; c->cnt.n_extjobs += 2ull * m;
	c->fused_ran = true;
	if(c->sw.profile) fprintf(stderr, "[ext-profile] fused launch: %u items in %u group(s), rows (upper bound) sum %llu, %.2f ms; items of the 32-bit form so far: dealt %llu, declined by the packed form %llu\n", m, ng, ext_sum, ms_l, c->ext_fr_total, c->ext_open_total);
	c->tpool_last_used = used_sum;
	if(acc){ const double seen = 1.3 * (double)c->tpool_last_used / (double)acc, keep = c->ext_use_ratio * 0.9; c->ext_use_ratio = seen > keep ? seen : keep; if(c->ext_use_ratio < 0.2) c->ext_use_ratio = 0.2; if(c->ext_use_ratio > 1.0) c->ext_use_ratio = 1.0; }
	return WTZ_OK;
}
#endif

/* K-sw3 jobs of a batch: one wavefront per job (wtz_sw_shift.h).  WTZ_SW_SCALAR=1 forces the scalar body,
 * WTZ_SW_CHECK=1 runs both and fails loudly on any difference (on-device cross-check). */
static int run_extjobs(wtz_ctx *c, const wtz_env_t &V, wtz_extjob_t *d_jobs, uint32_t m, bool leftover = false){
	if(m == 0) return WTZ_OK;
#ifdef WTZ_EMUL
	(void)c; (void)leftover;      /* the host emulation has the scalar body only */
	return wtz_launch_wave<K_extjob_scalar>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_extjob_scalar((uint32_t)t, V, d_jobs); });
#else
	if(leftover){
		/* behind the fused launch (run_stitch_fused): what is still open is outside the frame kernel's envelope - the general kernel takes it; every other wavefront leaves at once */
		if(!c->fused_ran) leftover = false;
		else {
			wtz_timer te; te.start();
			WTZ_LAUNCH((wtz_kernel_extjobs<2048, 1032>), m, 64, 0, g_stream, d_jobs, (const uint32_t*)NULL, m, V.P, V.pool, V.pool + 1);
			c->cnt.ms_ext += te.stop();
			return tpool_check(c, "K-sw3 extension jobs");
		}
	}
	const int mode = c->sw.sw_mode;
	if(mode == 1) return wtz_launch_wave<K_extjob_scalar>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_extjob_scalar((uint32_t)t, V, d_jobs); });
	std::vector<wtz_extjob_t> ref;
	if(mode == 2){
		wtz_extjob_t *d_copy = NULL; CHK(dev_alloc((void**)&d_copy, (size_t)m * sizeof(wtz_extjob_t)));
		HIPCHK(hipMemcpyAsync(d_copy, d_jobs, (size_t)m * sizeof(wtz_extjob_t), hipMemcpyDeviceToDevice, g_stream));
		CHK(wtz_launch_wave<K_extjob_scalar>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_extjob_scalar((uint32_t)t, V, d_copy); }));
		CHK(dev_sync());
		ref.resize(m); CHK(dev_d2h(ref.data(), d_copy, (size_t)m * sizeof(wtz_extjob_t)));
	}
	/* longest-processing-time-first: the rows of an extension are sequential, so the longest job bounds the launch;
	 * start the long ones first (key = query-side length, the row count upper bound) */
	uint32_t *d_order = NULL; unsigned long long ext_sum = 0; int32_t ext_max = 0;
	std::vector<uint32_t> ord(m); std::vector<uint64_t> need(m); std::vector<uint8_t> cw(m, 0);
	unsigned long long geo_n[9] = {0}, geo_rows[9] = {0}, geo_cells[9] = {0};
	{
		/* (qlen, tlen, init_score, W) of every job: the order key, and the job's geometry = an upper bound of its trace bytes */
		int32_t *d_key = NULL; CHK(dev_alloc((void**)&d_key, (size_t)m * 16));
		CHK(wtz_launch<K_misc>(m, [=] WTZ_LAMBDA (uint64_t t){ const wtz_extjob_t &j = d_jobs[t]; d_key[4 * t] = j.valid ? j.qlen : -1; d_key[4 * t + 1] = j.tlen; d_key[4 * t + 2] = j.init_score; d_key[4 * t + 3] = j.W; }));
		std::vector<int32_t> key4((size_t)m * 4); CHK(dev_d2h(key4.data(), d_key, (size_t)m * 16));
		std::vector<int32_t> key(m);
		for(uint32_t i = 0; i < m; i++){ key[i] = key4[(size_t)i * 4]; if(key[i] > 0){ ext_sum += (unsigned long long)key[i]; if(key[i] > ext_max) ext_max = key[i]; } }
		std::vector<int32_t> rows(m, -1);       /* the order key: the rows the job can run at most (the shorter side + W, not the query side alone: most long overhangs face a short one) */
		for(uint32_t i = 0; i < m; i++){
			const int32_t qlen = key4[(size_t)i * 4], tlen = key4[(size_t)i * 4 + 1];
			need[i] = 0;
			if(qlen <= 0 || tlen <= 0) continue;
			int32_t ql = 0, n_col = 0;
			need[i] = ext_trace_need(c, qlen, tlen, key4[(size_t)i * 4 + 2], key4[(size_t)i * 4 + 3], &ql, &n_col);
			cw[i] = (uint8_t)((n_col + 63) / 64 > 255 ? 255 : (n_col + 63) / 64);
			rows[i] = ql;
			if(c->sw.profile){ const int b = (n_col + 63) / 64 > 32 ? 8 : ((n_col + 63) / 64 - 1) / 4; geo_n[b]++; geo_rows[b] += (unsigned long long)ql; geo_cells[b] += (unsigned long long)ql * (unsigned long long)n_col; }
		}
		for(uint32_t i = 0; i < m; i++) ord[i] = i;
		std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b){ return rows[a] > rows[b]; });
		CHK(dev_alloc((void**)&d_order, (size_t)m * 4)); CHK(dev_h2d(d_order, ord.data(), (size_t)m * 4));
		if(c->sw.profile){
			fprintf(stderr, "[ext-profile] geometry by columns per lane (upper bounds):");
			for(int b = 0; b < 9; b++) if(geo_n[b]) fprintf(stderr, " C<=%d: %llu jobs %.1f Mrows %.1f Gcells;", b < 8 ? 4 * b + 4 : 999, geo_n[b], (double)geo_rows[b] / 1e6, (double)geo_cells[b] / 1e9);
			fprintf(stderr, "\n");
		}
	}
	{
		wtz_timer te; te.start();
		/* launch groups: consecutive jobs of the order whose trace upper bounds fit the transient pool together; the pool is reset
		 * between groups (the CIGARs went to the main pool).  One group is the normal case. */
		const uint64_t budget = (c->pool_bytes - c->main_bytes) / 16 * 15;
		uint32_t g0 = 0, n_groups = 0;
		while(g0 < m){
			uint32_t g1 = g0; uint64_t acc = 0;
			while(g1 < m && (g1 == g0 || acc + need[ord[g1]] <= budget)){ acc += need[ord[g1]]; g1++; }
			CHK(tpool_reset(c));      /* the traces of the previous group / the previous stage are dead: their CIGARs are in the main pool */
			/* one wavefront per job, longest first: the packed form, the 32-bit frame form (wtz_sw_frame.h) for what is outside the packed form's window, the
			 * general kernel for what is outside the frame forms' envelope.  The forms these replaced are in the git history; CHANGELOG.md has their numbers. */
			if(c->sw.ext_pk){      /* two 16-bit cells per register (wtz_sw_frame16.h); what is outside its window stays open for the 32-bit form */
				WTZ_LAUNCH_SP(c, wtz_kernel_extjobs_pk, 1032, g1 - g0, 64, 0, g_stream, d_jobs, (const uint32_t*)d_order + g0, g1 - g0, V.P, V.pool, V.pool + 1);
			}
			WTZ_LAUNCH_SP(c, wtz_kernel_extjobs_fr, 1032, g1 - g0, 64, 0, g_stream, d_jobs, (const uint32_t*)d_order + g0, g1 - g0, V.P, V.pool, V.pool + 1);
			WTZ_LAUNCH((wtz_kernel_extjobs<2048, 1032>), g1 - g0, 64, 0, g_stream, d_jobs, (const uint32_t*)d_order + g0, g1 - g0, V.P, V.pool, V.pool + 1);     /* whatever the frame forms left */
			if(g1 < m || n_groups){ CHK(dev_sync()); CHK(tpool_check(c, "K-sw3 extension jobs")); }
			g0 = g1; n_groups++;
		}
		const double ms_l = te.stop();
		CHK(tpool_check(c, "K-sw3 extension jobs"));
		c->cnt.ms_ext += ms_l; c->cnt.n_extjobs += m;
		if(c->sw.profile){
			std::vector<int32_t> key(m); uint32_t nv = 0, n256 = 0, n512 = 0, n1k = 0, n2k = 0, n4k = 0; unsigned long long s512 = 0;
			CHK(dev_sync());
			{ std::vector<wtz_extjob_t> jj(m); CHK(dev_d2h(jj.data(), d_jobs, (size_t)m * sizeof(wtz_extjob_t))); uint32_t nd[4] = {0, 0, 0, 0}; for(uint32_t i = 0; i < m; i++){ key[i] = jj[i].valid ? jj[i].x.qe : -1; if(jj[i].valid) nd[jj[i].done & 3]++; }
			  if(const char *dp = getenv("WTZ_EXT_DUMP")){      /* job geometry of this call, 8 int32 per valid job: the input of tools/ubench/ksw3_bench.py */
				if(FILE *df = fopen(dp, "ab")){ for(uint32_t i = 0; i < m; i++) if(jj[i].valid){ const int32_t r[8] = {jj[i].qlen, jj[i].tlen, jj[i].init_score, jj[i].W, jj[i].x.qe, jj[i].x.te, (int32_t)(jj[i].cells > 0x7FFFFFFFull ? 0x7FFFFFFF : jj[i].cells), (int32_t)jj[i].done}; fwrite(r, 4, 8, df); } fclose(df); } }
			  fprintf(stderr, "[ext-profile] %u launch group(s); valid jobs finished by: nobody %u, 32-bit frame form %u, packed form or general kernel %u\n", n_groups, nd[0], nd[1], nd[3]); }
			for(uint32_t i = 0; i < m; i++){ if(key[i] < 0) continue; nv++; if(key[i] >= 256) n256++; if(key[i] >= 512){ n512++; s512 += key[i]; } if(key[i] >= 1024) n1k++; if(key[i] >= 2048) n2k++; if(key[i] >= 4096) n4k++; }
			fprintf(stderr, "[ext-profile] %u jobs (%u valid), rows (upper bound) sum %llu max %d, %.2f ms; qe>=256 %u >=512 %u (sum %llu) >=1k %u >=2k %u >=4k %u; transient pool peak %.2f GB\n", m, nv, ext_sum, ext_max, ms_l, n256, n512, s512, n1k, n2k, n4k, c->tpool_peak_call / 1073741824.0);
		}
	}
	if(mode == 2){
		CHK(dev_sync());
		std::vector<wtz_extjob_t> got(m); CHK(dev_d2h(got.data(), d_jobs, (size_t)m * sizeof(wtz_extjob_t)));
		for(uint32_t i = 0; i < m; i++){
			if(!got[i].valid) continue;
			if(memcmp(&got[i].x, &ref[i].x, sizeof(wtz_aln_t)) || got[i].cigar_len != ref[i].cigar_len || got[i].cells != ref[i].cells)
				return wtz_fail(WTZ_E_STATE, "K-sw3 wave kernel differs from the scalar body on job %u: qlen %d tlen %d init %d W %d; score %d/%d qe %d/%d te %d/%d aln %d/%d cigar %u/%u cells %llu/%llu",
					i, got[i].qlen, got[i].tlen, got[i].init_score, got[i].W, got[i].x.score, ref[i].x.score, got[i].x.qe, ref[i].x.qe, got[i].x.te, ref[i].x.te,
					got[i].x.aln, ref[i].x.aln, got[i].cigar_len, ref[i].cigar_len, (unsigned long long)got[i].cells, (unsigned long long)ref[i].cells);
			if(got[i].cigar_len){
				std::vector<uint32_t> a(got[i].cigar_len), b(got[i].cigar_len);
				CHK(dev_d2h(a.data(), got[i].cigar, a.size() * 4)); CHK(dev_d2h(b.data(), ref[i].cigar, b.size() * 4));
				if(a != b) return wtz_fail(WTZ_E_STATE, "K-sw3 wave kernel: CIGAR differs on job %u", i);
			}
		}
	}
	return WTZ_OK;
#endif
}

/* ------------------------------------------------------------------------------------------------ */
/* A9 with one lane per K-sw1 problem (wtz_sw_lane.h)                                                */
/* ------------------------------------------------------------------------------------------------ */
#ifdef WTZ_EMUL
#define WTZ_HOST_WAVE 1u
#else
#define WTZ_HOST_WAVE 64u
#endif
/* a block of the main (0) / transient (1) device pool for a host-side array */
static int pool_alloc_host(wtz_ctx *c, int which, size_t bytes, void **out){
	unsigned long long *d_p = NULL; CHK(dev_alloc((void**)&d_p, 8));
	wtz_pool_t *pool = c->dpool + which;
	CHK(wtz_launch<K_poolalloc>(1, [=] WTZ_LAMBDA (uint64_t){ *d_p = (unsigned long long)(uintptr_t)wtz_pool_alloc(pool, bytes); }));
	unsigned long long h = 0; CHK(dev_d2h(&h, d_p, 8));
	if(h == 0) return wtz_fail(WTZ_E_POOL, "device scratch pool exhausted (%zu bytes for the K-sw1 problem lists)", bytes);
	*out = (void*)(uintptr_t)h; return WTZ_OK;
}
/* the four band classes of a lane launch (ccnt: problems per class, narrowest first) cut into wave ranges, widest class first; returns the number of waves */
static uint32_t lane_classes(const uint32_t ccnt[4], wtz_lclass_t *L){
	uint32_t lo = 0, wv = 0;
	for(int k = 0; k < 4; k++){ const uint32_t n = ccnt[3 - k]; L->lo[k] = lo; L->hi[k] = lo + n; wv += (n + WTZ_HOST_WAVE - 1) / WTZ_HOST_WAVE; L->wend[k] = wv; lo += n; }
	return wv;
}
/* one pool block cut into 256-byte-aligned arrays: carve_bytes sizes an array, carve takes it from the front of the block */
static size_t carve_bytes(size_t n, size_t elem){ return (n * elem + 255) & ~(size_t)255; }
template<typename T> static void carve(uint8_t *&blk, T *&out, size_t n){ out = (T*)blk; blk += carve_bytes(n, sizeof(T)); }
/* a leftover list (d_list[0] = count, nl entries behind it) of more than 64 entries is put heaviest first: launch_keys(d_k2) writes the inverted weight of
 * entry i to d_k2[i].  The kernels that fill these lists append in the order their lanes arrive, and a launch of wave-sized tasks of very different lengths
 * ends in the tail of whichever long one started last. */
template<typename KEYS> static int sort_leftovers(uint32_t *d_list, uint32_t nl, KEYS launch_keys){
	if(nl <= 64) return WTZ_OK;
	uint64_t *d_k2 = NULL; CHK(dev_alloc((void**)&d_k2, (size_t)nl * 8));
	CHK(launch_keys(d_k2));
	return dev_sort_pairs_u64_u32(d_k2, d_list + 1, nl, 32);
}
/* windows d_wt[0, nwt): plan -> shape sort -> relative-mode DP per class -> fold.  d_fb ([0] = count, room for nwt + 1) receives the
 * windows the chained kernel has to do (outside the envelope, or an absolute test of kswx_extend_align_core would have fired). */
static int run_winalign_lane(wtz_ctx *c, const wtz_env_t &V, const wtz_wintask_t *d_wt, uint64_t nwt, const wtz_alnitem_t *d_items, uint32_t *d_fb, uint32_t *n_fb){
	*n_fb = 0;
	if(nwt == 0) return WTZ_OK;
	const bool prof = c->sw.profile; double tp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tp0 = 0;
	if(prof){ (void)dev_sync(); tp0 = wtz_wall(); }
	auto lap = [&](int k){ if(prof){ (void)dev_sync(); const double t = wtz_wall(); tp[k] += t - tp0; tp0 = t; } };
	uint32_t *d_na = NULL, *d_woff = NULL;
	CHK(dev_alloc((void**)&d_na, (nwt + 1) * 4)); CHK(dev_alloc((void**)&d_woff, (nwt + 1) * 4));
	CHK(dev_set(d_na, 0, (nwt + 1) * 4));
	CHK(wtz_launch<K_lcount>(nwt, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_lcount((uint32_t)t, d_wt, d_items, d_na); }));
	CHK(dev_exclusive_scan_u32(d_na, d_woff, nwt + 1));
	uint32_t NS = 0; CHK(dev_d2h(&NS, d_woff + nwt, 4));
	lap(0);
	wtz_lprob_t *d_prob = NULL; uint32_t *d_cap = NULL, *d_roff = NULL, *d_val = NULL, *d_ccnt = NULL, *d_uidx = NULL, *d_nu = NULL; uint64_t *d_key = NULL; uint8_t *d_flag = NULL; wtz_lres_t *d_res = NULL;
	{   /* per-slot arrays: one block of the main pool */
		const size_t nsp = (size_t)NS + 64;
		uint8_t *blk = NULL; CHK(pool_alloc_host(c, 0, carve_bytes(nsp, sizeof(wtz_lprob_t)) + carve_bytes(nsp, sizeof(wtz_lres_t)) + 4 * carve_bytes(nsp, 4) + carve_bytes(nsp, 8), (void**)&blk));
		carve(blk, d_prob, nsp); carve(blk, d_res, nsp); carve(blk, d_cap, nsp); carve(blk, d_roff, nsp); carve(blk, d_val, nsp); carve(blk, d_uidx, nsp); carve(blk, d_key, nsp);
	}
	CHK(dev_alloc((void**)&d_flag, nwt + 16)); CHK(dev_alloc((void**)&d_nu, (nwt + 1) * 4)); CHK(dev_alloc((void**)&d_ccnt, 32)); CHK(dev_set(d_ccnt, 0, 32));
	CHK(dev_set(d_cap, 0, ((size_t)NS + 1) * 4));
	CHK(dev_set(d_res, 0, ((size_t)NS + 1) * sizeof(wtz_lres_t)));
	CHK(wtz_launch<K_lplan>(nwt, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_lplan((uint32_t)t, V, d_wt, d_items, d_woff, d_prob, d_cap, d_key, d_val, d_flag, d_ccnt, d_uidx, d_nu); }));
	lap(1);
	CHK(dev_exclusive_scan_u32(d_cap, d_roff, (uint64_t)NS + 1));
	uint32_t NR = 0, ccnt[4] = {0, 0, 0, 0};
	CHK(dev_d2h(&NR, d_roff + NS, 4)); CHK(dev_d2h(ccnt, d_ccnt, 16));
	uint32_t *d_runs = NULL; CHK(pool_alloc_host(c, 0, ((size_t)NR + 16) * 4, (void**)&d_runs));
	lap(2);
	CHK(dev_sort_pairs_u64_u32(d_key, d_val, NS, 16));
	lap(3);                 /* ascending inverted key = widest band first, longest first inside a width */
	CHK(dev_set(d_fb, 0, 4));
	{
		const uint32_t *d_ord = d_val; const wtz_lprob_t *pp = d_prob; const uint32_t *ro = d_roff; uint32_t *rn = d_runs; wtz_lres_t *rs = d_res;
		wtz_lclass_t L; const uint32_t wv = lane_classes(ccnt, &L);
		uint64_t *d_wtr = NULL; uint32_t *d_wrm = NULL;
		CHK(dev_alloc((void**)&d_wtr, ((size_t)wv + 1) * 8)); CHK(dev_alloc((void**)&d_wrm, ((size_t)wv + 1) * 4)); CHK(dev_set(d_wtr, 0, ((size_t)wv + 1) * 8));
		if(wv && ext_split(c)) CHK(wtz_launch_coop<K_ldp>(wv, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_ldp_all<true>((uint32_t)t, L, V, d_wt, d_items, d_ord, pp, rs, d_wtr, d_wrm); }, 0));
		else if(wv) CHK(wtz_launch_coop<K_ldp>(wv, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_ldp_all<false>((uint32_t)t, L, V, d_wt, d_items, d_ord, pp, rs, d_wtr, d_wrm); }, 0));
		lap(4);
		if(wv) CHK(wtz_launch_coop<K_ltb>(wv, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_ltb_all((uint32_t)t, L, V, d_wt, d_items, d_ord, pp, ro, rn, rs, d_wtr, d_wrm); }, 0));
		lap(6);
		CHK(wtz_launch<K_lfold>(nwt, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_lfold((uint32_t)t, V, d_wt, d_items, d_woff, pp, ro, rn, rs, d_flag, d_fb, d_uidx, d_nu); }));
	}
	CHK(dev_d2h(n_fb, d_fb, 4));
	{
		/* the windows left to the chained wave kernel, the ones with the most anchors first (a window's chain of problems is sequential) */
		const uint32_t nl = *n_fb; const uint32_t *lst = d_fb + 1;
		CHK(sort_leftovers(d_fb, nl, [&](uint64_t *d_k2){ return wtz_launch<K_misc>(nl, [=] WTZ_LAMBDA (uint64_t i){
			const wtz_wintask_t tk = d_wt[lst[i]];
			const wtz_win_t &w = d_items[tk.item].win[tk.widx];
			d_k2[i] = 0xFFFFFFFFull - (unsigned long long)(w.anchors[1] - w.anchors[0]);
		}); }));
	}
	lap(5);
	if(c->sw.profile) fprintf(stderr, "[lane-profile] %llu windows, %u anchor slots, K-sw1 problems by band class <=16 / <=32 / <=64 / <=104: %u / %u / %u / %u, %u run entries, %u windows left to the chained kernel; ms: count+scan %.2f plan %.2f scan+alloc %.2f sort %.2f dp %.2f traceback %.2f fold %.2f\n",
		(unsigned long long)nwt, NS, ccnt[0], ccnt[1], ccnt[2], ccnt[3], NR, *n_fb, tp[0] * 1e3, tp[1] * 1e3, tp[2] * 1e3, tp[3] * 1e3, tp[4] * 1e3, tp[6] * 1e3, tp[5] * 1e3);
	return WTZ_OK;
}

/* K-sw2 gaps of the window slots d_wt[0, nwt) with one lane per gap (wtz_lane_global); d_list ([0] = count, room for nwt + 1) = the slots
 * the wavefront kernel still has to do (empty sides, bands beyond 104 columns, gaps whose band has to be doubled again) */
static int run_gap_lane(wtz_ctx *c, const wtz_env_t &V, const wtz_wintask_t *d_wt, uint64_t nwt, const wtz_alnitem_t *d_items, wtz_gapres_t *d_gaps, uint32_t *d_list, uint32_t *n_list){
	*n_list = 0;
	if(nwt == 0) return WTZ_OK;
	wtz_lgap_t *d_gp = NULL; uint32_t *d_cap = NULL, *d_roff = NULL, *d_val = NULL, *d_ccnt = NULL; uint64_t *d_key = NULL; uint8_t *d_done = NULL;
	{
		const size_t nsp = (size_t)nwt + 64;
		uint8_t *blk = NULL; CHK(pool_alloc_host(c, 0, carve_bytes(nsp, sizeof(wtz_lgap_t)) + 3 * carve_bytes(nsp, 4) + carve_bytes(nsp, 8) + carve_bytes(nsp, 1), (void**)&blk));
		carve(blk, d_gp, nsp); carve(blk, d_cap, nsp); carve(blk, d_roff, nsp); carve(blk, d_val, nsp); carve(blk, d_key, nsp); carve(blk, d_done, nsp);
	}
	CHK(dev_alloc((void**)&d_ccnt, 32)); CHK(dev_set(d_ccnt, 0, 32));
	CHK(dev_set(d_cap, 0, ((size_t)nwt + 1) * 4));
	CHK(wtz_launch<K_gplan>(nwt, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_gplan((uint32_t)t, V, d_wt, d_items, d_gaps, d_gp, d_cap, d_key, d_val, d_done, d_ccnt); }));
	CHK(dev_exclusive_scan_u32(d_cap, d_roff, nwt + 1));
	uint32_t NR = 0, ccnt[4] = {0, 0, 0, 0};
	CHK(dev_d2h(&NR, d_roff + nwt, 4)); CHK(dev_d2h(ccnt, d_ccnt, 16));
	uint32_t *d_runs = NULL; CHK(pool_alloc_host(c, 0, ((size_t)NR + 16) * 4, (void**)&d_runs));
	CHK(dev_sort_pairs_u64_u32(d_key, d_val, nwt, 18));
	CHK(dev_set(d_list, 0, 4));
	{
		const uint32_t *d_ord = d_val; const wtz_lgap_t *gp = d_gp; const uint32_t *ro = d_roff; uint32_t *rn = d_runs; uint8_t *dn = d_done;
		wtz_lclass_t L; const uint32_t wv = lane_classes(ccnt, &L);
		uint64_t *d_wtr = NULL; uint32_t *d_wrm = NULL; wtz_lres_t *d_res = NULL;
		CHK(dev_alloc((void**)&d_wtr, ((size_t)wv + 1) * 8)); CHK(dev_alloc((void**)&d_wrm, ((size_t)wv + 1) * 4)); CHK(dev_set(d_wtr, 0, ((size_t)wv + 1) * 8));
		CHK(pool_alloc_host(c, 0, ((size_t)nwt + 1) * sizeof(wtz_lres_t), (void**)&d_res)); CHK(dev_set(d_res, 0, ((size_t)nwt + 1) * sizeof(wtz_lres_t)));
		if(wv && ext_split(c)) CHK(wtz_launch_coop<K_gdp>(wv, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_gdp_all<true>((uint32_t)t, L, V, d_wt, d_items, d_ord, gp, d_res, d_wtr, d_wrm); }, 0));
		else if(wv) CHK(wtz_launch_coop<K_gdp>(wv, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_gdp_all<false>((uint32_t)t, L, V, d_wt, d_items, d_ord, gp, d_res, d_wtr, d_wrm); }, 0));
		if(wv) CHK(wtz_launch_coop<K_gtb>(wv, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_gtb_all((uint32_t)t, L, V, d_wt, d_items, d_ord, gp, ro, rn, d_res, d_gaps, dn, d_wtr, d_wrm); }, 0));
		CHK(wtz_launch<K_glist>(nwt, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_glist((uint32_t)t, dn, d_list); }));
	}
	CHK(dev_d2h(n_list, d_list, 4));
	{
		/* the gaps left to the wavefront kernel, heaviest first (rows x lane-columns of the first band) */
		const uint32_t nl = *n_list; const wtz_lgap_t *gp = d_gp; const uint32_t *lst = d_list + 1;
		CHK(sort_leftovers(d_list, nl, [&](uint64_t *d_k2){ return wtz_launch<K_misc>(nl, [=] WTZ_LAMBDA (uint64_t i){
			const wtz_lgap_t G = gp[lst[i]];
			const int32_t nc = G.dq < 2 * G.w + 1 ? G.dq : 2 * G.w + 1;
			unsigned long long wgt = (unsigned long long)(G.dt > 0 ? G.dt : 0) * (unsigned long long)((nc > 0 ? nc : 0) / 64 + 1);
			if(wgt > 0xFFFFFFFEull) wgt = 0xFFFFFFFEull;
			d_k2[i] = 0xFFFFFFFFull - wgt;
		}); }));
	}
	if(c->sw.profile) fprintf(stderr, "[lane-profile] %llu window slots, K-sw2 gaps by band class <=16 / <=32 / <=64 / <=104: %u / %u / %u / %u, %u left to the wavefront kernel\n",
		(unsigned long long)nwt, ccnt[0], ccnt[1], ccnt[2], ccnt[3], *n_list);
	return WTZ_OK;
}

/* chained K-sw1, one window per wavefront, over the windows listed behind d_list[0] (d_list == NULL: the windows d_wt[0, n) themselves): the lean form of the kernel
 * first (register DP with one / two band columns per lane, no scalar body: fewer VGPRs); a window with a problem outside its envelope queues itself for the full
 * task.  The host emulation has one body, the scalar one.  n_redone (optional): the windows the full task redid. */
static int run_winalign_chained(wtz_ctx *c, const wtz_env_t &V, const wtz_wintask_t *d_wt, const wtz_alnitem_t *d_items, uint32_t *d_list, uint64_t n, uint32_t *n_redone = NULL){
	if(n_redone) *n_redone = 0;
	if(n == 0) return WTZ_OK;
#ifdef WTZ_EMUL
	if(d_list) return wtz_launch_coop<K_winalign>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_winalign((uint32_t)t, V, d_wt, d_items, (uint32_t*)NULL, d_list); }, WTZ_WINALIGN_LDS_BYTES + WTZ_WINALIGN_QW_BYTES);
	return wtz_launch_coop<K_winalign>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_winalign((uint32_t)t, V, d_wt, d_items); }, WTZ_WINALIGN_LDS_BYTES + WTZ_WINALIGN_QW_BYTES);
#else
	uint32_t *d_defer = NULL, n_def = 0; CHK(dev_alloc((void**)&d_defer, ((size_t)n + 1) * 4)); CHK(dev_set(d_defer, 0, 4));
	if(d_list) CHK(wtz_launch_coop<K_winalign>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_winalign<false>((uint32_t)t, V, d_wt, d_items, d_defer, d_list); }, WTZ_WINALIGN_LDS_BYTES + WTZ_WINALIGN_QW_BYTES));
	else CHK(wtz_launch_coop<K_winalign>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_winalign<false>((uint32_t)t, V, d_wt, d_items, d_defer, NULL); }, WTZ_WINALIGN_LDS_BYTES + WTZ_WINALIGN_QW_BYTES));
	CHK(dev_d2h(&n_def, d_defer, 4));
	if(n_def) CHK(wtz_launch_coop<K_winalign_big>(n_def, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_winalign<true>((uint32_t)t, V, d_wt, d_items, NULL, d_defer); }, WTZ_WINALIGN_LDS_BYTES + WTZ_WINALIGN_QW_BYTES));
	if(n_redone) *n_redone = n_def;
	return WTZ_OK;
#endif
}

/* WTZ_WINALIGN_LANE=2: every window was aligned by the lane pipeline (rb) AND by the chained kernel (ra): any difference is fatal */
static int compare_lane_with_chained(const wtz_reg_t *ra, const wtz_reg_t *rb, uint64_t nreg){
	unsigned int *d_bad = NULL; CHK(dev_alloc((void**)&d_bad, 16)); CHK(dev_set(d_bad, 0, 16));
	CHK(wtz_launch<K_misc>(nreg, [=] WTZ_LAMBDA (uint64_t i){
		const wtz_reg_t &a = ra[i], &b = rb[i];
		bool same = a.pass == 2 || b.pass == 2 || (a.x.score == b.x.score && a.x.tb == b.x.tb && a.x.te == b.x.te && a.x.qb == b.x.qb && a.x.qe == b.x.qe && a.x.aln == b.x.aln && a.x.mat == b.x.mat && a.x.mis == b.x.mis && a.x.ins == b.x.ins && a.x.del == b.x.del && a.pass == b.pass && a.cigar_len == b.cigar_len && (a.cells == b.cells || a.cells == 0 || b.cells == 0));      /* pass 2 = scratch exhausted (reported as such); the host emulation's scalar body does not count cells */
		if(same && a.pass != 2 && b.pass != 2) for(uint32_t k = 0; k < a.cigar_len; k++) if(a.cigar[k] != b.cigar[k]){ same = false; break; }
		if(!same){ const unsigned int z = WTZ_ATOMIC_INC32(&d_bad[0]); if(z == 0) d_bad[1] = (unsigned int)i; }
	}));
	unsigned int hb[4]; CHK(dev_d2h(hb, d_bad, 16));
	if(hb[0]){
		wtz_reg_t a, b; CHK(dev_d2h(&a, ra + hb[1], sizeof a)); CHK(dev_d2h(&b, rb + hb[1], sizeof b));
		return wtz_fail(WTZ_E_STATE, "K-sw1 lane pipeline differs from the chained kernel on %u of %llu windows; first: window slot %u chained/lane score %d/%d tb %d/%d te %d/%d qb %d/%d qe %d/%d aln %d/%d mat %d/%d mis %d/%d ins %d/%d del %d/%d cigar %u/%u pass %u/%u cells %llu/%llu",
			hb[0], (unsigned long long)nreg, hb[1], a.x.score, b.x.score, a.x.tb, b.x.tb, a.x.te, b.x.te, a.x.qb, b.x.qb, a.x.qe, b.x.qe, a.x.aln, b.x.aln, a.x.mat, b.x.mat, a.x.mis, b.x.mis, a.x.ins, b.x.ins, a.x.del, b.x.del, a.cigar_len, b.cigar_len, a.pass, b.pass, a.cells, b.cells);
	}
	return WTZ_OK;
}

/* K-sw2 on a wavefront for the window slots listed behind d_glist[0] (d_glist == NULL: all nwt slots); gaps whose band outgrew the register forms (repeats) are
 * redone by the LDS-ring wave DP with 8192-column rings, 72 KB of LDS per wave.  Launches on the calling thread's current stream. */
static int run_gap_wave(wtz_ctx *c, const wtz_env_t &V, const wtz_wintask_t *d_wt, const wtz_alnitem_t *d_items, wtz_gapres_t *d_gaps, const uint32_t *d_glist, uint32_t n_glist, uint64_t nwt){
#ifdef WTZ_EMUL
	(void)nwt;      /* the emulation keeps the one instantiation that reads both costs */
	(void)c;
	return wtz_launch_coop<K_gap>(n_glist, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_gap((uint32_t)t, V, d_wt, d_items, d_gaps, (uint32_t*)NULL, (const uint32_t*)d_glist); }, WTZ_GAP_LDS_BYTES);
#else
	uint32_t *d_defer = NULL, n_def = 0; CHK(dev_alloc((void**)&d_defer, (size_t)(nwt + 1) * 4)); CHK(dev_set(d_defer, 0, 4));
	STAGE(c, "K_gap");
	if(ext_split(c)) CHK(wtz_launch_coop<K_gap>(n_glist, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_gap<true>((uint32_t)t, V, d_wt, d_items, d_gaps, d_defer, (const uint32_t*)d_glist, 0u); }, WTZ_GAP_LDS_BYTES));
	else CHK(wtz_launch_coop<K_gap>(n_glist, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_gap<false>((uint32_t)t, V, d_wt, d_items, d_gaps, d_defer, (const uint32_t*)d_glist, 0u); }, WTZ_GAP_LDS_BYTES));
	CHK(dev_d2h(&n_def, d_defer, 4));
	if(n_def) CHK(wtz_launch_coop<K_gap_wide>(n_def, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_gap((uint32_t)t, V, d_wt, d_items, d_gaps, NULL, d_defer, (uint32_t)WTZ_GAP_WIDE_LDS_BYTES); }, WTZ_GAP_WIDE_LDS_BYTES));
	if(c->sw.profile){ CHK(dev_sync()); fprintf(stderr, "[gap-profile] %llu window slots, %u wide gaps redone with 72 KB of LDS\n", (unsigned long long)nwt, n_def); }
	return WTZ_OK;
#endif
}

#ifdef WTZ_EMUL
/* host emulation: the prediction of the right extension's geometry (wtz_task_stitch_left's rgeo, what the product's fused launch is planned from) is compared with what K_stitch_mid asks for */
static int check_right_geometry(const int32_t *d_rgeo, const wtz_extjob_t *d_jr, const wtz_stitch_state_t *d_st, uint32_t m){
	for(uint32_t t = 0; t < m; t++){
		const wtz_extjob_t &jr = d_jr[t];
		const int32_t pq = d_rgeo[2 * (size_t)t], pt = d_rgeo[2 * (size_t)t + 1];
		if(jr.valid ? (pq != jr.qlen || pt != jr.tlen) : (pq >= 0 && !d_st[t].bad))
			return wtz_fail(WTZ_E_STATE, "stitch: predicted right extension of item %u (%d x %d) differs from the one K_stitch_mid asks for (valid %u: %d x %d)", t, pq, pt, jr.valid, jr.qlen, jr.tlen);
	}
	return WTZ_OK;
}
#endif

/* prepare items, K-sw1, stitch-left, K-sw2, extensions, stitch-mid, extensions, fin, refine, unpack */
extern "C" int wtz_pairs_align(wtz_ctx_t *c, const uint32_t *pair_idx, const uint8_t *dir, uint32_t m, wtz_aln_result_t *out){
	if(!c || !c->have_pairs) return wtz_fail(WTZ_E_STATE, "wtz_pairs_align before wtz_pairs_seed");
	if(m == 0) return WTZ_OK;
	CTX_ENTER(c);
	if(!pair_idx || !dir || !out) return wtz_fail(WTZ_E_ARG, "null argument");
	c->n_items = 0; c->have_items = false;
	const bool prof_wall = c->sw.profile; double tw[6] = {0, 0, 0, 0, 0, 0}; double tw0 = prof_wall ? wtz_wall() : 0;
	auto lapw = [&](int k){ if(prof_wall){ const double t = wtz_wall(); tw[k] += t - tw0; tw0 = t; } };
	CHK(reserve_items(c, m));
	std::vector<wtz_alnitem_t> items(m); uint64_t nreg = 0;      /* the window tasks (item, window) are listed on the device: one per region slot, in slot order */
	std::vector<uint32_t> h_q(c->n_pairs), h_c(c->n_pairs);
	CHK(dev_d2h(h_q.data(), c->d_qid, (size_t)c->n_pairs * 4)); CHK(dev_d2h(h_c.data(), c->d_cid, (size_t)c->n_pairs * 4));
	for(uint32_t i = 0; i < m; i++){
		if(pair_idx[i] >= c->n_pairs || dir[i] > 1) return wtz_fail(WTZ_E_ARG, "align item %u out of range", i);
		const wtz_pairres_t &r = c->h_pairres[pair_idx[i]];
		wtz_alnitem_t it; it.q = h_q[pair_idx[i]]; it.c = h_c[pair_idx[i]]; it.dir = dir[i];
		it.win = r.win[dir[i]]; it.anchors = r.anchors[dir[i]]; it.nwin = r.nwin[dir[i]]; it.regs = (wtz_reg_t*)(uintptr_t)nreg;
		nreg += it.nwin; items[i] = it;
	}
	const uint64_t nwt = (size_t)nreg;
	wtz_reg_t *d_regs = NULL; wtz_alnitem_t *d_items = NULL; wtz_wintask_t *d_wt = NULL;
	CHK(dev_alloc((void**)&d_regs, (size_t)(nreg + 1) * sizeof(wtz_reg_t)));
	for(uint32_t i = 0; i < m; i++) items[i].regs = d_regs + (uintptr_t)items[i].regs;
	CHK(dev_alloc((void**)&d_items, (size_t)m * sizeof(wtz_alnitem_t))); CHK(dev_h2d(d_items, items.data(), (size_t)m * sizeof(wtz_alnitem_t)));
	CHK(dev_alloc((void**)&d_wt, (size_t)(nreg + 1) * sizeof(wtz_wintask_t)));
	{ const wtz_alnitem_t *di = d_items; wtz_wintask_t *dw = d_wt; const wtz_reg_t *r0 = d_regs;
	  CHK(wtz_launch<K_misc>(m, [=] WTZ_LAMBDA (uint64_t i){ const wtz_alnitem_t &it = di[i]; wtz_wintask_t *w = dw + (it.regs - r0); for(uint32_t k = 0; k < it.nwin; k++){ w[k].item = (uint32_t)i; w[k].widx = k; } })); }
	const wtz_env_t V = ctx_env(c); wtz_alnres_dev_t *d_res = c->d_alnres;
	lapw(0);
	/* K-sw1: the windows */
	wtz_timer tm; tm.start();
	wtz_reg_t *d_regs_chk = NULL;
	if(c->sw.lane){
		/* one lane per K-sw1 problem (wtz_sw_lane.h); what it leaves (d_fb) goes through the chained kernel */
		uint32_t *d_fb = NULL, n_fb = 0;
		CHK(dev_alloc((void**)&d_fb, (nwt + 1) * 4));
		STAGE(c, "K-sw1 lane pipeline");
		CHK(run_winalign_lane(c, V, d_wt, nwt, d_items, d_fb, &n_fb));
		CHK(run_winalign_chained(c, V, d_wt, d_items, d_fb, n_fb));
		if(c->sw.lane == 2){ CHK(dev_sync()); CHK(dev_alloc((void**)&d_regs_chk, (size_t)(nreg + 1) * sizeof(wtz_reg_t))); CHK(dev_d2d(d_regs_chk, d_regs, (size_t)nreg * sizeof(wtz_reg_t))); }
	}
	if(c->sw.lane == 0 || c->sw.lane == 2){
		uint32_t n_redone = 0;
		STAGE(c, "K_winalign");
		CHK(run_winalign_chained(c, V, d_wt, d_items, NULL, nwt, &n_redone));
		if(c->sw.profile) fprintf(stderr, "[winalign-profile] %zu windows, %u redone by the full task\n", (size_t)nreg, n_redone);
	}
	CHK(dev_sync());
	if(d_regs_chk) CHK(compare_lane_with_chained(d_regs, d_regs_chk, nreg));
	c->cnt.ms_winalign += tm.stop(); c->cnt.n_winalign += (size_t)nreg;
	lapw(1);
	tm.start();
	wtz_stitch_state_t *d_st = NULL; wtz_extjob_t *d_jl = NULL, *d_jr = NULL; wtz_gapres_t *d_gaps = NULL; int32_t *d_rgeo = NULL;
	CHK(dev_alloc((void**)&d_st, (size_t)m * sizeof(wtz_stitch_state_t)));
	CHK(dev_alloc((void**)&d_jl, (size_t)m * sizeof(wtz_extjob_t))); CHK(dev_alloc((void**)&d_jr, (size_t)m * sizeof(wtz_extjob_t)));
	CHK(dev_alloc((void**)&d_gaps, (size_t)(nreg + 1) * sizeof(wtz_gapres_t)));
#ifndef WTZ_EMUL
	const bool fused = c->sw.ext_fused && c->sw.sw_mode == 0, gap_side = c->sw.gap_side != 0;      /* both end extensions on one wavefront (run_stitch_fused) / K-sw2 on its own stream */
	if(fused) CHK(dev_alloc((void**)&d_rgeo, (size_t)m * 8));
#else
	const bool fused = false, gap_side = false;
	CHK(dev_alloc((void**)&d_rgeo, (size_t)m * 8));      /* for check_right_geometry */
#endif
	STAGE(c, "K_stitch_left");
	CHK(wtz_launch_wave<K_stitch_left>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_stitch_left((uint32_t)t, V, d_items, d_st, d_jl, d_rgeo); }));
	/* K-sw2: the gaps between the windows, lane pipeline + wavefront kernel */
	uint32_t *d_glist = NULL, n_glist = (uint32_t)nwt;
	wtz_timer tgap; tgap.start();
	if(c->sw.gap_lane){
		CHK(dev_alloc((void**)&d_glist, (size_t)(nwt + 1) * 4));
		STAGE(c, "K-sw2 lane pipeline");
		CHK(run_gap_lane(c, V, d_wt, nwt, d_items, d_gaps, d_glist, &n_glist));
	}
#ifndef WTZ_EMUL
	/* the gaps between windows (many short K-sw2 tasks) and the left extensions (few long K-sw3 jobs) are independent: the
	 * gap kernel can run on its own stream and fill the CUs the extension tail leaves idle; stitch_mid waits for both */
	/* measured: ~5 ms of 150 on the E. coli shape, inside run-to-run noise, and it folds K_gap's contention into the K-sw3 stage
	 * time that bench.py reports against the roofline -> opt-in (WTZ_GAP_SIDESTREAM=1) */
	if(gap_side){ HIPCHK(hipEventRecord(c->ev_gap_fork, g_stream)); HIPCHK(hipStreamWaitEvent(c->stream_gap, c->ev_gap_fork, 0)); }
	{ wtz_stream_scope on_gap_stream(gap_side ? c->stream_gap : g_stream); CHK(run_gap_wave(c, V, d_wt, d_items, d_gaps, d_glist, n_glist, nwt)); }
	if(gap_side) HIPCHK(hipEventRecord(c->ev_gap_join, c->stream_gap));
#else
	CHK(run_gap_wave(c, V, d_wt, d_items, d_gaps, d_glist, n_glist, nwt));
#endif
	if(!gap_side) tgap.lap();
	/* K-sw3: the two end extensions with K_stitch_mid between them */
#ifndef WTZ_EMUL
	if(fused){
		if(gap_side) HIPCHK(hipStreamWaitEvent(g_stream, c->ev_gap_join, 0));      /* the join inside the fused launch reads the gaps */
		STAGE(c, "extjobs left + join + right on one wavefront"); CHK(run_stitch_fused(c, V, d_items, d_st, d_jl, d_jr, d_gaps, d_rgeo, m));
	}
#endif
	STAGE(c, "extjobs left");
	CHK(run_extjobs(c, V, d_jl, m, fused));
#ifndef WTZ_EMUL
	if(gap_side) HIPCHK(hipStreamWaitEvent(g_stream, c->ev_gap_join, 0));
#endif
	if(!gap_side) c->cnt.ms_gap += tgap.read();      /* after the extension jobs: no extra synchronisation for the lap */
	STAGE(c, "K_stitch_mid");
	CHK(wtz_launch_coop<K_stitch_mid>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_stitch_mid((uint32_t)t, V, d_items, d_st, d_jl, d_jr, d_gaps); }));
	STAGE(c, "extjobs right");
#ifdef WTZ_EMUL
	CHK(check_right_geometry(d_rgeo, d_jr, d_st, m));
#endif
	CHK(run_extjobs(c, V, d_jr, m, fused));
	STAGE(c, "K_stitch_fin");
	CHK(wtz_launch_coop<K_stitch_fin>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_stitch_fin((uint32_t)t, V, d_items, d_st, d_jl, d_jr, d_res); }));
	if(c->P.refine) STAGE(c, "K_refine");
	if(c->P.refine) CHK(wtz_launch_coop<K_refine>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_refine((uint32_t)t, V, d_items, d_res); }, WTZ_REFINE_LDS_BYTES));
	CHK(dev_sync());
	c->cnt.ms_stitch += tm.stop(); c->cnt.n_stitch += m;
	lapw(2);
	c->h_alnres.resize(m); c->n_items = m; c->have_items = true;
	CHK(dev_d2h(c->h_alnres.data(), c->d_alnres, (size_t)m * sizeof(wtz_alnres_dev_t)));
	CHK(pool_check(c, "wtz_pairs_align"));
	uint64_t coff = 0, toff = 0;
	for(uint32_t i = 0; i < m; i++){
		const wtz_alnres_dev_t &r = c->h_alnres[i];
		if(r.bad) return wtz_fail(WTZ_E_POOL, "wtz_pairs_align: item %u ran out of scratch", i);
		wtz_aln_result_t o; memset(&o, 0, sizeof o);
		o.score = r.x.score; o.tb = r.x.tb; o.te = r.x.te; o.qb = r.x.qb; o.qe = r.x.qe; o.aln = r.x.aln; o.mat = r.x.mat; o.mis = r.x.mis; o.ins = r.x.ins; o.del = r.x.del;
		o.n_regs = r.n_regs; o.cigar_len = r.cigar_len; o.cigar_off = coff; coff += r.cigar_len; o.text_len = r.text_len; o.text_off = toff; toff += r.text_len;
		c->cnt.cells_shift += r.cells_shift; c->cnt.cells_fixed += r.cells_fixed; c->cnt.cells_global += r.cells_global;
		out[i] = o;
	}
	lapw(3);
	if(prof_wall) fprintf(stderr, "[align-profile] %u items: host wall ms prep %.2f winalign %.2f stitch %.2f results %.2f\n", m, tw[0] * 1e3, tw[1] * 1e3, tw[2] * 1e3, tw[3] * 1e3);
	return WTZ_OK;
}
