/*
 * wtz_lib_index.h — what is built once per read set: reads upload and on-device ingest (f4), the k-mer index (A2, whole and sharded),
 * the z-mer index of every read (A5) and the candidate search (A3).  Included by wtz_lib.cpp.
 */
extern "C" int wtz_upload_reads(wtz_ctx_t *c, const uint64_t *bits, uint64_t n_words, const uint64_t *rdoff, const uint32_t *rdlen, uint32_t n_reads){
	if(!c || !bits || !rdoff || !rdlen) return wtz_fail(WTZ_E_ARG, "null argument");
	CTX_ENTER(c);
	if(c->shares_indexes) return wtz_fail(WTZ_E_STATE, "wtz_upload_reads on a cloned context");
	dev_free_persist(c->bits); dev_free_persist(c->rdoff); dev_free_persist(c->rdlen); c->bits = NULL; c->rdoff = NULL; c->rdlen = NULL;
	free_kindex(c); free_zindex(c); free_batch(c);
	CHK(dev_alloc_persist((void**)&c->bits, (n_words + 2) * 8)); CHK(dev_set(c->bits, 0, (n_words + 2) * 8)); CHK(dev_h2d(c->bits, bits, n_words * 8));
	CHK(dev_alloc_persist((void**)&c->rdoff, (size_t)n_reads * 8)); CHK(dev_h2d(c->rdoff, rdoff, (size_t)n_reads * 8));
	CHK(dev_alloc_persist((void**)&c->rdlen, (size_t)n_reads * 4)); CHK(dev_h2d(c->rdlen, rdlen, (size_t)n_reads * 4));
	c->n_words = n_words; c->n_reads = n_reads; c->h_rdlen.assign(rdlen, rdlen + n_reads);
	return WTZ_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* f4: FASTA -> 2-bit on the device (seq2basebank, dna.h:397-410)                                    */
/* ------------------------------------------------------------------------------------------------ */
#include "wtz_ingest.h"
#ifndef WTZ_EMUL
/* dedicated streaming kernel: 256 threads, grid-stride over the HALF words of the chunk with four loads in flight per thread: a wave reads
 * 1 KB of text per instruction (16 bytes per lane, lanes contiguous) and writes 256 B of the bank (4 bytes per lane; the two halves of a
 * 64-bit word swap places: little-endian words, first base in the top bits) */
__global__ void __launch_bounds__(256) wtz_kernel_pack_ascii(const uint8_t *ascii, uint64_t n, uint64_t n_half, uint32_t *bits32, unsigned long long *n_pos, uint64_t *pos, uint64_t pos_cap, uint64_t pos_base){
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	for(; h + 3 * stride < n_half; h += 4 * stride){
		const uint32_t a = wtz_pack_half(ascii, n, h, n_pos, pos, pos_cap, pos_base), b = wtz_pack_half(ascii, n, h + stride, n_pos, pos, pos_cap, pos_base);
		const uint32_t c = wtz_pack_half(ascii, n, h + 2 * stride, n_pos, pos, pos_cap, pos_base), d = wtz_pack_half(ascii, n, h + 3 * stride, n_pos, pos, pos_cap, pos_base);
		bits32[h ^ 1] = a; bits32[(h + stride) ^ 1] = b; bits32[(h + 2 * stride) ^ 1] = c; bits32[(h + 3 * stride) ^ 1] = d;
	}
	for(; h < n_half; h += stride) bits32[h ^ 1] = wtz_pack_half(ascii, n, h, n_pos, pos, pos_cap, pos_base);
}
static int launch_pack_ascii(uint32_t nblk, const uint8_t *ascii, uint64_t n, uint64_t n_half, uint32_t *bits32, unsigned long long *n_pos, uint64_t *pos, uint64_t pos_cap, uint64_t pos_base){
	hipLaunchKernelGGL(wtz_kernel_pack_ascii, dim3(nblk), dim3(256), 0, g_stream, ascii, n, n_half, bits32, n_pos, pos, pos_cap, pos_base);
	if(hipGetLastError() != hipSuccess) return wtz_fail(WTZ_E_HIP, "wtz_kernel_pack_ascii launch failed");
	return WTZ_OK;
}
#endif
extern "C" int wtz_upload_reads_ascii(wtz_ctx_t *c, const char *seq, uint64_t n_bases, const uint64_t *rdoff, const uint32_t *rdlen, uint32_t n_reads, uint64_t rand_calls_before, uint64_t *n_random){
	if(!c || (!seq && n_bases) || !rdoff || !rdlen) return wtz_fail(WTZ_E_ARG, "null argument");
	CTX_ENTER(c);
	if(c->shares_indexes) return wtz_fail(WTZ_E_STATE, "wtz_upload_reads_ascii on a cloned context");
	dev_free_persist(c->bits); dev_free_persist(c->rdoff); dev_free_persist(c->rdlen); c->bits = NULL; c->rdoff = NULL; c->rdlen = NULL;
	free_kindex(c); free_zindex(c); free_batch(c);
	const uint64_t n_words = (n_bases + 31) / 32;
	c->n_words = 0; c->n_reads = 0; c->h_rdlen.clear();        /* "no reads uploaded" until the last chunk is packed: a failure below leaves the context in that state, not over a half-packed bank */
	const uint64_t CH = (uint64_t)256 << 20;             /* bases per chunk (a multiple of 32): 256 MB of text on the device at a time */
	uint8_t *d_txt = NULL; unsigned long long *d_np = NULL; uint64_t *d_pos = NULL; uint64_t pos_cap = (uint64_t)1 << 20;
	int rc = WTZ_OK;
	if((rc = dev_alloc_persist((void**)&c->bits, (n_words + 2) * 8)) || (rc = dev_set(c->bits, 0, (n_words + 2) * 8)) ||
	   (rc = dev_alloc_persist((void**)&c->rdoff, (size_t)n_reads * 8)) || (rc = dev_h2d(c->rdoff, rdoff, (size_t)n_reads * 8)) ||
	   (rc = dev_alloc_persist((void**)&c->rdlen, (size_t)n_reads * 4)) || (rc = dev_h2d(c->rdlen, rdlen, (size_t)n_reads * 4)) ||
	   (rc = dev_alloc_persist((void**)&d_txt, (size_t)WTZ_MIN(CH, n_bases) + 64)) || (rc = dev_alloc_persist((void**)&d_np, 16)) || (rc = dev_alloc_persist((void**)&d_pos, pos_cap * 8))){
		dev_free_persist(d_txt); dev_free_persist(d_np); dev_free_persist(d_pos);
		dev_free_persist(c->bits); dev_free_persist(c->rdoff); dev_free_persist(c->rdlen); c->bits = NULL; c->rdoff = NULL; c->rdlen = NULL;
		return rc;
	}
	uint64_t rank = rand_calls_before;
#ifndef WTZ_EMUL
	/* an empty launch first: the first kernel launch of a process loads the library's code object (several ms), which is not this kernel's time */
	(void)launch_pack_ascii(1, (const uint8_t*)d_txt, 0, 0, (uint32_t*)c->bits, d_np, d_pos, pos_cap, 0);
	(void)hipStreamSynchronize(g_stream);
#endif
	for(uint64_t b0 = 0; b0 < n_bases && rc == WTZ_OK; b0 += CH){
		const uint64_t nb = WTZ_MIN(CH, n_bases - b0), nw = (nb + 31) / 32;
		if((rc = dev_h2d(d_txt, seq + b0, (size_t)nb))) break;
		for(;;){
			if((rc = dev_set(d_np, 0, 16))) break;
			uint64_t *bits = c->bits + b0 / 32; unsigned long long *np = d_np; uint64_t *pos = d_pos; const uint8_t *txt = d_txt; const uint64_t cap = pos_cap;
			wtz_timer tm; tm.start();
#ifndef WTZ_EMUL
			{ const uint64_t nh = nw * 2; uint64_t nblk = (nh + 1023) / 1024; if(nblk > 256 * 32) nblk = 256 * 32; if(nblk < 1) nblk = 1;      /* at most 32 workgroups per CU; stride is even, so h ^ 1 stays inside the chunk's words */
			  if((rc = launch_pack_ascii((uint32_t)nblk, txt, nb, nh, (uint32_t*)bits, np, pos, cap, b0))) break; }
#else
			for(uint64_t h = 0; h < nw * 2; h++) ((uint32_t*)bits)[h ^ 1] = wtz_pack_half(txt, nb, h, np, pos, cap, b0);
#endif
			c->cnt.ms_ingest += tm.stop();                          /* HIP events around the kernel alone */
			unsigned long long cnt = 0;
			if((rc = dev_d2h(&cnt, d_np, 8))) break;
			if(cnt > pos_cap){       /* more non-bases than the list holds: grow it and pack the chunk again */
				dev_free_persist(d_pos); d_pos = NULL; pos_cap = cnt + cnt / 4;
				if((rc = dev_alloc_persist((void**)&d_pos, pos_cap * 8))) break;
				continue;
			}
			if(cnt){
				std::vector<uint64_t> hp((size_t)cnt);
				if((rc = dev_d2h(hp.data(), d_pos, (size_t)cnt * 8))) break;
				std::sort(hp.begin(), hp.end());                    /* file order = ascending position */
				if((rc = dev_h2d(d_pos, hp.data(), (size_t)cnt * 8))) break;
				uint64_t *allbits = c->bits; const uint64_t r0 = rank;
				wtz_timer tf; tf.start();
				if((rc = wtz_launch<K_pack_fix>(cnt, [=] WTZ_LAMBDA (uint64_t r){ wtz_fix_random_base(r, pos, r0, allbits); }))) break;
				if((rc = dev_sync())) break;
				c->cnt.ms_ingest += tf.stop();
				rank += cnt;
			}
			break;
		}
	}
	dev_free_persist(d_txt); dev_free_persist(d_np); dev_free_persist(d_pos);
	if(rc != WTZ_OK){ dev_free_persist(c->bits); dev_free_persist(c->rdoff); dev_free_persist(c->rdlen); c->bits = NULL; c->rdoff = NULL; c->rdlen = NULL; return rc; }
	c->n_words = n_words; c->n_reads = n_reads; c->h_rdlen.assign(rdlen, rdlen + n_reads);
	c->cnt.bytes_ingest_algo += n_bases + n_words * 8;
	if(n_random) *n_random = rank - rand_calls_before;
	return WTZ_OK;
}
extern "C" int wtz_append_revcomp_views(wtz_ctx_t *c){
	if(!c || !c->bits) return wtz_fail(WTZ_E_ARG, "reads not uploaded");
	CTX_ENTER(c);
	if(c->shares_indexes) return wtz_fail(WTZ_E_STATE, "wtz_append_revcomp_views on a cloned context");
	free_kindex(c); free_zindex(c); free_batch(c);
	const uint32_t n = c->n_reads;
	if((uint64_t)n * 2 > 0xFFFFFFFFull) return wtz_fail(WTZ_E_ARG, "too many reads for their reverse-complement views");
	std::vector<uint64_t> h_off((size_t)n * 2), vw((size_t)n + 1);      /* vw[i] = first word of view i behind the old bank */
	CHK(dev_d2h(h_off.data(), c->rdoff, (size_t)n * 8));
	uint64_t words = 0;
	for(uint32_t i = 0; i < n; i++){ vw[i] = words; words += ((uint64_t)c->h_rdlen[i] + 31) / 32; }
	vw[n] = words;
	const uint64_t old_w = c->n_words, new_w = old_w + words;
	uint64_t *nb = NULL; uint64_t *nro = NULL; uint32_t *nrl = NULL;
	CHK(dev_alloc_persist((void**)&nb, (new_w + 2) * 8)); CHK(dev_set(nb + old_w, 0, (words + 2) * 8)); CHK(dev_d2d(nb, c->bits, old_w * 8));
	std::vector<uint32_t> h_len((size_t)n * 2);
	for(uint32_t i = 0; i < n; i++){ h_len[i] = c->h_rdlen[i]; h_len[n + i] = c->h_rdlen[i]; h_off[n + i] = (old_w + vw[i]) * 32; }
	CHK(dev_alloc_persist((void**)&nro, (size_t)n * 2 * 8)); CHK(dev_h2d(nro, h_off.data(), (size_t)n * 2 * 8));
	CHK(dev_alloc_persist((void**)&nrl, (size_t)n * 2 * 4)); CHK(dev_h2d(nrl, h_len.data(), (size_t)n * 2 * 4));
	uint64_t *d_vw = NULL; CHK(dev_alloc((void**)&d_vw, ((size_t)n + 1) * 8)); CHK(dev_h2d(d_vw, vw.data(), ((size_t)n + 1) * 8));
	const uint64_t *src = c->bits; const uint64_t *ro = nro; const uint32_t *rl = nrl; uint64_t *dst = nb + old_w;
	CHK(wtz_launch<K_revcomp_views>(words, [=] WTZ_LAMBDA (uint64_t w){
		uint32_t lo = 0, hi = n;                         /* the view that holds word w: last i with vw[i] <= w */
		while(hi - lo > 1){ const uint32_t mid = (lo + hi) >> 1; if(d_vw[mid] <= w) lo = mid; else hi = mid; }
		dst[w] = wtz_revcomp_word(src, ro[lo], rl[lo], (uint32_t)(w - d_vw[lo]));
	}));
	CHK(dev_sync());
	dev_free_persist(c->bits); dev_free_persist(c->rdoff); dev_free_persist(c->rdlen);
	c->bits = nb; c->rdoff = nro; c->rdlen = nrl; c->n_words = new_w; c->n_reads = n * 2; c->h_rdlen = h_len;
	return WTZ_OK;
}
extern "C" int wtz_fetch_read_bits(wtz_ctx_t *c, uint64_t *bits, uint64_t n_words){
	if(!c || !bits || !c->bits) return wtz_fail(WTZ_E_ARG, "reads not uploaded / null argument");
	if(n_words > c->n_words) return wtz_fail(WTZ_E_ARG, "wtz_fetch_read_bits: %llu words asked, %llu uploaded", (unsigned long long)n_words, (unsigned long long)c->n_words);
	CTX_ENTER(c);
	CHK(dev_d2h(bits, c->bits, (size_t)n_words * 8));
	return WTZ_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* A2: k-mer index                                                                                   */
/* ------------------------------------------------------------------------------------------------ */
extern "C" int wtz_index_build(wtz_ctx_t *c, uint32_t id_beg, uint32_t id_end, uint32_t *max_kmer_freq, wtz_index_stats_t *stats){
	if(!c || !c->bits || !max_kmer_freq) return wtz_fail(WTZ_E_ARG, "reads not uploaded / null argument");
	if(id_end > c->n_reads) id_end = c->n_reads;
	if(id_beg > id_end) id_beg = id_end;
	const uint32_t nr = id_end - id_beg;
	CTX_ENTER(c);
	if(c->shares_indexes) return wtz_fail(WTZ_E_STATE, "wtz_index_build on a cloned context");
	const bool prof_ix = c->sw.profile; double tix[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tix0 = wtz_wall();
	auto lapix = [&](int k){ if(prof_ix){ (void)dev_sync(); const double t = wtz_wall(); tix[k] += t - tix0; tix0 = t; } };
	free_kindex(c);
	lapix(0);
	wtz_timer tm; tm.start();
	const wtz_reads_t R = ctx_reads(c); const uint32_t ksize = c->P.ksize, hk = c->P.hk, ksave = c->P.ksave;
	/* the walk of a read is a serial recurrence, but it restarts exactly anywhere (wtz_walk_warm_start): one lane per
	 * WTZ_WALK_CHUNK-base piece instead of one per read, pieces listed in read order */
	std::vector<uint32_t> p_rid, p_jb;
	for(uint32_t r = id_beg; r < id_end; r++) for(uint32_t jb = 0; jb == 0 || jb < c->h_rdlen[r]; jb += WTZ_WALK_CHUNK){ p_rid.push_back(r); p_jb.push_back(jb); }
	const size_t np = p_rid.size();
	uint32_t *d_prid = NULL, *d_pjb = NULL;
	CHK(dev_alloc((void**)&d_prid, (np + 1) * 4)); CHK(dev_alloc((void**)&d_pjb, (np + 1) * 4));
	CHK(dev_h2d(d_prid, p_rid.data(), np * 4)); CHK(dev_h2d(d_pjb, p_jb.data(), np * 4));
	lapix(1);
	uint64_t *d_cnt = NULL; CHK(dev_alloc((void**)&d_cnt, (np + 1) * 8));
	CHK(wtz_launch<K_kcount>(np, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_kcount((uint32_t)t, R, d_prid, d_pjb, ksize, hk, ksave, d_cnt); }));
	std::vector<uint64_t> h_cnt(np + 1);
	CHK(dev_d2h(h_cnt.data(), d_cnt, np * 8));
	uint64_t tot = 0; for(size_t i = 0; i < np; i++){ uint64_t v = h_cnt[i]; h_cnt[i] = tot; tot += v; } h_cnt[np] = tot;
	CHK(dev_h2d(d_cnt, h_cnt.data(), (np + 1) * 8));
	lapix(2);
	uint64_t *d_keys = NULL; uint32_t *d_vals = NULL;
	CHK(dev_alloc((void**)&d_keys, (tot + 1) * 8)); CHK(kalloc(c, 1, (void**)&d_vals, (tot + 1) * 4));
	lapix(3);
	CHK(wtz_launch<K_kfill>(np, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_kfill((uint32_t)t, R, d_prid, d_pjb, ksize, hk, ksave, d_cnt, d_keys, d_vals); }));
	CHK(dev_sync());
	(void)nr;
	lapix(4);
	CHK(dev_sort_pairs_u64_u32(d_keys, d_vals, tot, 2 * ksize));
	lapix(5);
	unsigned long long *d_stat = NULL; CHK(dev_alloc((void**)&d_stat, 4 * 8)); CHK(dev_set(d_stat, 0, 4 * 8));
	const uint64_t n_str = tot < (1ull << 18) ? (tot ? tot : 1) : (1ull << 18);      /* strided counting passes: one atomic per wavefront at the end */
	CHK(wtz_launch<K_kstats>(n_str, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_kstats_stride(t, n_str, d_keys, tot, d_stat + 0, d_stat + 1); }));
	unsigned long long h_stat[4]; CHK(dev_d2h(h_stat, d_stat, 4 * 8));
	const uint64_t ktot = tot - h_stat[0], ktyp = h_stat[1];     /* d_stat[0] accumulates the saturation excess */
	uint32_t K = *max_kmer_freq;
	if(K < 2){ uint32_t kavg = (uint32_t)(ktot / (ktyp + 1)); if(kavg < 20) kavg = 20; K = kavg * 5; }       /* wtzmo.c:380-393 */
	*max_kmer_freq = K;
	CHK(wtz_launch<K_kinsert>(n_str, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_kkept_stride(t, n_str, d_keys, tot, K, d_stat + 2); }));
	CHK(dev_d2h(h_stat, d_stat, 4 * 8));
	const uint64_t n_kept = h_stat[2];
	uint64_t cap = 1024; while(cap < n_kept * 2 + 2) cap <<= 1;
	CHK(kalloc(c, 0, (void**)&c->ktab, cap * sizeof(wtz_kslot_t))); CHK(dev_set(c->ktab, 0xFF, cap * sizeof(wtz_kslot_t)));
	c->kmask = cap - 1;
	wtz_kslot_t *tab = c->ktab; const uint64_t kmask = c->kmask;
	CHK(wtz_launch<K_kinsert>(tot, [=] WTZ_LAMBDA (uint64_t i){ wtz_task_kinsert(i, d_keys, tot, K, tab, kmask, d_stat + 2); }));
	CHK(dev_sync());
	c->kseeds = d_vals; c->n_kocc = tot;
	c->idx_beg = id_beg; c->idx_end = id_end; c->idx_len_sorted = true;
	for(uint32_t r = id_beg; r + 1 < id_end; r++) if(c->h_rdlen[r] < c->h_rdlen[r + 1]){ c->idx_len_sorted = false; break; }
	c->cnt.ms_index += tm.stop();
	lapix(6);
	if(prof_ix) fprintf(stderr, "[index-profile] ms: free %.1f pieces+h2d %.1f count %.1f alloc %.1f fill %.1f sort %.1f table %.1f\n", tix[0] * 1e3, tix[1] * 1e3, tix[2] * 1e3, tix[3] * 1e3, tix[4] * 1e3, tix[5] * 1e3, tix[6] * 1e3);
	if(stats){
		stats->n_occ = tot; stats->n_distinct = ktyp; stats->ktot = ktot; stats->n_kept = n_kept; stats->max_kmer_freq = K;
		uint64_t tl = 0; for(uint32_t i = 0; i < c->n_reads; i++) tl += c->h_rdlen[i];
		stats->avg_rdlen = c->n_reads ? (uint32_t)(tl / c->n_reads) : 10000;
	}
	return WTZ_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* A2 sharded by read-id range (see include/wtzmo_hip.h)                                             */
/* ------------------------------------------------------------------------------------------------ */
static void free_pending_index(wtz_ctx *c){
	dev_free_persist(c->pend_keys); dev_free_persist(c->pend_vals); dev_free_persist(c->pend_dk); dev_free_persist(c->pend_dc); dev_free_persist(c->pend_dstart);
	c->pend_keys = NULL; c->pend_vals = NULL; c->pend_dk = NULL; c->pend_dc = NULL; c->pend_dstart = NULL; c->pend_tot = 0; c->pend_nd = 0;
}
extern "C" int wtz_index_count(wtz_ctx_t *c, uint32_t id_beg, uint32_t id_end, uint64_t *n_distinct, uint64_t *n_occ){
	if(!c || !c->bits || !n_distinct) return wtz_fail(WTZ_E_ARG, "reads not uploaded / null argument");
	if(id_end > c->n_reads) id_end = c->n_reads;
	if(id_beg > id_end) id_beg = id_end;
	CTX_ENTER(c);
	if(c->shares_indexes) return wtz_fail(WTZ_E_STATE, "wtz_index_count on a cloned context");
	free_kindex(c); free_pending_index(c);
	wtz_timer tm; tm.start();
	const wtz_reads_t R = ctx_reads(c); const uint32_t ksize = c->P.ksize, hk = c->P.hk, ksave = c->P.ksave;
	std::vector<uint32_t> p_rid, p_jb;
	for(uint32_t r = id_beg; r < id_end; r++) for(uint32_t jb = 0; jb == 0 || jb < c->h_rdlen[r]; jb += WTZ_WALK_CHUNK){ p_rid.push_back(r); p_jb.push_back(jb); }
	const size_t np = p_rid.size();
	uint32_t *d_prid = NULL, *d_pjb = NULL; uint64_t *d_cnt = NULL;
	CHK(dev_alloc((void**)&d_prid, (np + 1) * 4)); CHK(dev_alloc((void**)&d_pjb, (np + 1) * 4)); CHK(dev_alloc((void**)&d_cnt, (np + 1) * 8));
	CHK(dev_h2d(d_prid, p_rid.data(), np * 4)); CHK(dev_h2d(d_pjb, p_jb.data(), np * 4));
	CHK(wtz_launch<K_kcount>(np, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_kcount((uint32_t)t, R, d_prid, d_pjb, ksize, hk, ksave, d_cnt); }));
	std::vector<uint64_t> h_cnt(np + 1);
	CHK(dev_d2h(h_cnt.data(), d_cnt, np * 8));
	uint64_t tot = 0; for(size_t i = 0; i < np; i++){ uint64_t v = h_cnt[i]; h_cnt[i] = tot; tot += v; } h_cnt[np] = tot;
	CHK(dev_h2d(d_cnt, h_cnt.data(), (np + 1) * 8));
	if(tot >= 0xFFFFFFFFull) return wtz_fail(WTZ_E_ARG, "wtz_index_count: more than 2^32 k-mer occurrences in one shard; use more shards");
	CHK(dev_alloc_persist((void**)&c->pend_keys, (tot + 1) * 8)); CHK(dev_alloc_persist((void**)&c->pend_vals, (tot + 1) * 4));
	uint64_t *d_keys = c->pend_keys; uint32_t *d_vals = c->pend_vals;
	CHK(wtz_launch<K_kfill>(np, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_kfill((uint32_t)t, R, d_prid, d_pjb, ksize, hk, ksave, d_cnt, d_keys, d_vals); }));
	CHK(dev_sync());
	CHK(dev_sort_pairs_u64_u32(d_keys, d_vals, tot, 2 * ksize));
	uint32_t *d_flag = NULL, *d_dpos = NULL;
	CHK(dev_alloc((void**)&d_flag, (tot + 2) * 4)); CHK(dev_alloc((void**)&d_dpos, (tot + 2) * 4)); CHK(dev_set(d_flag, 0, (tot + 2) * 4));
	CHK(wtz_launch<K_khead>(tot, [=] WTZ_LAMBDA (uint64_t i){ wtz_task_khead(i, d_keys, d_flag); }));
	CHK(dev_exclusive_scan_u32(d_flag, d_dpos, tot + 1));
	uint32_t nd = 0; CHK(dev_d2h(&nd, d_dpos + tot, 4));
	CHK(dev_alloc_persist((void**)&c->pend_dk, ((size_t)nd + 1) * 8)); CHK(dev_alloc_persist((void**)&c->pend_dc, ((size_t)nd + 1) * 4)); CHK(dev_alloc_persist((void**)&c->pend_dstart, ((size_t)nd + 1) * 8));
	uint64_t *dk = c->pend_dk, *dst = c->pend_dstart; uint32_t *dc = c->pend_dc;
	CHK(wtz_launch<K_kdistinct>(tot, [=] WTZ_LAMBDA (uint64_t i){ wtz_task_kdistinct(i, d_keys, tot, d_flag, d_dpos, dk, dc, dst); }));
	CHK(dev_sync());
	c->pend_tot = tot; c->pend_nd = nd; c->pend_beg = id_beg; c->pend_end = id_end;
	c->cnt.ms_index += tm.stop();
	*n_distinct = nd; if(n_occ) *n_occ = tot;
	return WTZ_OK;
}
extern "C" int wtz_index_counts_fetch(wtz_ctx_t *c, uint64_t *kmers, uint32_t *cnts){
	if(!c || !kmers || !cnts) return wtz_fail(WTZ_E_ARG, "null argument");
	if(!c->pend_keys) return wtz_fail(WTZ_E_STATE, "wtz_index_counts_fetch before wtz_index_count");
	CTX_ENTER(c);
	CHK(dev_d2h(kmers, c->pend_dk, (size_t)c->pend_nd * 8)); CHK(dev_d2h(cnts, c->pend_dc, (size_t)c->pend_nd * 4));
	return WTZ_OK;
}
extern "C" int wtz_index_finish(wtz_ctx_t *c, const uint32_t *total_cnt, uint32_t K, uint64_t *n_kept_out){
	if(!c || (!total_cnt && c && c->pend_nd)) return wtz_fail(WTZ_E_ARG, "null argument");
	if(!c->pend_keys) return wtz_fail(WTZ_E_STATE, "wtz_index_finish before wtz_index_count");
	CTX_ENTER(c);
	wtz_timer tm; tm.start();
	const uint64_t nd = c->pend_nd;
	uint32_t *d_tc = NULL; unsigned long long *d_stat = NULL;
	CHK(dev_alloc((void**)&d_tc, (nd + 1) * 4)); CHK(dev_h2d(d_tc, total_cnt, nd * 4));
	CHK(dev_alloc((void**)&d_stat, 8)); CHK(dev_set(d_stat, 0, 8));
	const uint64_t *dk = c->pend_dk, *dst = c->pend_dstart; const uint32_t *dc = c->pend_dc;
	CHK(wtz_launch<K_kinsert_total>(nd, [=] WTZ_LAMBDA (uint64_t d){ wtz_task_kinsert_total(d, dk, dc, dst, d_tc, K, (wtz_kslot_t*)NULL, 0, d_stat); }));
	unsigned long long n_kept = 0; CHK(dev_d2h(&n_kept, d_stat, 8));
	uint64_t cap = 1024; while(cap < n_kept * 2 + 2) cap <<= 1;
	CHK(dev_alloc_persist((void**)&c->ktab, cap * sizeof(wtz_kslot_t))); CHK(dev_set(c->ktab, 0xFF, cap * sizeof(wtz_kslot_t)));
	c->kmask = cap - 1;
	wtz_kslot_t *tab = c->ktab; const uint64_t kmask = c->kmask;
	CHK(wtz_launch<K_kinsert_total>(nd, [=] WTZ_LAMBDA (uint64_t d){ wtz_task_kinsert_total(d, dk, dc, dst, d_tc, K, tab, kmask, d_stat); }));
	CHK(dev_sync());
	c->kseeds = c->pend_vals; c->pend_vals = NULL; c->n_kocc = c->pend_tot;
	c->idx_beg = c->pend_beg; c->idx_end = c->pend_end; c->idx_len_sorted = true;
	for(uint32_t r = c->idx_beg; r + 1 < c->idx_end; r++) if(c->h_rdlen[r] < c->h_rdlen[r + 1]){ c->idx_len_sorted = false; break; }
	free_pending_index(c);
	c->cnt.ms_index += tm.stop();
	if(n_kept_out) *n_kept_out = n_kept;
	return WTZ_OK;
}
extern "C" void wtz_cand_tail_host(const uint64_t *groups, uint32_t ng, uint32_t kovl, uint32_t ncand, uint64_t *heap, uint32_t *hn){ wtz_cand_tail(groups, ng, kovl, ncand, heap, hn); }

/* ------------------------------------------------------------------------------------------------ */
/* A5: z-mer index of every read                                                                     */
/* ------------------------------------------------------------------------------------------------ */
/* members == NULL: the z-index of every read.  Else (ascending read ids): of those reads only - every other read gets an empty slice, so the
 * kernels address the index exactly as before.  The subset form is rebuilt per batch of queries (their candidate sets bound what a batch
 * can look up), which is what lets a 10 Gbp read set (160 GB of z-index at 16 B per base) run in 288 GB: its arrays are allocated once
 * with head-room and reused. */
static int zindex_build_impl(wtz_ctx_t *c, const uint32_t *members, uint32_t nm, int slot = 0){
	if(!c || !c->bits) return wtz_fail(WTZ_E_ARG, "reads not uploaded");
	CTX_ENTER(c);
	if(c->shares_indexes) return wtz_fail(WTZ_E_STATE, "wtz_zindex_build on a cloned context");
	const bool subset = members != NULL;
	wtz_ctx::zslot_t *z = &c->zs[slot];
	if(!subset || !z->sub){ zpark_all(z); if(subset) zflush_parked(z); z->zoff = NULL; memset(&z->Z, 0, sizeof z->Z); z->sub_cap = 0; }      /* the old arrays are recycled below */
	z->have = false;
	if(slot == 0) c->zs[1].have = false;       /* a query-side index belongs to the batch it was built for */
	wtz_timer tm; tm.start();
	const wtz_reads_t R = ctx_reads(c); const uint32_t nr = c->n_reads, zsize = c->P.zsize, hz = c->P.hz, zcut = c->P.max_zmer_freq;
	if(z->zoff == NULL) CHK(zalloc(z, (void**)&z->zoff, ((size_t)nr + 1) * 8));
	uint64_t *d_off = z->zoff;
	std::vector<uint32_t> p_rid, p_jb; std::vector<size_t> first_piece((size_t)nr + 1);
	{ uint32_t mi = 0;
	  for(uint32_t r = 0; r < nr; r++){
		first_piece[r] = p_rid.size();
		if(subset){ if(mi < nm && members[mi] == r) mi++; else continue; }
		for(uint32_t jb = 0; jb == 0 || jb < c->h_rdlen[r]; jb += WTZ_WALK_CHUNK){ p_rid.push_back(r); p_jb.push_back(jb); }
	  }
	  if(subset && mi != nm) return wtz_fail(WTZ_E_ARG, "wtz_zindex_build_subset: the read ids must be ascending, unique and in range");
	}
	const size_t np = p_rid.size(); first_piece[nr] = np;
	uint32_t *d_prid = NULL, *d_pjb = NULL; uint64_t *d_poff = NULL;
	CHK(dev_alloc((void**)&d_prid, (np + 1) * 4)); CHK(dev_alloc((void**)&d_pjb, (np + 1) * 4)); CHK(dev_alloc((void**)&d_poff, (np + 1) * 8));
	CHK(dev_h2d(d_prid, p_rid.data(), np * 4)); CHK(dev_h2d(d_pjb, p_jb.data(), np * 4));
	CHK(wtz_launch<K_zcount>(np, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_zcount((uint32_t)t, R, d_prid, d_pjb, zsize, hz, d_poff); }));
	std::vector<uint64_t> hp(np + 1), h((size_t)nr + 1);
	CHK(dev_d2h(hp.data(), d_poff, np * 8));
	uint64_t tot = 0; for(size_t i = 0; i < np; i++){ uint64_t v = hp[i]; hp[i] = tot; tot += v; } hp[np] = tot;
	for(uint32_t r = 0; r <= nr; r++) h[r] = hp[first_piece[r]];
	CHK(dev_h2d(d_poff, hp.data(), (np + 1) * 8));
	CHK(dev_h2d(d_off, h.data(), ((size_t)nr + 1) * 8));
	z->n_z = tot;
	wtz_zindex_t Z; memset(&Z, 0, sizeof Z); Z.zoff = z->zoff;
	if(subset && z->sub && tot + 1 <= z->sub_cap) Z = z->Z;      /* the arrays of the previous subset are large enough */
	else {
		if(subset && z->sub){ (void)dev_sync(); zpark_all(z); zflush_parked(z); CHK(zalloc(z, (void**)&z->zoff, ((size_t)nr + 1) * 8)); d_off = z->zoff; CHK(dev_h2d(d_off, h.data(), ((size_t)nr + 1) * 8)); Z.zoff = z->zoff; }
		const uint64_t cap = subset ? tot + tot / 4 + 1024 : tot + 1;      /* subsets: head-room, so that most batches reuse the allocation */
		CHK(zalloc(z, (void**)&Z.mer, cap * 4)); CHK(zalloc(z, (void**)&Z.pos, cap * 4)); CHK(zalloc(z, (void**)&Z.len, cap * 2));
		CHK(zalloc(z, (void**)&Z.ok, cap)); CHK(zalloc(z, (void**)&Z.sidx, cap * 4));
		CHK(zalloc(z, (void**)&Z.dmer, cap * 4)); CHK(zalloc(z, (void**)&Z.dfirst, cap * 4)); CHK(zalloc(z, (void**)&Z.dcnt, cap * 2));
		CHK(zalloc(z, (void**)&Z.dn, ((size_t)nr + 1) * 4));
		zflush_parked(z);                     /* whatever did not fit a request goes back to the driver */
		z->sub_cap = subset ? cap : 0;
	}
	z->sub = subset;
	z->members.assign(members, members + (subset ? nm : 0));
	z->Z = Z;
	{
		/* chunks of consecutive reads, so that the temporaries (sort keys and their double buffer, run flags / lengths / ranks: 32 B per z-mer beside the 25 B the
		 * index keeps) are bounded by the chunk and not by the read set: every step below is per read.  WTZ_ZCHUNK_M: z-mers per chunk in millions */
		static uint64_t chunk_z = 0;
		if(!chunk_z){ const char *e = getenv("WTZ_ZCHUNK_M"); chunk_z = (uint64_t)((e && atof(e) > 0 ? atof(e) : 256.0) * 1e6); if(chunk_z < 1) chunk_z = 1; }
		unsigned rbits = 1; while((1ull << rbits) < (uint64_t)nr + 1) rbits++;
		/* reads whose z-mers fit the LDS of a CU are indexed by one workgroup each (wtz_task_zread); the ids are in length order, so what does not fit is a
		 * prefix [0, rL) of the ids (plus whatever short read sits among them): that prefix goes through the device-wide form in chunks */
		uint32_t rL = nr;
		if(c->sw.zread){
			rL = 0;
			static const uint32_t cls[7] = { 2048u, 3072u, 4096u, 6144u, 8192u, 12288u, 16384u };      /* LDS per workgroup follows the class: finer classes = more workgroups per CU */
			for(uint32_t r = 0; r < nr; r++) if(h[r + 1] - h[r] > WTZ_ZR_MAXN || c->h_rdlen[r] > WTZ_ZR_MAXLEN(WTZ_ZR_MAXN)) rL = r + 1;
			std::vector<uint32_t> lst[7];
			for(uint32_t r = rL; r < nr; r++){
				const uint64_t nz = h[r + 1] - h[r]; if(!nz) continue;
				int k = 0; while(k < 6 && (nz > cls[k] || c->h_rdlen[r] > WTZ_ZR_MAXLEN(cls[k]))) k++;      /* the class holds the read's z-mers and its bases */
				lst[k].push_back(r);
			}
			if(nr > rL){ uint32_t *dn = Z.dn + rL; CHK(dev_set(dn, 0, (size_t)(nr - rL) * 4)); }
			for(int k = 6; k >= 0; k--){
				if(lst[k].empty()) continue;
				const uint32_t np = cls[k], nth = 512u, ldsb = wtz_zr_lds_bytes(np);
				uint32_t *d_lst = NULL; CHK(dev_alloc((void**)&d_lst, lst[k].size() * 4)); CHK(dev_h2d(d_lst, lst[k].data(), lst[k].size() * 4));
#ifdef WTZ_EMUL
				std::vector<uint32_t> emul_lds(ldsb / 4 + 16); uint32_t *lds_emul = emul_lds.data();
				CHK(wtz_launch_wg<K_zread>(lst[k].size(), [=] WTZ_LAMBDA (uint64_t t){ wtz_task_zread(d_lst[t], R, zsize, hz, zcut, Z, lds_emul, np); }, 1u, 0u));
#else
				CHK(wtz_launch_wg<K_zread>(lst[k].size(), [=] WTZ_LAMBDA (uint64_t t){ wtz_task_zread(d_lst[t], R, zsize, hz, zcut, Z, (uint32_t*)wtz_wave_scratch(), np); }, nth, ldsb));
#endif
			}
			CHK(dev_sync());
		}
		uint32_t r0 = 0;
		while(r0 < rL){
			uint32_t r1 = r0 + 1;
			while(r1 < rL && h[r1 + 1] - h[r0] <= chunk_z) r1++;
			const uint64_t base = h[r0], n = h[r1] - h[r0];
			const size_t p0 = first_piece[r0], p1 = first_piece[r1];
			if(n){
				wtz_arena_scope chunk_scope(g_arena);      /* the chunk's temporaries go back (to the arena / its cache) when this scope ends */
				uint64_t *d_key = NULL; uint32_t *d_flag = NULL, *d_cnt = NULL, *d_dpos = NULL; uint32_t *d_val = Z.sidx;
				CHK(dev_alloc((void**)&d_key, (n + 1) * 8));
				CHK(wtz_launch<K_zfill>(p1 - p0, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_zfill((uint32_t)(p0 + t), R, d_prid, d_pjb, d_poff, zsize, hz, Z, d_key, d_val, base); }));
				CHK(dev_sort_pairs_u64_u32(d_key, d_val + base, n, 32 + rbits));          /* stable: positions ascend inside a (read, mer) run */
				CHK(dev_alloc((void**)&d_flag, (n + 2) * 4)); CHK(dev_alloc((void**)&d_cnt, (n + 2) * 4)); CHK(dev_alloc((void**)&d_dpos, (n + 2) * 4));
				CHK(dev_set(d_flag, 0, (n + 2) * 4));
				const uint32_t *d_valb = d_val + base;
				CHK(wtz_launch<K_zrun>(n, [=] WTZ_LAMBDA (uint64_t i){ wtz_task_zrun(i, d_key, d_valb, n, zcut, Z, d_flag, d_cnt); }));
				CHK(dev_exclusive_scan_u32(d_flag, d_dpos, n + 1));
				CHK(wtz_launch<K_zdistinct>(n, [=] WTZ_LAMBDA (uint64_t i){ wtz_task_zdistinct(i, d_key, d_flag, d_cnt, d_dpos, Z, base); }));
				CHK(wtz_launch<K_zdn>(r1 - r0, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_zdn(r0 + (uint32_t)t, d_dpos, Z, base); }));
				CHK(dev_sync());
			} else {
				uint32_t *dn = Z.dn + r0; CHK(dev_set(dn, 0, (size_t)(r1 - r0) * 4));
			}
			r0 = r1;
		}
	}
	z->have = true;
	c->cnt.ms_zindex += tm.stop();
	return WTZ_OK;
}
extern "C" int wtz_zindex_build(wtz_ctx_t *c){ return zindex_build_impl(c, NULL, 0); }
extern "C" int wtz_zindex_build_subset(wtz_ctx_t *c, const uint32_t *ids, uint32_t n){
	if(!ids && n) return wtz_fail(WTZ_E_ARG, "null argument");
	static const uint32_t none = 0;
	return zindex_build_impl(c, ids ? ids : &none, n);
}
/* second index for the QUERY side of the pair stages: the listed reads' tables are read from it, the candidates' z-mers from the index of
 * wtz_zindex_build / _subset (which then only has to hold the reads this device sees as candidates).  ids == NULL && n == 0 drops it. */
extern "C" int wtz_zindex_build_queries(wtz_ctx_t *c, const uint32_t *ids, uint32_t n){
	if(!c) return wtz_fail(WTZ_E_ARG, "null argument");
	if(!ids && n) return wtz_fail(WTZ_E_ARG, "null argument");
	if(!ids){ c->zs[1].have = false; return WTZ_OK; }
	if(!c->zs[0].have) return wtz_fail(WTZ_E_STATE, "wtz_zindex_build_queries before wtz_zindex_build / wtz_zindex_build_subset");
	return zindex_build_impl(c, ids, n, 1);
}

/* ------------------------------------------------------------------------------------------------ */
/* A3: candidates                                                                                    */
/* ------------------------------------------------------------------------------------------------ */
/* the grow-only buffers of a candidate request (both forms) */
static int cq_reserve(wtz_ctx *c, uint32_t nq, uint32_t stride){
	if(nq <= c->cq_cap) return WTZ_OK;
	(void)dev_sync();
	dev_free_persist(c->cq_q); dev_free_persist(c->cq_nc); dev_free_persist(c->cq_cand); dev_free_persist(c->cq_bytes); dev_free_persist(c->cq_thr);
	uint32_t cap = c->cq_cap ? c->cq_cap : 1024; while(cap < nq) cap *= 2;
	CHK(dev_alloc_persist((void**)&c->cq_q, (size_t)cap * 4)); CHK(dev_alloc_persist((void**)&c->cq_nc, (size_t)cap * 4)); CHK(dev_alloc_persist((void**)&c->cq_thr, (size_t)cap * 4));
	CHK(dev_alloc_persist((void**)&c->cq_cand, (size_t)cap * stride * 8)); CHK(dev_alloc_persist((void**)&c->cq_bytes, 8));
	c->cq_cap = cap; return WTZ_OK;
}
/* per query: the first indexed read that is NOT longer than 1.2 x the query (lengths are non-increasing in the id); *d_thr stays NULL where the index is not in length order */
static int cq_thresholds(wtz_ctx *c, const uint32_t *qids, uint32_t nq, const uint32_t **d_thr){
	if(!(c->idx_len_sorted && c->idx_end > c->idx_beg)) return WTZ_OK;
	std::vector<uint32_t> thr(nq);
	for(uint32_t i = 0; i < nq; i++){
		const uint32_t up = (uint32_t)(c->h_rdlen[qids[i]] * 1.2);              /* double multiply, wtzmo.c:445 */
		uint32_t lo = c->idx_beg, hi = c->idx_end;
		while(lo < hi){ const uint32_t mid = lo + (hi - lo) / 2; if(c->h_rdlen[mid] > up) lo = mid + 1; else hi = mid; }
		thr[i] = lo;
	}
	CHK(dev_h2d(c->cq_thr, thr.data(), (size_t)nq * 4)); *d_thr = c->cq_thr; return WTZ_OK;
}
/* asynchronous form: _begin uploads and launches on the context's stream and returns; _end waits and fetches.  Nothing else
 * may run on the context in between (the scratch pool is the kernel's); the host is free meanwhile. */
extern "C" int wtz_candidates_begin(wtz_ctx_t *c, const uint32_t *qids, uint32_t nq, const uint64_t *cand, const uint32_t *ncand_in){
	if(!c || !c->ktab || !qids || !cand || !ncand_in) return wtz_fail(WTZ_E_ARG, "index not built / null argument");
	if(c->cq_pending) return wtz_fail(WTZ_E_STATE, "wtz_candidates_begin: a request is already in flight");
	c->cq_n = nq; c->cq_groups = false;
	if(nq == 0){ c->cq_pending = true; return WTZ_OK; }
	CTX_ENTER(c);
	for(uint32_t i = 0; i < nq; i++) if(qids[i] >= c->n_reads) return wtz_fail(WTZ_E_ARG, "query id %u out of range", qids[i]);
	CHK(pool_reset(c));
	const uint32_t stride = c->P.ncand + 1;
	CHK(cq_reserve(c, nq, stride));
	uint32_t *d_q = c->cq_q, *d_n = c->cq_nc; uint64_t *d_cand = c->cq_cand; unsigned long long *d_bytes = c->cq_bytes;
	CHK(dev_h2d(d_q, qids, (size_t)nq * 4)); CHK(dev_h2d(d_n, ncand_in, (size_t)nq * 4)); CHK(dev_h2d(d_cand, cand, (size_t)nq * stride * 8));
	CHK(dev_set(d_bytes, 0, 8));
	const uint32_t *d_thr = NULL; CHK(cq_thresholds(c, qids, nq, &d_thr));
	const wtz_reads_t R = ctx_reads(c); const wtz_params_t *dP = c->dP; const wtz_kslot_t *tab = c->ktab; const uint64_t kmask = c->kmask;
	const uint32_t *seeds = c->kseeds; wtz_pool_t *pool = c->dpool;
	STAGE(c, "K_candidates");
	c->cq_tm.start();
	/* one workgroup per query: partition by target read, sort each bucket in LDS (wtz_task_candidates_wg) */
	const uint32_t key_hi = c->idx_end << 1;
#ifdef WTZ_EMUL
	static thread_local uint32_t emul_cwg_lds[WTZ_CWG_LDS_BYTES / 4 + 16];
	uint32_t *lds_emul = emul_cwg_lds;
	CHK(wtz_launch_wg<K_candidates_wg>(nq, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_candidates_wg((uint32_t)t, R, d_q, dP, tab, kmask, seeds, pool, d_cand, d_n, stride, d_bytes, lds_emul, d_thr, key_hi); }, 1u, 0u));
#else
	CHK(wtz_launch_wg<K_candidates_wg>(nq, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_candidates_wg((uint32_t)t, R, d_q, dP, tab, kmask, seeds, pool, d_cand, d_n, stride, d_bytes, (uint32_t*)wtz_wave_scratch(), d_thr, key_hi); }, WTZ_CWG_THREADS, WTZ_CWG_LDS_BYTES));
#endif
	c->cq_tm.lap();
	c->cq_pending = true;
	return WTZ_OK;
}
extern "C" int wtz_candidates_end(wtz_ctx_t *c, uint64_t *cand, uint32_t *ncand_out){
	if(!c || !c->cq_pending) return wtz_fail(WTZ_E_STATE, "wtz_candidates_end without wtz_candidates_begin");
	c->cq_pending = false;
	const uint32_t nq = c->cq_n;
	if(nq == 0) return WTZ_OK;
	if(!cand || !ncand_out) return wtz_fail(WTZ_E_ARG, "null argument");
	CTX_ENTER(c);
	const uint32_t stride = c->P.ncand + 1;
	CHK(dev_sync());
	c->cnt.ms_candidates += c->cq_tm.read(); c->cnt.n_candidates_q += nq;
	{ unsigned long long hb = 0; CHK(dev_d2h(&hb, c->cq_bytes, 8)); c->cnt.bytes_seed_algo += hb; }
	CHK(dev_d2h(cand, c->cq_cand, (size_t)nq * stride * 8)); CHK(dev_d2h(ncand_out, c->cq_nc, (size_t)nq * 4));
	CHK(pool_check(c, "wtz_candidates"));
	return WTZ_OK;
}

/* A3 against a SHARD of the index: the (read, strand) groups with ol >= -d of every query, for the caller to join over the shards */
extern "C" int wtz_candidate_groups_begin(wtz_ctx_t *c, const uint32_t *qids, uint32_t nq){
	if(!c || !c->ktab || (nq && !qids)) return wtz_fail(WTZ_E_ARG, "index not built / null argument");
	if(c->cq_pending) return wtz_fail(WTZ_E_STATE, "wtz_candidate_groups_begin: a request is already in flight");
	c->cq_n = nq; c->cq_groups = true;
	if(nq == 0){ c->cq_pending = true; return WTZ_OK; }
	CTX_ENTER(c);
	for(uint32_t i = 0; i < nq; i++) if(qids[i] >= c->n_reads) return wtz_fail(WTZ_E_ARG, "query id %u out of range", qids[i]);
	CHK(pool_reset(c));
	const uint32_t stride = c->P.ncand + 1;
	CHK(cq_reserve(c, nq, stride));
	if(nq > c->cq_gcap){ (void)dev_sync(); dev_free_persist(c->cq_gptr); c->cq_gptr = NULL; uint32_t cap = c->cq_gcap ? c->cq_gcap : 1024; while(cap < nq) cap *= 2; CHK(dev_alloc_persist((void**)&c->cq_gptr, (size_t)cap * 8)); c->cq_gcap = cap; }
	uint32_t *d_q = c->cq_q, *d_n = c->cq_nc; uint64_t *d_cand = c->cq_cand, *d_gptr = c->cq_gptr; unsigned long long *d_bytes = c->cq_bytes;
	CHK(dev_h2d(d_q, qids, (size_t)nq * 4)); CHK(dev_set(d_n, 0, (size_t)nq * 4)); CHK(dev_set(d_gptr, 0, (size_t)nq * 8)); CHK(dev_set(d_bytes, 0, 8));
	const uint32_t *d_thr = NULL; CHK(cq_thresholds(c, qids, nq, &d_thr));
	const wtz_reads_t R = ctx_reads(c); const wtz_params_t *dP = c->dP; const wtz_kslot_t *tab = c->ktab; const uint64_t kmask = c->kmask;
	const uint32_t *seeds = c->kseeds; wtz_pool_t *pool = c->dpool; const uint32_t key_hi = c->idx_end << 1;
	STAGE(c, "K_candidates (groups)");
	c->cq_tm.start();
#ifdef WTZ_EMUL
	static thread_local uint32_t emul_cwg_lds[WTZ_CWG_LDS_BYTES / 4 + 16];
	uint32_t *lds_emul = emul_cwg_lds;
	CHK(wtz_launch_wg<K_candidates_wg>(nq, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_candidates_wg((uint32_t)t, R, d_q, dP, tab, kmask, seeds, pool, d_cand, d_n, stride, d_bytes, lds_emul, d_thr, key_hi, d_gptr); }, 1u, 0u));
#else
	CHK(wtz_launch_wg<K_candidates_wg>(nq, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_candidates_wg((uint32_t)t, R, d_q, dP, tab, kmask, seeds, pool, d_cand, d_n, stride, d_bytes, (uint32_t*)wtz_wave_scratch(), d_thr, key_hi, d_gptr); }, WTZ_CWG_THREADS, WTZ_CWG_LDS_BYTES));
#endif
	c->cq_tm.lap();
	c->cq_pending = true;
	return WTZ_OK;
}
extern "C" int wtz_candidate_groups_end(wtz_ctx_t *c, uint32_t *ngroups){
	if(!c || !c->cq_pending || !c->cq_groups) return wtz_fail(WTZ_E_STATE, "wtz_candidate_groups_end without wtz_candidate_groups_begin");
	c->cq_pending = false;
	const uint32_t nq = c->cq_n;
	c->cq_ng.assign(nq, 0);
	if(nq == 0) return WTZ_OK;
	if(!ngroups) return wtz_fail(WTZ_E_ARG, "null argument");
	CTX_ENTER(c);
	CHK(dev_sync());
	c->cnt.ms_candidates += c->cq_tm.read(); c->cnt.n_candidates_q += nq;
	{ unsigned long long hb = 0; CHK(dev_d2h(&hb, c->cq_bytes, 8)); c->cnt.bytes_seed_algo += hb; }
	CHK(dev_d2h(c->cq_ng.data(), c->cq_nc, (size_t)nq * 4));
	CHK(pool_check(c, "wtz_candidate_groups"));
	for(uint32_t i = 0; i < nq; i++){ if(c->cq_ng[i] == 0xFFFFFFFFu) return wtz_fail(WTZ_E_POOL, "wtz_candidate_groups: query %u ran out of scratch", i); ngroups[i] = c->cq_ng[i]; }
	return WTZ_OK;
}
extern "C" int wtz_candidate_groups_fetch(wtz_ctx_t *c, uint64_t *groups, uint64_t total){
	if(!c || !c->cq_groups) return wtz_fail(WTZ_E_STATE, "wtz_candidate_groups_fetch before wtz_candidate_groups_end");
	c->cq_groups = false;
	const uint32_t nq = c->cq_n;
	uint64_t tot = 0; for(uint32_t i = 0; i < nq; i++) tot += c->cq_ng[i];
	if(tot != total) return wtz_fail(WTZ_E_ARG, "wtz_candidate_groups_fetch: expected room for %llu groups, got %llu", (unsigned long long)tot, (unsigned long long)total);
	if(tot == 0) return WTZ_OK;
	if(!groups) return wtz_fail(WTZ_E_ARG, "null output");
	CTX_ENTER(c);
	std::vector<uint64_t> off((size_t)nq + 1);
	uint64_t o = 0; for(uint32_t i = 0; i < nq; i++){ off[i] = o; o += c->cq_ng[i]; } off[nq] = o;
	uint64_t *d_off = NULL, *d_g = NULL;
	CHK(dev_alloc((void**)&d_off, off.size() * 8)); CHK(dev_h2d(d_off, off.data(), off.size() * 8));
	CHK(dev_alloc((void**)&d_g, (size_t)tot * 8));
	const uint64_t *gp = c->cq_gptr;
	CHK(wtz_launch<K_pack_groups>(nq, [=] WTZ_LAMBDA (uint64_t t){ const uint64_t *src = (const uint64_t*)(uintptr_t)gp[t]; const uint64_t n = d_off[t + 1] - d_off[t]; for(uint64_t k = 0; k < n; k++) d_g[d_off[t] + k] = src[k]; }));
	CHK(dev_sync());
	CHK(dev_d2h(groups, d_g, (size_t)tot * 8));
	return WTZ_OK;
}
extern "C" int wtz_candidates(wtz_ctx_t *c, const uint32_t *qids, uint32_t nq, uint64_t *cand, uint32_t *ncand_io){
	if(!c || !c->ktab || !qids || !cand || !ncand_io) return wtz_fail(WTZ_E_ARG, "index not built / null argument");
	if(nq == 0) return WTZ_OK;
	int rc = wtz_candidates_begin(c, qids, nq, cand, ncand_io);
	if(rc != WTZ_OK) return rc;
	return wtz_candidates_end(c, cand, ncand_io);
}
