/*
 * wtz_lib_fetch.h — the CIGARs of the last wtz_pairs_align on their way to the caller: packed words, rendered text (synchronous, in two halves
 * beside the next range's kernels, or left on the device).  Included by wtz_lib.cpp.
 */
extern "C" int wtz_fetch_cigars(wtz_ctx_t *c, uint32_t *dst, uint64_t n_ops){
	if(!c || !c->have_items) return wtz_fail(WTZ_E_STATE, "wtz_fetch_cigars before wtz_pairs_align");
	CTX_ENTER(c);
	uint64_t tot = 0; for(uint32_t i = 0; i < c->n_items; i++) tot += c->h_alnres[i].cigar_len;
	if(tot != n_ops) return wtz_fail(WTZ_E_ARG, "wtz_fetch_cigars: expected room for %llu ops, got %llu", (unsigned long long)tot, (unsigned long long)n_ops);
	if(tot == 0) return WTZ_OK;
	if(!dst) return wtz_fail(WTZ_E_ARG, "null output");
	std::vector<uint64_t> off((size_t)c->n_items + 1);
	uint64_t o = 0; for(uint32_t i = 0; i < c->n_items; i++){ off[i] = o; o += c->h_alnres[i].cigar_len; } off[c->n_items] = o;
	uint64_t *d_off = NULL; uint32_t *d_c = NULL;
	CHK(dev_alloc((void**)&d_off, off.size() * 8)); CHK(dev_h2d(d_off, off.data(), off.size() * 8));
	CHK(dev_alloc((void**)&d_c, (size_t)tot * 4));
	const wtz_alnres_dev_t *dr = c->d_alnres;
	CHK(wtz_launch<K_pack_cigars>(c->n_items, [=] WTZ_LAMBDA (uint64_t t){ const wtz_alnres_dev_t &r = dr[t]; for(uint32_t k = 0; k < r.cigar_len; k++) d_c[d_off[t] + k] = r.cigar[k]; }));
	CHK(dev_sync());
	CHK(dev_d2h(dst, d_c, (size_t)tot * 4));
	return WTZ_OK;
}

/* the CIGAR text of the last wtz_pairs_align rendered into a device buffer of the context (grow-only, valid until the next call on this context) */
static int render_cigar_text(wtz_ctx_t *c, uint64_t n_bytes, char **d_text_out, bool wait = true){
	uint64_t tot = 0; for(uint32_t i = 0; i < c->n_items; i++) tot += c->h_alnres[i].text_len;
	if(tot != n_bytes) return wtz_fail(WTZ_E_ARG, "CIGAR text: expected room for %llu bytes, got %llu", (unsigned long long)tot, (unsigned long long)n_bytes);
	*d_text_out = NULL;
	if(tot == 0) return WTZ_OK;
#ifndef WTZ_EMUL
	{   /* the buffer may still be on its way out (the latest copy; the ones before it are in front of it on the same stream) */
		const uint64_t b = c->text_begun.load();
		if(b > c->text_known_done.load()){ HIPCHK(hipEventSynchronize(c->ev_text_done[(b - 1) & 1])); c->text_known_done.store(b); }
	}
#endif
	if(tot + 16 > c->cap_text){
		(void)dev_sync(); dev_free_persist(c->d_text); c->d_text = NULL; c->cap_text = 0;
		const size_t cap = (size_t)(tot + tot / 4 + 4096);
		CHK(dev_alloc_persist((void**)&c->d_text, cap)); c->cap_text = cap;
	}
	std::vector<uint64_t> off((size_t)c->n_items + 1);
	uint64_t o = 0; for(uint32_t i = 0; i < c->n_items; i++){ off[i] = o; o += c->h_alnres[i].text_len; } off[c->n_items] = o;
	uint64_t *d_off = NULL; char *d_t = c->d_text;
	CHK(dev_alloc((void**)&d_off, off.size() * 8)); CHK(dev_h2d(d_off, off.data(), off.size() * 8));
	const wtz_alnres_dev_t *dr = c->d_alnres;
	STAGE(c, "K_cigar_text");
	CHK(wtz_launch_coop<K_cigar_text>(c->n_items, [=] WTZ_LAMBDA (uint64_t t){ const wtz_alnres_dev_t &r = dr[t]; if(r.text_len) wtz_cigar_text_write_coop(r.cigar, r.cigar_len, d_t + d_off[t]); }));
	if(wait) CHK(dev_sync());
	*d_text_out = d_t;
	return WTZ_OK;
}
extern "C" int wtz_fetch_cigar_text(wtz_ctx_t *c, char *dst, uint64_t n_bytes){
	if(!c || !c->have_items) return wtz_fail(WTZ_E_STATE, "wtz_fetch_cigar_text before wtz_pairs_align");
	CTX_ENTER(c);
	char *d_t = NULL;
	CHK(render_cigar_text(c, n_bytes, &d_t));
	if(n_bytes == 0) return WTZ_OK;
	if(!dst) return wtz_fail(WTZ_E_ARG, "null output");
	CHK(dev_d2h(dst, d_t, (size_t)n_bytes));
	return WTZ_OK;
}
/* the same in two halves: _begin renders the text and starts its copy on a stream of its own, _end waits for the copy.  Between the two the context is free for
 * the next calls (wtz_batch_begin ... wtz_pairs_align of the next range): at configs[2] the text is 3.4 GB per step = 72 ms at the rate of the link, and the
 * scratch pool is not involved - the text is rendered into a buffer of its own.  dst must stay valid (and untouched) until _end returns. */
extern "C" int wtz_fetch_cigar_text_begin(wtz_ctx_t *c, char *dst, uint64_t n_bytes){
	if(!c || !c->have_items) return wtz_fail(WTZ_E_STATE, "wtz_fetch_cigar_text_begin before wtz_pairs_align");
	CTX_ENTER(c);
#ifdef WTZ_EMUL
	char *d_t = NULL; CHK(render_cigar_text(c, n_bytes, &d_t));
	if(n_bytes && !dst) return wtz_fail(WTZ_E_ARG, "null output");
	if(n_bytes) memcpy(dst, d_t, (size_t)n_bytes);
	return WTZ_OK;
#else
	if(!c->stream_copy){
		if(hipStreamCreateWithFlags(&c->stream_copy, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_text_ready, hipEventDisableTiming) != hipSuccess
			|| hipEventCreateWithFlags(&c->ev_text_done[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_text_done[1], hipEventDisableTiming) != hipSuccess) return wtz_fail(WTZ_E_HIP, "hipStreamCreate / hipEventCreate failed");
	}
	char *d_t = NULL;
	CHK(render_cigar_text(c, n_bytes, &d_t, false));
	if(n_bytes == 0) return WTZ_OK;
	if(!dst) return wtz_fail(WTZ_E_ARG, "null output");
	HIPCHK(hipEventRecord(c->ev_text_ready, g_stream));
	HIPCHK(hipStreamWaitEvent(c->stream_copy, c->ev_text_ready, 0));
	HIPCHK(hipMemcpyAsync(dst, d_t, (size_t)n_bytes, hipMemcpyDeviceToHost, c->stream_copy));
	{ const uint64_t k = c->text_begun.load(); HIPCHK(hipEventRecord(c->ev_text_done[k & 1], c->stream_copy)); c->text_begun.store(k + 1); }
	return WTZ_OK;
#endif
}
extern "C" int wtz_fetch_cigar_text_end(wtz_ctx_t *c){
	if(!c) return wtz_fail(WTZ_E_ARG, "null argument");
#ifndef WTZ_EMUL
	/* no CTX_ENTER: this may be called while another thread runs the next range's calls on the context; it touches the event only */
	const uint64_t e = c->text_ended.load();
	if(e >= c->text_begun.load()) return WTZ_OK;                /* nothing in flight that has not been ended */
	if(e >= c->text_known_done.load()){ HIPCHK(hipEventSynchronize(c->ev_text_done[e & 1])); }      /* at worst the event has been re-recorded for copy e + 2 (whose render waited for copy e + 1): a longer wait, never a shorter one */
	c->text_ended.store(e + 1);
#endif
	return WTZ_OK;
}
extern "C" int wtz_cigar_text_device(wtz_ctx_t *c, uint64_t n_bytes, void **dev_ptr){
	if(!c || !c->have_items || !dev_ptr) return wtz_fail(WTZ_E_STATE, "wtz_cigar_text_device before wtz_pairs_align / null argument");
	CTX_ENTER(c);
	char *d_t = NULL;
	CHK(render_cigar_text(c, n_bytes, &d_t));
	*dev_ptr = d_t;
	return WTZ_OK;
}
