/*
 * wtz_tool.h — what the drop-in tools on top of the batch services (wtcyc, pairaln, wtext; wtgbo for the parameter block and the halving driver) share, each
 * piece once: the default wtz_params_c, the way out on an error, the device options and the context with its 16 GB default, the records a tool refuses, the
 * block's arrays for wtz_upload_reads_ascii, the driver that halves a block on WTZ_E_POOL, the context made on a helper thread.  A tool's own file holds its options, its problems and its output.
 */
#ifndef WTZ_TOOL_H
#define WTZ_TOOL_H

#include <getopt.h>
#include <pthread.h>
#include <unistd.h>
#include "wtz_host.h"
#define HT_MAXLEN 65535      /* the longest sequence the batch services take */
/* the parameter block of a context that only runs batch services: every field but the scores, which the caller sets from its options (M, X, O, E, T) */
static inline void ht_default_params(wtz_params_c *P){
	memset(P, 0, sizeof *P);
	P->ksize = 16; P->zsize = 10; P->hk = 1; P->hz = 1; P->ksave = 4; P->kovl = 300; P->ncand = 500; P->nbest = 100; P->kwin = 800; P->kstep = 400; P->ztot = 300; P->zovl = 200;
	P->max_zmer_freq = 64; P->max_kmer_var = 2; P->win_rep_norm = 20; P->win_rep_cutoff = 100;
	P->w = 50; P->ew = 800; P->W = 3200; P->min_score = 200; P->min_id = 0.5f;
	P->xvar = 128; P->yvar = 64; P->min_block_len = 160; P->max_overhang = 256; P->deviation_penalty = 1.0f; P->gap_penalty = 0.05f;
}

/* the way out on an error: exit(1), or what the includer defines HT_EXIT() to be (wtext and wtgbo create their context on a helper thread and never exit() under it) */
#ifndef HT_EXIT
#define HT_EXIT() exit(1)
#endif
static inline void ht_die(const char *what){ fprintf(stderr, " -- %s failed: %s --\n", what, wtz_last_error()); HT_EXIT(); }
static inline int ht_no_device(const char *tool, const char *work){      /* 1 and the message: main returns 1 on it */
	if(wtz_device_count() <= 0) fprintf(stderr, " -- no HIP device visible: %s (MI355X build) has no CPU path for the %s: %s --\n", tool, work, wtz_last_error());
	return wtz_device_count() <= 0;
}

/* the device options; the size of a block goes by the tool's own name for it.  --pool-mb is a test hook (a pool small enough to force the halving path), as in wtzmo: no usage text names it */
typedef struct { int gpu; uint64_t pool_gb, pool_mb, block; } ht_devopt_t;
#define HT_LONGOPTS(block) {"gpu", required_argument, NULL, 1001}, {"pool-gb", required_argument, NULL, 1002}, {block, required_argument, NULL, 1003}, {"pool-mb", required_argument, NULL, 1004}
static inline int ht_devopt(ht_devopt_t *d, int c, const char *arg){      /* 1 if c was one of them */
	if(c == 1001) d->gpu = atoi(arg); else if(c == 1002) d->pool_gb = (uint64_t)atoll(arg); else if(c == 1003) d->block = (uint64_t)atoll(arg); else if(c == 1004) d->pool_mb = (uint64_t)atoll(arg); else return 0;
	return 1;
}
static inline uint64_t ht_pool_bytes(const ht_devopt_t *d){ return d->pool_mb ? d->pool_mb << 20 : (d->pool_gb ? d->pool_gb : 16) << 30; }
static inline wtz_ctx_t *ht_ctx_create(const ht_devopt_t *d, const wtz_params_c *P){ wtz_ctx_t *ctx = NULL; if(wtz_ctx_create(d->gpu, P, ht_pool_bytes(d), &ctx) != WTZ_OK) ht_die("wtz_ctx_create"); return ctx; }
/* the same on a helper thread, while the tool loads its input: above all the hipMalloc of the pool, ~35 ms per GB (wtext, wtgbo) */
typedef struct { const wtz_params_c *P; int device, rc, started; uint64_t pool_bytes; wtz_ctx_t *ctx; char err[256]; pthread_t th; } ht_ctxjob_t;
static inline void *ht_ctxjob_main(void *arg){
	ht_ctxjob_t *j = (ht_ctxjob_t*)arg;
	j->rc = wtz_ctx_create(j->device, j->P, j->pool_bytes, &j->ctx);
	if(j->rc != WTZ_OK) snprintf(j->err, sizeof j->err, "%s", wtz_last_error());
	return NULL;
}
static inline void ht_ctxjob_start(ht_ctxjob_t *j, const wtz_params_c *P, int device, uint64_t pool_bytes){ j->P = P; j->device = device; j->pool_bytes = pool_bytes; j->ctx = NULL; j->rc = WTZ_OK; j->started = (pthread_create(&j->th, NULL, ht_ctxjob_main, j) == 0); }
static inline wtz_ctx_t *ht_ctxjob_join(ht_ctxjob_t *j){
	if(j->started) pthread_join(j->th, NULL); else ht_ctxjob_main(j);
	if(j->rc != WTZ_OK){ fprintf(stderr, " -- wtz_ctx_create failed: %s --\n", j->err); HT_EXIT(); }
	return j->ctx;
}

/* the records a tool refuses when it reads them, under the word it has for them ("read", "record") */
static inline void ht_check_record(const char *word, const hx_str_t *name, const hx_str_t *seq){
	if(seq->n > HT_MAXLEN){ fprintf(stderr, " -- %s '%.*s' has %llu bases: more than %d, the longest %s this build aligns --\n", word, (int)name->n, name->s, (unsigned long long)seq->n, HT_MAXLEN, word); HT_EXIT(); }
	for(size_t i = 0; i < seq->n; i++) if(strchr("ACGTacgt", seq->s[i]) == NULL || seq->s[i] == 0){
		fprintf(stderr, " -- %s '%.*s' has a character outside ACGTacgt at base %llu (0x%02x) --\n", word, (int)name->n, name->s, (unsigned long long)i, (unsigned)(unsigned char)seq->s[i]); HT_EXIT(); }
}

/* a block of records kept as text (hx_store_t with keep_text): its offsets and lengths as wtz_upload_reads_ascii takes them, and the upload */
typedef struct { uint64_t *rdoff; uint32_t *rdlen; size_t cap; } ht_block_t;
static inline void ht_block_upload(wtz_ctx_t *ctx, ht_block_t *B, const hx_store_t *st){
	const uint32_t n = st->n_all;
	if(n > B->cap){ B->cap = n; B->rdoff = (uint64_t*)hx_realloc(B->rdoff, 8 * (size_t)n); B->rdlen = (uint32_t*)hx_realloc(B->rdlen, 4 * (size_t)n); }
	for(uint32_t i = 0; i < n; i++){ B->rdoff[i] = st->reads[i].off; B->rdlen[i] = st->reads[i].len; }
	if(wtz_upload_reads_ascii(ctx, st->text, st->nbase, B->rdoff, B->rdlen, n, 0, NULL) != WTZ_OK) ht_die("wtz_upload_reads_ascii");
}
static inline void ht_block_done(hx_store_t *st){ for(uint32_t i = 0; i < st->n_all; i++) free(st->reads[i].name); st->n_all = 0; st->nbase = 0; }

/* n items through a batch service: call(user, at, step) runs items [at, at + step) and returns the service's code.  The whole block first; on WTZ_E_POOL half as
 * many, down to one, where the run ends with the tool's noun for an item (and, with hint, the option the tool has for it).  Any other failure is `what`'s. */
static inline void ht_halving(uint32_t n, int (*call)(void *user, uint32_t at, uint32_t step), void *user, const char *what, const char *noun, int hint){
	for(uint32_t at = 0, step = n; at < n; ){
		if(step > n - at) step = n - at;
		const int rc = call(user, at, step);
		if(rc == WTZ_E_POOL){
			if(step == 1){ fprintf(stderr, " -- scratch pool too small even for one %s: %s%s --\n", noun, wtz_last_error(), hint ? " (use --pool-gb)" : ""); HT_EXIT(); }
			step = (step + 1) / 2; continue;
		}
		if(rc != WTZ_OK) ht_die(what);
		at += step;
	}
}
#endif
