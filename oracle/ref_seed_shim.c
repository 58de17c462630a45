/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.
 *
 * ref_seed_shim.c — the reference's own index_wtzmo (wtzmo.c:349-430) and query_wtzmo (wtzmo.c:433-573) behind four calls, so that tests can compare
 * the k-mer index and the seed lookup with the REAL reference function by function.  This file contains no reference code: it #includes the reference's
 * wtzmo.c where it lies (oracle/Makefile compiles it with `-iquote $(REF)` into oracle/_ref/libref_seed.so, which is git-ignored), with its `main`
 * renamed, and only calls into it.  oracle_lib.c exports the same four calls over the oracle's restatement, so one binding drives both.
 *
 * The reference prints its progress and its debug lines to `zmo_debug_out`, which wtzmo.c itself defines as `stderr` (so a definition in front of the
 * #include would be overridden); `stderr` is a macro of <stdio.h>, and redefining IT in front of the #include sends all of that to a memory stream of
 * the shim.  The groups of a query are then read from the reference's own "FAXIAN" lines (wtzmo.c:544-546, wt->debug = 3): reads are named by their id.
 *
 * What the table cannot give: index_wtzmo overwrites every count (wtzmo.c:401-407: 0 for a filtered k-mer, then the fill count), so seedx_index runs it
 * twice - once with max_kmer_freq = 0xFFFF, under which nothing is filtered by frequency and the fill stops at the saturated count (wtzmo.c:312), which
 * leaves count 1 <=> flt and the saturating count otherwise; then with the caller's cutoff, for the table proper.  n_distinct, ktot and n_kept follow
 * from the table; n_occ (occurrences before saturation) equals ktot only while no count is 0xFFFF and is NOT recoverable otherwise.
 */
#include <stdio.h>
#include <stdint.h>
static FILE *seedx_dbg;
#undef stderr
#define stderr seedx_dbg
#define main wtzmo_reference_main
#include "wtzmo.c"
#undef main

typedef struct { uint64_t mer, off; uint32_t cnt, run; uint8_t flt; } seedx_row_t;
typedef struct {
	WTZMO *wt;
	hzrefv *refs; u32list *heap, *hzoff; u64list *cand;
	seedx_row_t *tab; size_t n_tab;
} seedx_t;

static char *seedx_buf; static size_t seedx_len;
static void seedx_dbg_reset(void){
	if(seedx_dbg) fclose(seedx_dbg);
	free(seedx_buf); seedx_buf = NULL; seedx_len = 0;
	seedx_dbg = open_memstream(&seedx_buf, &seedx_len);
}
static int seedx_row_cmp(const void *a, const void *b){ const uint64_t x = ((const seedx_row_t*)a)->mer, y = ((const seedx_row_t*)b)->mer; return x < y ? -1 : x > y; }

/* prm = ksize hk ksave kovl ncand; codes = one byte 0..3 per base; reads are pushed in the order given (read id = position) */
void *seedx_open(const uint8_t *codes, const uint64_t *off, const uint32_t *len, uint32_t n, const uint32_t *prm){
	seedx_t *s = calloc(1, sizeof(seedx_t));
	uint32_t i, j, maxl = 0; char name[16], *seq;
	seedx_dbg_reset();
	s->wt = init_wtzmo(prm[0], 10, 50, 3200, 2, -5, -3, -1, -50, 200, 0.5);
	s->wt->hk = prm[1];
	s->wt->ksave = prm[2]; s->wt->hzmh_kmer_mod = HZMH_KMER_MOD * prm[2];      /* wtzmo.c:1672-1673 */
	s->wt->kovl = prm[3]; s->wt->ncand = prm[4];
	for(i = 0; i < n; i++) if(len[i] > maxl) maxl = len[i];
	seq = malloc(maxl + 1);
	for(i = 0; i < n; i++){
		for(j = 0; j < len[i]; j++) seq[j] = "ACGT"[codes[off[i] + j] & 3];
		push_long_read_wtzmo(s->wt, name, sprintf(name, "%u", i), seq, len[i]);
	}
	free(seq);
	s->refs = init_hzrefv(64); s->heap = init_u32list(64); s->hzoff = init_u32list(64); s->cand = init_u64list(64);
	return s;
}
void seedx_close(void *h){
	seedx_t *s = h;
	free_hzrefv(s->refs); free_u32list(s->heap); free_u32list(s->hzoff); free_u64list(s->cand); free(s->tab);
	free_wtzmo(s->wt); free(s);
}

static size_t seedx_walk(seedx_t *s, seedx_row_t *out){
	size_t n = 0; uint32_t i; hzmh_t *u;
	for(i = 0; i < HZMH_KMER_MOD; i++){
		reset_iter_hzmhash(s->wt->hashs[i]);
		while((u = ref_iter_hzmhash(s->wt->hashs[i]))){
			if(out){ out[n].mer = u->mer; out[n].off = u->off; out[n].cnt = u->flt ? 1 : u->cnt; out[n].run = u->flt ? 0 : u->cnt; out[n].flt = u->flt; }
			n++;
		}
	}
	return n;
}

/* io[0]: in = -K (0 / 1 = automatic), out = the resolved cutoff; out io[1] = avg_rdlen, io[2] = distinct sampled k-mers, io[3] = seed entries */
int seedx_index(void *h, uint32_t beg, uint32_t end, uint64_t *io){
	seedx_t *s = h; size_t n, i; seedx_row_t *sat;
	seedx_dbg_reset();
	s->wt->max_kmer_freq = 0xFFFF;
	index_wtzmo(s->wt, beg, end, 1);
	n = seedx_walk(s, NULL);
	sat = malloc((n + 1) * sizeof(seedx_row_t)); seedx_walk(s, sat);
	qsort(sat, n, sizeof(seedx_row_t), seedx_row_cmp);
	seedx_dbg_reset();
	s->wt->max_kmer_freq = (uint32_t)io[0];
	index_wtzmo(s->wt, beg, end, 1);
	if(seedx_walk(s, NULL) != n){ free(sat); return -1; }
	free(s->tab); s->tab = malloc((n + 1) * sizeof(seedx_row_t)); s->n_tab = n; seedx_walk(s, s->tab);
	qsort(s->tab, n, sizeof(seedx_row_t), seedx_row_cmp);
	for(i = 0; i < n; i++){
		if(s->tab[i].mer != sat[i].mer || (!s->tab[i].flt && s->tab[i].run != sat[i].cnt)){ free(sat); return -2; }
		s->tab[i].cnt = sat[i].cnt;
	}
	free(sat);
	io[0] = s->wt->max_kmer_freq; io[1] = s->wt->avg_rdlen; io[2] = n; io[3] = s->wt->seeds->size;
	return 0;
}
/* the table in k-mer order: saturating count, flt, and for the kept ones the seed run seeds[offs[i] .. offs[i] + runs[i]) as rd_id << 1 | dir */
void seedx_table(void *h, uint64_t *mers, uint32_t *cnts, uint8_t *flt, uint64_t *offs, uint32_t *runs, uint32_t *seeds){
	seedx_t *s = h; size_t i;
	for(i = 0; i < s->n_tab; i++){ mers[i] = s->tab[i].mer; cnts[i] = s->tab[i].cnt; flt[i] = s->tab[i].flt; offs[i] = s->tab[i].off; runs[i] = s->tab[i].run; }
	for(i = 0; i < s->wt->seeds->size; i++) seeds[i] = (s->wt->seeds->buffer[i].rd_id << 1) | s->wt->seeds->buffer[i].dir;
}
/* query_wtzmo on a heap preloaded with row[0 .. n_io); returns the new size, the heap array verbatim in row (room for max(n_io, ncand) + 1) */
uint32_t seedx_query(void *h, uint32_t pbid, uint64_t *row, uint32_t n_io){
	seedx_t *s = h; uint32_t i;
	seedx_dbg_reset();
	clear_u64list(s->cand);
	for(i = 0; i < n_io; i++) push_u64list(s->cand, row[i]);
	s->wt->debug = 0;
	query_wtzmo(s->wt, pbid, s->cand, s->refs, s->heap, s->hzoff);
	memcpy(row, s->cand->buffer, s->cand->size * 8);
	return (uint32_t)s->cand->size;
}
/* every (rd_id << 1 | dir, ol, cnt) of the query in merge order, from the reference's FAXIAN lines; returns their number (out holds cap triples) */
int seedx_groups(void *h, uint32_t pbid, uint32_t *out, uint32_t cap){
	seedx_t *s = h; int n = 0; char *p, *e; unsigned id; int ol, cnt; char sd;
	seedx_dbg_reset();
	clear_u64list(s->cand);
	s->wt->debug = 3;
	query_wtzmo(s->wt, pbid, s->cand, s->refs, s->heap, s->hzoff);
	s->wt->debug = 0;
	fflush(seedx_dbg);
	for(p = seedx_buf; p && p < seedx_buf + seedx_len; p = e + 1){
		e = memchr(p, '\n', seedx_buf + seedx_len - p); if(e == NULL) break;
		if(sscanf(p, "FAXIAN\t%u\t%d\t%d\t%c", &id, &ol, &cnt, &sd) != 4) continue;
		if((uint32_t)n < cap){ out[3 * n] = (id << 1) | (sd == '-'); out[3 * n + 1] = (uint32_t)ol; out[3 * n + 2] = (uint32_t)cnt; }
		n++;
	}
	return n;
}
