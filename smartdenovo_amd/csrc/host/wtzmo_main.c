/*
 * wtzmo — MI355X-native drop-in for SMARTdenovo's `wtzmo` (same argv, same .ovl / .contained files).
 *
 * Host side in plain C.  All hot-path computation (k-mer index + seed lookup, z-mer matching,
 * window detection / chaining or the dot-matrix engine, the three banded DPs) runs on the GPU
 * through the C ABI of libwtzmo_hip.so (include/wtzmo_hip.h).  What stays here is exactly the part
 * of the reference that is sequential by definition: the order-dependent commit of `wtzmo -t 1`
 * (closed pairs, contained-read masking, per-read coverage, record order; wtzmo.c:806-822, 933-986,
 * 1005-1123, 1170-1249, 1309-1334), replayed over device results that are pure functions of
 * (query, candidate).
 *
 * Execution shape: queries are taken in id order in batches; for a batch the GPU computes, for every
 * candidate pair not already closed when the batch is planned, the pair result and the alignment of
 * its best strand (a superset of what the reference would touch, because the closed/masked sets only
 * grow); the host then commits the batch strictly in query order.  Batch size adapts to the fraction
 * of speculative work that the commit discards.
 *
 * Extra options (not in the reference):  --gpu <id> | --gpus <n> | --gpu-list <id,...>, --pool-gb <n> | --pool-mb <n>, --batch <max queries>, --first-batch <n>, --workers <n>,
 * --shard-index, --zindex-batch <0|1>, --ingest <device|host>, --binary-out, --repeat <n>, --lib-check, --stats <file> (one line of 33 tab-separated columns per step: step_report).
 * This file: options, loading, device set-up, the step and its report; the rest is in the section headers included below (wtzmo_types.h lists them).
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <unistd.h>
#include <time.h>
#include <pthread.h>
#include <sys/uio.h>
#include <errno.h>
#include <sys/stat.h>
#include <fcntl.h>
#include "wtz_host.h"
#include "wtz_ovlb.h"
static int usage(void){
	printf(
	"WTZMO (MI355X): overlapper of long reads using homopolymer compressed k-mer seeding\n"
	"Drop-in for SMARTdenovo wtzmo 1.0 -- identical options and file formats; hot path on the GPU\n"
	"Usage: wtzmo [options]\n"
	" -t <int>    accepted for compatibility (the GPU path is deterministic and equals `wtzmo -t 1`)\n"
	" -P <int> -p <int>  total parallel jobs / index of this job\n"
	" -i <string> long reads (+) *   -I <string> query-only reads (+)   -b <string> clip regions (+)\n"
	" -J <int>    min read length    -o <string> output *  -f overwrite   -9 <string> tested pairs out\n"
	" -L <string> tested pairs in (+)  -F <string> reads to mask (+)  -C no .contained file  -N seeds only\n"
	" -H <int> -k <int> -K <int> -S <int> -d <int> -G <int>      k-mer seeding [3,16,0,4,300,1]\n"
	" -z <int> -Z <int> -l <int> -y <int> -R <int> -r <int> -q <int>  z-mer windows [10,64,2,800,200,300,100]\n"
	" -U <float>x5 | -U -1   dot-matrix engine    -A <int> -B <int> candidates / best [500,100]\n"
	" -w -e -W -M -X -O -E -T  alignment [50,800,3200,2,-5,-3,-1,-50]   -s <int> -m <float> [200,0.5]\n"
	" --gpu <int> | --gpus <int> (one process, N GPUs, ONE .ovl identical to -t 1)  --pool-gb <int> --batch <int> --stats <file>\n"
	" --shard-index  --zindex-batch <0|1>  --binary-out (64-byte records, include/wtz_ovlb.h; read by wtgbo --binary-in / wtovl)\n");
	return 1;
}
#include "wtzmo_types.h"
#include "wtzmo_out.h"
#include "wtzmo_commit.h"
#include "wtzmo_stages.h"
#include "wtzmo_ranks.h"
#include "wtzmo_ranges.h"
typedef struct { char **a; int n, cap; } strlist_t;
static void sl_push(strlist_t *l, char *s){ if(l->n == l->cap){ l->cap = l->cap ? l->cap * 2 : 4; l->a = (char**)hx_realloc(l->a, sizeof(char*) * (size_t)l->cap); } l->a[l->n++] = s; }
typedef struct {      /* the command line, where it is not a field of E */
	strlist_t pbs, flts, ovls, obts, tbas; char *output, *pairoutf, *statsf; const char *gpu_list;      /* -i -F -L -b -I, -o -9 */
	int min_rdlen, overwrite, write_contained, gpu, n_gpus, lib_check, repeat, max_batch_set; uint64_t pool_gb, pool_mb;
} opts_t;
/* --repeat (benchmarking): the previous repeat's output file is removed by a side thread, see the repeat loop in wtzmo_main */
typedef struct { char *path; int pending, running; pthread_t th; } stale_job_t;
static void *stale_main(void *arg){ unlink((const char*)arg); return NULL; }
static void stale_start(stale_job_t *j){
	if(!j->pending || j->running) return;
	if(pthread_create(&j->th, NULL, stale_main, j->path) == 0) j->running = 1; else unlink(j->path);
	j->pending = 0;
}
static void stale_join(stale_job_t *j){ if(j->running){ pthread_join(j->th, NULL); j->running = 0; } }
/* the device contexts - above all the hipMalloc of their scratch pools: ~35 ms per GB, 4.4 s for the default 128 GB - are created on a helper
 * thread while the main thread reads the FASTA (measured on wtgbo, E. coli shape: 5.4 s wall with the 128 GB pool created up front, 1.0 s with 16 GB) */
typedef struct { const wtz_params_c *P; uint64_t pool_bytes; int devs[8]; uint32_t ndev; wtz_ctx_t *ctxs[8]; int rc; char err[256]; pthread_t th; int started, joined; } ctxjob_t;
/* device bytes a read set of `bases` bases needs beside the scratch pool when the z-mer index holds every read: the index itself (25 B per z-mer, measured
 * 15.8 B per base), reads (2 bits per base), k-mer seeds + table (< 2.5 B per base), and - transient - the largest of the build temporaries (k-mer index: sort
 * keys + values of 0.19 occurrences per base, double-buffered = 6 B per base, gone before the z-mer index is allocated: BUILD_ZINDEX; z-mer chunks: 8 GB), the arena */
#define WTZ_ZALL_MIN_BASES 2400000000ull
static uint64_t zall_bytes(uint64_t bases){ return (uint64_t)((double)bases * 19.0) + (14ull << 30); }
static void *ctxjob_main(void *arg){
	ctxjob_t *j = (ctxjob_t*)arg;
	for(uint32_t d = 0; d < j->ndev; d++){
		j->rc = wtz_ctx_create(j->devs[d], j->P, j->pool_bytes, &j->ctxs[d]);
		if(j->rc != WTZ_OK){ snprintf(j->err, sizeof j->err, "%s", wtz_last_error()); break; }      /* wtz_last_error is thread-local: keep the text */
	}
	return NULL;
}
typedef struct { wtz_ctx_t *ctx; uint32_t n_rd, K; int rc; char err[256]; int zonly, nozidx; uint32_t zmod, zres; } ixjob_t;
/* the z-mer index of one device for the whole run: every read, or - several parts - the candidate side of its residue class of the indexed reads */
static int zindex_for_part(wtz_ctx_t *ctx, uint32_t n_rd, uint32_t zmod, uint32_t zres){
	if(zmod <= 1) return wtz_zindex_build(ctx);
	uint32_t *m = (uint32_t*)hx_realloc(NULL, 4 * ((size_t)n_rd / zmod + 2)), n = 0;
	for(uint32_t r = zres; r < n_rd; r += zmod) m[n++] = r;
	const int rc = wtz_zindex_build_subset(ctx, m, n);
	free(m); return rc;
}
static void *ixjob_main(void *arg){
	ixjob_t *j = (ixjob_t*)arg; wtz_index_stats_t ist;
	j->rc = j->nozidx ? WTZ_OK : zindex_for_part(j->ctx, j->n_rd, j->zmod, j->zres);
	if(j->rc == WTZ_OK && !j->zonly) j->rc = wtz_index_build(j->ctx, 0, j->n_rd, &j->K, &ist);
	if(j->rc != WTZ_OK){ strncpy(j->err, wtz_last_error(), sizeof j->err - 1); j->err[sizeof j->err - 1] = 0; }
	return NULL;
}

static void *pin_main(void *arg){
	eng_t *E = (eng_t*)arg;
	for(int k = 0; k < 2; k++){
		E->cig_keep[k] = (char*)wtz_host_alloc(E->cig_keep_cap[k] + 1);
		if(!E->cig_keep[k]) E->cig_keep_cap[k] = 0;
	}
	return NULL;
}
/* Benchmark hook (bench.py, in-process through libwtzmo_host.so): called with (rep, 0) right before the timed overlap
 * phase of repetition `rep` starts (reads already resident in HBM) and with (rep, 1) after its output is written. */
typedef void (*wtzmo_hook_fn)(int rep, int phase);
static wtzmo_hook_fn g_hook = NULL;
void wtzmo_set_hook(wtzmo_hook_fn f){ g_hook = f; }
/* the command line into E and o; -1: go on, otherwise what main returns (usage: 1, --lib-check: 0 or 3) */
static int parse_options(int argc, char **argv, eng_t *E, opts_t *o){
	wtz_params_c *P = &E->P; int c, dot_matrix = 0, refine = 0; float optval;
	o->write_contained = 1; o->repeat = 1; o->n_gpus = 1;
	/* defaults: wtzmo.c:1543-1588 */
	P->w = 50; P->ew = 800; P->W = 3200; P->M = 2; P->X = -5; P->O = -3; P->E = -1; P->T = -50;
	P->min_score = 200; P->min_id = 0.5f; P->hk = 1; P->hz = 1; P->ksize = 16; P->zsize = 10;
	P->kwin = 800; P->kovl = 300; P->ksave = 4; P->win_rep_norm = 20; P->win_rep_cutoff = 100; P->ncand = 500; P->nbest = 100;
	P->ztot = 300; P->zovl = 200; P->max_kmer_freq = 0; P->max_zmer_freq = 64; P->max_kmer_var = 2;
	P->xvar = 128; P->yvar = 64; P->min_block_len = 160; P->deviation_penalty = 1.0f; P->gap_penalty = 0.05f;
	E->do_align = 1; E->n_idx = 1; E->n_job = 1; E->i_job = 0; E->max_batch = 8192; E->first_batch = 256; E->n_workers = 1;
	static struct option lopts[] = { {"stats", required_argument, 0, 1000}, {"gpu", required_argument, 0, 1001}, {"pool-gb", required_argument, 0, 1002},
		{"batch", required_argument, 0, 1003}, {"lib-check", no_argument, 0, 1004}, {"repeat", required_argument, 0, 1005}, {"first-batch", required_argument, 0, 1006}, {"workers", required_argument, 0, 1007}, {"pool-mb", required_argument, 0, 1008}, {"gpus", required_argument, 0, 1010}, {"gpu-list", required_argument, 0, 1011}, {"shard-index", no_argument, 0, 1012}, {"zindex-batch", required_argument, 0, 1013}, {"ingest", required_argument, 0, 1014}, {"binary-out", no_argument, 0, 1015}, {0, 0, 0, 0} };
	while((c = getopt_long(argc, argv, "ht:P:p:Ni:b:J:I:o:9:S:fCH:k:G:z:Z:U:y:d:r:q:l:K:A:B:r:R:L:F:W:w:e:M:X:O:E:T:s:m:nv", lopts, NULL)) != -1){
		switch(c){
			case 1000: o->statsf = optarg; break;
			case 1001: o->gpu = atoi(optarg); break;
			case 1002: o->pool_gb = (uint64_t)atoll(optarg); break;
			case 1003: E->max_batch = (uint32_t)atoi(optarg); if(E->max_batch < 1) E->max_batch = 1; o->max_batch_set = 1; break;
			case 1004: o->lib_check = 1; break;
			case 1005: o->repeat = atoi(optarg); if(o->repeat < 1) o->repeat = 1; break;
			case 1006: E->first_batch = (uint32_t)atoi(optarg); if(E->first_batch < 1) E->first_batch = 1; E->first_batch_set = 1; break;
			case 1010: o->n_gpus = atoi(optarg); if(o->n_gpus < 1) o->n_gpus = 1; if(o->n_gpus > 8) o->n_gpus = 8; break;
			case 1015: E->binary_out = 1; break;      /* f3: binary record hand-off (include/wtz_ovlb.h) to a consumer that reads it (bin/wtgbo --binary-in, bin/wtovl) */
			case 1014: E->st.keep_text = (strcmp(optarg, "host") != 0); break;      /* f4: `device` (default) = the bases travel as text and are packed to 2 bits on the GPU (wtz_upload_reads_ascii), `host` = packed while reading */
			case 1013: E->zbatch = atoi(optarg) ? 1 : -1; break;      /* 1 = per-batch z-index, 0 = never (default: by the size of the read set) */
			case 1012: E->shard = 1; break;           /* k-mer index sharded over the devices of --gpus / --gpu-list (or over the ranks) */
			case 1011: o->gpu_list = optarg; break;      /* explicit device ids, e.g. 0,1,2,3 (an id may repeat: two contexts on one GPU, used by the tests) */
			case 1008: o->pool_mb = (uint64_t)atoll(optarg); break;      /* test hook: a pool small enough to force the batch-splitting path */
			case 1007: E->n_workers = (uint32_t)atoi(optarg); if(E->n_workers < 1) E->n_workers = 1; if(E->n_workers > 8) E->n_workers = 8; break;
			case 'h': return usage();
			case 't': break;
			case 'P': E->n_job = (uint32_t)atoi(optarg); break;
			case 'p': E->i_job = (uint32_t)atoi(optarg); break;
			case 'N': E->do_align = 0; break;
			case 'i': sl_push(&o->pbs, optarg); break;
			case 'b': sl_push(&o->obts, optarg); break;
			case 'J': o->min_rdlen = atoi(optarg); break;
			case 'I': sl_push(&o->tbas, optarg); break;
			case 'o': o->output = optarg; break;
			case '9': o->pairoutf = optarg; break;
			case 'S': { int v = atoi(optarg); if(v < 1) return usage(); P->ksave = (uint32_t)v; } break;
			case 'f': o->overwrite = 1; break;
			case 'C': o->write_contained = 0; break;          /* dead switch in the reference: only the side file is suppressed (wtzmo.c:1609,1781) */
			case 'H': { int hk = atoi(optarg); P->hz = (uint32_t)((hk >> 1) & 1); P->hk = (uint32_t)(hk & 1); } break;
			case 'k': P->ksize = (uint32_t)atoi(optarg); break;
			case 'K': P->max_kmer_freq = (uint32_t)atoi(optarg); break;
			case 'z': P->zsize = (uint32_t)atoi(optarg); break;
			case 'Z': P->max_zmer_freq = (uint32_t)atoi(optarg); break;
			case 'U': optval = (float)atof(optarg);
				if(optval < 0){ dot_matrix = 5; break; }
				switch(dot_matrix){
					case 0: P->xvar = (int)optval; break;
					case 1: P->yvar = (int)optval; break;
					case 2: P->min_block_len = (int)optval; break;
					case 3: P->deviation_penalty = optval; break;
					case 4: P->gap_penalty = optval; break;
					default: dot_matrix = 5;
				}
				dot_matrix++;
				break;
			case 'y': P->kwin = (uint32_t)atoi(optarg); break; case 'l': P->max_kmer_var = (uint32_t)atoi(optarg); break; case 'd': P->kovl = (uint32_t)(int)atof(optarg); break; case 'G': E->n_idx = (uint32_t)atoi(optarg); break;
			case 'r': P->ztot = (uint32_t)(int)atof(optarg); break; case 'R': P->zovl = (uint32_t)(int)atof(optarg); break; case 'q': P->win_rep_cutoff = (float)atoi(optarg); break;
			case 'A': P->ncand = (uint32_t)atoi(optarg); break; case 'B': P->nbest = (uint32_t)atoi(optarg); break;
			case 'w': P->w = atoi(optarg); break; case 'e': P->ew = atoi(optarg); break; case 'W': P->W = atoi(optarg); break; case 'M': P->M = atoi(optarg); break;
			case 'X': P->X = atoi(optarg); break; case 'O': P->O = atoi(optarg); break; case 'E': P->E = atoi(optarg); break; case 'T': P->T = atoi(optarg); break;
			case 'L': sl_push(&o->ovls, optarg); break;
			case 'F': sl_push(&o->flts, optarg); break;
			case 's': P->min_score = atoi(optarg); break; case 'm': P->min_id = (float)atof(optarg); break; case 'n': refine = 1; break; case 'v': break;
			default: return usage();
		}
	}
	E->keep_order = o->pairoutf != NULL;
	if(o->lib_check){ printf("libwtzmo_hip: %d device(s)\n", wtz_device_count()); return wtz_device_count() > 0 ? 0 : 3; }
	if(o->output == NULL) return usage();
	if(!o->overwrite && strcmp(o->output, "-") && access(o->output, F_OK) == 0){ fprintf(stderr, "File exists! '%s'\n\n", o->output); return usage(); }
	if(o->pbs.n == 0) return usage();
	if(P->ksize > 32 || P->ksize < 5) return usage();
	if(P->zsize > 16 || P->zsize < 5) return usage();
	P->refine = refine;
	if(E->n_idx < 1) E->n_idx = 1;
	if(E->n_job < 1) E->n_job = 1;
	P->max_overhang = 2 * P->xvar; P->kstep = P->kwin / 2; P->dot_matrix = dot_matrix;
	/* devices: --gpu <id> (one), --gpus N (ids 0..N-1) or --gpu-list; every device gets the reads and builds both indexes (replicated) */
	E->ndev = 0;
	if(o->gpu_list){ const char *q = o->gpu_list; while(*q && E->ndev < 8){ E->devs[E->ndev++] = atoi(q); while(*q && *q != ',') q++; if(*q == ',') q++; } }
	else if(o->n_gpus > 1){ for(int d = 0; d < o->n_gpus; d++) E->devs[E->ndev++] = d; }
	if(E->ndev == 0){ E->devs[0] = o->gpu; E->ndev = 1; }
	if(E->ndev > 1 && (E->n_idx > 1 || E->n_workers > 1)){
		fprintf(stderr, "[wtzmo-mi355x] -G / --workers run on one device: --gpus ignored\n"); E->ndev = 1;
	}
	return -1;
}
/* Large inputs on ONE device (configs[3]: 10 Gbp): the all-reads z-mer index (16 B per base, built once, in chunks) beats the per-batch one (rebuilt for every
 * batch's queries + candidates: 8.1 of 28.8 s per configs[3]-shape step) whenever it fits BESIDE the scratch pool - so the pool, which is allocated now, on a
 * helper thread, while the reads are still being parsed, is sized from the input files' sizes (a byte of FASTA is at most a base; gz: x4): what the indexes
 * will need stays free.  The exact test follows once the reads are counted (below); a pipe or an underestimate just means the per-batch form as before. */
static uint64_t pool_auto_bytes(const eng_t *E, const opts_t *o){
	uint64_t pool_auto = 0;
	if(!o->pool_gb && !o->pool_mb && E->ndev == 1 && g_dist.world == 1 && E->n_workers == 1 && E->zbatch <= 0 && !getenv("WTZ_NO_ZALL")){
		uint64_t est = 0; int known = 1;
		for(int k = 0; k < o->pbs.n + o->tbas.n; k++){
			const char *fn = k < o->pbs.n ? o->pbs.a[k] : o->tbas.a[k - o->pbs.n]; struct stat sb;
			if(stat(fn, &sb) != 0 || !S_ISREG(sb.st_mode)){ known = 0; break; }
			const size_t ln = strlen(fn);
			est += (ln > 3 && !strcmp(fn + ln - 3, ".gz")) ? (uint64_t)sb.st_size * 4 : (uint64_t)sb.st_size;
		}
		uint64_t fr_b = 0, tot_b = 0;
		if(known && est > WTZ_ZALL_MIN_BASES && wtz_device_memory(E->devs[0], &fr_b, &tot_b) == WTZ_OK){
			const uint64_t need = zall_bytes(est);
			if(fr_b > need + (56ull << 30)){ pool_auto = fr_b - need - (8ull << 30); if(pool_auto > (128ull << 30)) pool_auto = 128ull << 30; }      /* 8 GB: the arena, and the estimate against the exact count */
		}
	}
	return pool_auto;
}
/* ---- load reads (wtzmo.c:1691-1729) ---- */
static uint32_t reads_from(eng_t *E, hx_reader_t *fr, int min_rdlen){
	hx_str_t name = {0}, seq = {0}; uint32_t n = 0;
	while(hx_reader_seq(fr, &name, &seq)){
		if((int)seq.n < min_rdlen) continue;
		hx_store_add(&E->st, name.s ? name.s : "", name.n, seq.s ? seq.s : "", seq.n);
		n++;
	}
	hx_reader_close(fr); free(name.s); free(seq.s);
	return n;
}
static void load_reads(eng_t *E, opts_t *o){
	hx_reader_t *fr = hx_reader_open(o->pbs.a, o->pbs.n);
	if(fr == NULL){ fprintf(stderr, " -- Cannot open %s --\n", o->pbs.a[0]); DIE_NOW(); }
	fprintf(stderr, "[wtzmo-mi355x] loading long reads\n");
	E->st.n_rd = reads_from(E, fr, o->min_rdlen);
	hx_sort_exact(E->st.reads, E->st.n_rd, sizeof(hx_read_t), gt_read, NULL);
	if(o->tbas.n == 0) return; else if((fr = hx_reader_open(o->tbas.a, o->tbas.n)) == NULL) DIE_NOW();
	E->st.n_qr = reads_from(E, fr, o->min_rdlen);
}
/* the first columns of a line, cut in place at tabs and blanks */
static int split_cols(char *p, char **cols, int max){ int nc = 0; while(nc < max){ cols[nc++] = p; while(*p && *p != '\t' && *p != ' ') p++; if(!*p) break; *p++ = 0; } return nc; }
typedef void (*side_line_fn)(eng_t *E, const hx_names_t *nm, char *line);
static void load_side_input(eng_t *E, const hx_names_t *nm, strlist_t *l, side_line_fn f){
	hx_reader_t *fr = NULL;
	if(!l->n) return; else if((fr = hx_reader_open(l->a, l->n)) == NULL) DIE_NOW();
	while(hx_reader_line(fr) != -1) if(fr->line[0] != '#') f(E, nm, fr->line);
	hx_reader_close(fr);
}
static void clip_line(eng_t *E, const hx_names_t *nm, char *line){      /* -b: name, offset and length of the region that stays */
	char *cols[4];
	if(split_cols(line, cols, 4) < 3) return;
	uint32_t id = hx_names_get(nm, cols[0]); int coff = atoi(cols[1]), clen = atoi(cols[2]);
	if(id == 0xFFFFFFFFu) return;
	hx_read_t *rd = &E->st.reads[id];
	if(coff < 0 || coff + clen > (int)rd->len) return;
	rd->off += (uint64_t)coff; rd->len = (uint32_t)clen;
}
static void mask_line(eng_t *E, const hx_names_t *nm, char *line){ const uint32_t id = hx_names_get(nm, line); if(id != 0xFFFFFFFFu) E->masked[id] = 1; }      /* -F */
static void closed_line(eng_t *E, const hx_names_t *nm, char *line){      /* -L: pairs tested already */
	char *cols[4];
	if(split_cols(line, cols, 4) < 2) return;
	uint32_t a = hx_names_get(nm, cols[0]), b = hx_names_get(nm, cols[1]);
	if(a == 0xFFFFFFFFu || b == 0xFFFFFFFFu) return;
	if(hx_set_put(&E->closed, hx_pair_key(a, b))) order_push(E, hx_pair_key(a, b));
	else order_push(E, hx_pair_key(a, b) | 1u);        /* a repeated -L line is still a put_u64hash of the reference (wtzmo.c:1769): bit 0 marks it for the -9 replay */
}
/* ranks and the form of the z-mer index: split over the parts, all reads at once, or per batch */
static void choose_zindex_form(eng_t *E, const opts_t *o, ctxjob_t *cj){
	if(g_dist.world > 1){
		if(g_dist.world > WTZ_DIST_MAX || !g_dist.bcast || !g_dist.send || !g_dist.recv){ fprintf(stderr, " -- wtzmo_set_dist: bad rank setup --\n"); DIE_NOW(); }
		if(E->n_idx > 1 || E->n_workers > 1 || E->ndev > 1 || E->n_job > 1){ fprintf(stderr, " -- ranks (one process per GPU) exclude -G, -P, --workers and --gpus --\n"); DIE_NOW(); }
	}
	E->zsplit = (g_dist.world > 1 || E->ndev > 1) && !getenv("WTZ_NO_ZSPLIT");
	{ /* all-reads z-index: 16 B per base - with several parts only 1 / nparts of it per device, so the per-batch form starts nparts times later */
	  const uint64_t zparts = E->zsplit ? (g_dist.world > 1 ? (uint64_t)g_dist.world : E->ndev) : 1;
	  int zall = 0;
	  if(E->zbatch == 0 && E->st.nbase > WTZ_ZALL_MIN_BASES * zparts && E->n_workers == 1 && zparts == 1 && !getenv("WTZ_NO_ZALL")){
		/* the contexts (scratch pools) exist by now: does the all-reads index fit into what they left? */
		if(cj->started){ pthread_join(cj->th, NULL); cj->started = 0; cj->joined = 1; }
		uint64_t fr_b = 0, tot_b = 0;
		if(cj->joined && cj->rc == WTZ_OK && wtz_device_memory(E->devs[0], &fr_b, &tot_b) == WTZ_OK && fr_b > zall_bytes(E->st.nbase)){
			zall = 1;
			/* the seed lookup's scratch grows with the tuples of a query (coverage x length: ~450 k at the configs[3] shape = 26 MB per query) and the pool is the smaller one
			 * chosen above: batches of 1 024 queries until the first request has been measured, then what 0.6 of the pool holds (round 5: 2 048 queries had asked for 54.4 GB of a 49 GB main pool before the group list took the place of the dead tuple list) */
			if(!o->max_batch_set) E->cand_cap0 = 1024;      /* until the first request has been measured (cand_batch_cap) */
			fprintf(stderr, "[wtzmo-mi355x] %llu read bases: all-reads z-mer index (%.0f GB of %.0f GB free beside the scratch pool)\n", (unsigned long long)E->st.nbase, zall_bytes(E->st.nbase) / 1e9, fr_b / 1e9);
		}
	  }
	  if(!zall && E->zbatch == 0 && E->st.nbase > WTZ_ZALL_MIN_BASES * zparts && E->n_workers == 1){ E->zbatch = 1; fprintf(stderr, "[wtzmo-mi355x] %llu read bases: the z-mer index is built per batch of queries (--zindex-batch 0 to force the all-reads index)\n", (unsigned long long)E->st.nbase); } }
	if(E->zbatch > 0 && E->n_workers > 1){ fprintf(stderr, " -- --zindex-batch excludes --workers --\n"); DIE_NOW(); }
	{ const uint32_t zb_max = getenv("WTZ_ZBATCH_MAX") ? (uint32_t)atoi(getenv("WTZ_ZBATCH_MAX")) : 1024u;      /* queries per batch when the z-mer index is rebuilt per batch: bounds its size (queries + <= -A candidates each); configs[3]-shape whole job: 36.0 s with 512, 33.3 s with 1 024, 33.1 s with 2 048 */
	  if(E->zbatch > 0 && E->max_batch > zb_max) E->max_batch = zb_max; }
	if(E->shard && (E->n_idx > 1 || E->n_workers > 1)){ fprintf(stderr, " -- --shard-index excludes -G and --workers --\n"); DIE_NOW(); }
}
/* the contexts (created beside the loading: ctxjob_main) get the reads */
static void contexts_upload(eng_t *E, ctxjob_t *cj, const uint64_t *rdoff){
	const uint32_t n_all = E->st.n_all;
	int rc;
	if(cj->started) pthread_join(cj->th, NULL); else if(!cj->joined) ctxjob_main(cj);
	if(cj->rc != WTZ_OK){ fprintf(stderr, " -- wtz_ctx_create failed: %s --\n", cj->err); DIE_NOW(); }
	for(uint32_t d = 0; d < E->ndev; d++){
		E->ctxs[d] = cj->ctxs[d];
		if(E->st.keep_text && E->st.bits == NULL){
			/* f4: seq2basebank on the device (dna.h:397-410); the packed bank comes back once for the other contexts of this process */
			const double ti0 = now_s(); uint64_t n_other = 0;
			rc = wtz_upload_reads_ascii(E->ctxs[d], E->st.text, E->st.nbase, rdoff, E->rdlen, n_all, 0, &n_other); DIE_WTZ(rc, "wtz_upload_reads_ascii");
			const uint64_t nw = (E->st.nbase + 31) / 32;
			E->st.bits = (uint64_t*)hx_realloc(NULL, 8 * (nw + 2)); E->st.capw = nw + 2; E->st.bits[nw] = E->st.bits[nw + 1] = 0;
			rc = wtz_fetch_read_bits(E->ctxs[d], E->st.bits, nw); DIE_WTZ(rc, "wtz_fetch_read_bits");
			free(E->st.text); E->st.text = NULL; E->st.captext = 0;
			{ wtz_counters_t ic; if(wtz_get_counters(E->ctxs[d], &ic) == WTZ_OK){ E->ing_ms = ic.ms_ingest; E->ing_bytes = ic.bytes_ingest_algo; } }
			{ wtz_counters_t ic; if(wtz_get_counters(E->ctxs[d], &ic) == WTZ_OK) fprintf(stderr, "[wtzmo-mi355x] %llu bases packed on the device (%llu not ACGT): kernels %.2f ms = %.0f GB/s, with the copies %.0f ms\n",
				(unsigned long long)E->st.nbase, (unsigned long long)n_other, ic.ms_ingest, ic.ms_ingest > 0 ? (double)ic.bytes_ingest_algo / ic.ms_ingest / 1e6 : 0.0, 1e3 * (now_s() - ti0)); }
			continue;
		}
		rc = wtz_upload_reads(E->ctxs[d], E->st.bits, (E->st.nbase + 31) / 32, rdoff, E->rdlen, n_all); DIE_WTZ(rc, "wtz_upload_reads");
	}
	E->ctx = E->ctxs[0];
	{ wtz_pool_info_t pi; if(wtz_pool_info(E->ctx, &pi) == WTZ_OK) E->main_cap = pi.main_cap * E->ndev; }
}
/* --repeat: every step starts from the state after loading.  The counters of the step are one sub-struct; masks, coverage, closed pairs and the output file follow for the repeats */
static void step_reset(eng_t *E, const opts_t *o, int rep, stale_job_t *stale_job){
	const uint32_t n_all = E->st.n_all; const char *output = o->output;
	memset(&E->step, 0, sizeof E->step);      /* bytes_per_pair = 0: every repeat plans like a cold run, probe range first */
	E->step.last_mask_rate = -1.0; E->step.pair_row_ratio = 1.0;
	if(!rep) return;
	memcpy(E->masked, E->masked0, (size_t)n_all + 1); memset(E->rdcovs, 0, 4 * ((size_t)n_all + 1));
	free(E->closed.tab); memset(&E->closed, 0, sizeof E->closed);
	for(size_t i = 0; i < E->nclosed0; i++) hx_set_put(&E->closed, E->closed0[i]);
	E->n_order = E->n_order0;
	memset(E->closed_touch, 0, 4 * ((size_t)n_all + 1));
	E->pend.rd_id = 0xFFFFFFFFu; E->pend.nhit = E->pend.nmask = E->pend.nclosed = E->pend.nseed = 0;
	if(strcmp(output, "-")){
		/* the previous repeat's file (3 GB at configs[2]) is neither truncated in place nor removed inline: freeing its pages took
		 * ~0.4 s of the next repeat's timed region, and on a side thread BESIDE THE INDEX BUILDS it slowed their device allocations
		 * (z-index 140 -> 800 ms).  A regular file is renamed to <output>.prev and removed by a side thread once this repeat's
		 * index builds are done (stale_start below): at most ONE stale file exists at any time, whatever --repeat says.  Anything that
		 * is not a regular file (/dev/null, a FIFO, a symlink) is never renamed: it is simply opened again. */
		stale_join(stale_job);
		struct stat sb;
		if(lstat(output, &sb) == 0 && S_ISREG(sb.st_mode)){
			unlink(stale_job->path);
			if(rename(output, stale_job->path) == 0) stale_job->pending = 1;
		}
		E->out = fopen(output, "w"); if(E->out == NULL){ fprintf(stderr, " -- Cannot write %s: %s --\n", output, strerror(errno)); DIE_NOW(); } setvbuf(E->out, NULL, _IOFBF, 8u << 20);
	}
	wtz_reset_counters(E->ctx);
}
/* the z-mer index of this context is built AFTER its (last) k-mer index: only the pair stages read it, and the k-mer build's sort buffers (6 B per base) are
 * gone by then - on a 10 Gbp read set the two do not fit side by side next to the scratch pool */
static void build_zindex(eng_t *E, uint32_t zmod){
	const int rc = E->zbatch > 0 ? WTZ_OK : zindex_for_part(E->ctx, E->st.n_rd, zmod, g_dist.world > 1 ? (uint32_t)g_dist.rank : 0u); DIE_WTZ(rc, "wtz_zindex_build");
}
static void ixjobs_join(eng_t *E, pthread_t *ixth, ixjob_t *ixj){
	for(uint32_t d = 1; d < E->ndev; d++){ pthread_join(ixth[d], NULL); if(ixj[d].rc != WTZ_OK){ fprintf(stderr, " -- index build on device %d failed: %s --\n", E->devs[d], ixj[d].err); DIE_NOW(); } }
}
/* between two -G passes: closed filter + exact sort + trim of a read's accumulated candidate rows, as cq_prepare does for a batch's (wtzmo.c:813-823) */
static void g_pass_keep_rows(eng_t *E, uint32_t id, const uint64_t *row, uint32_t nc){
	cand_t *cd = (cand_t*)hx_realloc(NULL, sizeof(cand_t) * (nc + 1));
	for(uint32_t x = 0; x < nc; x++){ cd[x].e = row[x]; cd[x].pidx = 0; cd[x].pad = 0;
		if(hx_set_has(&E->closed, hx_pair_key(id, cd[x].e >> 32))) cd[x].e &= 0xFFFFFFFF00000000ULL; }
	sort_cands_exact(cd, nc);
	while(nc && (uint32_t)cd[nc - 1].e == 0) nc--;
	for(uint32_t x = 0; x < nc; x++) E->rows[(size_t)id * E->stride + x] = cd[x].e;
	E->nrow[id] = nc; free(cd);
}
/* the indexes of a step: the other devices' on their own threads, this context's k-mer index in -G parts (wtzmo.c:1276-1303) or sharded, then its z-mer index; returns the k-mer index seconds */
static double build_indexes(eng_t *E){
	wtz_params_c *P = &E->P; const uint32_t n_rd = E->st.n_rd, n_all = E->st.n_all; int rc;
	pthread_t ixth[8]; ixjob_t ixj[8];
	const uint32_t zmod = E->zsplit ? (g_dist.world > 1 ? (uint32_t)g_dist.world : E->ndev) : 1u;
	for(uint32_t d = 1; d < E->ndev; d++){ ixj[d].ctx = E->ctxs[d]; ixj[d].n_rd = n_rd; ixj[d].K = P->max_kmer_freq; ixj[d].zonly = E->shard; ixj[d].nozidx = E->zbatch > 0; ixj[d].zmod = zmod; ixj[d].zres = d; if(pthread_create(&ixth[d], NULL, ixjob_main, &ixj[d]) != 0) DIE_NOW(); }
	uint32_t pbbeg = 0, pbend = 0, K = P->max_kmer_freq;
	wtz_index_stats_t ist;
	uint32_t *ids = (uint32_t*)hx_realloc(NULL, 4 * ((size_t)n_all + 1));
	if(E->n_idx > 1){ E->step.rows_all = 1; E->rows = (uint64_t*)hx_realloc(E->rows, (size_t)n_all * E->stride * 8); E->nrow = (uint32_t*)hx_realloc(E->nrow, (size_t)n_all * 4); memset(E->nrow, 0, (size_t)n_all * 4); }
	double t_index = 0;
	if(E->shard){
		ixjobs_join(E, ixth, ixj);      /* the other devices' z-index threads use their contexts: join them first */
		const double ti = now_s();
		shard_index_build(E, n_rd, &K);
		t_index += now_s() - ti;
		build_zindex(E, zmod);
	}
	for(uint32_t i_idx = 0; i_idx < E->n_idx && !E->shard; i_idx++){
		pbbeg = pbend; pbend = pbbeg + (n_rd + E->n_idx - 1) / E->n_idx;
		const double ti = now_s();
		rc = wtz_index_build(E->ctx, pbbeg, pbend > n_rd ? n_rd : pbend, &K, &ist); DIE_WTZ(rc, "wtz_index_build");
		t_index += now_s() - ti;
		fprintf(stderr, "[wtzmo-mi355x] index %u/%u: %llu k-mer occurrences, %llu distinct, %llu kept, cutoff %u\n", i_idx + 1, E->n_idx,
			(unsigned long long)ist.n_occ, (unsigned long long)ist.n_distinct, (unsigned long long)ist.n_kept, K);
		if(i_idx + 1 >= E->n_idx){ build_zindex(E, zmod); break; }
		/* just_query pass: accumulate candidate heaps of every unmasked read of this job */
		uint32_t n = 0;
		for(uint32_t j = 0; j < n_rd; j++){ if((j % E->n_job) != E->i_job) continue; if(E->masked[j]) continue; ids[n++] = j; }
		for(uint32_t a = 0; a < n; a += 4096){
			uint32_t m = n - a < 4096 ? n - a : 4096;
			uint64_t *tmp_rows = (uint64_t*)hx_realloc(NULL, (size_t)m * E->stride * 8); uint32_t *tmp_n = (uint32_t*)hx_realloc(NULL, (size_t)m * 4);
			for(uint32_t k = 0; k < m; k++){ memcpy(tmp_rows + (size_t)k * E->stride, E->rows + (size_t)ids[a + k] * E->stride, (size_t)E->stride * 8); tmp_n[k] = E->nrow[ids[a + k]]; }
			rc = wtz_candidates(E->ctx, ids + a, m, tmp_rows, tmp_n); DIE_WTZ(rc, "wtz_candidates");
			for(uint32_t k = 0; k < m; k++) g_pass_keep_rows(E, ids[a + k], tmp_rows + (size_t)k * E->stride, tmp_n[k]);
			free(tmp_rows); free(tmp_n);
		}
	}
	if(!E->shard) ixjobs_join(E, ixth, ixj);
	free(ids); return t_index;
}
/* counters of a context other than E->ctx: work adds up, kernel times of parallel devices do not (the longest counts) */
static void ctx_counters_fold(eng_t *E, wtz_ctx_t *ctx, uint32_t w){
		wtz_counters_t cw; wtz_get_counters(ctx, &cw);
		if(w){ E->step.extra_ms[0] += cw.ms_candidates; E->step.extra_ms[1] += cw.ms_pairs; E->step.extra_ms[2] += cw.ms_winalign; E->step.extra_ms[3] += cw.ms_stitch; E->step.extra_ms[4] += cw.ms_ext; E->step.extra_ms[5] += cw.ms_gap; }
		E->step.extra_u64[0] += cw.cells_shift; E->step.extra_u64[1] += cw.cells_fixed; E->step.extra_u64[2] += cw.cells_global; E->step.extra_u64[3] += cw.bytes_seed_algo; E->step.extra_u64[4] += cw.n_extjobs; E->step.extra_u64[6] += cw.bytes_zmer_algo;
		if(cw.pool_peak > E->step.extra_u64[5]) E->step.extra_u64[5] = cw.pool_peak;
		if(w) wtz_ctx_destroy(ctx); else wtz_reset_counters(ctx);
}
/* the batches of a step: n_run worker batches (+ n_alt alternates on the same contexts), every one with a part per device or rank */
static batch_t *batches_create(eng_t *E, uint32_t nw_run, int nalt, uint64_t pool_bytes){
	const uint32_t nw = nw_run + (uint32_t)nalt; int rc; batch_t *bs = (batch_t*)calloc(nw, sizeof(batch_t));
	const uint32_t nparts = g_dist.world > 1 ? (uint32_t)g_dist.world : (nw_run == 1 ? E->ndev : 1);
	for(uint32_t w = 0; w < nw; w++){
		bs[w].E = E;
		bs[w].nparts = nparts; bs[w].parts = (part_t*)calloc(nparts, sizeof(part_t)); bs[w].spare = (part_t*)calloc(nparts, sizeof(part_t)); bs[w].cparts = bs[w].parts;
		for(uint32_t d = 0; d < nparts; d++){
			part_t *pt = &bs[w].parts[d]; const uint32_t slot = w * nparts + d;
			pt->ext_base = slot < 8 ? (int)slot * 2 : -1;
			if(slot < 8) for(int k = 0; k < 2; k++){ pt->cigs[k] = E->cig_keep[slot * 2 + k]; pt->capcigs[k] = E->cig_keep_cap[slot * 2 + k]; E->cig_keep[slot * 2 + k] = NULL; E->cig_keep_cap[slot * 2 + k] = 0; }
			if(g_dist.world > 1){ pt->remote = (int)d; pt->ctx = d == 0 ? E->ctx : NULL; }       /* part r belongs to rank r */
			else if(w == 0 || (nalt && w == 1)) pt->ctx = E->ctxs[d];       /* the alternate batch runs on the same contexts, never at the same time */
			else { rc = wtz_ctx_clone(E->ctx, pool_bytes, &pt->ctx); DIE_WTZ(rc, "wtz_ctx_clone"); }
		}
		bs[w].ctx = bs[w].parts[0].ctx;
	}
	if(nalt){ bs[0].alt = &bs[1]; bs[1].alt = &bs[0]; bs[1].shares_ctx = 1; }
	return bs;
}
static void batches_destroy(eng_t *E, batch_t *bs, uint32_t nw){
	const uint32_t nparts = nw ? bs[0].nparts : 0;
	for(uint32_t w = 0; w < nw; w++){
		for(uint32_t d = 0; d < nparts; d++){
			part_t *pt = &bs[w].parts[d]; const uint32_t slot = w * nparts + d;
			if((w || d) && pt->ctx && !bs[w].shares_ctx) ctx_counters_fold(E, pt->ctx, w);
			free(pt->cq_ids); free(pt->cq_nr); free(pt->cq_rows);
			free(pt->pq); free(pt->pc); free(pt->sum); free(pt->box_off); free(pt->boxes); free(pt->item_of); free(pt->it_pair); free(pt->it_dir); free(pt->aln);
			for(int k = 0; k < 2; k++){ if(slot < 8){ E->cig_keep[slot * 2 + k] = pt->cigs[k]; E->cig_keep_cap[slot * 2 + k] = pt->capcigs[k]; } else wtz_host_free(pt->cigs[k]); }
		}
		for(uint32_t d = 0; d < nparts; d++){ part_t *sp = &bs[w].spare[d]; free(sp->sum); free(sp->box_off); free(sp->boxes); free(sp->item_of); free(sp->it_pair); free(sp->it_dir); free(sp->aln); }
		free(bs[w].spare);
		free(bs[w].parts); free(bs[w].start_job);
		free(bs[w].bq); free(bs[w].want); free(bs[w].ids); free(bs[w].rows); free(bs[w].nrow); free(bs[w].rowpair); free(bs[w].pf_ids); free(bs[w].pf_rows); free(bs[w].pf_nr);
	}
	free(bs);
}
/* ---- queries: pipelined batches on n_workers contexts (own stream + pool each, indexes shared) ---- */
static void run_queries(eng_t *E, uint64_t pool_bytes){
	const uint32_t n_rd = E->st.n_rd;
	const uint32_t qbeg = E->st.n_qr ? n_rd : 0;
	E->step.qend = E->st.n_qr ? n_rd + E->st.n_qr : n_rd;
	E->step.cursor = qbeg; E->step.B = E->max_batch < E->first_batch ? E->max_batch : E->first_batch;
	if(!E->first_batch_set && E->n_workers == 1){
		/* a job with few queries (a stripe of -P N on a small input) runs them as ONE batch: every batch costs a fixed set of launch
		 * tails (the longest extension of each launch), which outweighs the extra speculation of a large first batch
		 * (measured on the E. coli shape with -P 8: 0.186 -> 0.165 s; any batch size gives the same output) */
		uint32_t nq = 0; for(uint32_t j = qbeg; j < E->step.qend; j++) if((j % E->n_job) == E->i_job) nq++;
		if(nq <= E->max_batch) E->step.B = E->max_batch;
	}
	uint32_t nw = E->step.rows_all ? 1 : E->n_workers;          /* -G keeps per-read heaps that the commit rewrites: one batch at a time */
	/* one worker, one process: a SECOND batch on the same context(s), formed and started in front of the first one's last commit (process_batch);
	 * WTZ_BATCH_OVERLAP=0 / WTZ_RANGE_OVERLAP=0 keep one batch at a time */
	const int nalt = (nw == 1 && g_dist.world == 1 && !E->step.rows_all && !(getenv("WTZ_BATCH_OVERLAP") && !atoi(getenv("WTZ_BATCH_OVERLAP"))) && !(getenv("WTZ_RANGE_OVERLAP") && !atoi(getenv("WTZ_RANGE_OVERLAP")))) ? 1 : 0;
	batch_t *bs = batches_create(E, nw, nalt, pool_bytes); pthread_t th[8];
	if(g_dist.rank > 0){
		/* this rank serves rank 0's requests with its GPU; plan, commit and output are rank 0's */
		part_t *me = &bs[0].parts[0]; me->ctx = E->ctx; me->remote = 0; me->ext_base = -1;
		remote_loop(E, me);
	} else {
		for(uint32_t w = 1; w < nw; w++) pthread_create(&th[w], NULL, worker_main, &bs[w]);
		worker_main(&bs[0]); for(uint32_t w = 1; w < nw; w++) pthread_join(th[w], NULL);
		if(g_dist.world > 1){ wtz_dist_hdr_t h; memset(&h, 0, sizeof h); h.cmd = WTZ_CMD_DONE; g_dist.bcast(&h, sizeof h); }
	}
	batches_destroy(E, bs, nw + (uint32_t)nalt);
}
/* the cloned contexts' counters folded into this context's, the report lines and the --stats line of a step */
static void step_report(eng_t *E, const opts_t *o, double t_step, double t_index){
	const char *statsf = o->statsf;
	wtz_counters_t cn; wtz_get_counters(E->ctx, &cn);
	cn.ms_candidates += E->step.extra_ms[0]; cn.ms_pairs += E->step.extra_ms[1]; cn.ms_winalign += E->step.extra_ms[2]; cn.ms_stitch += E->step.extra_ms[3]; cn.ms_ext += E->step.extra_ms[4]; cn.ms_gap += E->step.extra_ms[5];
	cn.cells_shift += E->step.extra_u64[0]; cn.cells_fixed += E->step.extra_u64[1]; cn.cells_global += E->step.extra_u64[2]; cn.bytes_seed_algo += E->step.extra_u64[3]; cn.n_extjobs += E->step.extra_u64[4]; cn.bytes_zmer_algo += E->step.extra_u64[6];
	if(E->step.extra_u64[5] > cn.pool_peak) cn.pool_peak = E->step.extra_u64[5];
	memset(E->step.extra_ms, 0, sizeof E->step.extra_ms); memset(E->step.extra_u64, 0, sizeof E->step.extra_u64);
	fprintf(stderr, "[wtzmo-mi355x] %llu records, %llu pairs aligned, %llu pair-bp, %.3f s (index %.3f s)\n", (unsigned long long)E->step.nrec, (unsigned long long)E->step.n_pairs, (unsigned long long)E->step.pair_bp, t_step, t_index);
	fprintf(stderr, "[wtzmo-mi355x] host seconds: in GPU-stage calls %.3f, commit %.3f, per-batch z-index %.3f; writer thread: formatting %.3f, write %.3f; waiting for it: %.3f before buffer reuse, %.3f at the end\n", E->step.t_gpu, E->step.t_commit, E->step.t_zbatch, g_ow.t_format, g_ow.t_write, E->step.t_io[0], E->step.t_io[1]);
	fprintf(stderr, "[wtzmo-mi355x] commit sections: candidate rows + closed filter + order %.3f, window depth + seed weights %.3f, hits %.3f; planning the pairs of the ranges %.3f\n", E->step.t_cq[0], E->step.t_cq[1], E->step.t_cq[2], E->step.t_cq[3]);
	fprintf(stderr, "[wtzmo-mi355x] queries prepared ahead of the commit by helper threads: %llu taken, %llu prepared again (their read's closed pairs had moved), %.3f s waited for a helper, %.3f s starting / joining them; merging the queries' results into the global state (flush) %.3f s; the sections below count the committing thread only\n", (unsigned long long)E->step.n_spec_hit, (unsigned long long)E->step.n_spec_miss, E->step.t_spec_wait, E->step.t_spec_ctl, E->step.t_flush);
	fprintf(stderr, "[wtzmo-mi355x] window depth + seed weights in parts: window marks %.3f, running depth %.3f, seed weights %.3f, seed order %.3f\n", E->step.t_cq1[0], E->step.t_cq1[1], E->step.t_cq1[2], E->step.t_cq1[3]);
	fprintf(stderr, "[wtzmo-mi355x] wall seconds per call: candidates %.3f pairs_seed %.3f pairs_windows %.3f pairs_align %.3f cigar_text %.3f\n", E->step.t_call[0], E->step.t_call[1], E->step.t_call[2], E->step.t_call[3], E->step.t_call[4]);
	if(E->step.n_split) fprintf(stderr, "[wtzmo-mi355x] %llu range(s) had to be split after a scratch-pool overflow (planned at %.0f KB per pair)\n", (unsigned long long)E->step.n_split, E->step.bytes_per_pair / 1024.0);
	fprintf(stderr, "[wtzmo-mi355x] %llu batches in %llu ranges on %u worker context(s); speculation: queries %llu/%llu pairs %llu/%llu alignments %llu/%llu (used/planned)\n",
			(unsigned long long)E->step.n_batches, (unsigned long long)E->step.n_ranges, E->step.rows_all ? 1u : E->n_workers, (unsigned long long)E->step.used_queries, (unsigned long long)E->step.spec_queries, (unsigned long long)E->step.used_pairs, (unsigned long long)E->step.spec_pairs, (unsigned long long)E->step.used_items, (unsigned long long)E->step.spec_items);
	fprintf(stderr, "[wtzmo-mi355x] kernel ms: index %.1f zindex %.1f candidates %.1f pairs %.1f winalign %.1f stitch %.1f (K-sw3 wave %.1f, K-sw2 gaps %.1f); cells shift %llu fixed %llu global %llu; pool peak %.2f GB\n",
		cn.ms_index, cn.ms_zindex, cn.ms_candidates, cn.ms_pairs, cn.ms_winalign, cn.ms_stitch, cn.ms_ext, cn.ms_gap, (unsigned long long)cn.cells_shift, (unsigned long long)cn.cells_fixed, (unsigned long long)cn.cells_global, cn.pool_peak / 1073741824.0);
	if(statsf){ FILE *sf = fopen(statsf, "a"); if(sf){ fprintf(sf, "%llu\t%llu\t%.6f\t%.6f\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\t%llu\t%llu\t%llu\t%llu\t%llu\t%.3f\t%llu\t%llu\t%llu\t%.3f\t%llu\t%llu\t%llu\t%.4f\t%llu\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\t%llu\t%llu\n", (unsigned long long)E->step.n_pairs, (unsigned long long)E->step.pair_bp, t_step, t_index,
			cn.ms_index, cn.ms_zindex, cn.ms_candidates, cn.ms_pairs, cn.ms_winalign, cn.ms_stitch, (unsigned long long)cn.cells_shift, (unsigned long long)cn.cells_fixed, (unsigned long long)cn.cells_global, (unsigned long long)cn.bytes_seed_algo, (unsigned long long)E->step.nrec,
			cn.ms_ext, (unsigned long long)cn.n_extjobs, (unsigned long long)E->step.used_queries, (unsigned long long)cn.pool_peak, cn.ms_gap, (unsigned long long)E->step.n_ranges, (unsigned long long)E->step.n_split, (unsigned long long)cn.bytes_zmer_algo, E->ing_ms, (unsigned long long)E->ing_bytes,
			E->step.t_gpu, E->step.t_commit, E->step.t_cq[0], E->step.t_cq[1], E->step.t_cq[2], E->step.t_cq[3], (unsigned long long)E->step.n_batches, (unsigned long long)E->step.spec_queries); fclose(sf); } }      /* columns 25-32 (round 6): host seconds in the device-stage calls / in the commit / its four sections, batches, planned queries */
}
static void write_side_files(eng_t *E, const opts_t *o){
	const char *output = o->output, *pairoutf = o->pairoutf; const uint32_t n_rd = E->st.n_rd;
	if(o->write_contained && strcmp(output, "-")){
		char *maskf = (char*)hx_realloc(NULL, strlen(output) + 16); sprintf(maskf, "%s.contained", output);
		FILE *mf = fopen(maskf, "w");
		for(uint32_t i = 0; i < n_rd; i++) if(E->masked[i]) fprintf(mf, "%s\n", E->st.reads[i].name);
		fclose(mf); free(maskf);
	}
	if(pairoutf){
		/* the reference lists the pairs in the iteration order of its hash set: replay the insertions (wtz_host.h, hx_refslots) */
		FILE *pf = fopen(pairoutf, "w");
		hx_refslots_t T; hx_refslots_init(&T, 1023);                 /* init_u64hash(1023), wtzmo.c:138 */
		for(size_t i = 0; i < E->n_order; i++){ if(E->closed_order[i] & 1u) hx_refslots_touch(&T); else hx_refslots_put(&T, E->closed_order[i]); }
		for(uint64_t k = 0; k < T.size; k++) if(T.full[k]) fprintf(pf, "%s\t%s\n", E->st.reads[(uint32_t)(T.slot[k] >> 33)].name, E->st.reads[(uint32_t)((T.slot[k] & 0xFFFFFFFFu) >> 1)].name);
		fclose(pf); free(T.slot); free(T.full);
	}
}
#ifdef WTZ_AS_LIB
int wtzmo_main(int argc, char **argv){
	optind = 1;
#else
int main(int argc, char **argv){
#endif
	eng_t *E = (eng_t*)calloc(1, sizeof(eng_t));
	E->st.keep_text = 1;        /* --ingest device */
	E->bpp_decay = getenv("WTZ_BPP_DECAY") ? atof(getenv("WTZ_BPP_DECAY")) : 0.0;      /* experiment: 0 = the estimate only grows (default), e.g. 0.85 = it may fall by 15 % per range */
	wtz_params_c *P = &E->P;
	opts_t o; memset(&o, 0, sizeof o); pthread_mutex_init(&E->mu, NULL); pthread_cond_init(&E->cv, NULL);
	{ const int r = parse_options(argc, argv, E, &o); if(r >= 0) return r; }
	const char *output = o.output, *statsf = o.statsf; static ctxjob_t cj; memset(&cj, 0, sizeof cj);
	cj.P = P; cj.pool_bytes = o.pool_mb ? o.pool_mb << 20 : (o.pool_gb ? o.pool_gb << 30 : pool_auto_bytes(E, &o)); cj.ndev = E->ndev; for(uint32_t d = 0; d < E->ndev; d++) cj.devs[d] = E->devs[d];
	cj.started = (pthread_create(&cj.th, NULL, ctxjob_main, &cj) == 0);      /* from here to the join every error path leaves through DIE_NOW (_exit): exit() would tear HIP down under that thread */
	load_reads(E, &o);
	const uint32_t n_rd = E->st.n_rd, n_all = E->st.n_all;
	fprintf(stderr, "[wtzmo-mi355x] %u reads (+%u query-only), %llu bp\n", n_rd, E->st.n_qr, (unsigned long long)E->st.nbase);
	E->masked = (uint8_t*)calloc((size_t)n_all + 1, 1);
	E->rdcovs = (uint32_t*)calloc((size_t)n_all + 1, 4);
	E->closed_touch = (uint32_t*)calloc((size_t)n_all + 1, 4);
	g_pend_eng = E;
	hx_names_t nm; hx_names_build(&nm, E->st.reads, n_rd);
	load_side_input(E, &nm, &o.obts, clip_line); load_side_input(E, &nm, &o.flts, mask_line); load_side_input(E, &nm, &o.ovls, closed_line); free(nm.tab);
	/* ---- device ---- */
	const uint64_t pool_bytes = o.pool_mb ? o.pool_mb << 20 : o.pool_gb << 30;
	E->rdlen = (uint32_t*)hx_realloc(NULL, 4 * ((size_t)n_all + 1));
	uint64_t *rdoff = (uint64_t*)hx_realloc(NULL, 8 * ((size_t)n_all + 1));
	{ uint64_t tot = 0; uint32_t nq = E->st.n_qr ? E->st.n_qr : n_rd, b0 = E->st.n_qr ? n_rd : 0;
	  for(uint32_t i = 0; i < n_all; i++){ E->rdlen[i] = E->st.reads[i].len; rdoff[i] = E->st.reads[i].off; }
	  for(uint32_t i = 0; i < nq; i++) tot += E->rdlen[b0 + i];
	  E->avg_rdlen = nq ? (uint32_t)(tot / nq) : 10000; if(E->avg_rdlen == 0) E->avg_rdlen = 1; }        /* wtzmo.c:361-368 */
	choose_zindex_form(E, &o, &cj);
	contexts_upload(E, &cj, rdoff); free(rdoff);
	/* page-lock the first worker's CIGAR text buffer while the indexes are built (pinning ~100 MB takes about as long as they do) */
	pthread_t pin_th; int pin_started = 0;
	if(E->do_align && E->cig_keep[0] == NULL){
		uint64_t cap = E->st.nbase / 4 * 3; if(cap < ((uint64_t)16 << 20)) cap = (uint64_t)16 << 20; if(cap > ((uint64_t)256 << 20)) cap = (uint64_t)256 << 20;
		E->cig_keep_cap[0] = E->cig_keep_cap[1] = cap;
		pin_started = (pthread_create(&pin_th, NULL, pin_main, E) == 0);
		if(!pin_started) E->cig_keep_cap[0] = E->cig_keep_cap[1] = 0;
	}
	E->out = strcmp(output, "-") ? fopen(output, "w") : stdout;
	if(E->out == NULL){ fprintf(stderr, " -- Cannot write %s --\n", output); exit(1); }
	setvbuf(E->out, NULL, _IOFBF, 8u << 20);
	E->stride = P->ncand + 1;
	E->pend.rd_id = 0xFFFFFFFFu;
	/* --repeat: run the whole overlap phase several times on the reads already resident in HBM (benchmarking) */
	E->masked0 = (uint8_t*)hx_realloc(NULL, (size_t)n_all + 1); memcpy(E->masked0, E->masked, (size_t)n_all + 1); E->n_order0 = E->n_order;      /* the -F and -L preloads */
	E->closed0 = (uint64_t*)hx_realloc(NULL, 8 * (E->closed.n + 1));
	for(size_t i = 0; i < E->closed.cap; i++) if(E->closed.tab[i] != ~0ULL) E->closed0[E->nclosed0++] = E->closed.tab[i];
	if(statsf){ FILE *sf = fopen(statsf, "w"); if(sf) fclose(sf); }
	stale_job_t stale_job; memset(&stale_job, 0, sizeof stale_job);
	stale_job.path = (char*)hx_realloc(NULL, strlen(output) + 16); sprintf(stale_job.path, "%s.prev", output);
	for(int rep = 0; rep < o.repeat; rep++){
		step_reset(E, &o, rep, &stale_job);
		if(E->binary_out && g_dist.rank == 0){      /* the name table: ids in the records are this run's read ids */
			const char **nmv = (const char**)hx_realloc(NULL, sizeof(char*) * ((size_t)n_all + 1));
			for(uint32_t i = 0; i < n_all; i++) nmv[i] = E->st.reads[i].name;
			if(wtz_ovlb_write_header(E->out, n_all, nmv, E->rdlen) != 0){ fprintf(stderr, " -- cannot write the binary overlap header --\n"); DIE_NOW(); }
			free(nmv);
		}
		out_start(E->out, E->st.reads, E->binary_out);
		if(g_hook) g_hook(rep, 0);
		const double t0 = now_s();
		const double t_index = build_indexes(E);
		stale_start(&stale_job);       /* index builds (and their device allocations) are done: drop the previous repeat's file in the background */
		/* ---- queries: pipelined batches on n_workers contexts (own stream + pool each, indexes shared) ---- */
		if(pin_started){ pthread_join(pin_th, NULL); pin_started = 0; }
		run_queries(E, pool_bytes);
		flush_pending(E);
		{ const double tw0 = now_s(); out_finish(); E->step.t_io[1] += now_s() - tw0; }
		const double t1 = now_s();
		if(strcmp(output, "-")) fclose(E->out); else fflush(stdout);
		if(g_hook) g_hook(rep, 1);
		step_report(E, &o, t1 - t0, t_index);
	}
	stale_join(&stale_job); if(stale_job.pending) unlink(stale_job.path);
	free(stale_job.path);
	write_side_files(E, &o);
	for(int w = 0; w < 16; w++) wtz_host_free(E->cig_keep[w]);
	for(uint32_t d = 0; d < E->ndev; d++) wtz_ctx_destroy(E->ctxs[d]);
	free(E->cq.cand); free(E->cq.seeds); free(E->cq.dep);
	if(E->spec){ for(uint32_t k = 0; k < CQ_RING; k++){ free(E->spec->ring[k].w.cand); free(E->spec->ring[k].w.seeds); free(E->spec->ring[k].w.dep); } free(E->spec); }
	free(E->closed_touch);
	free(E->masked0); free(E->closed0); free(o.pbs.a); free(o.flts.a); free(o.ovls.a); free(o.obts.a); free(o.tbas.a);
	return 0;
}
