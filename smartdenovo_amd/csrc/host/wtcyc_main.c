/*
 * wtcyc_main.c — drop-in `wtcyc`: every read aligned against its own reverse complement (kswx_align, kswx.h:1495-1502), the alignment line (-a) and the
 * trimmed region of reads that fold back on themselves (-o).  Same options, same usage text, same output as the reference's wtcyc.c run with `-t 1`.
 *
 * Host (this file, plain C): options, the reader, the selection by -P / -p, output_alignment (wtcyc.c:75-90) in read order.
 * Device (libwtzmo_hip.so): reads are taken in blocks bounded by a byte budget; a block is uploaded as text (wtz_upload_reads_ascii) and ONE wtz_alignx_batch
 * call aligns all of its reads: q_read = t_read, q_rev = 1 (the query is the reverse-complement view of the same uploaded read), I = D = O.
 * There is no CPU implementation of the alignment in this program: without a HIP device it exits with an error.
 *
 * Where this program stops and the reference does not: a read longer than 65 535 bases (the limit of the batch services) and a read with a character outside
 * ACGTacgt (the reference indexes its 4 x 4 matrix out of bounds there) end the run with exit status 1 and a message that names the read, before anything of
 * the read's block is written.  An empty record gives the line of a read without a hit, as the reference's does.  -t is accepted and ignored.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wtzmo_hip.h"
#include "wtz_tool.h"

typedef struct { int32_t score, tb, te, qb, qe, aln, mat, mis, ins, del; } wc_kswx_t;      /* kswx_t */

static int usage(void){
	printf(
	"WTCYC: Align long read against its reverse complementary\n"
	"SMARTdenovo: Ultra-fast de novo assembler for high noisy long reads\n"
	"Author: Jue Ruan <ruanjue@gmail.com>\n"
	"Version: 1.0\n"
	"Usage: wtcyc [options] <long_read_file>\n"
	"Options:\n"
	" -t <int>    Number of threads, [1]\n"
	" -P <int>    Total parallel jobs, [1]\n"
	" -p <int>    Index of current job (0-based), [0]\n"
	"             Suppose to run it parallelly in 60 nodes. For node1, -P 60 -p 0; node2, -P 60 -p 1, ...\n"
	" -o <string> Output of reads' regions after trimming, [-]\n"
	" -a <string> Output of alignments, [NULL]\n"
	" -f          Force overwrite output file\n"
	" -s <int>    Mininum alignment score, [400]\n"
	" -m <int>    Mininum alignment identity, [0.7]\n"
	" -M <int>    Alignment penalty: match, [2]\n"
	" -X <int>    Alignment penalty: mismatch, [-5]\n"
	" -O <int>    Alignment penalty: gap open, [-3]\n"
	" -E <int>    Alignment penalty: gap extension, [-1]\n"
	" -T <int>    Alignment penalty: read end clipping, 0: distable HSP extension, otherwise set to -30 or other [-100]\n"
	" -W <int>    Bandwidth, [800]\n"
	"\n"
	"Example: \n"
	"$> wtcyc -t 32 wt.fa -fo wt.zmo.cyc -a wt.zmo.cyc.info\n"
	"\n"
	);
	return 1;
}

#define num_diff(a, b) (((a) < (b)) ? ((b) - (a)) : ((a) - (b)))
/* wtcyc.c:75-90 */
static void output_alignment(const char *name, int seqlen, wc_kswx_t x, int ms, float mi, FILE *alno, FILE *cbto){
	int bp;
	float identity;
	identity = (1.0 * x.mat) / (x.aln + 1);
	if(alno) fprintf(alno, "%s\t%d\t%d\t%0.3f\t%d\t%d\t%d\t%d\n", name, seqlen, x.score, identity, x.tb, x.te, seqlen - x.qe, seqlen - x.qb);
	if(x.score >= ms && identity >= mi){
		if((x.tb == 0 || x.te == seqlen) && (num_diff(x.tb, seqlen - x.qe) < 50 && num_diff(x.te, seqlen - x.qb) < 50)){
			bp = (x.tb + x.te) / 2;
			if(bp < seqlen / 2){
				fprintf(cbto, "%s\t%d\t%d\t%d\n", name, bp, seqlen - bp, seqlen);
			} else {
				fprintf(cbto, "%s\t%d\t%d\t%d\n", name, 0, bp, seqlen);
			}
		}
	}
}

typedef struct {
	wtz_ctx_t *ctx; int W, O, E, T, ms; float mi; FILE *alno, *cbto;
	hx_store_t st; ht_block_t blk;                   /* the block: names, lengths, the bases as text */
	wtz_dp_problem_t *pr; wtz_alignx_result_t *rs; uint32_t *slot; size_t cap;
} wc_t;

static int wc_align(void *user, uint32_t at, uint32_t step){
	wc_t *C = (wc_t*)user;
	return wtz_alignx_batch(C->ctx, C->pr + at, step, C->W, C->O, C->O, C->E, C->T, C->rs + at, NULL, 0);
}

/* one block: upload, one wtz_alignx_batch over its non-empty reads (halved on WTZ_E_POOL), the lines in read order */
static void wc_block(wc_t *C){
	hx_store_t *st = &C->st;
	const uint32_t n = st->n_all;
	if(n == 0) return;
	if(n > C->cap){
		C->cap = n; C->slot = (uint32_t*)hx_realloc(C->slot, 4 * (size_t)n);
		C->pr = (wtz_dp_problem_t*)hx_realloc(C->pr, sizeof(wtz_dp_problem_t) * n); C->rs = (wtz_alignx_result_t*)hx_realloc(C->rs, sizeof(wtz_alignx_result_t) * n);
	}
	uint32_t m = 0;
	for(uint32_t i = 0; i < n; i++){
		C->slot[i] = UINT32_MAX;
		if(st->reads[i].len == 0) continue;          /* an empty record: no hit, nothing for the device */
		wtz_dp_problem_t *p = &C->pr[m]; memset(p, 0, sizeof *p);
		p->q_read = p->t_read = i; p->q_rev = 1; p->t_rev = 0; p->q_strand = p->t_strand = 1; p->q_len = p->t_len = (int32_t)st->reads[i].len;
		C->slot[i] = m++;
	}
	if(m){
		ht_block_upload(C->ctx, &C->blk, st);
		ht_halving(m, wc_align, C, "wtz_alignx_batch", "read", 1);
	}
	for(uint32_t i = 0; i < n; i++){
		wc_kswx_t x; memset(&x, 0, sizeof x);            /* KSWX_NULL */
		if(C->slot[i] != UINT32_MAX && C->rs[C->slot[i]].found){
			const wtz_alignx_result_t *r = &C->rs[C->slot[i]];
			x.score = r->score; x.tb = r->tb; x.te = r->te; x.qb = r->qb; x.qe = r->qe; x.aln = r->aln; x.mat = r->mat; x.mis = r->mis; x.ins = r->ins; x.del = r->del;
		}
		if(x.score >= 0) output_alignment(st->reads[i].name, (int)st->reads[i].len, x, C->ms, C->mi, C->alno, C->cbto);      /* wtcyc.c:169 */
	}
	ht_block_done(st);
}

int main(int argc, char **argv){
	char *alnf = NULL, *cbtf = NULL;
	int c, n_job = 1, i_job = 0, W = 800, M = 2, X = -5, O = -3, E = -1, T = -100, ms = 400, overwrite = 0;
	ht_devopt_t dev = { 0, 0, 0, (uint64_t)256 << 20 };
	float mi = 0.7;
	static const struct option longopts[] = { HT_LONGOPTS("block-bytes"), {NULL, 0, NULL, 0} };
	while((c = getopt_long(argc, argv, "ht:P:p:o:a:fs:m:M:X:O:E:W:T:", longopts, NULL)) != -1){
		switch(c){
			case 'h': return usage();
			case 't': break;
			case 'P': n_job = atoi(optarg); break;
			case 'p': i_job = atoi(optarg); break;
			case 'a': alnf = optarg; break;
			case 'o': cbtf = optarg; break;
			case 'f': overwrite = 1; break;
			case 's': ms = atoi(optarg); break;
			case 'm': mi = atof(optarg); break;
			case 'M': M = atoi(optarg); break;
			case 'X': X = atoi(optarg); break;
			case 'O': O = atoi(optarg); break;
			case 'E': E = atoi(optarg); break;
			case 'W': W = atoi(optarg); break;
			case 'T': T = atoi(optarg); break;
			default: if(!ht_devopt(&dev, c, optarg)) return usage();
		}
	}
	if(optind == argc) return usage();
	if(ms < 1) ms = 1;
	if(n_job < 1) n_job = 1;
	if(alnf && !overwrite && strcmp(alnf, "-") && access(alnf, F_OK) == 0){
		fprintf(stderr, "File exists! '%s'\n\n", alnf);
		return usage();
	}
	if(cbtf && !overwrite && strcmp(cbtf, "-") && access(cbtf, F_OK) == 0){
		fprintf(stderr, "File exists! '%s'\n\n", cbtf);
		return usage();
	}
	if(ht_no_device("wtcyc", "alignment")) return 1;
	wtz_params_c P; ht_default_params(&P);
	P.M = M; P.X = X; P.O = O; P.E = E; P.T = T;
	wc_t C; memset(&C, 0, sizeof C);
	C.ctx = ht_ctx_create(&dev, &P);
	C.W = W; C.O = O; C.E = E; C.T = T; C.ms = ms; C.mi = mi; C.st.keep_text = 1;
	C.alno = alnf ? ((strcmp(alnf, "-") == 0) ? stdout : fopen(alnf, "w")) : NULL;
	C.cbto = cbtf ? ((strcmp(cbtf, "-") == 0) ? stdout : fopen(cbtf, "w")) : stdout;
	if((alnf && !C.alno) || !C.cbto){ fprintf(stderr, " -- cannot open an output file for writing --\n"); return 1; }
	hx_reader_t *fr = hx_reader_open(argv + optind, argc - optind);
	if(fr == NULL){ fprintf(stderr, " -- cannot open '%s' --\n", argv[optind]); return 1; }
	hx_str_t name = {0}, seq = {0};
	uint64_t n_rd = 0;
	while(hx_reader_seq(fr, &name, &seq)){
		if(((int)(n_rd ++) % n_job) != i_job) continue;
		ht_check_record("read", &name, &seq);
		if(C.st.n_all && C.st.nbase + seq.n > dev.block) wc_block(&C);
		hx_store_add(&C.st, name.s, name.n, seq.s, seq.n);
	}
	wc_block(&C);
	hx_reader_close(fr);
	wtz_ctx_destroy(C.ctx);
	if(C.cbto && C.cbto != stdout) fclose(C.cbto);
	if(C.alno && C.alno != stdout) fclose(C.alno);
	return 0;
}
