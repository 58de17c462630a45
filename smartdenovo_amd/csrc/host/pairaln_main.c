/*
 * pairaln_main.c — drop-in `pairaln`: record 1 against record 2, record 3 against record 4, ... (kswx_align_with_cigar, kswx.h:1513-1520), one line per pair and
 * strand and, with -a, the three-line picture of the alignment.  Same options, same usage text, same output as the reference's pairaln.c.
 *
 * Host (this file, plain C): options, the reader, the pairing, the three fprintf of pairaln.c:107-109 in input order.
 * Device (libwtzmo_hip.so): pairs are taken in blocks bounded by a byte budget; a block is uploaded as text (wtz_upload_reads_ascii), ONE wtz_alignx_batch call
 * aligns all of its problems (query = record 1, target = record 2; with -s a second problem per pair with t_rev = 1, which is pairaln.c:103) and, with -a, ONE
 * wtz_pwtext_batch call renders all pictures from (qb, tb) and the CIGAR slices that call returned.
 * There is no CPU implementation of the alignment in this program: without a HIP device it exits with an error.
 *
 * Where this program stops and the reference does not: a record longer than 65 535 bases (the limit of the batch services), a record with a character outside
 * ACGTacgt (the reference indexes its 4 x 4 matrix out of bounds there), -W above 1 023 and a negative -W together with -T < 0 end the run with exit status 1
 * and a message (that names the record), before anything of the record's block is written.  So does a pair whose extended hit lies further off the diagonal than the
 * band of kswx.h:1452-1461 allows (WTZ_E_STATE of wtz_alignx_batch): there ksw_global2 returns MINUS_INF (the reference prints a score of -1073741824) and walks back
 * through trace bytes it never wrote, so the rest of that line is not defined.  With -s the unrelated strand of a pair can be such a case.  A pair with an empty record gives the line of a pair without a hit
 * and an empty picture, as the reference's does (tests/golden/pairaln_manifest.json, "empty_record").  A trailing unpaired record is dropped (pairaln.c:94).
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wtzmo_hip.h"
#include "wtz_tool.h"

#define PA_MAXW 1023

static int usage(void){
	printf(
	"Program: pairaln\n"
	" pairaln read paired sequences (fasta or fastq) from STDIN, here is an example input\n"
	" >read1\n"
	" AAGGCCTT\n"
	" >read2\n"
	" AAGCCTT\n"
	" and so on, read3, read4, ...\n"
	" pairaln will perform alignment on read1 and read2, read3 and read4, ...\n"
	" The default parameters is used for pacbio long reads\n"
	"Usage: pairaln [options]\n"
	"Author: Jue Ruan\n"
	"Options:\n"
	" -s          Try both strands\n"
	" -M <int>    Alignment penalty: match, [2]\n"
	" -X <int>    Alignment penalty: mismatch, [-5]\n"
	" -O <int>    Alignment penalty: insertion or deletion, [-3]\n"
	" -E <int>    Alignment penalty: gap extension, [-1]\n"
	" -T <int>    Alignment penalty: read end clipping, 0: distable HSP extension, otherwise set to -100 or other [-100]\n"
	" -W <int>    Bandwidth, [800]\n"
	" -a          Output alignment\n"
	"\n"
	);
	return 1;
}

typedef struct {
	wtz_ctx_t *ctx; int W, O, E, T, bidir, has_aln;
	hx_store_t st; ht_block_t blk;                   /* the block: names, lengths, the bases as text; records 2k and 2k + 1 are pair k */
	wtz_dp_problem_t *pr; wtz_alignx_result_t *rs; wtz_pwtext_in_t *in; wtz_pwtext_result_t *tx, *tx2; uint32_t *slot; size_t cap_pr;
	uint32_t *cigar; uint64_t cap_cigar; char *text; uint64_t cap_text;
	uint32_t m; uint64_t cig_at, need_text;          /* of the block in hand: its problems, its CIGAR words so far, the bytes of its pictures */
} pa_t;

/* problems [at, at + step): their CIGARs go behind those of the problems before */
static int pa_align(void *user, uint32_t at, uint32_t step){
	pa_t *C = (pa_t*)user;
	const int rc = wtz_alignx_batch(C->ctx, C->pr + at, step, C->W, C->O, C->O, C->E, C->T, C->rs + at, C->cigar + C->cig_at, C->cap_cigar - C->cig_at);
	if(rc == WTZ_E_STATE){      /* which pair: its problem alone */
		for(uint32_t i = at; i < at + step; i++) if(wtz_alignx_batch(C->ctx, C->pr + i, 1, C->W, C->O, C->O, C->E, C->T, C->rs + i, NULL, 0) == WTZ_E_STATE){
			fprintf(stderr, " -- records '%s' and '%s' (%c strand): the extended hit lies outside the band of its global alignment, where the reference reads memory it never wrote: %s --\n",
				C->st.reads[C->pr[i].q_read].name, C->st.reads[C->pr[i].t_read].name, "+-"[C->pr[i].t_rev], wtz_last_error());
			HT_EXIT();
		}
	}
	if(rc != WTZ_OK) return rc;
	uint64_t used = 0;
	for(uint32_t i = at; i < at + step; i++){ C->rs[i].cigar_off += C->cig_at; used += C->rs[i].cigar_len; }
	C->cig_at += used;
	return WTZ_OK;
}
/* the offsets of the sizing call stay: pictures lie one behind the other, a part of the block renders into its own stretch of the buffer */
static int pa_render(void *user, uint32_t at, uint32_t step){
	pa_t *C = (pa_t*)user;
	const uint64_t t0 = C->tx[at].text_off, t1 = at + step < C->m ? C->tx[at + step].text_off : C->need_text;
	return wtz_pwtext_batch(C->ctx, C->pr + at, C->in + at, step, C->cigar, C->cig_at, C->tx2 + at, C->text + t0, t1 - t0);
}

/* one block: upload, wtz_alignx_batch over the problems of its pairs without an empty record (halved on WTZ_E_POOL), wtz_pwtext_batch over the same problems, the lines */
static void pa_block(pa_t *C){
	hx_store_t *st = &C->st;
	const uint32_t n = st->n_all, npair = n / 2, nd = C->bidir == 3 ? 2 : 1;
	if(n == 0) return;
	if((size_t)npair * nd > C->cap_pr){
		C->cap_pr = (size_t)npair * nd;
		C->pr = (wtz_dp_problem_t*)hx_realloc(C->pr, sizeof(wtz_dp_problem_t) * C->cap_pr); C->rs = (wtz_alignx_result_t*)hx_realloc(C->rs, sizeof(wtz_alignx_result_t) * C->cap_pr);
		C->in = (wtz_pwtext_in_t*)hx_realloc(C->in, sizeof(wtz_pwtext_in_t) * C->cap_pr); C->tx = (wtz_pwtext_result_t*)hx_realloc(C->tx, sizeof(wtz_pwtext_result_t) * C->cap_pr); C->tx2 = (wtz_pwtext_result_t*)hx_realloc(C->tx2, sizeof(wtz_pwtext_result_t) * C->cap_pr);
		C->slot = (uint32_t*)hx_realloc(C->slot, 4 * C->cap_pr);
	}
	uint32_t m = 0; uint64_t need_cigar = 2;
	for(uint32_t k = 0; k < npair; k++) for(uint32_t d = 0; d < nd; d++){
		C->slot[k * nd + d] = UINT32_MAX;
		if(st->reads[2 * k].len == 0 || st->reads[2 * k + 1].len == 0) continue;      /* an empty record: no hit, nothing for the device */
		wtz_dp_problem_t *p = &C->pr[m]; memset(p, 0, sizeof *p);
		p->q_read = 2 * k; p->t_read = 2 * k + 1; p->q_rev = 0; p->t_rev = d; p->q_strand = p->t_strand = 1;
		p->q_len = (int32_t)st->reads[2 * k].len; p->t_len = (int32_t)st->reads[2 * k + 1].len;
		need_cigar += (uint64_t)p->q_len + (uint64_t)p->t_len + 2;
		C->slot[k * nd + d] = m++;
	}
	if(m){
		if(need_cigar > C->cap_cigar){ C->cap_cigar = need_cigar; C->cigar = (uint32_t*)hx_realloc(C->cigar, 4 * (size_t)need_cigar); }
		ht_block_upload(C->ctx, &C->blk, st);
		C->m = m; C->cig_at = 0;
		ht_halving(m, pa_align, C, "wtz_alignx_batch", "pair", 1);
		if(C->has_aln){
			for(uint32_t i = 0; i < m; i++){
				wtz_pwtext_in_t *x = &C->in[i]; memset(x, 0, sizeof *x);
				x->qb = C->rs[i].qb; x->tb = C->rs[i].tb; x->cigar_off = C->rs[i].cigar_off; x->cigar_len = C->rs[i].cigar_len;
			}
			if(wtz_pwtext_batch(C->ctx, C->pr, C->in, m, C->cigar, C->cig_at, C->tx, NULL, 0) != WTZ_OK) ht_die("wtz_pwtext_batch");
			C->need_text = C->tx[m - 1].text_off + 3ull * ((uint64_t)C->tx[m - 1].cols + 1);
			if(C->need_text > C->cap_text){ C->cap_text = C->need_text; C->text = (char*)hx_realloc(C->text, (size_t)C->need_text); }
			ht_halving(m, pa_render, C, "wtz_pwtext_batch", "picture", 1);
		}
	}
	for(uint32_t k = 0; k < npair; k++){
		const hx_read_t *r1 = &st->reads[2 * k], *r2 = &st->reads[2 * k + 1];
		for(uint32_t d = 0; d < nd; d++){
			wtz_alignx_result_t x; memset(&x, 0, sizeof x);            /* KSWX_NULL */
			const uint32_t s = C->slot[k * nd + d];
			if(s != UINT32_MAX && C->rs[s].found) x = C->rs[s];
			fprintf(stdout, "%s\t%c\t%d\t%d\t%d"  , r1->name, '+', (int)r1->len, x.qb, x.qe);
			fprintf(stdout, "\t%s\t%c\t%d\t%d\t%d", r2->name, "+-"[d], (int)r2->len, x.tb, x.te);
			if(x.aln) fprintf(stdout, "\t%d\t%0.2f\t%d\t%d\t%d\t%d\n", x.score, 1.0 * x.mat / x.aln, x.mat, x.mis, x.ins, x.del);
			else fprintf(stdout, "\t%d\t-nan\t%d\t%d\t%d\t%d\n", x.score, x.mat, x.mis, x.ins, x.del);      /* 0 / 0 as the reference's build prints it (manifest: "no_hit") */
			if(C->has_aln){
				if(s != UINT32_MAX) fwrite(C->text + C->tx[s].text_off, 1, 3 * ((size_t)C->tx[s].cols + 1), stdout);
				else fwrite("\n\n\n", 1, 3, stdout);
			}
		}
	}
	ht_block_done(st);
}

int main(int argc, char **argv){
	int c, W = 800, M = 2, X = -5, O = -3, E = -1, T = -100, bidir = 1, has_aln = 0;
	ht_devopt_t dev = { 0, 0, 0, (uint64_t)64 << 20 };
	static const struct option longopts[] = { HT_LONGOPTS("block-bytes"), {NULL, 0, NULL, 0} };
	while((c = getopt_long(argc, argv, "hsW:M:X:O:E:T:a", longopts, NULL)) != -1){
		switch(c){
			case 'h': return usage();
			case 's': bidir = 3; break;
			case 'a': has_aln = 1; break;
			case 'W': W = atoi(optarg); break;
			case 'M': M = atoi(optarg); break;
			case 'X': X = atoi(optarg); break;
			case 'O': O = atoi(optarg); break;
			case 'E': E = atoi(optarg); break;
			case 'T': T = atoi(optarg); break;
			default: if(!ht_devopt(&dev, c, optarg)) return usage();
		}
	}
	if(W > PA_MAXW || W < -PA_MAXW){ fprintf(stderr, " -- -W %d: this build aligns with a bandwidth of at most %d --\n", W, PA_MAXW); return 1; }
	if(W < 0 && T < 0){ fprintf(stderr, " -- -W %d with -T %d: a negative bandwidth (the exact band) needs -T 0 or above --\n", W, T); return 1; }
	if(ht_no_device("pairaln", "alignment")) return 1;
	wtz_params_c P; ht_default_params(&P);
	P.M = M; P.X = X; P.O = O; P.E = E; P.T = T;
	pa_t C; memset(&C, 0, sizeof C);
	C.ctx = ht_ctx_create(&dev, &P);
	C.W = W; C.O = O; C.E = E; C.T = T; C.bidir = bidir; C.has_aln = has_aln; C.st.keep_text = 1;
	char *dash[1] = { (char*)"-" };
	hx_reader_t *fr = optind < argc ? hx_reader_open(argv + optind, argc - optind) : hx_reader_open(dash, 1);
	if(fr == NULL){ fprintf(stderr, " -- cannot open '%s' --\n", optind < argc ? argv[optind] : "-"); return 1; }
	hx_str_t name[2] = {{0}, {0}}, seq[2] = {{0}, {0}};
	for(;;){
		if(!hx_reader_seq(fr, &name[0], &seq[0]) || !hx_reader_seq(fr, &name[1], &seq[1])) break;      /* pairaln.c:94: a trailing unpaired record is dropped */
		uint64_t add = 0;
		for(int k = 0; k < 2; k++){
			ht_check_record("record", &name[k], &seq[k]);
			add += seq[k].n;
		}
		if(C.st.n_all && C.st.nbase + add > dev.block) pa_block(&C);
		for(int k = 0; k < 2; k++) hx_store_add(&C.st, name[k].s, name[k].n, seq[k].s, seq[k].n);
	}
	pa_block(&C);
	hx_reader_close(fr);
	wtz_ctx_destroy(C.ctx);
	fflush(stdout);
	return 0;
}
