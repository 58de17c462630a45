/*
 * ORACLE — TEST INFRASTRUCTURE ONLY (see ora_util.h).
 * liboracle.so: function-level entry points of the CPU restatement for ctypes-driven tests.
 */
#include "ora_overlap.h"

typedef ora_aln_t shim_aln_t;

int ora_extend_fixed_c(int qlen, uint8_t *q, int tlen, uint8_t *t, int strand, int init_score, int W, int M, int X, int I, int D, int E, int T, shim_aln_t *out, uint32_t *cigar_out){
	ora_swmem_t mem; memset(&mem, 0, sizeof mem); vec_u32 cg = {0};
	*out = ora_extend_fixed(qlen, q, tlen, t, strand, init_score, W, M, X, I, D, E, T, &mem, &cg);
	int n = (int)cg.n; memcpy(cigar_out, cg.a, 4 * cg.n);
	vec_i32_free(&mem.rh); vec_i32_free(&mem.re); vec_i32_free(&mem.zb); vec_u8_free(&mem.z); vec_u32_free(&cg);
	return n;
}
int ora_extend_shift_c(int qlen, uint8_t *q, int tlen, uint8_t *t, int strand, int init_score, int W, int M, int X, int I, int D, int E, int T, shim_aln_t *out, uint32_t *cigar_out){
	ora_swmem_t mem; memset(&mem, 0, sizeof mem); vec_u32 cg = {0};
	*out = ora_extend_shift(qlen, q, tlen, t, strand, init_score, W, M, X, I, D, E, T, &mem, &cg);
	int n = (int)cg.n; memcpy(cigar_out, cg.a, 4 * cg.n);
	vec_i32_free(&mem.rh); vec_i32_free(&mem.re); vec_i32_free(&mem.zb); vec_u8_free(&mem.z); vec_u32_free(&cg);
	return n;
}
int ora_global_c(int qlen, uint8_t *q, int tlen, uint8_t *t, int M, int X, int o_del, int e_del, int o_ins, int e_ins, int w, int *score, uint32_t *cigar_out){
	int8_t mat[16]; for(int i = 0; i < 16; i++) mat[i] = ((i % 4) == (i / 4)) ? (int8_t)M : (int8_t)X;
	ora_swmem_t mem; memset(&mem, 0, sizeof mem); vec_u32 cg = {0};
	*score = ora_global_banded(qlen, q, tlen, t, mat, o_del, e_del, o_ins, e_ins, w, &mem, &cg);
	int n = (int)cg.n; memcpy(cigar_out, cg.a, 4 * cg.n);
	vec_i32_free(&mem.rh); vec_i32_free(&mem.re); vec_i32_free(&mem.zb); vec_u8_free(&mem.z); vec_u32_free(&cg);
	return n;
}
void ora_sort_u64_lo32_desc(uint64_t *v, size_t n){ ora_sort_cand_desc(v, n, NULL); }
#define ORA_U32_GT(a, b) ((a) > (b))
ORA_DEFINE_SORT(ora_sort_u32_asc_impl, uint32_t, ORA_U32_GT)
void ora_sort_u32_asc(uint32_t *v, size_t n){ ora_sort_u32_asc_impl(v, n, NULL); }
int ora_median_c(int32_t *v, int32_t n){ return ora_median(v, n); }

/* ---- f1: align_hzmaux (hzm_aln.h:1684-1775), whole-read form as wtgbo calls it ---- */
#include "ora_hzmaux.h"
int ora_align_hzmaux_c(const uint8_t *tseq, int tlen, const uint8_t *rdseq, int rdlen, const int32_t *prm, float min_sm, int refine, shim_aln_t *out, uint32_t *cigar_out, int cigar_cap){
	static ora_hzmaux_t A;     /* scratch kept across calls */
	ora_auxparams_t P;
	P.zsize = (uint32_t)prm[0]; P.hz = (uint32_t)prm[1]; P.zwin = (uint32_t)prm[2]; P.zstep = (uint32_t)prm[3]; P.zovl = (uint32_t)prm[4]; P.zmax = (uint32_t)prm[5]; P.zvar = (uint32_t)prm[6];
	P.w = prm[7]; P.W = prm[8]; P.ew = prm[9]; P.rw = prm[10]; P.M = prm[11]; P.X = prm[12]; P.I = prm[13]; P.D = prm[14]; P.E = prm[15]; P.T = prm[16];
	ora_hzmaux_index(&A, &P, tseq, (uint32_t)tlen);
	if(!ora_align_hzmaux(&A, &P, rdseq, rdlen, refine, min_sm)) return -1;
	*out = A.hit;
	if((int)A.cigars.n > cigar_cap) return -2;
	memcpy(cigar_out, A.cigars.a, 4 * A.cigars.n);
	return (int)A.cigars.n;
}

/* ---- A2 / A3: the four calls of ref_seed_shim.c (index_wtzmo, query_wtzmo and its groups) over ora_index.h, with the same signatures ---- */
typedef struct { ora_store_t st; ora_kindex_t ix; ora_kparams_t P; vec_kgroup groups; vec_khit hits; vec_u64 cand; } seedx_t;
void *seedx_open(const uint8_t *codes, const uint64_t *off, const uint32_t *len, uint32_t n, const uint32_t *prm){
	seedx_t *s = (seedx_t*)calloc(1, sizeof(seedx_t));
	s->P.ksize = prm[0]; s->P.hk = prm[1]; s->P.ksave = prm[2]; s->P.kovl = prm[3]; s->P.ncand = prm[4];
	for(uint32_t i = 0; i < n; i++){
		ora_read_t r; r.off = s->st.nbase; r.len = len[i]; r.name = NULL;
		vec_read_push(&s->st.reads, r);
		for(uint32_t j = 0; j < len[i]; j++) ora_store_put(&s->st, codes[off[i] + j]);
		s->st.n_rd++;
	}
	if(s->st.bits == NULL) s->st.bits = (uint64_t*)calloc(2, 8);
	return s;
}
void seedx_close(void *h){
	seedx_t *s = (seedx_t*)h;
	ora_kindex_free(&s->ix); free(s->st.bits); vec_read_free(&s->st.reads); vec_kgroup_free(&s->groups); vec_khit_free(&s->hits); vec_u64_free(&s->cand); free(s);
}
int seedx_index(void *h, uint32_t beg, uint32_t end, uint64_t *io){
	seedx_t *s = (seedx_t*)h;
	s->P.max_kmer_freq = (uint32_t)io[0];
	ora_kindex_build(&s->ix, &s->st, beg, end, &s->P);
	io[0] = s->ix.max_kmer_freq; io[1] = s->ix.avg_rdlen; io[2] = s->ix.n_mer; io[3] = s->ix.n_seed;
	return 0;
}
void seedx_table(void *h, uint64_t *mers, uint32_t *cnts, uint8_t *flt, uint64_t *offs, uint32_t *runs, uint32_t *seeds){
	seedx_t *s = (seedx_t*)h;
	for(size_t i = 0; i < s->ix.n_mer; i++){ mers[i] = s->ix.mers[i]; cnts[i] = s->ix.sat[i]; flt[i] = s->ix.flt[i]; offs[i] = s->ix.offs[i]; runs[i] = s->ix.cnts[i]; }
	memcpy(seeds, s->ix.seeds, 4 * s->ix.n_seed);
}
static void seedx_run_groups(seedx_t *s, uint32_t pbid){ ora_query_groups(&s->st, &s->ix, &s->P, pbid, &s->groups, &s->hits); }
uint32_t seedx_query(void *h, uint32_t pbid, uint64_t *row, uint32_t n_io){
	seedx_t *s = (seedx_t*)h;
	seedx_run_groups(s, pbid);
	s->cand.n = 0; vec_u64_reserve(&s->cand, n_io + 1);
	memcpy(s->cand.a, row, 8 * (size_t)n_io); s->cand.n = n_io;
	ora_candidates_from_groups(s->groups.a, s->groups.n, s->P.kovl, s->P.ncand, &s->cand);
	memcpy(row, s->cand.a, 8 * s->cand.n);
	return (uint32_t)s->cand.n;
}
int seedx_groups(void *h, uint32_t pbid, uint32_t *out, uint32_t cap){
	seedx_t *s = (seedx_t*)h;
	seedx_run_groups(s, pbid);
	for(size_t i = 0; i < s->groups.n && i < cap; i++){ out[3 * i] = s->groups.a[i].key; out[3 * i + 1] = s->groups.a[i].ol; out[3 * i + 2] = s->groups.a[i].cnt; }
	return (int)s->groups.n;
}
