/*
 * wtz_lib.cpp — libwtzmo_hip.so: the one translation unit of the library behind the C ABI of include/wtzmo_hip.h.
 *
 * Built with:  hipcc -x hip --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC wtz_lib.cpp
 * (tests/emul/ also compiles this file with g++ -DWTZ_EMUL to run every "kernel" as a host loop; that
 *  build is a debugging aid for containers without a GPU and is never part of the product.)
 *
 * This file holds the kernel name tags, the includes in their order and the small counter / pool-info entry points.  The rest:
 *   wtz_tasks.h, wtz_sw_*.h, ...   device code: the task bodies the launches below run
 *   wtz_dev.h                      device layer, both back ends: errors, launchers, per-call arena, dev_*, timer, sort and scan
 *   wtz_ctx.h                      struct wtz_ctx, its switches, the two scratch pools, create / clone / destroy
 *   wtz_lib_index.h                reads upload and ingest, k-mer index, z-mer index, candidates
 *   wtz_lib_pairs.h                wtz_pairs_seed, wtz_pairs_seed_region, wtz_pairs_windows
 *   wtz_lib_align.h                wtz_pairs_align: lane pipelines, chained K-sw1, K-sw2, K-sw3 extension jobs, fused stitch
 *   wtz_lib_fetch.h                CIGAR fetch and text rendering
 *   wtz_lib_batch.h                the skeleton of the batch services, each step once; wtz_extend_batch, wtz_local_batch, wtz_kext_batch, wtz_align_batch
 *   wtz_lib_glob.h                 wtz_global_batch, wtz_alignx_batch and the CIGAR hand-out they share (included by wtz_lib_batch.h)
 *   wtz_lib_pwtext.h               wtz_pwtext_batch (included by wtz_lib_batch.h)
 *   wtz_lib_hzmaux.h               wtz_hzmaux_batch (included by wtz_lib_batch.h)
 *   wtz_testdp.h                   the test-only wtz_test_dp (included by wtz_lib_batch.h)
 *
 * Execution model: every stage is a flat grid of independent tasks (one lane, wavefront or workgroup per read / query / pair /
 * window), 64-thread workgroups so that each wave is scheduled on its own and the thousands of waves per launch spread over all
 * 256 CUs / 8 XCDs; all per-task scratch and results are carved from one HBM bump pool (wtz_pool_t) with a single 64-bit atomic
 * per allocation.
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdarg.h>
#include <vector>
#include <atomic>
#include <algorithm>

#include "wtz_tasks.h"
#include "wtz_sw_frame.h"
#include "wtz_stitch_fused.h"
#include "wtz_sw_local.h"
#include "wtz_sw_kext.h"
#include "wtz_sw_kglob.h"
#include "wtz_pwtext.h"

/* kernel name tags (rocprofv3 shows wtz_kernel_*<K_pair, ...>) */
struct K_candidates_wg;
struct K_extjob_scalar;
struct K_cigar_text;
struct K_misc;
struct K_gap;
struct K_gap_wide;
struct K_kcount;
struct K_lcount;
struct K_lplan;
struct K_ldp;
struct K_ltb;
struct K_lfold;
struct K_gplan;
struct K_gdp;
struct K_gtb;
struct K_glist;
struct K_poolalloc;
struct K_kfill;
struct K_kinsert;
struct K_khead;
struct K_kdistinct;
struct K_kinsert_total;
struct K_pack_groups;
struct K_kstats;
struct K_pack_cigars;
struct K_pack_windows;
struct K_pair;
struct K_pair_dm;
struct K_pair_big;
struct K_pair_region;
struct K_pair_chain;
struct K_refine;
struct K_pack_ascii;
struct K_pack_fix;
struct K_revcomp_views;
struct K_stitch_fin;
struct K_stitch_left;
struct K_stitch_mid;
struct K_winalign;
struct K_winalign_big;
struct K_zfill; struct K_zread;
struct K_zrun;
struct K_zdistinct;
struct K_zdn;
struct K_zcount;
struct K_extcopy;
struct K_globcopy;
struct K_glob_ring;
struct K_glob_scalar;
struct K_test_ldp;      /* form 65 of wtz_test_dp (wtz_testdp.h): the two launches of a lane pipeline, at K_ldp's / K_ltb's occupancy (wtz_dev.h) */
struct K_test_ltb;

#include "wtz_dev.h"
#include "wtz_ctx.h"
#include "wtz_lib_index.h"
#include "wtz_lib_pairs.h"
#include "wtz_lib_align.h"
#include "wtz_lib_fetch.h"
#include "wtz_lib_batch.h"

extern "C" const char *wtz_last_error(void){ return g_err; }
extern "C" void *wtz_host_alloc(uint64_t n_bytes){ return dev_host_alloc((size_t)(n_bytes ? n_bytes : 1)); }
extern "C" void wtz_host_free(void *p){ if(p) dev_host_free(p); }

extern "C" int wtz_pool_failure_kind(wtz_ctx_t *c){ return c ? c->last_pool_fail : 0; }

extern "C" int wtz_pool_info(wtz_ctx_t *c, wtz_pool_info_t *out){
	if(!c || !out) return wtz_fail(WTZ_E_ARG, "null argument");
	out->main_cap = c->main_bytes; out->main_used = c->main_used_call; out->transient_cap = c->pool_bytes - c->main_bytes; out->transient_peak = c->tpool_peak_call;
	return WTZ_OK;
}

extern "C" int wtz_get_counters(wtz_ctx_t *c, wtz_counters_t *out){
	if(!c || !out) return wtz_fail(WTZ_E_ARG, "null argument");
	*out = c->cnt;
#if !defined(WTZ_EMUL) && defined(WTZ_PROFILE)
	if(c->sw.profile){        /* device phase profiler: Mticks per slot since the last report */
		unsigned long long h[64], z[64]; memset(z, 0, sizeof z);
		if(hipMemcpyFromSymbol(h, HIP_SYMBOL(wtz_prof), sizeof h) == hipSuccess){
			fprintf(stderr, "[phase-profile] Mticks:");
			for(int k = 0; k < 64; k++) fprintf(stderr, " %d:%.1f", k, (double)h[k] / 1e6);
			fprintf(stderr, "\n");
			(void)hipMemcpyToSymbol(HIP_SYMBOL(wtz_prof), z, sizeof z);
		}
	}
#endif
#if !defined(WTZ_EMUL) && defined(WTZ_PROFILE_CAND)
	if(c->sw.profile){
		unsigned long long h[16], z[16]; memset(z, 0, sizeof z);
		if(hipMemcpyFromSymbol(h, HIP_SYMBOL(wtz_prof_cand), sizeof h) == hipSuccess){
			fprintf(stderr, "[cand-profile] Mticks / counts:");
			for(int k = 0; k < 16; k++) fprintf(stderr, " %d:%.1f", k, (double)h[k] / 1e6);
			fprintf(stderr, "\n");
			(void)hipMemcpyToSymbol(HIP_SYMBOL(wtz_prof_cand), z, sizeof z);
		}
	}
#endif
	return WTZ_OK;
}
extern "C" int wtz_reset_counters(wtz_ctx_t *c){ if(!c) return wtz_fail(WTZ_E_ARG, "null context"); memset(&c->cnt, 0, sizeof c->cnt); return WTZ_OK; }
