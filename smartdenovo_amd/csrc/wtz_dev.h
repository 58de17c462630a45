/*
 * wtz_dev.h — the device layer of libwtzmo_hip, both back ends and nothing else: HIP (the product) and the host emulation of the
 * launch geometry (-DWTZ_EMUL, tests only).  Error text, CHK / HIPCHK, the task launchers, the per-call arena and its scope,
 * dev_* memory and copies, wtz_timer, sort and scan.  Everything above this file is written once against these names.
 * Included by wtz_lib.cpp.
 */
static thread_local char g_err[512] = "";      /* wtz_last_error */
#define CHK(call) do { int rc_ = (call); if(rc_ != WTZ_OK) return rc_; } while(0)
static int wtz_fail(int code, const char *fmt, ...){
	va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
	return code;
}
#include <chrono>
static double wtz_wall(){ return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#ifndef WTZ_EMUL
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#define WTZ_LAMBDA __device__
#ifndef WTZ_OCC_WINALIGN
#define WTZ_OCC_WINALIGN 3
#endif
/* The pair kernels are latency-bound, so waves per SIMD pay - until the register budget of the occupancy target forces spills into the loops: with the window scan of
 * round 4 (K_pair needs 135 VGPRs, K_pair_dm 149) five waves = 96 VGPRs and 76 / 42 spilled registers cost more than the fifth wave brings.  configs[2], ms per step:
 * K_pair 1 731 (5 waves) / 773 (4) / 916 (3); K_pair_dm 5 384 / 5 149 / 5 282. */
#ifndef WTZ_OCC_PAIR_DM
#define WTZ_OCC_PAIR_DM 4
#endif
#ifndef WTZ_OCC_PAIR
#define WTZ_OCC_PAIR 5
#endif
/* K_gap (K-sw2 on a wavefront): 213 registers when left alone - two waves per SIMD, where its 12 KB LDS slice lets a CU hold thirteen.  At three (168 registers, 34 spilled
 * values outside the row loop) the K-sw2 stage of a configs[2] step goes from 200 to 188 ms (round 6). */
#ifndef WTZ_OCC_GAP
#define WTZ_OCC_GAP 3
#endif

/* every context owns a non-blocking HIP stream; the API entry points make it current for the calling host thread, so that
 * two host threads can drive two contexts (two batches in flight) whose kernels and copies overlap on the device */
static thread_local hipStream_t g_stream = 0;
#define HIPCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) return wtz_fail(WTZ_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while(0)

/* a raw kernel launch and its check in one statement (the launch cannot be written without the check); returns from the calling function on failure */
#define WTZ_LAUNCH(kernel, blocks, threads, lds_bytes, stream, ...) do { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, stream, __VA_ARGS__); HIPCHK(hipGetLastError()); } while(0)
/* the stream of the calling thread for the rest of the block: restored on every exit path, so that CHK may return from inside (the K-sw2 side stream of wtz_pairs_align) */
struct wtz_stream_scope { hipStream_t prev;
	wtz_stream_scope(hipStream_t st) : prev(g_stream) { g_stream = st; }
	~wtz_stream_scope(){ g_stream = prev; }
	wtz_stream_scope(const wtz_stream_scope&) = delete; wtz_stream_scope &operator=(const wtz_stream_scope&) = delete; };

/* TAG only names the kernel (rocprofv3 shows wtz_kernel_tasks<K_pair_seed, ...>) */
template<typename TAG, typename F> __global__ void __launch_bounds__(64) wtz_kernel_tasks(uint64_t n, F f){
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	WTZ_PROF_BEGIN();
	if(i < n) f(i);
	WTZ_PROF_END();
}
template<typename TAG, typename F> static int wtz_launch(uint64_t n, F f){
	if(n == 0) return WTZ_OK;
	const uint32_t bs = 64;
	uint64_t nb = (n + bs - 1) / bs;
	if(nb > 0x7FFFFFFFull) return wtz_fail(WTZ_E_ARG, "grid too large");
	WTZ_LAUNCH((wtz_kernel_tasks<TAG, F>), (uint32_t)nb, bs, 0, g_stream, n, f);
	return WTZ_OK;
}
/* Heavy, data-dependent tasks (whole pairs / windows / queries): one task per WAVEFRONT, executed by lane 0.  A flat
 * thread-per-task grid serialises up to 64 divergent control flows inside every wave; these tasks are chains of
 * dependent memory operations, so what hides their latency is the number of resident waves (up to 32 per CU, 8192 on
 * the chip), not the lanes of one wave.  Stages whose inner loops are regular get wave-cooperative kernels instead
 * (wtz_wave.h and the wtz_sw_*.h files built on it). */
template<typename TAG, typename F> __global__ void __launch_bounds__(64) wtz_kernel_wave_tasks(uint64_t n, F f){
	const uint64_t i = blockIdx.x;
	WTZ_PROF_BEGIN();
	if(i < n && threadIdx.x == 0) f(i);
	WTZ_PROF_END();
}
/* wave-cooperative tasks: every lane of the wavefront enters the task body (WTZ_LANE / wtz_coop_* inside).
 * These kernels are latency-bound chains: resident waves per SIMD are their throughput, so a TAG can ask the register
 * allocator for a minimum occupancy (wtz_occ<TAG>::waves) instead of the 512-VGPR budget a 64-thread block would get. */
template<typename TAG> struct wtz_occ { static constexpr int waves = 1; };
template<> struct wtz_occ<K_winalign> { static constexpr int waves = WTZ_OCC_WINALIGN; };
template<> struct wtz_occ<K_pair> { static constexpr int waves = WTZ_OCC_PAIR; };
template<> struct wtz_occ<K_pair_region> { static constexpr int waves = WTZ_OCC_PAIR; };      /* K_pair's body + the run cut of the interval form */
template<> struct wtz_occ<K_pair_chain> { static constexpr int waves = WTZ_OCC_PAIR; };       /* K_pair_region's body with chaining_hzmps for the per-window block of the scans */
template<> struct wtz_occ<K_pair_dm> { static constexpr int waves = WTZ_OCC_PAIR_DM; };
template<> struct wtz_occ<K_gap> { static constexpr int waves = WTZ_OCC_GAP; };
/* lane-per-problem K-sw1 (wtz_sw_lane.h): the band lives in 2 x (NC + 1) VGPRs */
#ifndef WTZ_OCC_LDP
#define WTZ_OCC_LDP 2
#endif
template<> struct wtz_occ<K_ldp> { static constexpr int waves = WTZ_OCC_LDP; };
template<> struct wtz_occ<K_gdp> { static constexpr int waves = WTZ_OCC_LDP; };
/* their tracebacks: chains of dependent loads, nothing to keep in registers */
template<> struct wtz_occ<K_ltb> { static constexpr int waves = 8; };
template<> struct wtz_occ<K_gtb> { static constexpr int waves = 8; };
/* form 65 of wtz_test_dp runs the same lane bodies in the same two launches: the same register budgets */
template<> struct wtz_occ<K_test_ldp> { static constexpr int waves = WTZ_OCC_LDP; };
template<> struct wtz_occ<K_test_ltb> { static constexpr int waves = 8; };
template<typename TAG, typename F> __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(wtz_occ<TAG>::waves, 8))) wtz_kernel_coop_tasks(uint64_t n, F f){
	const uint64_t i = blockIdx.x;
	WTZ_PROF_BEGIN();
	if(i < n) f(i);
	WTZ_PROF_END();
}
template<typename TAG, typename F> static int wtz_launch_coop(uint64_t n, F f, uint32_t lds_bytes = WTZ_WAVE_LDS_BYTES){
	if(n == 0) return WTZ_OK;
	if(n > 0x7FFFFFFFull) return wtz_fail(WTZ_E_ARG, "grid too large");
	if(lds_bytes > 65536u){ HIPCHK(hipFuncSetAttribute((const void*)&wtz_kernel_coop_tasks<TAG, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)); }      /* opt in to more than 64 KB of dynamic LDS */
	WTZ_LAUNCH((wtz_kernel_coop_tasks<TAG, F>), (uint32_t)n, 64, lds_bytes, g_stream, n, f);
	return WTZ_OK;
}
/* one task per WORKGROUP of NT threads (wave-size multiples): every thread enters the task body (WTZ_WG_TID / WTZ_WG_SYNC inside) */
template<typename TAG, typename F> __global__ void __launch_bounds__(WTZ_CWG_THREADS) wtz_kernel_wg_tasks(uint64_t n, F f){
	const uint64_t i = blockIdx.x;
	if(i < n) f(i);
}
template<typename TAG, typename F> static int wtz_launch_wg(uint64_t n, F f, uint32_t nthreads, uint32_t lds_bytes){
	if(n == 0) return WTZ_OK;
	if(n > 0x7FFFFFFFull) return wtz_fail(WTZ_E_ARG, "grid too large");
	if(lds_bytes > 65536u){ HIPCHK(hipFuncSetAttribute((const void*)&wtz_kernel_wg_tasks<TAG, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)); }
	WTZ_LAUNCH((wtz_kernel_wg_tasks<TAG, F>), (uint32_t)n, nthreads, lds_bytes, g_stream, n, f);
	return WTZ_OK;
}
template<typename TAG, typename F> static int wtz_launch_wave(uint64_t n, F f){
	if(n == 0) return WTZ_OK;
	if(n > 0x7FFFFFFFull) return wtz_fail(WTZ_E_ARG, "grid too large");
	WTZ_LAUNCH((wtz_kernel_wave_tasks<TAG, F>), (uint32_t)n, 64, WTZ_WAVE_LDS_BYTES, g_stream, n, f);
	return WTZ_OK;
}
/* transient device buffers come from a per-context arena (host-side bump pointer over one persistent allocation, released
 * stack-wise when the API call returns): no hipMalloc/hipFree - and therefore no device-wide synchronisation - on the batch
 * path, which is what lets two contexts overlap.  Requests that do not fit fall back to hipMalloc and are freed at release. */
/* Overflow buffers are not given back to the driver when the call returns: they are kept (up to WTZ_ARENA_CACHE_BYTES) for the next request of about that size.  The
 * index builds of a 1.2 Gbp read set take 2.4 + 2.4 + 1.2 GB of sort buffers beyond the arena; hipFree + hipMalloc of those cost 30 ms on one box and 850 ms on
 * another (every repeat of the step), and each hipFree is a device-wide synchronisation. */
#define WTZ_ARENA_CACHE_BYTES ((size_t)8 << 30)      /* the three sort buffers of a configs[2] index build are 6 GB; what does not fit is given back at once */
struct wtz_arena { uint8_t *base = NULL; size_t cap = 0, top = 0; std::vector<void*> overflow; std::vector<size_t> overflow_bytes; std::vector<std::pair<void*, size_t> > cache; size_t cache_bytes = 0; };
static thread_local wtz_arena *g_arena = NULL;
static void arena_cache_flush(wtz_arena *a);
static int dev_alloc(void **p, size_t n){
	n = (n + 255) & ~(size_t)255; if(n == 0) n = 256;
	if(g_arena && g_arena->top + n <= g_arena->cap){ *p = g_arena->base + g_arena->top; g_arena->top += n; return WTZ_OK; }
	if(g_arena){
		for(size_t i = 0; i < g_arena->cache.size(); i++){
			const size_t cb = g_arena->cache[i].second;
			if(cb >= n && cb <= n + n / 8 + ((size_t)1 << 20)){
				*p = g_arena->cache[i].first; g_arena->cache_bytes -= cb; g_arena->cache.erase(g_arena->cache.begin() + (long)i);
				g_arena->overflow.push_back(*p); g_arena->overflow_bytes.push_back(cb); return WTZ_OK;
			}
		}
	}
	if(hipMalloc(p, n) != hipSuccess){
		(void)hipGetLastError();
		if(g_arena && !g_arena->cache.empty()){ (void)hipDeviceSynchronize(); arena_cache_flush(g_arena); }
		HIPCHK(hipMalloc(p, n));
	}
	if(g_arena){ g_arena->overflow.push_back(*p); g_arena->overflow_bytes.push_back(n); }
	return WTZ_OK;
}
static void arena_cache_flush(wtz_arena *a){ for(size_t i = 0; i < a->cache.size(); i++) (void)hipFree(a->cache[i].first); a->cache.clear(); a->cache_bytes = 0; }
struct wtz_arena_scope { wtz_arena *a, *prev; size_t mark; size_t nover;
	wtz_arena_scope(wtz_arena *ar) : a(ar), prev(g_arena), mark(ar ? ar->top : 0), nover(ar ? ar->overflow.size() : 0) { g_arena = ar; }
	~wtz_arena_scope(){
		g_arena = prev;      /* never left pointing at an arena whose call has returned (its context may be destroyed next; wtz_ctx_destroy itself runs inside a scope) */
		if(!a) return;
		if(a->overflow.size() > nover){
			(void)hipStreamSynchronize(g_stream);
			while(a->overflow.size() > nover){
				void *q = a->overflow.back(); const size_t qb = a->overflow_bytes.back(); a->overflow.pop_back(); a->overflow_bytes.pop_back();
				if(a->cache_bytes + qb <= WTZ_ARENA_CACHE_BYTES && a->cache.size() < 16){ a->cache.push_back(std::make_pair(q, qb)); a->cache_bytes += qb; }
				else (void)hipFree(q);
			}
		}
		a->top = mark;
	} };
static int dev_alloc_persist(void **p, size_t n){
	if(hipMalloc(p, n ? n : 16) == hipSuccess) return WTZ_OK;
	(void)hipGetLastError();
	if(g_arena && !g_arena->cache.empty()){ (void)hipDeviceSynchronize(); arena_cache_flush(g_arena); }      /* the kept overflow buffers go first */
	HIPCHK(hipMalloc(p, n ? n : 16)); return WTZ_OK;
}
static void dev_free_persist(void *p){ if(p) (void)hipFree(p); }
static int dev_h2d(void *d, const void *h, size_t n){ if(n){ HIPCHK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, g_stream)); HIPCHK(hipStreamSynchronize(g_stream)); } return WTZ_OK; }
static int dev_d2h(void *h, const void *d, size_t n){ if(n){ HIPCHK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, g_stream)); HIPCHK(hipStreamSynchronize(g_stream)); } return WTZ_OK; }
static int dev_set(void *d, int v, size_t n){ if(n) HIPCHK(hipMemsetAsync(d, v, n, g_stream)); return WTZ_OK; }
static int dev_d2d(void *d, const void *s, size_t n){ if(n) HIPCHK(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, g_stream)); return WTZ_OK; }
static int dev_sync(){ HIPCHK(hipStreamSynchronize(g_stream)); return WTZ_OK; }

struct wtz_timer { hipEvent_t a, b; bool ok;
	wtz_timer(){ ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
	~wtz_timer(){ if(ok){ (void)hipEventDestroy(a); (void)hipEventDestroy(b); } }
	void start(){ if(ok) (void)hipEventRecord(a, g_stream); }
	double stop(){ float ms = 0; if(ok){ (void)hipEventRecord(b, g_stream); (void)hipEventSynchronize(b); (void)hipEventElapsedTime(&ms, a, b); } return ms; }
	void lap(){ if(ok) (void)hipEventRecord(b, g_stream); }                 /* end mark now, read later */
	double read(){ float ms = 0; if(ok){ (void)hipEventSynchronize(b); (void)hipEventElapsedTime(&ms, a, b); } return ms; } };

static int dev_sort_pairs_u64_u32(uint64_t *keys, uint32_t *vals, uint64_t n, unsigned end_bit){
	if(n < 2) return WTZ_OK;
	uint64_t *k2 = NULL; uint32_t *v2 = NULL; void *tmp = NULL; size_t tmp_bytes = 0; int rc;
	if((rc = dev_alloc((void**)&k2, n * 8))) return rc;
	if((rc = dev_alloc((void**)&v2, n * 4))) return rc;
	rocprim::double_buffer<uint64_t> kb(keys, k2); rocprim::double_buffer<uint32_t> vb(vals, v2);
	hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, kb, vb, (size_t)n, 0u, end_bit, g_stream);
	if(e == hipSuccess && (rc = dev_alloc(&tmp, tmp_bytes)) == WTZ_OK){
		e = rocprim::radix_sort_pairs(tmp, tmp_bytes, kb, vb, (size_t)n, 0u, end_bit, g_stream);
		if(e == hipSuccess) e = hipStreamSynchronize(g_stream);
		if(e == hipSuccess && kb.current() != keys){ e = hipMemcpyAsync(keys, kb.current(), n * 8, hipMemcpyDeviceToDevice, g_stream); if(e == hipSuccess) e = hipMemcpyAsync(vals, vb.current(), n * 4, hipMemcpyDeviceToDevice, g_stream); if(e == hipSuccess) e = hipStreamSynchronize(g_stream); }
	}
	if(e != hipSuccess) return wtz_fail(WTZ_E_HIP, "radix_sort_pairs failed: %s", hipGetErrorString(e));
	return rc;
}
static int dev_exclusive_scan_u32(const uint32_t *in, uint32_t *out, uint64_t n){
	if(n == 0) return WTZ_OK;
	void *tmp = NULL; size_t tmp_bytes = 0;
	hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), g_stream);
	if(e != hipSuccess) return wtz_fail(WTZ_E_HIP, "exclusive_scan failed: %s", hipGetErrorString(e));
	CHK(dev_alloc(&tmp, tmp_bytes));
	e = rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), g_stream);
	if(e == hipSuccess) e = hipStreamSynchronize(g_stream);
	if(e != hipSuccess) return wtz_fail(WTZ_E_HIP, "exclusive_scan failed: %s", hipGetErrorString(e));
	return WTZ_OK;
}
#else  /* ---------------- host emulation of the launch geometry (tests only) ---------------- */
#define WTZ_LAMBDA
template<typename TAG, typename F> static int wtz_launch(uint64_t n, F f){ for(uint64_t i = 0; i < n; i++) f(i); return WTZ_OK; }
template<typename TAG, typename F> static int wtz_launch_wave(uint64_t n, F f){ return wtz_launch<TAG>(n, f); }
template<typename TAG, typename F> static int wtz_launch_coop(uint64_t n, F f, uint32_t = 0){ return wtz_launch<TAG>(n, f); }
template<typename TAG, typename F> static int wtz_launch_wg(uint64_t n, F f, uint32_t, uint32_t){ for(uint64_t i = 0; i < n; i++) f(i); return WTZ_OK; }
/* transient buffers belong to the scope of the API call, as in the product: dev_alloc registers the block with the arena in scope, the scope's
 * destructor frees what was registered since its construction (scopes nest).  An allocation outside a scope would never be released by the
 * product: here it fails, so that the CPU suite catches one. */
struct wtz_arena { std::vector<void*> blocks; };
static thread_local wtz_arena *g_arena = NULL;
static int dev_alloc_persist(void **p, size_t n){ *p = malloc(n ? n : 16); return *p ? WTZ_OK : wtz_fail(WTZ_E_HIP, "malloc(%zu) failed", n); }
static void dev_free_persist(void *p){ free(p); }
static int dev_alloc(void **p, size_t n){
	if(!g_arena){ *p = NULL; return wtz_fail(WTZ_E_STATE, "dev_alloc(%zu) outside the arena scope of an API call", n); }
	CHK(dev_alloc_persist(p, n)); g_arena->blocks.push_back(*p); return WTZ_OK;
}
struct wtz_arena_scope { wtz_arena *a, *prev; size_t mark;
	wtz_arena_scope(wtz_arena *ar) : a(ar), prev(g_arena), mark(ar ? ar->blocks.size() : 0) { g_arena = ar; }
	~wtz_arena_scope(){ g_arena = prev; if(!a) return; while(a->blocks.size() > mark){ free(a->blocks.back()); a->blocks.pop_back(); } } };
static int dev_h2d(void *d, const void *h, size_t n){ if(n) memcpy(d, h, n); return WTZ_OK; }
static int dev_d2h(void *h, const void *d, size_t n){ if(n) memcpy(h, d, n); return WTZ_OK; }
static int dev_set(void *d, int v, size_t n){ if(n) memset(d, v, n); return WTZ_OK; }
static int dev_d2d(void *d, const void *s, size_t n){ if(n) memcpy(d, s, n); return WTZ_OK; }
static int dev_sync(){ return WTZ_OK; }
#include <time.h>
struct wtz_timer { struct timespec t0; void start(){ clock_gettime(CLOCK_MONOTONIC, &t0); }
	double stop(){ struct timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1); return 1e3 * (double)(t1.tv_sec - t0.tv_sec) + 1e-6 * (double)(t1.tv_nsec - t0.tv_nsec); }
	double lapv = 0; void lap(){ lapv = stop(); } double read(){ return lapv; } };
static int dev_exclusive_scan_u32(const uint32_t *in, uint32_t *out, uint64_t n){ uint32_t a = 0; for(uint64_t i = 0; i < n; i++){ uint32_t v = in[i]; out[i] = a; a += v; } return WTZ_OK; }
static int dev_sort_pairs_u64_u32(uint64_t *keys, uint32_t *vals, uint64_t n, unsigned){
	std::vector<std::pair<uint64_t, uint32_t> > v((size_t)n);
	for(uint64_t i = 0; i < n; i++) v[(size_t)i] = std::make_pair(keys[i], vals[i]);
	std::stable_sort(v.begin(), v.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b){ return a.first < b.first; });
	for(uint64_t i = 0; i < n; i++){ keys[i] = v[(size_t)i].first; vals[i] = v[(size_t)i].second; }
	return WTZ_OK;
}
#endif

/* page-locked host memory for the caller's result buffers (wtz_host_alloc) */
#ifndef WTZ_EMUL
static void *dev_host_alloc(size_t n){ void *p = NULL; if(hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess){ (void)hipGetLastError(); return NULL; } return p; }
static void dev_host_free(void *p){ (void)hipHostFree(p); }
#else
static void *dev_host_alloc(size_t n){ return malloc(n); }
static void dev_host_free(void *p){ free(p); }
#endif
