/*
 * isg_walk_hip.inc -- the walk engine (isg_walk.h) on the device, and replay-schedule update_P on top of it.
 *
 * update_P (mcmc.c:799-861) draws K L Dirichlets from the one stream in (cluster, locus) order (mcmc.c:846-857); where a
 * Dirichlet starts depends on how many attempts every gamma before it needed (random.c:233-250).  Rounds 1 and 2 walked that
 * recurrence on the host (counts down, 6e4 dependent gammas at 26 ns, frequencies up: 1.8 ms of every 9.7 ms iteration at
 * config 3, 24 of 155 ms at config 5).  The shapes are the allele counts + 1 -- known when k_count is done -- so every accept
 * bit is a pure function of (shape, stream position): wk_table evaluates them on the whole chip, the hierarchical walk
 * resolves every Dirichlet's start, and k_pdirich_at then draws all Dirichlets at once at their resolved positions with the
 * plain sequential sampler, checking that each consumed exactly what the resolution said.  Nothing crosses PCIe but the
 * final stream position.  A window miss or a failed check sends the sweep to the host loop (same values either way).
 */
#include "isg_walk_plan.h"

__global__ void __launch_bounds__(64) k_wk_bpred(WkCenterArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_bpred_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
__global__ void __launch_bounds__(256) k_wk_centers(WkCenterArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_centers_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
/* dynamic LDS: the body's (wk_table_lds_bytes) + the skip-ahead tables at tab_off.  MODE (WK_MODE_EXACT: update_P, WK_MODE_INTERVAL: update_ZQ)
 * is a template parameter: each instance only carries its own attempt test (and shows up under its own name in a profile) */
template <int MODE>
__global__ void __launch_bounds__(256) k_wk_table(WkTableArgs A, unsigned tab_off)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	{
		const uint16_t *src = (const uint16_t *)A.tab;
		uint16_t *dst = (uint16_t *)(wk_lds + tab_off);
		for (int k = threadIdx.x; k < (int)(sizeof(isg_wh_tables) / 2); k += blockDim.x) dst[k] = src[k];
	}
	__syncthreads();
	A.tab = (const isg_wh_tables *)(wk_lds + tab_off);
	A.mode = MODE;
	wk_table_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
__global__ void __launch_bounds__(1024) k_wk_block(WkWalkArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_block_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
__global__ void __launch_bounds__(512) k_wk_compose(WkWalkArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_compose_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
__global__ void __launch_bounds__(512) k_wk_top(WkWalkArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_top_body(A, (int)blockDim.x, wk_lds);
}
__global__ void __launch_bounds__(256) k_wk_expand(WkWalkArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_expand_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
__global__ void __launch_bounds__(256) k_wk_final(WkWalkArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_final_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
/* the walk in three launches (isg_walk.h): k_wk_block (k_wk_block_z before a second walk's first segment), k_wk_compose2, k_wk_down */
__global__ void __launch_bounds__(1024) k_wk_block_z(WkWalkArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_zero_body(A, (int)blockIdx.x, (int)blockDim.x);
	wk_block_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
__global__ void __launch_bounds__(512) k_wk_compose2(WkWalkArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_compose2_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}
__global__ void __launch_bounds__(256) k_wk_down(WkWalkArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char wk_lds[];
	wk_down_body(A, (int)blockIdx.x, (int)blockDim.x, wk_lds);
}

/* one run's device buffers and plan */
struct WalkRun {
	WkPlan plan;
	bool plan_ok = false, attrs_set = false;
	int mode = WK_MODE_EXACT;
	DevBuf<WkBlock> d_blk;
	DevBuf<WkSuper> d_sup;
	DevBuf<WkSeg> d_seg;
	DevBuf<int> d_hw, d_ent_sup, d_ent_blk;
	DevBuf<float> d_bpred;
	DevBuf<unsigned char> d_table;
	DevBuf<unsigned short> d_maps;
	DevBuf<unsigned long long> d_T;
	DevBuf<WkState> d_st;
	/* window statistics, carried from run to run */
	double sigma = 1.0, kwin = 4.0, rho_hi = 0.8; /* windows of +-kwin sigma sqrt(gammas): a miss (6e-5 per entry at 4 sigma) costs one sweep by the other path */
	double kwin0 = 0.0; /* what kwin returns to after a clean stretch */
	hvec<unsigned char> stage; /* the plan's arrays on their way to the device */
	int clean = 0;
	float scale = 1.0f;
	int seg_groups = 8192;
	int plan_seg_groups = 0, plan_slack = 0; /* what the current plan was built for */
	long runs = 0, fails = 0;
	/* the tables' rows are evaluated at the columns a row can be entered at only (wk_trim_range); trim_k: their spread in sigma, 0 = the walk's kwin */
	bool trim = true;
	double trim_k = 0.0;
	/* the walk in three launches (k_wk_block, k_wk_compose2, k_wk_down); false, or a plan that does not fit them: the five launches */
	bool fused = true, plan_fused = false;
};
/* INSTRUCT_WALK_TRIM / INSTRUCT_WALK_TRIM_K / INSTRUCT_WALK_FUSED, read where a run's context is created */
static void walk_read_trim_env(WalkRun &w)
{
	w.trim = env_flag(getenv("INSTRUCT_WALK_TRIM"), true);
	w.trim_k = env_double(getenv("INSTRUCT_WALK_TRIM_K"), 0.0, 0.0);
	w.fused = env_flag(getenv("INSTRUCT_WALK_FUSED"), true);
}
#define WK_LDS_LIMIT ((size_t)160 * 1024) /* dynamic LDS a workgroup of the walk kernels may ask for */
static bool walk_fused(const WalkRun &w) { return w.fused && w.plan_fused; }
/* the spread the next plan trims its rows with: it widens with the windows after a miss (walk_adapt) */
static double walk_trim_k(const WalkRun &w)
{
	if (!w.trim) return 0.0;
	if (!(w.trim_k > 0.0)) return w.kwin;
	return w.trim_k * (w.kwin0 > 0.0 ? w.kwin / w.kwin0 : 1.0);
}

/* (re)builds the plan for the current window statistics and makes the buffers fit; false: the run does not fit the engine */
static int walk_prepare(isg_ctx *c, WalkRun &w, const int *gam0_h, int G, int mode, bool reuse, bool *ok, int entry_slack = 0)
{
	*ok = false;
	const double trim_k = walk_trim_k(w);
	if (w.plan_ok && w.mode == mode && w.plan.groups == G && w.plan.rho_hi == w.rho_hi && w.plan.sigma == w.sigma && w.plan.kwin == w.kwin && w.plan.reuse == reuse &&
	    w.plan_seg_groups == w.seg_groups && w.plan_slack == entry_slack && w.plan.trim_k == trim_k) { /* same statistics as last time: same plan (building one costs the host 0.1 ms at 25000 groups) */
		*ok = true;
		return 0;
	}
	WkPlan np;
	if (!wk_plan_build(np, gam0_h, G, w.rho_hi, w.sigma, w.kwin, w.seg_groups, reuse, mode, entry_slack, trim_k)) { w.plan_ok = false; return 0; }
	w.plan_seg_groups = w.seg_groups;
	w.plan_slack = entry_slack;
	const bool same = w.plan_ok && np.blk.size() == w.plan.blk.size() && np.sup.size() == w.plan.sup.size() && np.seg.size() == w.plan.seg.size() &&
			  memcmp(np.blk.data(), w.plan.blk.data(), sizeof(WkBlock) * np.blk.size()) == 0 && memcmp(np.hw.data(), w.plan.hw.data(), sizeof(int) * np.hw.size()) == 0;
	w.mode = mode;
	if (!same) {
		/* the old plan may still be in use by kernels of the previous sweep */
		HIPCHK(hipStreamSynchronize(c->stream));
		w.plan = np;
		HIPCHK(w.d_blk.grow(np.blk.size()));
		HIPCHK(w.d_hw.grow(np.blk.size()));
		HIPCHK(w.d_ent_blk.grow(np.blk.size()));
		HIPCHK(w.d_bpred.grow(np.blk.size()));
		HIPCHK(w.d_sup.grow(np.sup.size()));
		HIPCHK(w.d_ent_sup.grow(np.sup.size()));
		HIPCHK(w.d_table.grow(np.table_bytes + 64));
		HIPCHK(w.d_maps.grow(np.maps_elems + 64));
		HIPCHK(w.d_T.grow((size_t)G + 1));
		if (!w.d_st) HIPCHK(w.d_st.alloc(2)); /* (the word behind the state: WkWalkArgs.fail_in) */
		if (!w.d_seg) HIPCHK(w.d_seg.alloc(WK_MAXSEG));
		{ /* through one page-aligned staging block (see PageAlloc): the plan's own vectors sit anywhere in the heap */
			const size_t b0 = sizeof(WkSeg) * np.seg.size(), b1 = sizeof(WkBlock) * np.blk.size(), b2 = sizeof(WkSuper) * np.sup.size(), b3 = sizeof(int) * np.hw.size();
			const size_t o1 = (b0 + 63) & ~(size_t)63, o2 = o1 + ((b1 + 63) & ~(size_t)63), o3 = o2 + ((b2 + 63) & ~(size_t)63);
			w.stage.resize(o3 + b3 + 64);
			memcpy(w.stage.data(), w.plan.seg.data(), b0);
			memcpy(w.stage.data() + o1, w.plan.blk.data(), b1);
			memcpy(w.stage.data() + o2, w.plan.sup.data(), b2);
			memcpy(w.stage.data() + o3, w.plan.hw.data(), b3);
			HIPCHK(hipMemcpyAsync(w.d_seg, w.stage.data(), b0, hipMemcpyHostToDevice, c->stream));
			HIPCHK(hipMemcpyAsync(w.d_blk, w.stage.data() + o1, b1, hipMemcpyHostToDevice, c->stream));
			HIPCHK(hipMemcpyAsync(w.d_sup, w.stage.data() + o2, b2, hipMemcpyHostToDevice, c->stream));
			HIPCHK(hipMemcpyAsync(w.d_hw, w.stage.data() + o3, b3, hipMemcpyHostToDevice, c->stream));
			HIPCHK(hipStreamSynchronize(c->stream)); /* (the copies are done when this returns) */
		}
		w.plan_ok = true;
	} else { /* the same layout for slightly different statistics */
		w.plan.sigma = np.sigma;
		w.plan.kwin = np.kwin;
		w.plan.rho_hi = np.rho_hi;
		w.plan.trim_k = np.trim_k;
	}
	if (!w.attrs_set) {
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_table<WK_MODE_EXACT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_table<WK_MODE_INTERVAL>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_block, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_compose, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_top, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_expand, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_block_z, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_compose2, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		HIPCHK(hipFuncSetAttribute((const void *)k_wk_down, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
		w.attrs_set = true;
	}
	w.plan_fused = wk_plan_fused_ok(w.plan, WK_LDS_LIMIT);
	*ok = true;
	return 0;
}

struct WalkInputs {
	const int *gam0;
	const unsigned long long *gpos;
	const int *gcnt;
	const float *alo, *ahi;
	isg_wh base;
	const float *tape = nullptr; /* the phase's uniforms as floats, if somebody generated them */
	unsigned long long tape_len = 0;
};
/* where every block's window sits: the shapes' expected rejections per block, their running sums per segment (once per run, all segments) */
static void walk_launch_centers(isg_ctx *c, WalkRun &w, const WalkInputs &in, const char *pname)
{
	WkCenterArgs C;
	C.blk = w.d_blk; C.hw = w.d_hw; C.bpred = w.d_bpred; C.st = w.d_st; C.gam0 = in.gam0; C.gcnt = in.gcnt; C.alo = in.alo; C.ahi = in.ahi; C.seg = w.plan.seg[0]; C.segs = w.d_seg;
	C.mode = w.mode; C.scale = w.scale;
	int nbmax = 0;
	for (const WkSeg &S : w.plan.seg) nbmax = S.nb > nbmax ? S.nb : nbmax;
	prof_begin(c);
	hipLaunchKernelGGL(k_wk_bpred, dim3((unsigned)w.plan.blk.size()), dim3(64), sizeof(float) * 64, c->stream, C);
	hipLaunchKernelGGL(k_wk_centers, dim3((unsigned)w.plan.seg.size()), dim3(256), sizeof(float) * (size_t)nbmax, c->stream, C);
	prof_end(c, pname);
}
/* tables of segment s (stream order: after the walk of segment s - 1, which says where s is entered) */
static void walk_launch_tables(isg_ctx *c, WalkRun &w, const WalkInputs &in, int s, const char *pname)
{
	const WkSeg S = w.plan.seg[s];
	WkTableArgs A;
	A.blk = w.d_blk; A.gam0 = in.gam0; A.gpos = in.gpos; A.gcnt = in.gcnt; A.alo = in.alo; A.ahi = in.ahi; A.table = w.d_table; A.st = w.d_st; A.base = in.base; A.tab = c->d.tab; A.tape = in.tape; A.tape_len = in.tape_len;
	A.seg_b0 = S.b0; A.seg_g0 = S.g0; A.bg = S.bg; A.seg = s; A.mode = w.mode;
	const unsigned tab_off = (unsigned)((w.plan.lds_table + 15) & ~(size_t)15);
	prof_begin(c);
	if (w.mode == WK_MODE_INTERVAL) hipLaunchKernelGGL(k_wk_table<WK_MODE_INTERVAL>, dim3((unsigned)(S.g1 - S.g0)), dim3(256), tab_off + sizeof(isg_wh_tables), c->stream, A, tab_off);
	else hipLaunchKernelGGL(k_wk_table<WK_MODE_EXACT>, dim3((unsigned)(S.g1 - S.g0)), dim3(256), tab_off + sizeof(isg_wh_tables), c->stream, A, tab_off);
	prof_end(c, pname);
}
/* what the first launch of a second walk zeroes in place of the caller's memsets (three-launch walk only) */
struct WalkZero {
	unsigned *words = nullptr;
	int n = 0;
	bool tail = false; /* the per-walk tail of WkState */
};
/* the walk through segment s: block maps, super-block maps, the segment, back down to every group */
static void walk_launch_walk(isg_ctx *c, WalkRun &w, const WalkInputs &in, int s, int strict, int keep_origin, const char *pname, const WalkZero *z = nullptr)
{
	const WkSeg S = w.plan.seg[s];
	WkWalkArgs A;
	A.blk = w.d_blk; A.sup = w.d_sup; A.table = w.d_table; A.maps = w.d_maps; A.ent_sup = w.d_ent_sup; A.ent_blk = w.d_ent_blk; A.T = w.d_T; A.st = w.d_st;
	A.seg = S; A.segno = s; A.mode = w.mode; A.strict = strict; A.keep_origin = keep_origin; A.total_groups = w.plan.groups; A.bpred = w.d_bpred; A.gam0 = in.gam0; A.scale = w.scale;
	A.fail_in = (unsigned *)(w.d_st.get() + 1);
	A.zero_words = nullptr; A.nzero = 0; A.zero_tail = 0;
	prof_begin(c);
	if (walk_fused(w)) {
		if (z) {
			A.zero_words = z->words; A.nzero = z->n; A.zero_tail = z->tail ? 1 : 0;
			hipLaunchKernelGGL(k_wk_block_z, dim3((unsigned)S.nb), dim3(1024), w.plan.lds_block, c->stream, A);
		} else {
			hipLaunchKernelGGL(k_wk_block, dim3((unsigned)S.nb), dim3(1024), w.plan.lds_block, c->stream, A);
		}
		hipLaunchKernelGGL(k_wk_compose2, dim3((unsigned)S.ns), dim3(512), w.plan.lds_compose + (size_t)WK_C2_HDR, c->stream, A);
		hipLaunchKernelGGL(k_wk_down, dim3((unsigned)S.nb), dim3(256), w.plan.lds_down, c->stream, A);
		prof_end(c, pname);
		return;
	}
	hipLaunchKernelGGL(k_wk_block, dim3((unsigned)S.nb), dim3(1024), w.plan.lds_block, c->stream, A);
	hipLaunchKernelGGL(k_wk_compose, dim3((unsigned)S.ns), dim3(512), w.plan.lds_compose, c->stream, A);
	hipLaunchKernelGGL(k_wk_top, dim3(1), dim3(512), w.plan.lds_top, c->stream, A);
	hipLaunchKernelGGL(k_wk_expand, dim3((unsigned)S.ns), dim3(256), w.plan.lds_compose, c->stream, A);
	hipLaunchKernelGGL(k_wk_final, dim3((unsigned)S.nb), dim3(256), (size_t)WK_BG * WK_STRIP, c->stream, A);
	prof_end(c, pname);
}
/* after a run: the next plan's window statistics from this run's (host copy of the state) */
static void walk_adapt(WalkRun &w, const WkState &hs)
{
	w.runs++;
	if (w.kwin0 == 0.0) w.kwin0 = w.kwin;
	if (hs.fail) {
		w.fails++;
		if ((hs.fail & 1u) && w.kwin < 12.0) { /* a window was missed: wider for a while */
			w.kwin *= 1.25;
			w.clean = 0;
		}
		return;
	}
	if (++w.clean >= 512 && w.kwin > w.kwin0) {
		w.kwin = (w.kwin / 1.25 > w.kwin0) ? w.kwin / 1.25 : w.kwin0;
		w.clean = 0;
	}
	if (hs.pred > 0.0 && hs.nblk > 0) {
		const double sc = (double)hs.sum_d / hs.pred;
		if (sc > 0.5 && sc < 2.0) w.scale = (float)(0.7 * w.scale + 0.3 * sc);
	}
	if (hs.ngam > 64.0) {
		const double var = hs.resid2 / hs.ngam;
		double sg = sqrt(var > 0.25 ? var : 0.25);
		if (sg > 3.0) sg = 3.0;
		/* quantised, so that the plan (and its upload) only changes when the statistics really move */
		sg = ceil((0.5 * w.sigma + 0.5 * sg) * 20.0) / 20.0;
		if (sg < 0.9) sg = 0.9;
		w.sigma = sg;
	}
}

/* ------------------------------------------------------------------------------------------ */
/* update_P on the device (replay schedule)                                                     */
/* ------------------------------------------------------------------------------------------ */
struct PDevCtx {
	WalkRun walk;
	int G = 0, NG = 0;          /* groups = (cluster, locus with more than one allele) in stream order; gammas */
	std::vector<int> gam0_h;
	DevBuf<int> d_gam0;      /* [G + 1] */
	DevBuf<int> d_gidx;      /* [NG] index of a gamma's count in d.cnt ([L][Amax][K]) */
	DevBuf<int> d_gcnt;      /* [NG] its count */
	DevBuf<unsigned long long> d_gpos; /* [NG + 1] */
	DevBuf<unsigned> d_part; /* k_pd_gather's totals per chunk of 1024 gammas */
	DevBuf<float> d_tapef;   /* the run's uniforms as floats */
	unsigned long long tape_len = 0;
	bool usable = false;
	int test_abort = 0; /* INSTRUCT_P_TEST_ABORT=n: the n-th device sweep is treated as lost (tests) */
	long sweeps = 0, fallbacks = 0, retried = 0; /* retried: sweeps whose tables were built a second time, with wider windows, after a missed one */
};

/* counts in stream order and the gammas' minimal stream positions: pos[g + 1] = pos[g] + (count == 0 ? 1 : 2) (shape 1 is an
 * exponential draw of ONE uniform, random.c:243-244).  Chunks of 1024 gammas per workgroup: k_pd_gather collects the counts and every
 * chunk's total, k_pd_scan turns them into positions (a chunk's base = the sum of the totals before it). */
__global__ void __launch_bounds__(256) k_pd_gather(const int *cnt, const int *gidx, int ng, int *gcnt, unsigned *part)
{
	__shared__ unsigned red[4];
	const int k0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
	unsigned s = 0;
#pragma unroll
	for (int q = 0; q < 4; q++) {
		if (k0 + q < ng) {
			const int v = cnt[gidx[k0 + q]];
			gcnt[k0 + q] = v;
			s += v == 0 ? 1u : 2u;
		}
	}
	s = wave_sum_u32(s);
	if (lane_id() == 0) red[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(256) k_pd_scan(const int *gcnt, int ng, const unsigned *part, unsigned long long *gpos)
{
	__shared__ unsigned long long red[4];
	__shared__ unsigned sm[256 / 64 + 1];
	const int t = threadIdx.x;
	unsigned long long b = 0;
	for (int k = t; k < (int)blockIdx.x; k += 256) b += part[k];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) b += __shfl_down(b, o, 64);
	if (lane_id() == 0) red[t >> 6] = b;
	__syncthreads();
	const unsigned long long base = red[0] + red[1] + red[2] + red[3];
	const int k0 = ((int)blockIdx.x * 256 + t) * 4;
	unsigned u[4], s = 0;
#pragma unroll
	for (int q = 0; q < 4; q++) {
		u[q] = (k0 + q < ng) ? (gcnt[k0 + q] == 0 ? 1u : 2u) : 0u;
		s += u[q];
	}
	unsigned tot;
	unsigned pre = block_excl_scan<256>(s, sm, &tot);
#pragma unroll
	for (int q = 0; q < 4; q++) {
		if (k0 + q < ng) gpos[k0 + q] = base + pre;
		pre += u[q];
	}
	if (k0 <= ng && ng < k0 + 4) gpos[ng] = base + pre; /* the thread whose chunk holds the end: the run's minimal consumption */
}

/* every Dirichlet at its resolved position: freq[k][j][.] ~ Dirichlet(count + 1) (mcmc.c:846-857, rdirich random.c:264-280), and the
 * check that it consumed what the resolution said.  One lane per group. */
__global__ void __launch_bounds__(128) k_pdirich_at(DevView d, isg_wh base, const int *gam0, const int *gidx, const int *gcnt, const unsigned long long *gpos,
						     const unsigned long long *T, int G, WkState *st)
{
	const int g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= G || st->fail) return;
	const int g0 = gam0[g], n = gam0[g + 1] - g0;
	const unsigned long long p = gpos[g0] + 2ull * T[g], p1 = gpos[g0 + n] + 2ull * T[g + 1];
	isg_cursor c;
	c.s = isg_wh_jump(d.tab, base, p);
	c.used = 0;
	c.tape = nullptr;
	double sum = 0;
	for (int a = 0; a < n; a++) {
		const double v = isg_rgamma(&c, (double)gcnt[g0 + a] + 1.0);
		/* gidx = (j Amax + a) K + k  ->  freq[(j Amax + a) KP + k] */
		const int ix = gidx[g0 + a], row = ix / d.K, k = ix - row * d.K;
		d.freq[(size_t)row * d.KP + k] = v;
		sum += v;
	}
	for (int a = 0; a < n; a++) {
		const int ix = gidx[g0 + a], row = ix / d.K, k = ix - row * d.K;
		d.freq[(size_t)row * d.KP + k] /= sum;
	}
	if ((unsigned long long)c.used != p1 - p) atomicOr(&st->fail, 8u);
}

/* groups in the reference's order: for k < K, for j < L with allelenum[j] > min_alleles (mcmc.c:846-857 skips allelenum <= 1;
 * update_P_auto, poly_geno.c:426-434, does not), the alleles of (k, j).  The allotetraploid chain's list -- two groups per (k, j), the second
 * subgenome's counts at cnt + sub_stride -- comes from pgroups_build (isg_pgroups.h) through pdev_create_allo (isg_poly_hip.inc) */
static int pdev_create(isg_ctx *c, PDevCtx **out, int L, int K, int Amax, const int *allelenum, int min_alleles)
{
	*out = nullptr;
	if (!env_flag(getenv("INSTRUCT_P_DEVICE"), true)) return 0;
	PDevCtx *p = new PDevCtx();
	std::vector<int> gidx;
	p->gam0_h.push_back(0);
	for (int k = 0; k < K; k++)
		for (int j = 0; j < L; j++) {
			const int Aj = allelenum[j];
			if (Aj <= min_alleles) continue;
			if (Aj > WK_NGMAX) { delete p; return 0; } /* more alleles than a group's bit rows hold: the host loop */
			for (int a = 0; a < Aj; a++) gidx.push_back((j * Amax + a) * K + k);
			p->gam0_h.push_back((int)gidx.size());
		}
	p->G = (int)p->gam0_h.size() - 1;
	p->NG = (int)gidx.size();
	if (p->G < 1) { delete p; return 0; }
	p->walk.seg_groups = (int)env_int(getenv("INSTRUCT_WALK_SEG"), 12800, 64, INT_MAX); /* (config 3's 25000 groups: two segments, measured best of 4096 .. 25600; config 5 does not care) */
	p->walk.kwin = env_double(getenv("INSTRUCT_WALK_K"), p->walk.kwin, 1.0);
	walk_read_trim_env(p->walk);
	p->test_abort = (int)env_int(getenv("INSTRUCT_P_TEST_ABORT"), 0);
	*out = p; /* the context owns it from here on, whatever fails below (usable only at the end) */
	HIPCHK(p->d_gam0.alloc((size_t)p->G + 1));
	HIPCHK(p->d_gidx.alloc(p->NG));
	HIPCHK(p->d_gcnt.alloc(p->NG));
	HIPCHK(p->d_gpos.alloc((size_t)p->NG + 1));
	HIPCHK(p->d_part.alloc((size_t)(p->NG + 1023) / 1024 + 2));
	p->tape_len = 2ull * (unsigned long long)p->NG + (unsigned long long)(1.7 * p->NG) + (unsigned long long)(12.0 * sqrt((double)p->NG)) + 8192ull;
	HIPCHK(p->d_tapef.alloc(p->tape_len));
	HIPCHK(hipMemcpy(p->d_gam0, p->gam0_h.data(), sizeof(int) * (p->G + 1), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(p->d_gidx, gidx.data(), sizeof(int) * p->NG, hipMemcpyHostToDevice));
	p->usable = true;
	return 0;
}

/* the counts in d.cnt gathered into stream order and scanned into the gammas' minimal positions (no stream position goes in) */
static void pdev_launch_prep(isg_ctx *c, PDevCtx *p)
{
	const unsigned nchunk = (unsigned)((p->NG + 1023) / 1024) + 1u; /* (+ 1: gpos[NG] when NG is a multiple of 1024) */
	prof_begin(c);
	hipLaunchKernelGGL(k_pd_gather, dim3(nchunk), dim3(256), 0, c->stream, (const int *)c->d.cnt, (const int *)p->d_gidx, p->NG, p->d_gcnt, p->d_part);
	hipLaunchKernelGGL(k_pd_scan, dim3(nchunk), dim3(256), 0, c->stream, (const int *)p->d_gcnt, p->NG, (const unsigned *)p->d_part, p->d_gpos);
	prof_end(c, "k_pd_prep");
}
/* what update_P's look brings back (the mailbox's slot MAIL_P) */
struct MailP {
	WkState st;
	unsigned long long tail[2]; /* minimal consumption of the run; rejected attempts in all */
};
static_assert(sizeof(MailP) <= MAIL_G - MAIL_P, "update_P's slot of the mailbox");

/* counts are in d.cnt (k_count has been launched; prepped: k_pd_gather and k_pd_scan too, behind update_alpha's look).  *done = false: nothing
 * was consumed, the caller runs the host loop. */
static int pdev_update_P_once(isg_ctx *c, PDevCtx *p, bool *done, bool second, bool *again, bool prepped)
{
	*done = false;
	*again = false;
	if (!p || !p->usable) return 0;
	bool ok = false;
	if (walk_prepare(c, p->walk, p->gam0_h.data(), p->G, WK_MODE_EXACT, true, &ok)) return 1;
	if (!ok) { p->usable = false; return 0; }
	WalkRun &w = p->walk;
	HIPCHK(hipMemsetAsync(w.d_st, 0, sizeof(WkState), c->stream));
	if (!prepped) pdev_launch_prep(c, p);
	/* the run's stretch of the stream as floats: at most 2 NG uniforms if nothing is rejected, about half an attempt per gamma on top */
	prof_begin(c);
	hipLaunchKernelGGL(k_tapef, dim3((unsigned)((p->tape_len + 2047) / 2048)), dim3(256), 0, c->stream, c->d.tab, c->rng, (unsigned long long)p->tape_len, p->d_tapef);
	prof_end(c, "k_tapef_P");
	WalkInputs in;
	in.gam0 = p->d_gam0; in.gpos = p->d_gpos; in.gcnt = p->d_gcnt; in.alo = nullptr; in.ahi = nullptr; in.base = c->rng;
	in.tape = p->d_tapef; in.tape_len = p->tape_len;
	walk_launch_centers(c, w, in, "k_wk_centers_P");
	for (int s = 0; s < (int)w.plan.seg.size(); s++) {
		walk_launch_tables(c, w, in, s, "k_wk_table_P");
		walk_launch_walk(c, w, in, s, 0, 0, "k_wk_walk_P");
	}
	prof_begin(c);
	hipLaunchKernelGGL(k_pdirich_at, dim3((unsigned)((p->G + 127) / 128)), dim3(128), 0, c->stream, c->d, c->rng, (const int *)p->d_gam0, (const int *)p->d_gidx, (const int *)p->d_gcnt,
			   (const unsigned long long *)p->d_gpos, (const unsigned long long *)w.d_T, p->G, w.d_st);
	prof_end(c, "k_pdirich_at");
	HIPCHK(hipGetLastError());
	MailP *m = mail_slot<MailP>(c, MAIL_P);
	HIPCHK(hipMemcpyAsync(&m->st, w.d_st, sizeof(m->st), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&m->tail[0], p->d_gpos + p->NG, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&m->tail[1], w.d_T + p->G, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	if (look_record(c, AH_LOOK_P)) return 1;
	if (c->la_on) { /* launch-ahead: freq is final if the look says so (if not, it is rewritten and its copies are made again) */
		if (refresh_freqf(c)) return 1;
		ahead_set(&c->ah, AH_FREQF);
	}
	if (look_wait(c, AH_LOOK_P)) return 1;
	WkState hs = m->st;
	const unsigned long long tail[2] = {m->tail[0], m->tail[1]};
	walk_adapt(w, hs);
	if (p->test_abort > 0 && --p->test_abort == 0) hs.fail |= 8u; /* (tests: as if k_pdirich_at's check had failed; the host loop redraws all of freq) */
	if (hs.fail) ahead_wrote_freq(&c->ah);
	if (!second && hs.fail == 1u) { /* only a window was missed (nothing has been drawn: k_pdirich_at does not start then): once more with the wider windows */
		*again = true;
		return 0;
	}
	p->sweeps++;
	if (hs.fail) { /* a window was missed again or a check failed: freq may be partly overwritten, but the host loop rewrites all of it */
		p->fallbacks++;
		return 0;
	}
	host_advance(c, tail[0] + 2ull * tail[1]);
	*done = true;
	return 0;
}
static int pdev_update_P(isg_ctx *c, PDevCtx *p, bool *done, bool prepped = false)
{
	bool again = false;
	if (pdev_update_P_once(c, p, done, false, &again, prepped)) return 1;
	if (!again) return 0;
	p->retried++;
	return pdev_update_P_once(c, p, done, true, &again, false);
}
