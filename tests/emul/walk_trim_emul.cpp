/*
 * walk_trim_emul.cpp -- TEST INFRASTRUCTURE.  The walk engine's kernel bodies (instruct_amd/csrc/isg_walk.h: the very source the device
 * compiles) on the host, with the tables' rows trimmed to the columns a row can be entered at (wk_trim_range): next to the plain
 * sequential sampler, and next to the same tables built untrimmed.  No product path links this.
 */
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../instruct_amd/csrc/isg_walk_plan.h"

struct Run {
	WkPlan P;
	std::vector<WkBlock> blk;
	std::vector<unsigned char> table;
	std::vector<unsigned short> maps;
	std::vector<int> ent_sup, ent_blk;
	std::vector<float> bpred, tape;
	WkState st;
	isg_wh_tables tab;
	isg_wh base;
	int mode = WK_MODE_EXACT, nthreads = 256;
	float scale = 1.0f;
	const int *gam0 = nullptr, *gcnt = nullptr;
	const unsigned long long *gpos = nullptr;
	const float *alo = nullptr, *ahi = nullptr;
};

static bool run_init(Run &R, const int *gam0, int G, double rho_hi, double sigma, double kwin, int seg_groups, bool reuse, int mode, int entry_slack, double trim_k, long s1, long s2, long s3)
{
	if (!wk_plan_build(R.P, gam0, G, rho_hi, sigma, kwin, seg_groups, reuse, mode, entry_slack, trim_k)) return false;
	isg_wh_tables_init(&R.tab);
	R.base.s1 = (uint32_t)(s1 % ISG_M1); R.base.s2 = (uint32_t)(s2 % ISG_M2); R.base.s3 = (uint32_t)(s3 % ISG_M3);
	R.blk = R.P.blk;
	R.table.assign(R.P.table_bytes + 64, 0);
	R.maps.assign(R.P.maps_elems + 64, 0);
	R.ent_sup.assign(R.P.sup.size(), 0);
	R.ent_blk.assign(R.P.blk.size(), 0);
	R.bpred.assign(R.P.blk.size(), 0.f);
	memset(&R.st, 0, sizeof(R.st));
	R.mode = mode;
	R.gam0 = gam0;
	return true;
}
/* the run's uniforms as floats, stream order (what k_tapef hands update_P's tables) */
static void run_make_tape(Run &R, size_t n)
{
	R.tape.resize(n);
	isg_wh s = R.base;
	for (size_t i = 0; i < n; i++) R.tape[i] = (float)isg_wh_next(&s);
}
static void run_segment(Run &R, int s, int strict, bool build_table, int keep_origin, unsigned long long *T)
{
	const WkSeg S = R.P.seg[s];
	std::vector<unsigned char> lds(160 * 1024);
	if (build_table) {
		WkCenterArgs C;
		memset(&C, 0, sizeof(C));
		C.bpred = R.bpred.data(); C.st = &R.st; C.blk = R.blk.data(); C.hw = R.P.hw.data(); C.gam0 = R.gam0; C.gcnt = R.gcnt; C.alo = R.alo; C.ahi = R.ahi; C.seg = S; C.mode = R.mode;
		C.scale = R.scale; C.segs = nullptr;
		for (int wg = 0; wg < S.nb; wg++) wk_bpred_body(C, S.b0 + wg, 64, lds.data());
		wk_centers_body(C, 0, R.nthreads, lds.data());
		WkTableArgs A;
		memset(&A, 0, sizeof(A));
		A.blk = R.blk.data(); A.gam0 = R.gam0; A.gpos = R.gpos; A.gcnt = R.gcnt; A.alo = R.alo; A.ahi = R.ahi; A.table = R.table.data(); A.st = &R.st; A.base = R.base; A.tab = &R.tab;
		A.tape = R.tape.empty() ? nullptr : R.tape.data(); A.tape_len = R.tape.size();
		A.seg_b0 = S.b0; A.seg_g0 = S.g0; A.bg = S.bg; A.seg = s; A.mode = R.mode;
		for (int wg = 0; wg < S.g1 - S.g0; wg++) wk_table_body(A, wg, R.nthreads, lds.data());
	}
	WkWalkArgs W;
	memset(&W, 0, sizeof(W));
	W.blk = R.blk.data(); W.sup = R.P.sup.data(); W.table = R.table.data(); W.maps = R.maps.data(); W.ent_sup = R.ent_sup.data(); W.ent_blk = R.ent_blk.data(); W.T = T; W.st = &R.st;
	W.bpred = R.bpred.data(); W.gam0 = R.gam0; W.scale = R.scale;
	W.seg = S; W.segno = s; W.mode = R.mode; W.strict = strict; W.keep_origin = keep_origin; W.total_groups = R.P.groups;
	for (int wg = 0; wg < S.nb; wg++) wk_block_body(W, wg, R.nthreads, lds.data());
	for (int wg = 0; wg < S.ns; wg++) wk_compose_body(W, wg, R.nthreads, lds.data());
	wk_top_body(W, R.nthreads, lds.data());
	for (int wg = 0; wg < S.ns; wg++) wk_expand_body(W, wg, R.nthreads, lds.data());
	for (int wg = 0; wg < S.nb; wg++) wk_final_body(W, wg, R.nthreads, lds.data());
}
/* (gamma, column) decisions wk_table evaluates for the blocks as they stand after wk_centers, and with every column */
static void run_count(const Run &R, unsigned long long *evaluated, unsigned long long *all, unsigned long long *trimmed_rows)
{
	for (const WkBlock &B : R.blk)
		for (int r = 0; r < B.ng; r++) {
			const int g = B.g0 + r, ng = R.gam0[g + 1] - R.gam0[g];
			int lo, hi;
			const int tr = wk_trim_range(B, R.gam0[g] - R.gam0[B.g0], R.gam0[B.g0 + B.ng] - R.gam0[B.g0], &lo, &hi);
			*evaluated += (unsigned long long)ng * (unsigned long long)(hi + WK_PADC - lo);
			*all += (unsigned long long)ng * (unsigned long long)(B.W + WK_PADC);
			if (tr && (lo > 0 || hi < B.W)) *trimmed_rows += 1;
		}
}

static std::vector<unsigned long long> exact_gpos(const int *gam0, int G, const int *gcnt)
{
	const int NG = gam0[G];
	std::vector<unsigned long long> gpos(NG + 1, 0);
	for (int k = 0; k < NG; k++) gpos[k + 1] = gpos[k] + (gcnt[k] == 0 ? 1u : 2u);
	return gpos;
}

/* exact mode end to end; out[8]: total uniforms, fail, nfail_block, blocks, segments, decisions evaluated, decisions of untrimmed tables, rows trimmed */
extern "C" int wt_exact(const int *gam0, int G, const int *gcnt, long s1, long s2, long s3, double rho_hi, double sigma, double kwin, int seg_groups, float scale, int nthreads, double trim_k,
			int with_tape, unsigned long long *T, unsigned long long *out)
{
	Run R;
	if (!run_init(R, gam0, G, rho_hi, sigma, kwin, seg_groups, true, WK_MODE_EXACT, 0, trim_k, s1, s2, s3)) return 1;
	const std::vector<unsigned long long> gpos = exact_gpos(gam0, G, gcnt);
	R.gpos = gpos.data(); R.gcnt = gcnt; R.scale = scale; R.nthreads = nthreads;
	if (with_tape) run_make_tape(R, (size_t)gpos[gam0[G]] + (size_t)(2.2 * gam0[G]) + 8192);
	memset(out, 0, 8 * sizeof(*out));
	for (size_t s = 0; s < R.P.seg.size(); s++) run_segment(R, (int)s, 0, true, 0, T);
	run_count(R, &out[5], &out[6], &out[7]); /* (reuse: the blocks of all segments keep what wk_centers wrote) */
	out[0] = R.st.fail ? 0 : gpos[gam0[G]] + 2ull * T[G];
	out[1] = R.st.fail;
	out[2] = R.st.nfail_block;
	out[3] = R.P.blk.size();
	out[4] = R.P.seg.size();
	return 0;
}

/* the sequential sampler: T[g] = rejected attempts before group g, total = uniforms consumed */
extern "C" int wt_ref_exact(const int *gam0, int G, const int *gcnt, long s1, long s2, long s3, unsigned long long *T, unsigned long long *total)
{
	isg_cursor c;
	c.s.s1 = (uint32_t)(s1 % ISG_M1); c.s.s2 = (uint32_t)(s2 % ISG_M2); c.s.s3 = (uint32_t)(s3 % ISG_M3);
	c.used = 0;
	c.tape = nullptr;
	unsigned long long used = 0, minimal = 0;
	for (int g = 0; g < G; g++) {
		T[g] = (used - minimal) / 2;
		for (int k = gam0[g]; k < gam0[g + 1]; k++) {
			const uint32_t u0 = c.used;
			(void)isg_rgamma(&c, (double)gcnt[k] + 1.0);
			used += c.used - u0;
			minimal += gcnt[k] == 0 ? 1 : 2;
			if (c.used > (1u << 30)) c.used = 0;
		}
	}
	T[G] = (used - minimal) / 2;
	*total = used;
	return 0;
}

/*
 * The same tables built with every column and trimmed (no walk).  Exact mode: gcnt (gpos is formed here); interval mode: gpos, alo, ahi.
 * out[11]: bytes inside the rows' ranges that differ, bytes outside that are not WK_IRR, bytes inside, bytes outside, decisions evaluated,
 * decisions of the untrimmed tables, rows trimmed, blocks that must keep every column (a segment's last, a window clamped at 0), such
 * blocks that were trimmed all the same, blocks, blocks with a clamped window among them.
 */
extern "C" int wt_tables(const int *gam0, int G, const int *gcnt, const unsigned long long *gpos_in, const float *alo, const float *ahi, long s1, long s2, long s3, double rho_hi, double sigma,
			 double kwin, int seg_groups, float scale, int nthreads, double trim_k, int with_tape, int entry_slack, unsigned long long *out)
{
	const int mode = gcnt ? WK_MODE_EXACT : WK_MODE_INTERVAL;
	Run R[2];
	std::vector<unsigned long long> gpos_own;
	if (gcnt) gpos_own = exact_gpos(gam0, G, gcnt);
	const unsigned long long *gpos = gcnt ? gpos_own.data() : gpos_in;
	for (int v = 0; v < 2; v++) {
		if (!run_init(R[v], gam0, G, rho_hi, sigma, kwin, seg_groups, false, mode, entry_slack, v ? trim_k : 0.0, s1, s2, s3)) return 1;
		R[v].gpos = gpos; R[v].gcnt = gcnt; R[v].alo = alo; R[v].ahi = ahi; R[v].scale = scale; R[v].nthreads = nthreads;
		if (with_tape) run_make_tape(R[v], (size_t)gpos[gam0[G]] + (size_t)(2.2 * gam0[G]) + 8192);
	}
	/* both walk from the same entries: the untrimmed run's walk says where the next segment is entered */
	std::vector<unsigned long long> T(G + 1, 0);
	for (size_t s = 0; s < R[0].P.seg.size(); s++) {
		run_segment(R[0], (int)s, 0, true, 0, T.data());
		R[1].st.xin[s] = R[0].st.xin[s];
		run_segment(R[1], (int)s, 0, true, 0, T.data());
		if (R[0].st.fail || R[1].st.fail) return 2;
	}
	memset(out, 0, 11 * sizeof(*out));
	if (R[0].P.table_bytes != R[1].P.table_bytes || R[0].blk.size() != R[1].blk.size()) return 3;
	for (size_t s = 0; s < R[1].P.seg.size(); s++) {
		const WkSeg S = R[1].P.seg[s];
		float run = 0.f;
		for (int b = S.b0; b < S.b0 + S.nb; b++) {
			const WkBlock &B = R[1].blk[b], &B0 = R[0].blk[b];
			if (B.wlo != B0.wlo || B.W != B0.W || B.toff != B0.toff || B.ein != B0.ein) return 4;
			const bool clamped = (S.g0 == 0) && ((int)(run * scale) - R[1].P.hw[b] < 0);
			run += R[1].bpred[b];
			const bool whole = clamped || b == S.b0 + S.nb - 1;
			if (whole) out[7]++;
			if (clamped && b != S.b0 + S.nb - 1) out[10]++;
			bool any = false;
			for (int r = 0; r < B.ng; r++) {
				const int g = B.g0 + r;
				int lo, hi;
				(void)wk_trim_range(B, gam0[g] - gam0[B.g0], gam0[B.g0 + B.ng] - gam0[B.g0], &lo, &hi);
				if (lo > 0 || hi < B.W) any = true;
				const unsigned char *a = &R[0].table[B.toff + (size_t)r * B.W], *t = &R[1].table[B.toff + (size_t)r * B.W];
				for (int col = 0; col < B.W; col++) {
					if (col >= lo && col < hi) { out[2]++; if (a[col] != t[col]) out[0]++; }
					else { out[3]++; if (t[col] != WK_IRR) out[1]++; }
				}
			}
			if (whole && any) out[8]++;
		}
	}
	run_count(R[1], &out[4], &out[5], &out[6]);
	out[9] = R[1].blk.size();
	return 0;
}

/* uniforms consumed by rdirich over `n` gammas of the given shapes when it starts `pos` uniforms after the seeds */
static unsigned ref_consumed(const isg_wh_tables *tab, isg_wh base, unsigned long long pos, const double *shape, int n)
{
	isg_cursor c;
	c.s = isg_wh_jump(tab, base, pos);
	c.used = 0;
	c.tape = nullptr;
	for (int k = 0; k < n; k++) (void)isg_rgamma(&c, shape[k]);
	return c.used;
}

/* the interval resolver end to end with trimmed tables: a lenient walk, every uncertain byte within +-band of its trajectory replaced by the
 * sequential sampler's consumption for the TRUE shapes, a strict walk over the same tables.  Tref: the sequential sampler's trajectory.
 * out[8]: fail of the lenient walk, of the strict walk, probes, segments, decisions evaluated, decisions of untrimmed tables, rows trimmed */
extern "C" int wt_spec(const int *gam0, int G, const unsigned long long *gpos, const float *alo, const float *ahi, const double *atrue, long s1, long s2, long s3, double sigma, double kwin,
		       int seg_groups, int band, int entry_slack, int nthreads, double trim_k, unsigned long long *T, unsigned long long *Tref, unsigned long long *out)
{
	Run R;
	if (!run_init(R, gam0, G, 0.8, sigma, kwin, seg_groups, false, WK_MODE_INTERVAL, entry_slack, trim_k, s1, s2, s3)) return 1;
	R.gpos = gpos; R.alo = alo; R.ahi = ahi; R.nthreads = nthreads;
	memset(out, 0, 8 * sizeof(*out));
	for (size_t s = 0; s < R.P.seg.size(); s++) run_segment(R, (int)s, 0, true, 0, T);
	out[0] = R.st.fail;
	run_count(R, &out[4], &out[5], &out[6]);
	unsigned long long nprobe = 0;
	if (!R.st.fail) {
		for (size_t s = 0; s < R.P.seg.size(); s++)
			for (int b = R.P.seg[s].b0; b < R.P.seg[s].b0 + R.P.seg[s].nb; b++)
				for (int r = 0; r < R.blk[b].ng; r++) {
					const WkBlock &B = R.blk[b];
					const int g = B.g0 + r, n = gam0[g + 1] - gam0[g];
					for (int j = -band; j <= band; j++) {
						const long long x = (long long)T[g] + j, col = x - (long long)R.st.xin[s] - B.wlo;
						if (x < 0 || col < 0 || col >= B.W) continue;
						unsigned char &v = R.table[B.toff + (size_t)r * B.W + col];
						if (v == WK_IRR || !(v & WK_UFLAG)) continue;
						const unsigned used = ref_consumed(&R.tab, R.base, gpos[gam0[g]] + 2ull * (unsigned long long)x, atrue + gam0[g], n);
						const unsigned c = (used - 2u * (unsigned)n) / 2u;
						v = c <= 126u ? (unsigned char)c : (unsigned char)WK_IRR;
						nprobe++;
					}
				}
		memset((char *)&R.st + offsetof(WkState, sum_d), 0, sizeof(WkState) - offsetof(WkState, sum_d));
		for (size_t s = 0; s < R.P.seg.size(); s++) run_segment(R, (int)s, 1, false, 1, T);
	}
	out[1] = R.st.fail;
	out[2] = nprobe;
	out[3] = R.P.seg.size();
	unsigned long long x = 0;
	for (int g = 0; g < G; g++) {
		const int n = gam0[g + 1] - gam0[g];
		Tref[g] = x;
		x += (ref_consumed(&R.tab, R.base, gpos[gam0[g]] + 2ull * x, atrue + gam0[g], n) - 2u * (unsigned)n) / 2u;
	}
	Tref[G] = x;
	return 0;
}

/*
 * How far the in-block drift of the sequential sampler is from what wk_trim_range goes by: over all rows of all blocks of a plan, the largest
 * |rejections of the block's rows before r - (block's scaled prediction) gammas before r / gammas of the block| in units of the row's
 * spread  kwin sigma sqrt(gammas before r) + WK_TRIM_MARGIN  (out[0], in 1e-6; out[2]: the same against the per-row sum of wk_expected_rej).
 * T: the sequential sampler's trajectory (wt_ref_exact).
 */
extern "C" int wt_drift(const int *gam0, int G, const int *gcnt, const unsigned long long *T, double rho_hi, double sigma, double kwin, int seg_groups, float scale, unsigned long long *out)
{
	WkPlan P;
	if (!wk_plan_build(P, gam0, G, rho_hi, sigma, kwin, seg_groups, true, WK_MODE_EXACT)) return 1;
	double worst = 0, worst_sum = 0;
	for (const WkBlock &B : P.blk) {
		float pred = 0.f;
		for (int gm = gam0[B.g0]; gm < gam0[B.g0 + B.ng]; gm++) pred += wk_expected_rej((float)gcnt[gm] + 1.0f);
		const double nin = gam0[B.g0 + B.ng] - gam0[B.g0];
		double run = 0; /* the per-row sum of the predictions, for comparison */
		for (int r = 0; r < B.ng; r++) {
			const double nb = gam0[B.g0 + r] - gam0[B.g0];
			const double drift = (double)(T[B.g0 + r] - T[B.g0]), spread = kwin * sigma * sqrt(nb) + WK_TRIM_MARGIN;
			const double rel = fabs(drift - (double)pred * scale * nb / nin) / spread, rel_sum = fabs(drift - run * scale) / spread;
			if (rel > worst) worst = rel;
			if (rel_sum > worst_sum) worst_sum = rel_sum;
			for (int gm = gam0[B.g0 + r]; gm < gam0[B.g0 + r + 1]; gm++) run += wk_expected_rej((float)gcnt[gm] + 1.0f);
		}
	}
	out[0] = (unsigned long long)(1e6 * worst);
	out[1] = P.blk.size();
	out[2] = (unsigned long long)(1e6 * worst_sum);
	return 0;
}
