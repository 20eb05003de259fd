/*
 * walk_down_emul.cpp -- TEST INFRASTRUCTURE.  The walk in three launches (wk_block_body, wk_compose2_body, wk_down_body of
 * instruct_amd/csrc/isg_walk.h: the very source the device compiles) on the host next to the five bodies it replaces, workgroup by
 * workgroup on two copies of the same state, compared with memcmp: every map, every entry, T, the whole WkState.  The LDS of the new
 * bodies is allocated exactly as large as the plan says, so a sanitizer build (the same file with -DWD_MAIN, a program of its own) sees an
 * overrun of a staged region.  No product path links this.
 */
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../instruct_amd/csrc/isg_walk_plan.h"

struct Patch {
	int walk;     /* which walk of the scenario (0: the first, 1..: the re-walks) */
	int mid;      /* 0: before the walk's first launch (the maps see it), 1: between the way up and the way down */
	int kind;     /* 0: table byte on the path of group `at` := val, 1: |= val, 2: F1 delta of block `at` on the path := WK_OUT16, 3: F2 of super-block `at` */
	int at;
	unsigned val;
};
struct Problem { /* one run of groups */
	int G = 0, mode = WK_MODE_EXACT;
	std::vector<int> gam0, gcnt;
	std::vector<unsigned long long> gpos;
	std::vector<float> alo, ahi;
	std::vector<double> atrue;
};
struct Run {
	WkPlan P;
	std::vector<WkBlock> blk;
	std::vector<unsigned char> table;
	std::vector<unsigned short> maps;
	std::vector<int> ent_sup, ent_blk;
	std::vector<float> bpred;
	std::vector<unsigned long long> T;
	WkState st;
	unsigned fail_in = 0;
	unsigned dev[4] = {0, 0, 0, 0}; /* SpecDev's words: the two list counters, then two that no walk touches */
	isg_wh_tables tab;
	isg_wh base;
	int nthreads = 256;
	float scale = 1.0f;
};
struct Clean { /* what the unpatched scenario left after each walk */
	std::vector<std::vector<unsigned long long>> T;
	std::vector<std::vector<int>> ent_sup, ent_blk;
	std::vector<WkState> st;
};
struct Scenario {
	double rho_hi = 0.8, sigma = 1.0, kwin = 5.0, trim_k = 5.0;
	int seg_groups = 4096, entry_slack = 0, rewalks = 0, strict_last = 0, prefail_seg = -1, nthreads = 256;
	bool reuse = true;
	std::vector<Patch> patches;
};

static unsigned long long g_lcg = 88172645463325252ull;
static unsigned rnd(unsigned n) { g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)((g_lcg >> 33) % n); }

static Problem make_exact(int G, int ng, int cnt_lo, int cnt_hi)
{
	Problem Q;
	Q.G = G; Q.mode = WK_MODE_EXACT;
	Q.gam0.resize(G + 1);
	for (int g = 0; g <= G; g++) Q.gam0[g] = g * ng;
	Q.gcnt.resize((size_t)G * ng);
	for (int &c : Q.gcnt) c = cnt_lo + (int)rnd((unsigned)(cnt_hi - cnt_lo));
	Q.gpos.assign((size_t)G * ng + 1, 0);
	for (int k = 0; k < G * ng; k++) Q.gpos[k + 1] = Q.gpos[k] + (Q.gcnt[k] == 0 ? 1u : 2u);
	return Q;
}
/* update_ZQ's shape: N individuals of K gammas behind 2 nv uniforms each, the shapes known as intervals (as tests/test_walk_trim.py builds them) */
static Problem make_interval(int N, int K, int nv)
{
	Problem Q;
	Q.G = N; Q.mode = WK_MODE_INTERVAL;
	Q.gam0.resize(N + 1);
	for (int i = 0; i <= N; i++) Q.gam0[i] = i * K;
	Q.gpos.assign((size_t)N * K + 1, 0);
	const unsigned long long per = 2ull * nv + 2ull * K;
	for (int i = 0; i < N; i++)
		for (int m = 0; m < K; m++) Q.gpos[(size_t)i * K + m] = per * i + 2ull * nv + 2ull * m;
	Q.gpos[(size_t)N * K] = per * N;
	Q.alo.resize((size_t)N * K); Q.ahi.resize((size_t)N * K); Q.atrue.resize((size_t)N * K);
	const double alpha = 3.7;
	for (size_t k = 0; k < (size_t)N * K; k++) {
		const double lam = 150 + rnd(4850);
		const double half = ceil(4.5 * sqrt(lam * 0.8)) + 1;
		Q.alo[k] = (float)(lam - half + alpha);
		Q.ahi[k] = (float)(lam + half + alpha);
		Q.atrue[k] = lam + floor(((double)rnd(20001) / 10000.0 - 1.0) * (half - 1) + 0.5) + alpha;
	}
	return Q;
}

static bool run_init(Run &R, const Problem &Q, const Scenario &S)
{
	if (!wk_plan_build(R.P, Q.gam0.data(), Q.G, S.rho_hi, S.sigma, S.kwin, S.seg_groups, S.reuse, Q.mode, S.entry_slack, S.trim_k)) return false;
	isg_wh_tables_init(&R.tab);
	R.base.s1 = 13; R.base.s2 = 4; R.base.s3 = 1972;
	R.blk = R.P.blk;
	R.table.assign(R.P.table_bytes + 64, 0);
	R.maps.assign(R.P.maps_elems + 64, 0);
	R.ent_sup.assign(R.P.sup.size(), 0);
	R.ent_blk.assign(R.P.blk.size(), 0);
	R.bpred.assign(R.P.blk.size(), 0.f);
	R.T.assign((size_t)Q.G + 1, 0);
	memset(&R.st, 0, sizeof(R.st));
	R.fail_in = 0;
	R.dev[0] = 5; R.dev[1] = 1; R.dev[2] = 7; R.dev[3] = 2;
	R.nthreads = S.nthreads;
	return true;
}
static void build_tables(Run &R, const Problem &Q, int s)
{
	const WkSeg S = R.P.seg[s];
	std::vector<unsigned char> lds(160 * 1024);
	WkCenterArgs C;
	memset(&C, 0, sizeof(C));
	C.bpred = R.bpred.data(); C.st = &R.st; C.blk = R.blk.data(); C.hw = R.P.hw.data(); C.gam0 = Q.gam0.data(); C.gcnt = Q.gcnt.data(); C.alo = Q.alo.data(); C.ahi = Q.ahi.data();
	C.seg = S; C.mode = Q.mode; C.scale = R.scale; C.segs = nullptr;
	for (int wg = 0; wg < S.nb; wg++) wk_bpred_body(C, S.b0 + wg, 64, lds.data());
	wk_centers_body(C, 0, R.nthreads, lds.data());
	WkTableArgs A;
	memset(&A, 0, sizeof(A));
	A.blk = R.blk.data(); A.gam0 = Q.gam0.data(); A.gpos = Q.gpos.data(); A.gcnt = Q.gcnt.data(); A.alo = Q.alo.data(); A.ahi = Q.ahi.data(); A.table = R.table.data(); A.st = &R.st;
	A.base = R.base; A.tab = &R.tab; A.tape = nullptr; A.tape_len = 0;
	A.seg_b0 = S.b0; A.seg_g0 = S.g0; A.bg = S.bg; A.seg = s; A.mode = Q.mode;
	for (int wg = 0; wg < S.g1 - S.g0; wg++) wk_table_body(A, wg, R.nthreads, lds.data());
}
static int block_of(const Run &R, int s, int g) { const WkSeg S = R.P.seg[s]; return S.b0 + (g - S.g0) / S.bg; }
/* patches of this walk and moment that fall into segment s, placed by the clean scenario's trajectory */
static void apply_patches(Run &R, const Scenario &Sc, const Clean *cl, int walk, int mid, int s)
{
	if (!cl) return;
	const WkSeg S = R.P.seg[s];
	for (const Patch &p : Sc.patches) {
		if (p.walk != walk || p.mid != mid) continue;
		if (p.kind <= 1) {
			if (p.at < S.g0 || p.at >= S.g1) continue;
			const WkBlock &B = R.blk[block_of(R, s, p.at)];
			const long long col = (long long)cl->T[walk][p.at] - (long long)cl->st[walk].xin[s] - B.wlo;
			if (col < 0 || col >= B.W) continue;
			unsigned char &v = R.table[B.toff + (size_t)(p.at - B.g0) * B.W + col];
			v = p.kind == 0 ? (unsigned char)p.val : (unsigned char)(v | p.val);
		} else if (p.kind == 2) {
			if (p.at < S.b0 || p.at >= S.b0 + S.nb) continue;
			const WkBlock &B = R.blk[p.at];
			const int e = cl->ent_blk[walk][p.at] - B.wlo;
			if (e >= 0 && e < B.ein) R.maps[B.foff + e] = (unsigned short)WK_OUT16;
		} else {
			if (p.at < S.s0 || p.at >= S.s0 + S.ns) continue;
			const WkSuper &U = R.P.sup[p.at];
			const WkBlock &B = R.blk[U.b0];
			const int e = cl->ent_sup[walk][p.at] - B.wlo;
			if (e >= 0 && e < B.ein) R.maps[U.foff + e] = (unsigned short)WK_OUT16;
		}
	}
}
/* route 0: the five bodies; 1: the three.  zero (route 1): this is a re-walk's first segment, its first launch zeroes the counters and the tail */
static void walk_segment(Run &R, const Problem &Q, const Scenario &Sc, const Clean *cl, int route, int walk, int s, int strict, int keep, bool zero)
{
	const WkSeg S = R.P.seg[s];
	const int nt = R.nthreads;
	WkWalkArgs W;
	memset(&W, 0, sizeof(W));
	W.blk = R.blk.data(); W.sup = R.P.sup.data(); W.table = R.table.data(); W.maps = R.maps.data(); W.ent_sup = R.ent_sup.data(); W.ent_blk = R.ent_blk.data(); W.T = R.T.data(); W.st = &R.st;
	W.bpred = R.bpred.data(); W.gam0 = Q.gam0.data(); W.scale = R.scale;
	W.seg = S; W.segno = s; W.mode = Q.mode; W.strict = strict; W.keep_origin = keep; W.total_groups = R.P.groups;
	W.fail_in = &R.fail_in;
	if (route == 0) {
		std::vector<unsigned char> lds(160 * 1024);
		for (int wg = 0; wg < S.nb; wg++) wk_block_body(W, wg, nt, lds.data());
		for (int wg = 0; wg < S.ns; wg++) wk_compose_body(W, wg, nt, lds.data());
		apply_patches(R, Sc, cl, walk, 1, s);
		wk_top_body(W, nt, lds.data());
		for (int wg = 0; wg < S.ns; wg++) wk_expand_body(W, wg, nt, lds.data());
		for (int wg = 0; wg < S.nb; wg++) wk_final_body(W, wg, nt, lds.data());
		return;
	}
	if (zero) { W.zero_words = R.dev; W.nzero = 2; W.zero_tail = 1; }
	/* LDS of exactly the sizes the launches ask for, filled with rubbish before every workgroup */
	std::vector<unsigned char> lb(R.P.lds_block), lc(R.P.lds_compose + (size_t)WK_C2_HDR), ld(R.P.lds_down);
	for (int wg = 0; wg < S.nb; wg++) {
		memset(lb.data(), 0xcd, lb.size());
		if (zero) wk_zero_body(W, wg, nt);
		wk_block_body(W, wg, nt, lb.data());
	}
	for (int wg = 0; wg < S.ns; wg++) {
		memset(lc.data(), 0xcd, lc.size());
		wk_compose2_body(W, wg, nt, lc.data());
	}
	apply_patches(R, Sc, cl, walk, 1, s);
	for (int wg = 0; wg < S.nb; wg++) {
		memset(ld.data(), 0xcd, ld.size());
		wk_down_body(W, wg, nt, ld.data());
	}
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
/* what k_zq_probe does: uncertain bytes within +-band of the trajectory (of every `step`-th group) get the true shapes' consumption */
static unsigned long long probe(Run &R, const Problem &Q, int band, int step)
{
	unsigned long long n = 0;
	if (R.st.fail) return 0;
	for (size_t s = 0; s < R.P.seg.size(); s++)
		for (int b = R.P.seg[s].b0; b < R.P.seg[s].b0 + R.P.seg[s].nb; b++) {
			const WkBlock &B = R.blk[b];
			for (int r = 0; r < B.ng; r++) {
				const int g = B.g0 + r, ng = Q.gam0[g + 1] - Q.gam0[g];
				if (g % step) continue;
				for (int j = -band; j <= band; j++) {
					const long long x = (long long)R.T[g] + j, col = x - (long long)R.st.xin[s] - B.wlo;
					if (x < 0 || col < 0 || col >= B.W) continue;
					unsigned char &v = R.table[B.toff + (size_t)r * B.W + col];
					if (v == WK_IRR || !(v & WK_UFLAG)) continue;
					const unsigned used = ref_consumed(&R.tab, R.base, Q.gpos[Q.gam0[g]] + 2ull * (unsigned long long)x, Q.atrue.data() + Q.gam0[g], ng);
					const unsigned c = (used - 2u * (unsigned)ng) / 2u;
					v = c <= 126u ? (unsigned char)c : (unsigned char)WK_IRR;
					n++;
				}
			}
		}
	return n;
}
static void run_scenario(Run &R, const Problem &Q, const Scenario &Sc, int route, const Clean *cl, Clean *rec, unsigned long long *nprobes)
{
	const int nseg = (int)R.P.seg.size();
	auto record = [&]() {
		if (!rec) return;
		rec->T.push_back(R.T); rec->ent_sup.push_back(R.ent_sup); rec->ent_blk.push_back(R.ent_blk); rec->st.push_back(R.st);
	};
	for (int s = 0; s < nseg; s++) {
		build_tables(R, Q, s);
		if (Sc.prefail_seg == s) R.st.fail |= 8u;
		apply_patches(R, Sc, cl, 0, 0, s);
		walk_segment(R, Q, Sc, cl, route, 0, s, 0, 0, false);
	}
	record();
	for (int w = 1; w <= Sc.rewalks; w++) {
		*nprobes += (w < Sc.rewalks) ? probe(R, Q, 0, 2) : probe(R, Q, 24, 1);
		if (route == 0) { /* the memsets of the five-launch route */
			memset((char *)&R.st + offsetof(WkState, sum_d), 0, sizeof(WkState) - offsetof(WkState, sum_d));
			R.dev[0] = R.dev[1] = 0;
		}
		for (int s = 0; s < nseg; s++) {
			apply_patches(R, Sc, cl, w, 0, s);
			walk_segment(R, Q, Sc, cl, route, w, s, (w == Sc.rewalks) ? Sc.strict_last : 0, 1, s == 0);
		}
		R.dev[0] += 3; /* (k_zs_band adds to the counters behind every walk) */
		record();
	}
}
/* bit k set: the k-th of (table, maps, ent_sup, ent_blk, T, WkState, counters, the noted fail word) differs */
static unsigned compare(const Run &A, const Run &B)
{
	unsigned m = 0;
	if (A.table.size() != B.table.size() || memcmp(A.table.data(), B.table.data(), A.table.size())) m |= 1u;
	if (A.maps.size() != B.maps.size() || memcmp(A.maps.data(), B.maps.data(), sizeof(unsigned short) * A.maps.size())) m |= 2u;
	if (memcmp(A.ent_sup.data(), B.ent_sup.data(), sizeof(int) * A.ent_sup.size())) m |= 4u;
	if (memcmp(A.ent_blk.data(), B.ent_blk.data(), sizeof(int) * A.ent_blk.size())) m |= 8u;
	if (memcmp(A.T.data(), B.T.data(), sizeof(unsigned long long) * A.T.size())) m |= 16u;
	if (memcmp(&A.st, &B.st, sizeof(WkState))) m |= 32u;
	if (memcmp(A.dev, B.dev, sizeof(A.dev))) m |= 64u;
	return m;
}

/*
 * One scenario by both routes.  out[12]: differences (compare's bits), fail, nfail_block, segments, super-blocks, blocks, blocks whose path
 * leaves the strip of WK_STRIP columns, lds_down, whether the plan takes the three launches, probes, sum_d, the clean scenario's fail.
 */
static int run_case(const Problem &Q, const Scenario &Sc, unsigned long long *out)
{
	memset(out, 0, 12 * sizeof(*out));
	Run R0, RA, RB;
	Clean cl;
	unsigned long long np0 = 0, npa = 0, npb = 0;
	if (!run_init(R0, Q, Sc) || !run_init(RA, Q, Sc) || !run_init(RB, Q, Sc)) return 1;
	Scenario clean = Sc;
	clean.patches.clear();
	clean.prefail_seg = -1;
	run_scenario(R0, Q, clean, 0, nullptr, &cl, &np0);
	run_scenario(RA, Q, Sc, 0, &cl, nullptr, &npa);
	run_scenario(RB, Q, Sc, 1, &cl, nullptr, &npb);
	out[0] = compare(RA, RB) | (npa != npb ? 128u : 0u);
	out[1] = RB.st.fail;
	out[2] = RB.st.nfail_block;
	out[3] = RB.P.seg.size();
	out[4] = RB.P.sup.size();
	out[5] = RB.P.blk.size();
	if (!Sc.reuse || RB.P.seg.size() == 1)
		for (size_t s = 0; s < RB.P.seg.size(); s++)
			for (int b = RB.P.seg[s].b0; b < RB.P.seg[s].b0 + RB.P.seg[s].nb; b++) {
				const WkBlock &B = RB.blk[b];
				const int ent = RB.ent_blk[b];
				if (ent == WK_NOENT || RB.st.fail) continue;
				const long long last = (long long)RB.T[B.g0 + B.ng - 1] - (long long)RB.st.xin[s] - B.wlo;
				if (last - ((ent - B.wlo) & ~15) >= WK_STRIP) out[6]++;
			}
	out[7] = RB.P.lds_down;
	out[8] = wk_plan_fused_ok(RB.P, (size_t)160 * 1024) ? 1 : 0;
	out[9] = npb;
	out[10] = RB.st.sum_d;
	out[11] = R0.st.fail;
	if (RB.dev[2] != 7 || RB.dev[3] != 2) out[0] |= 256u; /* the words behind the counters are nobody's to zero */
	return 0;
}

static const char *const g_names[] = {
	"exact_3seg", "interval_rewalks_1seg", "interval_rewalks_segs", "trimmed_tight", "miss_top", "miss_blocks", "miss_rows", "irregular", "irregular_untrimmed",
	"uncertain_strict", "uncertain_strict_rows", "carried_failure", "leaves_strip", "short_last_block", "threads_64",
};
extern "C" int wd_ncases(void) { return (int)(sizeof(g_names) / sizeof(g_names[0])); }
extern "C" const char *wd_case_name(int id) { return (id >= 0 && id < wd_ncases()) ? g_names[id] : ""; }
extern "C" int wd_case(int id, unsigned long long *out)
{
	g_lcg = 88172645463325252ull + 977ull * (unsigned)id;
	Scenario S;
	switch (id) {
	case 0: { /* exact mode, three segments of two super-blocks and a partial one, two gammas per group */
		S.seg_groups = 2560;
		return run_case(make_exact(3 * 2560 - 37, 2, 50, 9000), S, out);
	}
	case 1: { /* interval mode, one segment of three super-blocks, two re-walks with kept origins after probes */
		S.reuse = false; S.rewalks = 2; S.strict_last = 1; S.entry_slack = 80;
		return run_case(make_interval(2500, 5, 600), S, out);
	}
	case 2: { /* the same over segments of 320: the re-walks enter the later segments off the first walk's entries */
		S.reuse = false; S.rewalks = 2; S.strict_last = 1; S.entry_slack = 80; S.seg_groups = 320;
		return run_case(make_interval(1200, 5, 600), S, out);
	}
	case 3: { /* rows trimmed to the margin alone: windows are missed */
		S.trim_k = 0.02;
		return run_case(make_exact(1000, 16, 50, 9000), S, out);
	}
	case 4: { /* a super-block's map has no delta for the path's entry: the walk fails among the F2 maps */
		S.seg_groups = 2560;
		S.patches.push_back({0, 1, 3, 1, 0});
		return run_case(make_exact(2560, 2, 50, 9000), S, out);
	}
	case 5: { /* ... a block's map has none: among a super-block's F1 maps */
		S.seg_groups = 2560;
		S.patches.push_back({0, 1, 2, 16 + 5, 0});
		return run_case(make_exact(2560, 2, 50, 9000), S, out);
	}
	case 6: { /* a byte on the way down sends the path out of the next row's columns: a missed window named by wk_trim_range */
		S.seg_groups = 2560;
		S.patches.push_back({0, 1, 0, 64 * 7 + 40, 250});
		return run_case(make_exact(2560, 2, 50, 9000), S, out);
	}
	case 7: { /* an irregular byte on the path when the maps are built */
		S.seg_groups = 2560;
		S.patches.push_back({0, 0, 0, 64 * 20 + 3, WK_IRR});
		return run_case(make_exact(2560, 2, 50, 9000), S, out);
	}
	case 8: { /* ... and one met on the way down only, tables untrimmed: reported as irregular */
		S.seg_groups = 2560; S.trim_k = 0.0;
		S.patches.push_back({0, 1, 0, 64 * 20 + 3, WK_IRR});
		return run_case(make_exact(2560, 2, 50, 9000), S, out);
	}
	case 9: { /* an uncertain byte left on the path of the strict walk when its maps are built */
		S.reuse = false; S.rewalks = 2; S.strict_last = 1; S.entry_slack = 80;
		S.patches.push_back({2, 0, 1, 700, WK_UFLAG});
		return run_case(make_interval(1200, 5, 600), S, out);
	}
	case 10: { /* ... and one that appears on the way down */
		S.reuse = false; S.rewalks = 2; S.strict_last = 1; S.entry_slack = 80;
		S.patches.push_back({2, 1, 1, 700, WK_UFLAG});
		return run_case(make_interval(1200, 5, 600), S, out);
	}
	case 11: { /* a segment entered with a failure noted already */
		S.seg_groups = 2560; S.prefail_seg = 1;
		return run_case(make_exact(3 * 2560 - 37, 2, 50, 9000), S, out);
	}
	case 12: { /* 1024 gammas of shape 3..4 per block reject some 700 attempts: the path leaves the strip of 512 columns */
		return run_case(make_exact(256 + 21, 16, 2, 3), S, out);
	}
	case 13: { /* a run of one short block, and one of a block and a bit */
		unsigned long long o2[12];
		const int rc = run_case(make_exact(23, 3, 50, 9000), S, o2);
		if (rc || o2[0] || o2[1]) { memcpy(out, o2, sizeof(o2)); return rc ? rc : 0; }
		return run_case(make_exact(64 + 9, 3, 50, 9000), S, out);
	}
	case 14: { /* a workgroup of one wave: fewer threads than descriptors and strip words to stage */
		S.seg_groups = 2560; S.nthreads = 64;
		return run_case(make_exact(2 * 2560 + 100, 2, 50, 9000), S, out);
	}
	}
	return 1;
}
/* the plan of a run with windows this wide asks for more LDS than `limit`: out[3]: lds_down, lds_top, whether it takes the three launches */
extern "C" int wd_plan_limit(int G, double sigma, double kwin, int seg_groups, unsigned long long limit, unsigned long long *out)
{
	const Problem Q = make_exact(G, 2, 50, 9000);
	WkPlan P;
	if (!wk_plan_build(P, Q.gam0.data(), G, 0.8, sigma, kwin, seg_groups, true, WK_MODE_EXACT)) return 1;
	out[0] = P.lds_down;
	out[1] = P.lds_top;
	out[2] = wk_plan_fused_ok(P, (size_t)limit) ? 1 : 0;
	return 0;
}

#ifdef WD_MAIN
int main(void)
{
	int bad = 0;
	for (int id = 0; id < wd_ncases(); id++) {
		unsigned long long out[12];
		const int rc = wd_case(id, out);
		printf("%-24s rc %d diff %llu fail %llu nfail_block %llu seg %llu sup %llu blk %llu off-strip %llu lds_down %llu fused %llu probes %llu sum_d %llu\n", wd_case_name(id), rc,
		       out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[8], out[9], out[10]);
		if (rc || out[0]) bad++;
	}
	printf("%d of %d cases differ\n", bad, wd_ncases());
	return bad ? 1 : 0;
}
#endif
