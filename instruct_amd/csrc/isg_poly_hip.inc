/*
 * isg_poly_hip.inc -- ploidy 4 (autotetraploid, -ap 1) sweeps of the reference's poly_geno.c on the
 * MI355X.  Included by isg_hip.hip (same translation unit: shares the reductions, the stream helpers and
 * the Dirichlet block of the diploid path).  First correct version: replay RNG schedule only, exact
 * double-precision Z draws, one locus (4 allele copies) per lane; see DESIGN.md for what is not tuned yet.
 *
 *   update_P_auto      poly_geno.c:390-438   k4_count + Dirichlets on the host (stream order)
 *   calc_exfreq_auto   poly_geno.c:1515-1590 k4_exfreq  (one lane per (cluster, locus) table)
 *   update_S_POP       poly_geno.c:584-643   k4_classcount (ONE sweep: genotype-class counts per cluster and
 *                                            locus + the mixed-assignment terms) then per cluster
 *                                            k4_genfreq (auto_genfreq :1803-2028) + k4_dsum; the reference's
 *                                            2K full sweeps (cal_lkd_props :645, cal_lkd :715) become
 *                                            O(K L G) table work on exact integer accumulators
 *   update_ZQ          poly_geno.c:750-836   k4_zq (serial over individuals as in the diploid replay path)
 *   update_geno        poly_geno.c:520-580   k4_geno (one uniform per ambiguous locus: positions are static)
 *   cal_lkd            poly_geno.c:715-735   k4_lkd
 */
#define PT_NAME(x) ptd_##x
#define PT_LOG(x) isg_log(x)
#define PT_EXP(x) isg_exp(x)
#include "isg_poly_tables.h"
#include "isg_pgroups.h"
#undef PT_NAME
#undef PT_LOG
#undef PT_EXP

#define ISG_POLY_ACAP 16 /* alleles per locus: 3876 (auto) / 18496 (allo) genotypes at 16; rows are found through a code -> row map of n^4 shorts */
#define ISG_POLY_ACAP_W 32 /* wide-allele contexts (Amax 17..32): 52360 (auto) / 278784 (allo) genotypes at 32, rows in closed form, own table kernels */

struct PolyDev {
	int N, L, Lp, K, KP, Amax, GS, nwv;
	const uint8_t *obs; /* [N][Lp][4] sorted distinct allele codes, 0xFF padded (SEQDATA.seqdata for ploidy 4) */
	uint8_t *geno;      /* [N][Lp][4] imputed genotype (UPMCMC.geno) */
	uint8_t *z;         /* [N][Lp][4] */
	const int *nvalid;
	const unsigned *rankwave;          /* [N][nwv] used loci of the individual before locus 64 w */
	const unsigned long long *ambwave; /* [N][nwv] ambiguous loci (2 or 3 distinct alleles) before (i, 64 w), all individuals */
	const int *lclass;                 /* [L] index of the locus' allele count among the distinct counts */
	const isg_polyclass *pc;           /* device copies (list pointers are device pointers) */
	const short *gidmap;               /* genotype code -> row of the class tables */
	const int *gidoff;
	double *freq;  /* [L][Amax][KP] */
	int *cnt;      /* [L][Amax][K] */
	/* allotetraploid (-ap 0): copies 0, 1 of a genotype belong to the first subgenome (freq, cnt), copies 2, 3 to the second */
	int allo;
	int allo_pref; /* the allotetraploid genotype draw decides in single precision first (INSTRUCT_ALLO_PREFILTER=0: not): freqf is then followed
	                * by the same copy of freq2, at freqf + Lp Amax KPF.  (Here, where the struct had padding: its size and offsets stay.) */
	double *freq2; /* [L][Amax][KP]  UPMCMC.freq2 (update_P_allo, poly_geno.c:441-518) */
	int *cnt2;     /* [L][Amax][K] */
	int *cntmix2;  /* the second subgenome's copies of mixed-assignment loci */
	double *qq;
	int *qqnum;
	double *indvlkh;
	float *exfreq, *genofreq; /* [K][L][GS] */
	float *tabtmp;            /* [K][L][GS] proposal tables */
	int *ccnt;                /* [K][L][GS] genotype-class counts of same-cluster loci */
	unsigned long long *accbuf; /* exact accumulators as 5-word limb groups */
	const isg_wh_tables *tab;
	unsigned *err;
	double log4, log6; /* isg_log(4), isg_log(6): the same bits as evaluating them per locus (poly_geno.c:880-882) */
	const float *freqf; /* [L][Amax][KPF] single precision copy of freq (pre-filters); allo_pref: followed by freq2's at freqf + Lp Amax KPF */
	int KPF;
	/* cal_lkd's tables, LOCUS INNERMOST (its lanes take consecutive loci: the lanes that need the same row read one contiguous stretch of it; in the
	 * [locus][...] layouts every lane's 4 or 8 bytes cost a line of their own), rebuilt before cal_lkd reads them (k4_logfreq):
	 * lfreq / lfreq2 [Amax][KP][Lp] = isg_log(freq / freq2); genofreqT [K][GS][Lp] = genofreq.  (Tried: entries as the 128-bit fixed-point images
	 * isg_acc adds, 16 bytes each, so that the sweep only adds integers -- slower, 4.6 against 3.8 ms: the sweep is bound by its lookups, not by the conversions.) */
	double *lfreq, *lfreq2;
	float *genofreqT;
};

struct PolyCtx {
	PolyDev p; /* a view of the buffers below (freqf, tab and err: of the context's) */
	DevBuf<uint8_t> obs, geno, z;
	DevBuf<int> nvalid, lclass, gidoff, cnt, cntmix2, qqnum, ccnt; /* allotetraploid: cnt holds cnt2 behind it, freq holds freq2 (isg_pgroups.h) */
	DevBuf<unsigned> rankwave;
	DevBuf<unsigned long long> ambwave, accbuf;
	DevBuf<short> gidmap;
	std::vector<DevBuf<int>> dlists; /* the classes' genotype lists: what the device copies of isg_polyclass point to */
	DevBuf<isg_polyclass> pc;
	DevBuf<double> freq, lfreq, lfreq2, qq, indvlkh;
	DevBuf<float> exfreq, genofreq, genofreqT, tabtmp;
	std::vector<int> classes;            /* distinct allele counts, ascending */
	std::vector<std::vector<int>> lists; /* genotype lists per class */
	std::vector<int> lclass_h;
	unsigned long long total_amb;
	DevBuf<int> d_cntmix;
	DevBuf<float> d_self; /* [2][KCAP] current and proposed selfing rates as the tables take them (float) */
	DevBuf<unsigned long long> d_catcnt;
	bool counts_valid; /* cnt / cntmix / ccnt / catcnt describe the current (geno, Z) */
	bool freq_host;    /* the host mirror of freq is current (replay: drawn on the host) */
	bool wide;         /* Amax 17..32: closed-form rows (no gidmap), k4_exfreq_w / k4_genfreq_w and the *_w sweeps */
	DevBuf<float> d_zpart; /* k4_zexpect: [N][8][2 K] partial sums */
	hvec<double> freq2_h; /* [K][L][Amax] second subgenome (allo) */
	hvec<int> cnt2_h;
	std::vector<float> tab_h;
};

/* the single precision copy of freq2 behind freqf's (the allotetraploid genotype draw's pre-decision) */
__global__ void k4_freq2f(PolyDev p)
{
	const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const size_t rows = (size_t)p.L * p.Amax;
	if (id >= rows * p.KPF) return;
	const size_t r = id / p.KPF;
	const int m = (int)(id - r * p.KPF);
	((float *)p.freqf)[(size_t)p.Lp * p.Amax * p.KPF + id] = (m < p.K) ? (float)p.freq2[r * p.KP + m] : 0.f;
}

/* pdev_create (isg_walk_hip.inc) for the allotetraploid chain: the group list of update_P_allo (pgroups_build, isg_pgroups.h: two Dirichlets per
 * (k, j), the second's counts at cnt + sub_stride), twice the gammas, tape and segments; everything else of the engine is shared.  No context
 * (*out stays null: the host loop draws) with INSTRUCT_P_DEVICE=0 or more alleles at a locus than a group holds; a plan that does not fit the
 * engine (more than WK_MAXSEG segments) clears `usable` at the first sweep (pdev_update_P_once). */
static int pdev_create_allo(isg_ctx *c, PDevCtx **out, int L, int K, int Amax, const int *allelenum, long long sub_stride)
{
	*out = nullptr;
	if (!env_flag(getenv("INSTRUCT_P_DEVICE"), true)) return 0;
	PGroups pg;
	if (!pgroups_build(pg, L, K, Amax, allelenum, 0, 2, sub_stride, WK_NGMAX) || pg.gam0.size() < 2) return 0;
	PDevCtx *p = new PDevCtx();
	p->gam0_h = pg.gam0;
	p->G = (int)pg.gam0.size() - 1;
	p->NG = (int)pg.gidx.size();
	p->walk.seg_groups = (int)env_int(getenv("INSTRUCT_WALK_SEG"), 12800, 64, INT_MAX);
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
	HIPCHK(hipMemcpy(p->d_gidx, pg.gidx.data(), sizeof(int) * p->NG, hipMemcpyHostToDevice));
	p->usable = true;
	return 0;
}

/* ---- exact accumulators in global memory: 4 x 32-bit limbs in 64-bit words + flags ---- */
__device__ __forceinline__ void acc_global_add(unsigned long long *slot, const isg_acc &a)
{
	AccLimbs s = acc_to_limbs(a);
	atomicAdd(&slot[0], s.l0);
	atomicAdd(&slot[1], s.l1);
	atomicAdd(&slot[2], s.l2);
	atomicAdd(&slot[3], s.l3);
	if (s.flags) atomicOr(&slot[4], (unsigned long long)s.flags);
}
/* acc += count * v (v added `count` times: the fixed-point image of v is multiplied) */
__host__ __device__ inline void acc_add_times(isg_acc *a, double v, unsigned long long count)
{
	isg_acc one;
	isg_acc_zero(&one);
	isg_acc_add(&one, v);
	a->flags |= one.flags;
	if (!count) return;
	/* two's complement 128-bit times 32-bit */
	const unsigned long long c = count; /* < 2^32 */
	const unsigned long long a0 = one.lo & 0xffffffffULL, a1 = one.lo >> 32, a2 = one.hi & 0xffffffffULL, a3 = one.hi >> 32;
	unsigned long long t0 = a0 * c, t1 = a1 * c + (t0 >> 32), t2 = a2 * c + (t1 >> 32), t3 = a3 * c + (t2 >> 32);
	const unsigned long long lo = (t0 & 0xffffffffULL) | (t1 << 32), hi = (t2 & 0xffffffffULL) | (t3 << 32);
	isg_acc_add_raw(a, lo, hi);
}

__device__ __forceinline__ int poly_gid(const PolyDev &p, int j, unsigned g0, unsigned g1, unsigned g2, unsigned g3)
{
	const int cl = p.lclass[j], n = p.pc[cl].n;
	return p.gidmap[p.gidoff[cl] + (int)(((g0 * n + g1) * n + g2) * n + g3)];
}
/* the same row in a wide-allele context (more than 16 alleles at some locus): closed form instead of the map */
template <bool ALLO>
__device__ __forceinline__ int poly_row_w(const PolyDev &p, int j, unsigned g0, unsigned g1, unsigned g2, unsigned g3)
{
	const int n = p.pc[p.lclass[j]].n;
	return ALLO ? isg_allo_row(n, (int)g0, (int)g1, (int)g2, (int)g3) : isg_poly_rank(n, (int)g0, (int)g1, (int)g2, (int)g3);
}
/* category from the table row (rows are grouped by class): 0 iiii 1 iiij 2 iijj 3 iijk 4 ijkl */
__device__ __forceinline__ int poly_cat(const PolyDev &p, int j, int gid)
{
	const isg_polyclass &c = p.pc[p.lclass[j]];
	int b = c.g[1];
	if (gid < b) return 0;
	b += c.g[2];
	if (gid < b) return 1;
	b += c.g[3];
	if (gid < b) return 2;
	b += c.g[4];
	return gid < b ? 3 : 4;
}
__device__ __forceinline__ double poly_coef_log(int cat) /* log 4, 6, 12, 24 (poly_geno.c:1265-1270) */
{
	return cat == 1 ? isg_log(4.0) : cat == 2 ? isg_log(6.0) : cat == 3 ? isg_log(12.0) : cat == 4 ? isg_log(24.0) : 0.0;
}
__device__ __forceinline__ double allo_coef_log(int cat) /* log 2, 2, 4 (poly_geno.c:1275-1280) */
{
	return (cat == 1 || cat == 2) ? isg_log(2.0) : cat == 3 ? isg_log(4.0) : 0.0;
}
/* two / tri / tetra_allele_allo (poly_geno.c:2466-2507, 2532-2612, 2614-2656): candidate -> positions into the observed
 * allele list, 4 x 2 bits (first subgenome's pair in the low bits).  7 candidates for two observed alleles, 12 for three,
 * 6 for four (POLY.num_allogeno, poly_geno.c:146-149) */
__device__ __forceinline__ unsigned allo_pattern(int naid, int cand)
{
#define AP(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
	const unsigned t2[7] = {AP(0, 0, 0, 1), AP(0, 1, 0, 0), AP(0, 0, 1, 1), AP(1, 1, 0, 0), AP(0, 1, 1, 1), AP(1, 1, 0, 1), AP(0, 1, 0, 1)};
	const unsigned t3[12] = {AP(0, 0, 1, 2), AP(1, 2, 0, 0), AP(1, 1, 0, 2), AP(0, 2, 1, 1), AP(2, 2, 0, 1), AP(0, 1, 2, 2),
				 AP(0, 1, 1, 2), AP(1, 2, 0, 1), AP(1, 2, 0, 2), AP(0, 2, 1, 2), AP(0, 2, 0, 1), AP(0, 1, 0, 2)};
	const unsigned t4[6] = {AP(0, 1, 2, 3), AP(2, 3, 0, 1), AP(0, 2, 1, 3), AP(1, 3, 0, 2), AP(0, 3, 1, 2), AP(1, 2, 0, 3)};
#undef AP
	return naid == 2 ? t2[cand] : naid == 3 ? t3[cand] : t4[cand];
}
#ifdef ISG_DIAG_ALLO_PREFILTER /* diagnostic builds only: draws of update_geno and how many of them the double precision path redid */
__device__ unsigned long long isg_diag_allo_draws[2];
#endif
__device__ __forceinline__ float allo_sel4(const float (&v)[4], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3]; }
/* initial_geno (uniform over the candidates, choose_unif poly_geno.c:840-852) and update_geno with choose_two / tri /
 * tetra_allo (poly_geno.c:962-1215) for -ap 0: one uniform per locus with two or more observed alleles */
template <int KMAX>
__device__ __forceinline__ void geno_one_allo(const PolyDev &p, const isg_wh &base, int init, const double *tape, int i, int j, const float (&qf)[KMAX])
{
	const size_t id = (size_t)i * p.Lp + j;
	unsigned o[4] = {0xff, 0xff, 0xff, 0xff};
	int naid = 0;
	if (j < p.L) {
		const unsigned w = *(const unsigned *)(p.obs + id * 4);
		for (int k = 0; k < 4; k++) {
			o[k] = (w >> (8 * k)) & 0xff;
			naid += (o[k] != 0xff);
		}
	}
	const bool amb = naid >= 2;
	const unsigned long long am = __ballot(amb);
	if (naid == 0) return;
	unsigned g[4] = {o[0], o[0], o[0], o[0]};
	if (amb) {
		const unsigned long long pos = p.ambwave[(size_t)i * p.nwv + (j >> 6)] + (unsigned)__popcll(am & ((1ull << lane_id()) - 1ull));
		double x;
		if (tape) x = tape[pos];
		else {
			isg_wh s = isg_wh_jump(p.tab, base, pos);
			x = isg_wh_next(&s);
		}
		const int nc = naid == 2 ? 7 : naid == 3 ? 12 : 6;
		double cum[12];
		int pick = -1; /* decided by the single precision pre-decision below, else by the double precision path */
		if (init) {
			for (int a = 0; a < nc; a++) cum[a] = (double)(a + 1) / (double)nc;
		} else {
			const uint8_t *zz = p.z + id * 4;
			const int n = p.pc[p.lclass[j]].n;
			/*
			 * Single precision pre-decision (as geno_one's, for 7, 12 or 6 candidates).  The weights are w_a = exp(t_a - t_0), the running sums
			 * c_m = w_0 + .. + w_m, and the draw picks #{m < nc - 1 : c_m / tot < x} (isg_bucket: the LAST i with c_{i-1} < x tot <= c_i, 0 if
			 * none; the c_m do not decrease, so that is the count).  With u = 2^-24, K clusters and M = max |log| that enters:
			 *   f   K products of two rounded inputs and K - 1 additions of positive terms       relative (K + 2) u
			 *   l   v_log_f32 (1 ulp of log2 f), times the rounded ln 2                           absolute (K + 2) u + 4 M u
			 *   t   a constant and four logs, four additions of partial sums <= 4 M + 0.7         absolute (4 K + 11 + 32 M) u
			 *   d   t_a - t_0, |d| <= 8 M + 1.4, one rounding                                     absolute (8 K + 24 + 72 M) u
			 *   w   d times the rounded log2 e (2 u |d|), v_exp_f32 (1 ulp = 2 u)                  relative e = (8 K + 29 + 88 M) u
			 * (same-cluster loci read t from the float table the double path reads too: only the last two rows apply, e covers them with M = max |t|).
			 * c_m / tot = A / (A + B) with A and B sums of weights, each within a factor 1 +- e: it moves by at most 2 e r (1 - r) <= e / 2; the
			 * up to 11 float additions of each sum and x tot (x rounded, one product) add 24 u.  The band is twice that first-order bound,
			 * e + 48 u = (8 K + 77 + 88 M) u of tot around every one of the nc - 1 thresholds: 4e-5 for K = 10 and frequencies around 0.1.
			 * M <= 60 is required (f >= 9e-27: products flushed to zero, < 1.2e-38 each, stay below u f; e < 4e-4, so first order holds);
			 * beyond it, inside a band, or with tot not finite (overflow, NaN) the double precision path below decides.
			 */
			if (p.allo_pref) {
				const float *freq2f = p.freqf + (size_t)p.Lp * p.Amax * p.KPF;
				const bool samez_f = (zz[0] == zz[1] && zz[0] == zz[2] && zz[0] == zz[3]);
				float l1f[4] = {0.f, 0.f, 0.f, 0.f}, l2f[4] = {0.f, 0.f, 0.f, 0.f}, lmax = 0.f;
				const float *tbf = p.genofreq + ((size_t)zz[0] * p.L + j) * p.GS;
				if (!samez_f) {
#pragma unroll
					for (int a = 0; a < 4; a++) {
						if (a >= naid) continue;
						const size_t r = ((size_t)j * p.Amax + o[a]) * p.KPF; /* whole rows with 16-byte loads (zero padded to KPF = K up to 4) */
						const float4 *R1 = (const float4 *)(p.freqf + r), *R2 = (const float4 *)(freq2f + r);
						float f1 = 0.f, f2 = 0.f;
#pragma unroll
						for (int b = 0; b < KMAX / 4; b++) {
							if (4 * b >= p.KPF) continue;
							const float4 r1 = R1[b], r2 = R2[b];
							f1 += qf[4 * b] * r1.x + qf[4 * b + 1] * r1.y + qf[4 * b + 2] * r1.z + qf[4 * b + 3] * r1.w;
							f2 += qf[4 * b] * r2.x + qf[4 * b + 1] * r2.y + qf[4 * b + 2] * r2.z + qf[4 * b + 3] * r2.w;
						}
						l1f[a] = __builtin_amdgcn_logf(f1) * 0.693147180559945f;
						l2f[a] = __builtin_amdgcn_logf(f2) * 0.693147180559945f;
						lmax = __builtin_fmaxf(lmax, __builtin_fmaxf(__builtin_fabsf(l1f[a]), __builtin_fabsf(l2f[a])));
					}
				}
				float cf[12], t0 = 0.f;
#pragma unroll
				for (int a = 0; a < 12; a++) {
					cf[a] = 0.f;
					if (a >= nc) continue;
					const unsigned pt = allo_pattern(naid, a);
					const int p0 = pt & 3, p1 = (pt >> 2) & 3, p2 = (pt >> 4) & 3, p3 = (pt >> 6) & 3;
					float t;
					if (samez_f) {
						t = tbf[isg_allo_row(n, (int)o[p0], (int)o[p1], (int)o[p2], (int)o[p3])];
						lmax = __builtin_fmaxf(lmax, __builtin_fabsf(t));
					} else {
						t = (p0 != p1 && p2 != p3 && naid < 4) ? 0.693147180559945f + allo_sel4(l1f, p0) : allo_sel4(l1f, p0);
						t += allo_sel4(l1f, p1);
						t += allo_sel4(l2f, p2);
						t += allo_sel4(l2f, p3);
					}
					if (a == 0) { t0 = t; cf[0] = 1.f; }
					else cf[a] = cf[a - 1] + __builtin_amdgcn_exp2f((t - t0) * 1.44269504f);
				}
				float tot = cf[0];
#pragma unroll
				for (int a = 1; a < 12; a++) tot = (a < nc) ? cf[a] : tot;
				const float pf = (float)x * tot, band = ((float)(8 * p.K + 77) + 88.f * lmax) * 5.9604645e-8f * tot;
				bool clear = (tot < 1e30f) && (lmax <= 60.f);
				int below = 0;
#pragma unroll
				for (int m = 0; m < 11; m++) {
					if (m >= nc - 1) continue;
					clear = clear && (__builtin_fabsf(pf - cf[m]) > band);
					below += (pf > cf[m]) ? 1 : 0;
				}
				if (clear) pick = below;
			}
#ifdef ISG_DIAG_ALLO_PREFILTER
			atomicAdd(&isg_diag_allo_draws[0], 1ull);
			if (pick < 0) atomicAdd(&isg_diag_allo_draws[1], 1ull);
#endif
			if (pick < 0) {
			double tmp[12];
			if (zz[0] == zz[1] && zz[0] == zz[2] && zz[0] == zz[3]) {
				const float *tb = p.genofreq + ((size_t)zz[0] * p.L + j) * p.GS;
				for (int a = 0; a < nc; a++) {
					const unsigned pt = allo_pattern(naid, a);
					tmp[a] = (double)tb[isg_allo_row(n, (int)o[pt & 3], (int)o[(pt >> 2) & 3], (int)o[(pt >> 4) & 3], (int)o[(pt >> 6) & 3])];
				}
			} else {
				double l1[4], l2[4]; /* log of the individual's expected allele frequency in the two subgenomes */
				for (int a = 0; a < naid; a++) {
					double f1 = 0, f2 = 0;
					for (int b = 0; b < p.K; b++) {
						const double q = p.qq[(size_t)i * p.K + b];
						f1 += q * p.freq[((size_t)j * p.Amax + o[a]) * p.KP + b];
						f2 += q * p.freq2[((size_t)j * p.Amax + o[a]) * p.KP + b];
					}
					l1[a] = isg_log(f1);
					l2[a] = isg_log(f2);
				}
				const double log2c = isg_log(2.0);
				for (int a = 0; a < nc; a++) { /* the reference's sums, term by term in its order (poly_geno.c:1010-1022, 1099-1121, 1193-1203) */
					const unsigned pt = allo_pattern(naid, a);
					const int p0 = pt & 3, p1 = (pt >> 2) & 3, p2 = (pt >> 4) & 3, p3 = (pt >> 6) & 3;
					const bool hetA = p0 != p1, hetB = p2 != p3;
					double v;
					if (hetA && hetB && naid < 4) v = log2c + l1[p0] + l1[p1];
					else if (hetA) v = l1[p0] + l1[p1];
					else v = 2 * l1[p0];
					if (hetB) { v += l2[p2]; v += l2[p3]; }
					else v += 2 * l2[p2];
					tmp[a] = v;
				}
			}
			const double tm = tmp[0];
			cum[0] = 1.0; /* exp(tmp[0] - tmp[0]): isg_exp(0) == 1 exactly (checked at context creation) */
			for (int a = 1; a < nc; a++) cum[a] = isg_exp(tmp[a] - tm) + cum[a - 1];
			}
		}
		if (pick < 0) pick = isg_bucket(x, cum, nc);
		const unsigned pt = allo_pattern(naid, pick);
		g[0] = o[pt & 3]; g[1] = o[(pt >> 2) & 3]; g[2] = o[(pt >> 4) & 3]; g[3] = o[(pt >> 6) & 3];
	}
	*(unsigned *)(p.geno + id * 4) = g[0] | (g[1] << 8) | (g[2] << 8 * 2) | (g[3] << 8 * 3);
}
__device__ __forceinline__ void poly_set(unsigned num, int naid, const unsigned o[4], unsigned g[4])
{
	/* two_allele_auto (poly_geno.c:2440-2464) / tri_allele_auto (:2509-2530) */
	if (naid == 2) {
		if (num == 1) { g[0] = o[0]; g[1] = o[0]; g[2] = o[0]; g[3] = o[1]; }
		else if (num == 2) { g[0] = o[1]; g[1] = o[1]; g[2] = o[1]; g[3] = o[0]; }
		else { g[0] = o[0]; g[1] = o[0]; g[2] = o[1]; g[3] = o[1]; }
	} else {
		if (num == 1) { g[0] = o[0]; g[1] = o[0]; g[2] = o[1]; g[3] = o[2]; }
		else if (num == 2) { g[0] = o[1]; g[1] = o[1]; g[2] = o[0]; g[3] = o[2]; }
		else { g[0] = o[2]; g[1] = o[2]; g[2] = o[0]; g[3] = o[1]; }
	}
}

/* initial_geno (poly_geno.c:316-369, uniform choice) and update_geno (:520-580, choose_two/tri_auto :854-960) */
template <int KMAX, bool WIDE>
__device__ __forceinline__ void geno_one(const PolyDev &p, const isg_wh &base, int init, const double *tape, int i, int j, const float (&qf)[KMAX])
{
	const size_t id = (size_t)i * p.Lp + j;
	unsigned o[4] = {0xff, 0xff, 0xff, 0xff};
	int naid = 0;
	if (j < p.L) {
		const unsigned w = *(const unsigned *)(p.obs + id * 4);
		for (int k = 0; k < 4; k++) {
			o[k] = (w >> (8 * k)) & 0xff;
			naid += (o[k] != 0xff);
		}
	}
	const bool amb = (naid == 2 || naid == 3);
	const unsigned long long am = __ballot(amb);
	if (naid == 0) return;
	unsigned g[4];
	if (naid == 1) { g[0] = g[1] = g[2] = g[3] = o[0]; }
	else if (naid == 4) { g[0] = o[0]; g[1] = o[1]; g[2] = o[2]; g[3] = o[3]; }
	else {
		const unsigned long long pos = p.ambwave[(size_t)i * p.nwv + (j >> 6)] + (unsigned)__popcll(am & ((1ull << lane_id()) - 1ull));
		double x;
		if (tape) x = tape[pos];
		else {
			isg_wh s = isg_wh_jump(p.tab, base, pos);
			x = isg_wh_next(&s);
		}
		double cum[3];
		int pick = -1; /* decided by the single precision pre-filter below, else by the double precision path */
		if (init) { /* choose_unif(3), poly_geno.c:840-852 */
			cum[0] = 1.0 / 3.0; cum[1] = 2.0 / 3.0; cum[2] = 3.0 / 3.0;
		} else {
			const uint8_t *zz = p.z + id * 4;
			const int n = p.pc[p.lclass[j]].n;
			const bool samez = (zz[0] == zz[1] && zz[0] == zz[2] && zz[0] == zz[3]);
			int num[3] = {0, 0, 0};
			if (samez) {
				if (naid == 2) {
					num[0] = o[0] * n * (n * n + n + 1) + o[1];
					num[1] = o[1] * n * (n * n + n + 1) + o[0];
					num[2] = (o[0] * n * n + o[1]) * (n + 1);
				} else {
					num[0] = o[0] * n * n * (n + 1) + o[1] * n + o[2];
					num[1] = o[1] * n * n * (n + 1) + o[0] * n + o[2];
					num[2] = o[2] * n * n * (n + 1) + o[0] * n + o[1];
				}
				if (WIDE) { /* the same three genotypes, rows in closed form */
					num[0] = naid == 2 ? isg_poly_rank(n, o[0], o[0], o[0], o[1]) : isg_poly_rank(n, o[0], o[0], o[1], o[2]);
					num[1] = naid == 2 ? isg_poly_rank(n, o[1], o[1], o[1], o[0]) : isg_poly_rank(n, o[1], o[1], o[0], o[2]);
					num[2] = naid == 2 ? isg_poly_rank(n, o[0], o[0], o[1], o[1]) : isg_poly_rank(n, o[2], o[2], o[0], o[1]);
				} else
				for (int a = 0; a < 3; a++) num[a] = p.gidmap[p.gidoff[p.lclass[j]] + num[a]];
			}
			/*
			 * Single precision pre-filter.  The three candidate weights are exp(t_a - t_0); the draw picks
			 * #{m < 2 : cum_m / tot < x}.  Evaluated in float (v_log_f32 / v_exp_f32, 1 ulp each; K-term sums
			 * of float products) every cum_m / tot is within ~1.5e-5 of its double precision value, so outside
			 * a band of 1e-4 around the two thresholds the float comparison IS the reference's choice; inside
			 * the band, or with non-finite intermediates, the double precision path below decides.
			 */
			{
				float tf[3];
				if (samez) {
					const float *tb = p.genofreq + ((size_t)zz[0] * p.L + j) * p.GS;
					for (int a = 0; a < 3; a++) tf[a] = tb[num[a]];
				} else {
					float lf[3] = {0.f, 0.f, 0.f};
					/* whole rows with 16-byte loads, all in flight together (rows are zero padded to KPF = K up to 4) */
					float4 row[3][KMAX / 4];
#pragma unroll
					for (int a = 0; a < 3; a++) {
						const float4 *R = (const float4 *)(p.freqf + ((size_t)j * p.Amax + o[a < naid ? a : 0]) * p.KPF);
#pragma unroll
						for (int b = 0; b < KMAX / 4; b++) row[a][b] = (4 * b < p.KPF) ? R[b] : make_float4(0.f, 0.f, 0.f, 0.f);
					}
#pragma unroll
					for (int a = 0; a < 3; a++) {
						float f = 0.f;
#pragma unroll
						for (int b = 0; b < KMAX / 4; b++)
							f += qf[4 * b] * row[a][b].x + qf[4 * b + 1] * row[a][b].y + qf[4 * b + 2] * row[a][b].z + qf[4 * b + 3] * row[a][b].w;
						lf[a] = __builtin_amdgcn_logf(f) * 0.693147180559945f;
					}
					if (naid == 2) {
						tf[0] = 1.38629436f + 3.f * lf[0] + lf[1];
						tf[1] = 1.38629436f + 3.f * lf[1] + lf[0];
						tf[2] = 1.79175947f + 2.f * lf[0] + 2.f * lf[1];
					} else {
						tf[0] = 2.f * lf[0] + lf[1] + lf[2];
						tf[1] = 2.f * lf[1] + lf[0] + lf[2];
						tf[2] = 2.f * lf[2] + lf[1] + lf[0];
					}
				}
				const float e1 = __builtin_amdgcn_exp2f((tf[1] - tf[0]) * 1.44269504f), e2 = __builtin_amdgcn_exp2f((tf[2] - tf[0]) * 1.44269504f);
				const float c0 = 1.f, c1 = 1.f + e1, tot = c1 + e2;
				const float pf = (float)x * tot, band = 1e-4f * tot;
				const bool clear = (tot < 1e30f) && (__builtin_fabsf(pf - c0) > band) && (__builtin_fabsf(pf - c1) > band);
				if (clear) pick = (pf > c0 ? 1 : 0) + (pf > c1 ? 1 : 0);
			}
			if (pick < 0) {
			double tmp[3];
			if (samez) {
				const float *tb = p.genofreq + ((size_t)zz[0] * p.L + j) * p.GS;
				for (int a = 0; a < 3; a++) tmp[a] = (double)tb[num[a]];
			} else {
				double fq[3];
				for (int a = 0; a < naid; a++) {
					fq[a] = 0;
					for (int b = 0; b < p.K; b++) fq[a] += p.qq[(size_t)i * p.K + b] * p.freq[((size_t)j * p.Amax + o[a]) * p.KP + b];
				}
				const double l0 = isg_log(fq[0]), l1 = isg_log(fq[1]);
				if (naid == 2) {
					tmp[0] = p.log4 + 3 * l0 + l1;
					tmp[1] = p.log4 + 3 * l1 + l0;
					tmp[2] = p.log6 + 2 * l0 + 2 * l1;
				} else {
					const double l2 = isg_log(fq[2]);
					tmp[0] = 2 * l0 + l1 + l2;
					tmp[1] = 2 * l1 + l0 + l2;
					tmp[2] = 2 * l2 + l1 + l0;
				}
			}
			const double tm = tmp[0];
			tmp[0] = 1.0; /* exp(tmp[0] - tmp[0]): isg_exp(0) == 1 exactly (checked at context creation) */
			for (int a = 1; a < 3; a++) tmp[a] = isg_exp(tmp[a] - tm);
			cum[0] = tmp[0];
			cum[1] = tmp[1] + cum[0];
			cum[2] = tmp[2] + cum[1];
			}
		}
		if (pick < 0) pick = isg_bucket(x, cum, 3);
		poly_set((unsigned)pick + 1u, naid, o, g);
	}
	*(unsigned *)(p.geno + id * 4) = g[0] | (g[1] << 8) | (g[2] << 8 * 2) | (g[3] << 8 * 3);
}

/*
 * A workgroup keeps a tile of 256 loci and walks a chunk of individuals; blocks are dealt round-robin over the 8
 * XCDs, so block b serves tile (b / 8 / nchunk) * 8 + b % 8: all chunks of a tile run on ONE XCD, whose 4 MB L2 then
 * holds the frequency rows and genotype-class tables of the handful of tiles in flight (without this every
 * individual re-streams the tables from the memory side: 23 GB per sweep at config 5).
 * One wave = 64 consecutive loci of ONE individual (the stream rank of a locus is a ballot prefix).
 */
/* ALLO: the allotetraploid genotype draw (a template parameter: the autotetraploid kernel does not carry its registers).
 * WIDE: the autotetraploid draw of a wide-allele context (the allotetraploid draw has closed-form rows already: ALLO && WIDE is not used) */
template <int KMAX, bool ALLO, bool WIDE = false>
__global__ void __launch_bounds__(256) k4_geno(PolyDev p, isg_wh base, int init, const double *tape, int chunk, int nchunk)
{
	const int b = (int)blockIdx.x, r = b >> 3;
	const int tile = (r / nchunk) * 8 + (b & 7), ch = r % nchunk;
	const int j = tile * 256 + (int)threadIdx.x, i0 = ch * chunk, i1 = min(p.N, i0 + chunk);
	if (tile * 256 >= p.Lp) return;
	for (int i = i0; i < i1; i++) {
		float qf[KMAX]; /* the individual's admixture row in single precision (pre-filter only) */
#pragma unroll
		for (int m = 0; m < KMAX; m++) qf[m] = (m < p.K && !init) ? (float)p.qq[(size_t)i * p.K + m] : 0.f;
		if (ALLO) geno_one_allo<KMAX>(p, base, init, tape, i, j, qf);
		else geno_one<KMAX, WIDE>(p, base, init, tape, i, j, qf);
	}
}

#ifdef ISG_DIAG_ALLO_PREFILTER
extern "C" int isg_diag_allo_prefilter(long out[2]) /* {draws of update_geno, of them redone in double precision} since the library was loaded */
{
	unsigned long long v[2] = {0, 0};
	HIPCHK(hipMemcpyFromSymbol(v, HIP_SYMBOL(isg_diag_allo_draws), sizeof(v)));
	out[0] = (long)v[0];
	out[1] = (long)v[1];
	return 0;
}
#endif

/*
 * THE sweep over (genotype, Z) of an iteration, shared by update_P_auto and update_S_POP:
 *   cnt    [L][Amax][K]  allele counts of the imputed genotypes (update_P_auto, poly_geno.c:406-425)
 *   cntmix [L][Amax][K]  the same restricted to loci whose 4 copies sit in different clusters
 *   ccnt   [K][L][GS]    genotype counts of the loci whose 4 copies sit in ONE cluster
 *   catcnt [5]           loci of the first kind per genotype category (their multinomial coefficient)
 * With these the log-likelihoods update_S_POP compares (cal_lkd_props :645, cal_lkd :715) are sums over the
 * tables: sum cntmix log freq + sum catcnt log coef + sum ccnt genofreq -- no further pass over N x L.
 * A workgroup takes 64 loci (one wave = 256 contiguous bytes of a row) x a chunk of individuals and keeps both
 * allele count tiles in LDS ([allele][cluster][locus]: lanes of a wave hit distinct banks).
 */
/* WIDE: a wide-allele context, where same-cluster loci find their row in closed form */
template <bool TILE, bool ALLO, bool WIDE>
__global__ void __launch_bounds__(256) k4_sweep_counts(PolyDev p, int chunk, int *cntmix, unsigned long long *catcnt)
{
	extern __shared__ int tile[]; /* [2][Amax * K][64] */
	const int AK = p.Amax * p.K, lane = (int)lane_id(), wave = threadIdx.x >> 6;
	const int j = blockIdx.x * 64 + lane, i0 = blockIdx.y * chunk, i1 = min(p.N, i0 + chunk);
	if (TILE) {
		for (int e = threadIdx.x; e < 2 * AK * 64; e += 256) tile[e] = 0;
		__syncthreads();
	}
	unsigned ncat[5] = {0, 0, 0, 0, 0};
	if (j < p.L) {
		for (int i = i0 + wave; i < i1; i += 4) {
			const size_t id = (size_t)i * p.Lp + j;
			const unsigned g = *(const unsigned *)(p.geno + id * 4);
			if ((g & 0xff) == 0xff) continue;
			const unsigned z = *(const unsigned *)(p.z + id * 4);
			const bool same = (z == (z & 0xff) * 0x01010101u);
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const int a = (g >> (8 * c)) & 0xff, k = (z >> (8 * c)) & 0xff;
				if (TILE) {
					atomicAdd(&tile[(a * p.K + k) * 64 + lane], 1);
					if (!same) atomicAdd(&tile[(AK + a * p.K + k) * 64 + lane], 1);
				} else if (ALLO && c >= 2) { /* the second subgenome's copies (seqpop2, poly_geno.c:481-492) */
					atomicAdd(&p.cnt2[((size_t)j * p.Amax + a) * p.K + k], 1);
					if (!same) atomicAdd(&p.cntmix2[((size_t)j * p.Amax + a) * p.K + k], 1);
				} else {
					atomicAdd(&p.cnt[((size_t)j * p.Amax + a) * p.K + k], 1);
					if (!same) atomicAdd(&cntmix[((size_t)j * p.Amax + a) * p.K + k], 1);
				}
			}
			const unsigned g0 = g & 0xff, g1 = (g >> 8) & 0xff, g2 = (g >> 16) & 0xff, g3 = g >> 24;
			if (same) {
				atomicAdd(&p.ccnt[((size_t)(z & 0xff) * p.L + j) * p.GS + (WIDE ? poly_row_w<ALLO>(p, j, g0, g1, g2, g3) : poly_gid(p, j, g0, g1, g2, g3))], 1);
			} else if (ALLO) { /* get_cat_allo (poly_geno.c:1341-1372) */
				ncat[(g0 != g1 ? 2 : 0) + (g2 != g3 ? 1 : 0)]++;
			} else {
				/* get_cat_auto (poly_geno.c:1313-1339): distinct alleles; two of them: 2+2 or 3+1 */
				const int nd = 1 + (g1 != g0) + (g2 != g0 && g2 != g1) + (g3 != g0 && g3 != g1 && g3 != g2);
				const int m0 = 1 + (g1 == g0) + (g2 == g0) + (g3 == g0);
				ncat[nd == 1 ? 0 : nd == 2 ? (m0 == 2 ? 2 : 1) : nd]++;
			}
		}
	}
	if (TILE) {
		__syncthreads();
		for (int e = threadIdx.x; e < 2 * AK * 64; e += 256) {
			const int v = tile[e];
			const int l = e & 63, r = e >> 6, jj = blockIdx.x * 64 + l;
			if (v && jj < p.L) {
				if (r < AK) atomicAdd(&p.cnt[(size_t)jj * AK + r], v);
				else atomicAdd(&cntmix[(size_t)jj * AK + (r - AK)], v);
			}
		}
	}
#pragma unroll
	for (int q = 1; q < 5; q++) {
		unsigned v = ncat[q];
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
		if (lane == 0 && v) atomicAdd(&catcnt[q], (unsigned long long)v);
	}
}

/* sum over (locus, allele, cluster) of cntmix * log freq -> accbuf slot 0 (exact) */
__global__ void __launch_bounds__(256) k4_mixsum(PolyDev p, const int *cntmix, const double *freq)
{
	__shared__ unsigned long long sm[4 * 5];
	const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
	isg_acc a;
	isg_acc_zero(&a);
	if (id < (size_t)p.L * p.Amax * p.K) {
		const unsigned c = (unsigned)cntmix[id];
		if (c) {
			const size_t r = id / p.K;
			acc_add_times(&a, isg_log(freq[r * p.KP + (id - r * p.K)]), c);
		}
	}
	const isg_acc r = block_reduce_acc<256>(a, sm);
	if (threadIdx.x == 0) acc_global_add(p.accbuf, r);
}

/* calc_exfreq_auto: one lane per (cluster, locus) */
template <bool ALLO>
__global__ void k4_exfreq(PolyDev p)
{
	const int id = blockIdx.x * blockDim.x + threadIdx.x;
	if (id >= p.K * p.L) return;
	const int k = id / p.L, j = id - k * p.L;
	const isg_polyclass pc = p.pc[p.lclass[j]];
	double f[ISG_POLY_ACAP];
	for (int a = 0; a < pc.n; a++) f[a] = p.freq[((size_t)j * p.Amax + a) * p.KP + k];
	if (ALLO) { /* calc_exfreq_allo, poly_geno.c:1592-1670 */
		double f2[ISG_POLY_ACAP];
		for (int a = 0; a < pc.n; a++) f2[a] = p.freq2[((size_t)j * p.Amax + a) * p.KP + k];
		ptd_exfreq_row_allo(&pc, f, f2, p.exfreq + (size_t)id * p.GS);
		return;
	}
	ptd_exfreq_row(&pc, f, p.exfreq + (size_t)id * p.GS);
}

/* auto_genfreq for all (cluster, locus) tables at the selfing rates self[k]: into genofreq (own) or tabtmp (proposals) */
template <bool ALLO>
__global__ void k4_genfreq(PolyDev p, const float *self, int own)
{
	const int id = blockIdx.x * blockDim.x + threadIdx.x;
	if (id >= p.K * p.L) return;
	const int k = id / p.L, j = id - k * p.L;
	const isg_polyclass pc = p.pc[p.lclass[j]];
	int e = 0;
	float *out = (own ? p.genofreq : p.tabtmp) + (size_t)id * p.GS;
	if (ALLO) ptd_genfreq_row_allo(self[k], &pc, p.exfreq + (size_t)id * p.GS, out, &e); /* allo_genfreq, poly_geno.c:2122-2304 */
	else ptd_genfreq_row(self[k], &pc, p.exfreq + (size_t)id * p.GS, out, &e);
	if (e) atomicOr(p.err, 4u); /* the reference stops on it for current and proposed rates alike (poly_geno.c:2021-2025) */
}

/*
 * Wide-allele contexts (more than 16 alleles at some locus, up to 32): one lane per table no longer scales, so here a workgroup takes one
 * (cluster, locus) table and its lanes share the rows.  The rows themselves are the per-row functions of isg_poly_tables.h, the ones the
 * kernels above run serially.  k4_genfreq_w takes the classes in dependency order -- autotetraploid: quadri -> tri (one lane per triple)
 * -> duplex -> simplex -> mono; allotetraploid: ijkl -> iikl and ijkk -> iikk.  A row reads only rows of earlier classes, so a workgroup
 * barrier between two classes is all the ordering it needs.
 */
/* calc_exfreq_auto / calc_exfreq_allo: one workgroup per (cluster, locus) table, blockIdx.x = k L + j */
template <bool ALLO>
__global__ void __launch_bounds__(256) k4_exfreq_w(PolyDev p)
{
	__shared__ double fs[2][ISG_POLY_ACAP_W];
	const int id = (int)blockIdx.x, k = id / p.L, j = id - k * p.L, t = (int)threadIdx.x;
	const isg_polyclass pc = p.pc[p.lclass[j]];
	if (t < pc.n) {
		fs[0][t] = p.freq[((size_t)j * p.Amax + t) * p.KP + k];
		if (ALLO) fs[1][t] = p.freq2[((size_t)j * p.Amax + t) * p.KP + k];
	}
	__syncthreads();
	float *ex = p.exfreq + (size_t)id * p.GS;
	for (int r = t; r < pc.G; r += 256) ex[r] = ALLO ? ptd_exfreq_allo_at(&pc, fs[0], fs[1], r) : ptd_exfreq_at(&pc, fs[0], r);
}

/* auto_genfreq / allo_genfreq at the selfing rates self[k] into genofreq (own) or tabtmp: one workgroup per table, blockIdx.x = k L + j */
template <bool ALLO>
__global__ void __launch_bounds__(256) k4_genfreq_w(PolyDev p, const float *self, int own)
{
	const int id = (int)blockIdx.x, k = id / p.L, j = id - k * p.L, t = (int)threadIdx.x;
	const isg_polyclass pc = p.pc[p.lclass[j]];
	const int G = pc.G, b1 = pc.g[1], b2 = b1 + pc.g[2], b3 = b2 + pc.g[3], b4 = b3 + pc.g[4];
	const float s = self[k];
	const float *ex = p.exfreq + (size_t)id * p.GS;
	float *fr = (own ? p.genofreq : p.tabtmp) + (size_t)id * p.GS;
	int e = 0;
	if (ALLO) {
		for (int r = b3 + t; r < G; r += 256) ptd_genfreq_allo_ijkl_at(s, ex, fr, r, &e);
		__syncthreads();
		for (int r = b1 + t; r < b3; r += 256) ptd_genfreq_allo_het_at(s, &pc, ex, fr, r, &e);
		__syncthreads();
		for (int r = t; r < b1; r += 256) ptd_genfreq_allo_iikk_at(s, &pc, ex, fr, r, &e);
	} else {
		for (int r = b4 + t; r < G; r += 256) ptd_genfreq_quadri_at(s, ex, fr, r, &e);
		__syncthreads();
		for (int r = b3 + 3 * t; r < b4; r += 3 * 256) ptd_genfreq_tri_at(s, &pc, ex, fr, r, &e);
		__syncthreads();
		for (int r = b2 + t; r < b3; r += 256) ptd_genfreq_duplex_at(s, &pc, ex, fr, r, &e);
		__syncthreads();
		for (int r = b1 + t; r < b2; r += 256) ptd_genfreq_simplex_at(s, &pc, ex, fr, r, &e);
		__syncthreads();
		for (int r = t; r < b1; r += 256) ptd_genfreq_mono_at(s, &pc, ex, fr, r, &e);
	}
	if (e) atomicOr(p.err, 4u);
}

/* D = sum over (locus, genotype) of count * table value: blockIdx.y = k for the current tables (slot 1 + k),
 * K + k for the proposal tables (slot 1 + K + k) */
__global__ void __launch_bounds__(256) k4_dsum(PolyDev p)
{
	__shared__ unsigned long long sm[4 * 5];
	const int use_tmp = (int)blockIdx.y >= p.K, k = (int)blockIdx.y - (use_tmp ? p.K : 0);
	const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
	isg_acc a;
	isg_acc_zero(&a);
	if (id < (size_t)p.L * p.GS) {
		const int j = (int)(id / p.GS), g = (int)(id - (size_t)j * p.GS);
		if (g < p.pc[p.lclass[j]].G) {
			const size_t e = ((size_t)k * p.L + j) * p.GS + g;
			const unsigned c = (unsigned)p.ccnt[e];
			if (c) acc_add_times(&a, (double)(use_tmp ? p.tabtmp[e] : p.genofreq[e]), c);
		}
	}
	const isg_acc r = block_reduce_acc<256>(a, sm);
	if (threadIdx.x == 0) acc_global_add(p.accbuf + 5 * (1 + (int)blockIdx.y), r);
}
/* the same sums in a wide-allele context (up to 278 784 genotypes per locus: one lane per entry made the block reductions and their atomics
 * the cost): a workgroup per (locus, blockIdx.y), its lanes striding over the locus' own genotypes.  The accumulators are exact integers,
 * so the grouping does not change the sums. */
__global__ void __launch_bounds__(256) k4_dsum_w(PolyDev p)
{
	__shared__ unsigned long long sm[4 * 5];
	const int use_tmp = (int)blockIdx.y >= p.K, k = (int)blockIdx.y - (use_tmp ? p.K : 0), j = (int)blockIdx.x;
	const int G = p.pc[p.lclass[j]].G;
	const size_t row = ((size_t)k * p.L + j) * p.GS;
	const float *tab = use_tmp ? p.tabtmp : p.genofreq;
	isg_acc a;
	isg_acc_zero(&a);
	for (int g = (int)threadIdx.x; g < G; g += 256) {
		const unsigned c = (unsigned)p.ccnt[row + g];
		if (c) acc_add_times(&a, (double)tab[row + g], c);
	}
	const isg_acc r = block_reduce_acc<256>(a, sm);
	if (threadIdx.x == 0) acc_global_add(p.accbuf + 5 * (1 + (int)blockIdx.y), r);
}

/* isg_log of every allele frequency, once per iteration (L Amax KP logarithms instead of four per mixed-cluster locus of every individual), and
 * the genotype table, both locus innermost; one lane per (row, locus), consecutive lanes consecutive loci */
__global__ void k4_logfreq(PolyDev p)
{
	const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const size_t nf = (size_t)p.Amax * p.KP * p.L, ng = (size_t)p.K * p.GS * p.L;
	if (id < nf) {
		const int j = (int)(id % p.L), row = (int)(id / p.L); /* row = a KP + k */
		const size_t src = (size_t)j * p.Amax * p.KP + row;
		p.lfreq[(size_t)row * p.Lp + j] = isg_log(p.freq[src]);
		if (p.allo) p.lfreq2[(size_t)row * p.Lp + j] = isg_log(p.freq2[src]);
	} else if (id - nf < ng) {
		const size_t e = id - nf;
		const int j = (int)(e % p.L), row = (int)(e / p.L); /* row = k GS + gid */
		const int k = row / p.GS, gid = row - k * p.GS;
		p.genofreqT[(size_t)row * p.Lp + j] = p.genofreq[((size_t)k * p.L + j) * p.GS + gid];
	}
}
/* cal_lkd: indvlkh[i] = exact sum of the individual's locus terms (calc_genofq, poly_geno.c:1235-1286) */
/* Four loci per lane and pass, every stage of the lookup chain (observation / genotype / assignment -> locus class -> class size and map offset ->
 * table row -> term) issued for all four before the next stage needs it: the chain is five dependent memory round trips, and one locus at a time the
 * waves waited for them 80 % of their cycles (SQ counters: 10 us per pass). */
template <bool ALLO, bool WIDE>
__device__ __forceinline__ void lkd_body(const PolyDev &p)
{
	__shared__ unsigned long long sm[4 * 5];
	const int i = blockIdx.x;
	isg_acc a;
	isg_acc_zero(&a);
	for (int jb = threadIdx.x; jb < p.L; jb += 4 * 256) {
		bool ok[4];
		unsigned g[4], z[4];
		int jj[4], cl[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int j = jb + 256 * u;
			jj[u] = (j < p.L) ? j : jb; /* (a locus past the end is its lane's first one again, not used) */
			const size_t id = (size_t)i * p.Lp + jj[u];
			ok[u] = (j < p.L) && p.obs[id * 4] != 0xff;
			g[u] = *(const unsigned *)(p.geno + id * 4);
			z[u] = *(const unsigned *)(p.z + id * 4);
			cl[u] = p.lclass[jj[u]];
		}
		int n[4], off[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			n[u] = p.pc[cl[u]].n;
			off[u] = WIDE ? 0 : p.gidoff[cl[u]];
		}
		int gid[4];
		bool same[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const unsigned g0 = g[u] & 0xff, g1 = (g[u] >> 8) & 0xff, g2 = (g[u] >> 16) & 0xff, g3 = g[u] >> 24;
			const unsigned code = ok[u] ? ((g0 * n[u] + g1) * n[u] + g2) * n[u] + g3 : 0u; /* (poly_gid) */
			if (WIDE) gid[u] = !ok[u] ? 0 : ALLO ? isg_allo_row(n[u], (int)g0, (int)g1, (int)g2, (int)g3) : isg_poly_rank(n[u], (int)g0, (int)g1, (int)g2, (int)g3);
			else gid[u] = p.gidmap[off[u] + (int)code];
			same[u] = (z[u] == (z[u] & 0xff) * 0x01010101u);
		}
		float gf[4];
		double lf[4][4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			gf[u] = 0.f;
			if (ok[u] && same[u]) gf[u] = p.genofreqT[((size_t)(z[u] & 0xff) * p.GS + gid[u]) * p.Lp + jj[u]];
			if (ok[u] && !same[u]) {
#pragma unroll
				for (int k = 0; k < 4; k++)
					lf[u][k] = ((ALLO && k >= 2) ? p.lfreq2 : p.lfreq)[((size_t)((g[u] >> (8 * k)) & 0xff) * p.KP + ((z[u] >> (8 * k)) & 0xff)) * p.Lp + jj[u]];
			}
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			if (!ok[u]) continue;
			if (same[u]) {
				isg_acc_add(&a, (double)gf[u]);
			} else {
#pragma unroll
				for (int k = 0; k < 4; k++) isg_acc_add(&a, lf[u][k]); /* log freq from the table (the same function of the same double: the same bits) */
				const int cat = poly_cat(p, jj[u], gid[u]);
				if (cat) isg_acc_add(&a, ALLO ? allo_coef_log(cat) : poly_coef_log(cat));
			}
		}
	}
	const isg_acc r = block_reduce_acc<256>(a, sm);
	if (threadIdx.x == 0) p.indvlkh[i] = isg_acc_value(&r);
}
template <bool ALLO>
__global__ void __launch_bounds__(256) k4_lkd(PolyDev p)
{
	lkd_body<ALLO, false>(p);
}
template <bool ALLO>
__global__ void __launch_bounds__(256) k4_lkd_w(PolyDev p) /* wide-allele contexts: closed-form rows */
{
	lkd_body<ALLO, true>(p);
}

/* update_ZQ (poly_geno.c:750-836): one workgroup walks the individuals in stream order */
/* CHAIN: one workgroup walks all individuals in stream order (replay schedule without the cooperative kernel);
 * !CHAIN: keyed schedule, one workgroup per individual, its stream position is pos0 + i * stride */
/* offs != null (with !CHAIN): the start positions resolved by k4_zq_block; individual i = blockIdx.x starts at offs[i] and its
 * consumption is checked against offs[i + 1] - offs[i]; rst: that launch sequence's state (nothing is done unless it finished) */
/* update_ZQ of individual i (poly_geno.c:763-830) started at stream state `cur`: its 4 nvalid Z draws, counts, Dirichlet; returns the uniforms
 * consumed.  WRITE = false: only that number is wanted (Z, qq, qqnum stay as they are).  sh.hist[par] zero on entry. */
/* The rare exact forms of a Z draw, out of line: their double precision arrays (the individual's qq row, the running sums) would otherwise be
 * live across the whole loop of k4_zq_one (235 registers, two waves per SIMD).  s = the generator's state AFTER the draw's step. */
template <int KMAX>
__device__ __attribute__((noinline)) int k4_draw_exact(const PolyDev *p, int i, int j, unsigned a, isg_wh s, int K)
{
	double q[KMAX], cum[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) q[m] = (m < K) ? p->qq[(size_t)i * K + m] : 0.0;
	const double x = isg_wh_value(&s);
	const double tot = weights<KMAX>(p->freq + ((size_t)j * p->Amax + a) * p->KP, q, cum, K);
	return bucket_fast<KMAX>(x, cum, tot, K);
}
template <int KMAX>
__device__ __attribute__((noinline)) int k4_draw_init(isg_wh s, int K) /* update_ZQ(init): uniform over the clusters */
{
	double cum[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) cum[m] = (m < K) ? (double)(m + 1) / K : 0.0;
	return bucket_fast<KMAX>(isg_wh_value(&s), cum, 1.0, K);
}
template <int BLOCK, int KMAX, bool WRITE>
__device__ __forceinline__ unsigned k4_zq_one(const PolyDev &p, const DevView &d, ZqShared &sh, int i, const isg_wh &cur, int init_flag, double alpha, int par)
{
	const int t = threadIdx.x, K = p.K;
	const int nvalid = p.nvalid[i];
	float qf[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) qf[m] = (m < K && !init_flag) ? (float)p.qq[(size_t)i * K + m] : 0.f;
	int wcnt[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) wcnt[m] = 0;
	for (int j = t; j - t < p.Lp; j += BLOCK) {
		const size_t id = (size_t)i * p.Lp + j;
		const bool valid = (j < p.L) && p.obs[id * 4] != 0xff;
		const unsigned long long vm = __ballot(valid);
		unsigned zout = 0xffffffffu;
		int zz[4] = {0xff, 0xff, 0xff, 0xff};
		if (valid) {
			const unsigned rank = p.rankwave[(size_t)i * p.nwv + (j >> 6)] + (unsigned)__popcll(vm & ((1ull << lane_id()) - 1ull));
			constexpr bool PREF = (KMAX <= 16); /* instances with the single precision pre-filter */
			isg_wh si = isg_wh_jump32(&sh.tab, cur, 4u * rank);
			isg_whf s = isg_whf_of(si);
			const unsigned g = *(const unsigned *)(p.geno + id * 4);
			zout = 0;
			for (int c = 0; c < 4; c++) {
				/* the pre-filter takes the uniform's single precision value (|error| < 1e-6: inside bucket_f32's band, as in the diploid zq_one), from
				 * the generator stepped in single precision (isg_whf); the exact value (three double precision divisions) only in the draws that
				 * are redone.  Without a pre-filter (KMAX > 16) every draw takes the exact value: the integer step stays */
				if (PREF) isg_whf_step(&s);
				else isg_wh_step(&si);
				if (init_flag) {
					zz[c] = k4_draw_init<KMAX>(PREF ? isg_whf_to(s) : si, K);
				} else {
					bool amb = true;
					if (KMAX <= 16) { /* single precision pre-filter (see bucket_f32); flagged draws redone in double */
						const float *R = d.freqf + ((size_t)j * p.Amax + ((g >> (8 * c)) & 0xff)) * d.KPF;
						float F[KMAX];
#pragma unroll
						for (int m = 0; m < KMAX; m += 4) {
							if (m < K) {
								const float4 f = *(const float4 *)(R + m);
								F[m] = f.x;
								if (m + 1 < KMAX) F[m + 1] = f.y;
								if (m + 2 < KMAX) F[m + 2] = f.z;
								if (m + 3 < KMAX) F[m + 3] = f.w;
							} else {
								F[m] = 0.f;
								if (m + 1 < KMAX) F[m + 1] = 0.f;
								if (m + 2 < KMAX) F[m + 2] = 0.f;
								if (m + 3 < KMAX) F[m + 3] = 0.f;
							}
						}
						zz[c] = bucket_f32<KMAX>(isg_whf_value_f32(&s), F, qf, K, &amb);
					}
					if (amb) zz[c] = k4_draw_exact<KMAX>(&p, i, j, (g >> (8 * c)) & 0xff, PREF ? isg_whf_to(s) : si, K);
				}
				zout |= (unsigned)zz[c] << (8 * c);
			}
		}
#pragma unroll
		for (int m = 0; m < KMAX; m++)
			if (m < K)
				wcnt[m] += __popcll(__ballot(zz[0] == m)) + __popcll(__ballot(zz[1] == m)) + __popcll(__ballot(zz[2] == m)) +
					   __popcll(__ballot(zz[3] == m));
		if (WRITE && j < p.Lp) *(unsigned *)(p.z + id * 4) = zout;
	}
	if (lane_id() == 0) {
#pragma unroll
		for (int m = 0; m < KMAX; m++)
			if (m < K && wcnt[m]) atomicAdd(&sh.hist[par][m], wcnt[m]);
	}
	lds_barrier();
	const isg_wh dstart = isg_wh_jump32(&sh.tab, cur, 4u * (unsigned)nvalid);
	return 4u * (unsigned)nvalid + dirichlet_block<BLOCK, KMAX, WRITE>(d, sh, i, dstart, alpha, par);
}

/* Four waves per SIMD (config 5, K = 10, ms per sweep): with the exact redo inline the compiler took 235 registers = 2 waves and the loop waited
 * for its table rows, 8.25; forced to 3 / 4 waves it spilt the redo's arrays, 6.66 / 6.30 (6 waves: 33); with the redo out of line
 * (k4_draw_exact) 148 registers = 3 waves, 6.47, and four waves cost 13 spilt registers, 6.00. */
template <int BLOCK, int KMAX, bool CHAIN>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4))) k4_zq(PolyDev p, DevView d, isg_wh base, uint64_t pos0, uint64_t stride, int init_flag, double alpha, uint64_t *pos_out,
					       const unsigned long long *offs = nullptr, const ResolveState *rst = nullptr)
{
	__shared__ ZqShared sh;
	const int t = threadIdx.x;
	if (rst && (!rst->done || rst->fail)) return;
	{
		const uint16_t *src = (const uint16_t *)p.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += BLOCK) dst[k] = src[k];
		if (t < 2 * ISG_KCAP) (&sh.hist[0][0])[t] = 0;
	}
	__syncthreads();
	isg_wh cur = isg_wh_jump(&sh.tab, base, CHAIN ? 0 : offs ? offs[blockIdx.x] : pos0 + (uint64_t)blockIdx.x * stride);
	uint64_t total = 0;
	for (int i = CHAIN ? 0 : (int)blockIdx.x; i < (CHAIN ? p.N : (int)blockIdx.x + 1); i++) {
		const int par = i & 1;
		const unsigned used = k4_zq_one<BLOCK, KMAX, true>(p, d, sh, i, cur, init_flag, alpha, par);
		cur = isg_wh_jump32(&sh.tab, cur, used);
		total += used;
		if (!CHAIN && offs && t == 0 && (unsigned long long)used != offs[i + 1] - offs[i]) atomicOr(d.err, 8u);
	}
	if (CHAIN && t == 0) *pos_out = total;
}

/* the interval resolver's kernels for ploidy 4 (isg_spec_hip.inc): expected cluster counts of an individual's 4 nvalid draws, and a probe */
/* Workgroup b takes the b % 8-th eighth of individual b / 8's loci: workgroups are dealt round-robin over the 8 XCDs, so every XCD only ever
 * touches one eighth of the frequency table (3.8 MB at config 5: it does not stay in a 4 MB L2 next to the genotype rows; an eighth does).
 * part[(i * 8 + e) * 2 K ..]: that eighth's sums of P and P (1 - P); k4_zexpect_fin adds the eighths in order and forms the intervals. */
/* SCR: a wave's 64 loci are 64 contiguous blocks of frequency rows ([Amax][KPF] floats each): the wave fetches that stretch as ONE flat
 * array (lane l takes 16-byte word q 64 + l: full lines) into its strip of LDS, and every lane then reads the rows of its four copies'
 * alleles from there.  Gathered directly, a 48-byte row costs its lane a 128-byte L2 line -- 700 L2 requests per wave and 64 loci
 * (SQ / TCC counters at config 5: waves waiting 90 % of the time, 280 GB of L2 traffic per sweep). */
#define K4Z_SCR_FLOATS 64 /* floats of a locus block the strip holds (config 5: 4 alleles x 12) */
#define K4Z_SCR_STRIDE (K4Z_SCR_FLOATS / 4 + 1) /* 16-byte words per locus in the strip (odd: the lanes' reads spread over the banks) */
typedef float f32x2 __attribute__((ext_vector_type(2)));
/* MI individuals per workgroup: the strip is fetched once for all of them (one individual per workgroup reads its eighth of the table from
 * the L2 again for every individual: N L Amax KPF floats = 38 GB per sweep at config 5, the kernel ran at the L2's bandwidth) */
template <int KMAX, bool SCR, int MI>
__global__ void __launch_bounds__(256) k4_zexpect(PolyDev p, DevView d, float *part)
{
	__shared__ float red[MI][4][2 * KMAX];
	__shared__ float4 scr[SCR ? 256 * K4Z_SCR_STRIDE : 1];
	const int i0 = (int)(blockIdx.x >> 3) * MI, e8 = (int)(blockIdx.x & 7), t = threadIdx.x, K = p.K, lane = (int)lane_id();
	const int Lq = ((p.L + 7) / 8 + 63) & ~63, j0 = e8 * Lq, j1 = (j0 + Lq < p.L) ? j0 + Lq : p.L;
	const int blk = p.Amax * d.KPF; /* floats per locus (a multiple of 4) */
	/* clusters in pairs: v_pk_mul_f32 / v_pk_add_f32 do two per lane and cycle */
	f32x2 qf[MI][KMAX / 2], lam[MI][KMAX / 2], var[MI][KMAX / 2];
#pragma unroll
	for (int m = 0; m < MI; m++)
#pragma unroll
		for (int h = 0; h < KMAX / 2; h++) {
			const int i = (i0 + m < p.N) ? i0 + m : p.N - 1;
			qf[m][h].x = (2 * h < K) ? (float)p.qq[(size_t)i * K + 2 * h] : 0.f;
			qf[m][h].y = (2 * h + 1 < K) ? (float)p.qq[(size_t)i * K + 2 * h + 1] : 0.f;
			lam[m][h] = (f32x2)(0.f);
			var[m][h] = (f32x2)(0.f);
		}
	const int nq = blk / 4; /* 16-byte words per locus (<= 16) */
	const unsigned nqinv = 65536u / (unsigned)nq + 1u; /* e / nq = (e * nqinv) >> 16 for e < 1024 */
	float4 *strip = scr + (SCR ? (t & ~63) * K4Z_SCR_STRIDE : 0); /* this wave's */
	for (int jb = j0; jb < j1; jb += 256) { /* (wave-uniform trip count: every lane helps with the wave's loads) */
		const int j = jb + t, jw = jb + (t & ~63);
		unsigned gs[MI];
#pragma unroll
		for (int m = 0; m < MI; m++) gs[m] = (j < j1 && i0 + m < p.N) ? *(const unsigned *)(p.geno + ((size_t)(i0 + m) * p.Lp + j) * 4) : 0xffffffffu;
		if (SCR) {
			int nl = j1 - jw; /* loci of this wave in range */
			nl = nl > 64 ? 64 : (nl < 0 ? 0 : nl);
			const float4 *src = (const float4 *)(d.freqf + (size_t)jw * blk);
			__builtin_amdgcn_wave_barrier(); /* (the previous pass's reads of the strip are done: same wave, program order + LDS in order) */
#pragma unroll
			for (int q = 0; q < K4Z_SCR_FLOATS / 4; q++) {
				const int e = q * 64 + lane; /* flat word of the wave's stretch */
				if (q < nq && e < nl * nq) {
					const int loc = (int)(((unsigned)e * nqinv) >> 16), wi = e - loc * nq;
					strip[loc * K4Z_SCR_STRIDE + wi] = src[e];
				}
			}
			__builtin_amdgcn_wave_barrier();
		}
		const float *mine = (const float *)(strip + (SCR ? lane * K4Z_SCR_STRIDE : 0));
#pragma unroll
		for (int m = 0; m < MI; m++) {
			const unsigned g = gs[m];
			if ((g & 0xff) == 0xff) continue; /* (unused locus: the imputed genotype is 0xFF padded as the observation is; or beyond the range) */
#pragma unroll
			for (int cp = 0; cp < 4; cp++) {
				const float *F = SCR ? mine + ((g >> (8 * cp)) & 0xff) * d.KPF : d.freqf + ((size_t)j * p.Amax + ((g >> (8 * cp)) & 0xff)) * d.KPF;
				f32x2 w[KMAX / 2], tot2 = (f32x2)(0.f);
#pragma unroll
				for (int k = 0; k < KMAX; k += 4) {
					if (k < K) {
						const float4 f = *(const float4 *)(F + k);
						w[k / 2] = qf[m][k / 2] * (f32x2){f.x, f.y};
						if (k + 2 < KMAX) w[k / 2 + 1] = qf[m][k / 2 + 1] * (f32x2){f.z, f.w};
					} else {
						w[k / 2] = (f32x2)(0.f);
						if (k + 2 < KMAX) w[k / 2 + 1] = (f32x2)(0.f);
					}
				}
#pragma unroll
				for (int h = 0; h < KMAX / 2; h++) tot2 += w[h];
				const float tot = tot2.x + tot2.y;
				const float inv = (tot > 0.f) ? 1.0f / tot : 0.f;
				const f32x2 inv2 = (f32x2)(inv), one2 = (f32x2)(1.0f);
#pragma unroll
				for (int h = 0; h < KMAX / 2; h++) {
					const f32x2 pr = w[h] * inv2;
					lam[m][h] += pr;
					var[m][h] += pr * (one2 - pr);
				}
			}
		}
	}
#pragma unroll
	for (int m = 0; m < MI; m++)
#pragma unroll
		for (int k = 0; k < KMAX; k++) {
			float l = (k & 1) ? lam[m][k / 2].y : lam[m][k / 2].x, v = (k & 1) ? var[m][k / 2].y : var[m][k / 2].x;
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				l += __shfl_down(l, o, 64);
				v += __shfl_down(v, o, 64);
			}
			if (lane == 0) {
				red[m][t >> 6][k] = l;
				red[m][t >> 6][KMAX + k] = v;
			}
		}
	__syncthreads();
	for (int e = t; e < MI * K; e += 256) {
		const int m = e / K, k = e - m * K, i = i0 + m;
		if (i >= p.N) break;
		part[((size_t)i * 8 + e8) * 2 * K + k] = red[m][0][k] + red[m][1][k] + red[m][2][k] + red[m][3][k];
		part[((size_t)i * 8 + e8) * 2 * K + K + k] = red[m][0][KMAX + k] + red[m][1][KMAX + k] + red[m][2][KMAX + k] + red[m][3][KMAX + k];
	}
}
/* The same sums with ONE LANE PER INDIVIDUAL (blocks of Amax KPF <= K4Z_SCR_FLOATS floats): a workgroup = 256 individuals x a range of loci;
 * 64 loci's blocks at a time are staged in LDS and all lanes walk them together -- every lane reads the rows of ITS genotype's alleles, the
 * block itself is fetched once per 256 individuals, and the sums stay in the lane: no strip per wave (17 KB: two waves per SIMD), no
 * per-individual accumulators times MI, no reduction.  A lane reads its individual's genotypes 16 bytes (4 loci) at a time.
 * part[(i * nrange + r) * 2 K ..] = the range's sums; k4_zexpect_fin adds the ranges in order. */
#define K4Z_NRANGE 32
template <int KMAX>
__global__ void __launch_bounds__(256) k4_zexpect_ind(PolyDev p, DevView d, float *part, int nrange)
{
	__shared__ float4 buf[64 * (K4Z_SCR_FLOATS / 4)];
	const int ib = (int)blockIdx.x / nrange, r = (int)blockIdx.x - ib * nrange, t = threadIdx.x, K = p.K;
	const int i = ib * 256 + t, ic = (i < p.N) ? i : p.N - 1;
	const int Lr = ((p.L + nrange - 1) / nrange + 63) & ~63, j0 = r * Lr, j1 = (j0 + Lr < p.L) ? j0 + Lr : p.L;
	const int blk = p.Amax * d.KPF, nq = blk / 4;
	f32x2 qf[KMAX / 2], lam[KMAX / 2], var[KMAX / 2];
#pragma unroll
	for (int h = 0; h < KMAX / 2; h++) {
		qf[h].x = (2 * h < K) ? (float)p.qq[(size_t)ic * K + 2 * h] : 0.f;
		qf[h].y = (2 * h + 1 < K) ? (float)p.qq[(size_t)ic * K + 2 * h + 1] : 0.f;
		lam[h] = (f32x2)(0.f);
		var[h] = (f32x2)(0.f);
	}
	const uint8_t *grow = p.geno + (size_t)ic * p.Lp * 4;
	for (int jb = j0; jb < j1; jb += 64) {
		const int nl = (j1 - jb < 64) ? j1 - jb : 64;
		__syncthreads(); /* (everybody is done with the previous 64 loci) */
		{
			const float4 *src = (const float4 *)(d.freqf + (size_t)jb * blk);
			for (int e = t; e < nl * nq; e += 256) buf[e] = src[e];
		}
		__syncthreads();
		for (int l4 = 0; l4 < nl; l4 += 4) { /* (Lp is a multiple of 4 and jb of 64: the 16 bytes are the lane's own row; loci beyond L are 0xFF) */
			const uint4 g4 = *(const uint4 *)(grow + (size_t)(jb + l4) * 4);
#pragma unroll
			for (int l = 0; l < 4; l++) {
				const unsigned g = (l == 0) ? g4.x : (l == 1) ? g4.y : (l == 2) ? g4.z : g4.w;
				if ((g & 0xff) == 0xff || l4 + l >= nl) continue; /* unused locus */
				const float *row = (const float *)(buf + (size_t)(l4 + l) * nq);
#pragma unroll
				for (int cp = 0; cp < 4; cp++) {
					const float *F = row + ((g >> (8 * cp)) & 0xff) * d.KPF;
					f32x2 w[KMAX / 2], tot2 = (f32x2)(0.f);
#pragma unroll
					for (int k = 0; k < KMAX; k += 4) {
						if (k < K) {
							const float4 f = *(const float4 *)(F + k);
							w[k / 2] = qf[k / 2] * (f32x2){f.x, f.y};
							if (k + 2 < KMAX) w[k / 2 + 1] = qf[k / 2 + 1] * (f32x2){f.z, f.w};
						} else {
							w[k / 2] = (f32x2)(0.f);
							if (k + 2 < KMAX) w[k / 2 + 1] = (f32x2)(0.f);
						}
					}
#pragma unroll
					for (int h = 0; h < KMAX / 2; h++) tot2 += w[h];
					const float tot = tot2.x + tot2.y;
					const float inv = (tot > 0.f) ? 1.0f / tot : 0.f;
					const f32x2 inv2 = (f32x2)(inv), one2 = (f32x2)(1.0f);
#pragma unroll
					for (int h = 0; h < KMAX / 2; h++) {
						const f32x2 pr = w[h] * inv2;
						lam[h] += pr;
						var[h] += pr * (one2 - pr);
					}
				}
			}
		}
	}
	if (i < p.N) {
		float *out = part + ((size_t)i * nrange + r) * 2 * K;
#pragma unroll
		for (int k = 0; k < KMAX; k++)
			if (k < K) {
				out[k] = (k & 1) ? lam[k / 2].y : lam[k / 2].x;
				out[K + k] = (k & 1) ? var[k / 2].y : var[k / 2].x;
			}
	}
}
/* one thread per (individual, cluster): the eighths' sums in order -> [lambda - k sigma, lambda + k sigma] + alpha */
__global__ void __launch_bounds__(256) k4_zexpect_fin(PolyDev p, const float *part, double alpha, float ksig, float *alo, float *ahi, int nrange)
{
	const int id = blockIdx.x * 256 + threadIdx.x, K = p.K;
	if (id >= p.N * K) return;
	const int i = id / K, m = id - i * K;
	float l = 0.f, v = 0.f;
	for (int e = 0; e < nrange; e++) {
		l += part[((size_t)i * nrange + e) * 2 * K + m];
		v += part[((size_t)i * nrange + e) * 2 * K + K + m];
	}
	v = v > 0.f ? v : 0.f;
	const float h = ksig * __builtin_sqrtf(v) + 1.0f + 1e-5f * l;
	float lo = __builtin_floorf(l - h), hi = __builtin_ceilf(l + h);
	const float tot = 4.0f * (float)p.nvalid[i];
	if (lo < 0.f) lo = 0.f;
	if (hi > tot) hi = tot;
	if (p.nvalid[i] == 0) lo = hi = 0.f;
	alo[id] = (float)((double)lo + alpha);
	ahi[id] = (float)((double)hi + alpha);
}
template <int BLOCK, int KMAX>
__global__ void __launch_bounds__(BLOCK) k4_zq_probe(PolyDev p, DevView d, isg_wh base, double alpha, const unsigned long long *Bpre, const SpecProbe *list, SpecDev *dev, int cap, unsigned char *table)
{
	__shared__ ZqShared sh;
	const int t = threadIdx.x;
	{
		const uint16_t *src = (const uint16_t *)p.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += BLOCK) dst[k] = src[k];
	}
	__syncthreads();
	const unsigned n = dev->nlist < (unsigned)cap ? dev->nlist : (unsigned)cap;
	if (blockIdx.x == 0 && t == 0 && n) { dev->nprobes += n; dev->rounds += 1u; }
	for (unsigned q = blockIdx.x; q < n; q += gridDim.x) {
		if (t < 2 * ISG_KCAP) (&sh.hist[0][0])[t] = 0;
		__syncthreads();
		const int i = list[q].i;
		const isg_wh cur = isg_wh_jump(&sh.tab, base, Bpre[i] + 2ull * list[q].x);
		const unsigned used = k4_zq_one<BLOCK, KMAX, false>(p, d, sh, i, cur, 0, alpha, 0);
		if (t == 0) {
			const unsigned minimal = 4u * (unsigned)p.nvalid[i] + 2u * (unsigned)p.K;
			unsigned char v = (unsigned char)WK_IRR;
			if (used >= minimal && !((used - minimal) & 1u) && (used - minimal) / 2u <= 126u) v = (unsigned char)((used - minimal) / 2u);
			table[list[q].taddr] = v;
		}
		__syncthreads();
	}
}

/*
 * k4_zq_block: the ploidy-4 form of k_zq_block (isg_resolve_hip.inc): for one individual and ISG_RS_CH candidate start
 * positions, the consumption of its Dirichlet.  A used locus takes four uniforms (one per allele copy, poly_geno.c:763-777), a
 * candidate step is two (one rejected gamma attempt): candidate c, locus rank r, copy k reads position off0 + 2 c + 4 r + k.
 * Single precision thresholds per copy (K - 1 of them), sign-bit counting, the few undecidable draws exactly; then the K
 * gammas of each candidate with the workgroup-wide attempt table (dirichlet_coop: K may exceed 8 here).
 */
template <int KMAX>
__global__ void __launch_bounds__(256) k4_zq_block(PolyDev p, DevView d, isg_wh base, double alpha, const ResolvePlan *plan, ResolveState *st, const unsigned long long *Bpre,
						   const float *tapef, unsigned long long tape_len, unsigned long long *offs, int b)
{
	constexpr int CH = ISG_RS_CH, T = (KMAX > 1) ? KMAX - 1 : 1, Q4 = (KMAX + 3) / 4, NX = 2 + CH; /* float2 per lane: 4 + 2 (CH - 1) uniforms */
	__shared__ ZqShared sh;
	__shared__ unsigned e_s[ISG_RS_DMAX];
	__shared__ unsigned long long blk_s[5];
	__shared__ __attribute__((aligned(16))) unsigned char cs[ISG_RS_DMAX * ISG_RS_WMAX];
	__shared__ int red[CH][KMAX];
	const int t = threadIdx.x, u = rs_unit_of_block((int)blockIdx.x, (int)gridDim.x), K = p.K, lane = (int)lane_id();
	{
		const uint16_t *src = (const uint16_t *)p.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += 256) dst[k] = src[k];
		if (t < CH * KMAX) (&red[0][0])[t] = 0;
		if (t < 2 * ISG_KCAP) {
			(&sh.hist[0][0])[t] = 0;
			(&sh.amask[0][0])[t] = 0;
			(&sh.rmask[0][0])[t] = 0;
			(&sh.ghist[0][0])[t] = 0;
		}
	}
	int i = 0;
	unsigned long long E = 0;
	if (rs_block_start<false>(u, p.N, plan, st, Bpre, offs, b, e_s, blk_s, cs, &i, &E, nullptr, nullptr) != RS_CONTINUE) return;
	const int nv = p.nvalid[i];
	const unsigned long long off0 = Bpre[i] + 2ull * (E + (unsigned long long)plan->uo[u]);
	const bool covered = off0 + 2ull * (CH - 1) + 4ull * (unsigned)nv + 8ull <= tape_len;
	float qf[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) qf[m] = (m < K) ? (float)p.qq[(size_t)i * K + m] : 0.f;
	const isg_wh cur = isg_wh_jump(&sh.tab, base, off0);
	const size_t rowb = (size_t)p.Lp * 4;
	unsigned cnt[CH][T]; /* draws of candidate c below threshold m = draws with Z <= m */
#pragma unroll
	for (int c = 0; c < CH; c++)
#pragma unroll
		for (int m = 0; m < T; m++) cnt[c][m] = 0;
	if (covered) {
		struct Geno { unsigned g, rw; };
		struct Data { unsigned g, rank; float2 xs[NX]; float4 R[4][Q4]; };
		const int NB = (p.Lp + 255) / 256;
		auto load_geno = [&](int bb, Geno &G) {
			const int j = bb * 256 + t, jc = (j < p.Lp) ? j : p.Lp - 1;
			const unsigned g = *(const unsigned *)(p.geno + (size_t)i * rowb + (size_t)jc * 4);
			G.g = (j < p.Lp) ? g : 0xffffffffu;
			G.rw = p.rankwave[(size_t)i * p.nwv + (jc >> 6)];
		};
		auto load_data = [&](int bb, const Geno &G, Data &X) {
			const int j = bb * 256 + t, jc = (j < p.Lp) ? j : p.Lp - 1;
			const bool valid = (G.g & 0xff) != 0xff;
			X.g = G.g;
			X.rank = G.rw + (unsigned)__popcll(__ballot(valid) & ((1ull << lane) - 1ull));
			const float2 *tp = (const float2 *)(tapef + off0 + 4ull * X.rank);
#pragma unroll
			for (int k = 0; k < NX; k++) X.xs[k] = tp[k];
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const float *P = d.freqf + ((size_t)jc * p.Amax + (valid ? (G.g >> (8 * k)) & 0xff : 0u)) * d.KPF;
#pragma unroll
				for (int q4 = 0; q4 < Q4; q4++) X.R[k][q4] = (4 * q4 < d.KPF) ? *(const float4 *)(P + 4 * q4) : make_float4(0.f, 0.f, 0.f, 0.f);
			}
		};
		auto compute = [&](int bb, const Data &X) {
			const int j = bb * 256 + t;
			const bool valid = (X.g & 0xff) != 0xff;
			float th[4][T];
			bool okrun = true;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				float F[KMAX], cum[KMAX];
#pragma unroll
				for (int m = 0; m < KMAX; m++) {
					const float4 v = X.R[k][m >> 2];
					F[m] = ((m & 3) == 0) ? v.x : ((m & 3) == 1) ? v.y : ((m & 3) == 2) ? v.z : v.w;
				}
				const float run = prefix_f32<KMAX>(F, qf, K, cum);
				okrun = okrun && (run > 1e-30f && run < 1e30f);
				const float inv = __builtin_amdgcn_rcpf(run);
#pragma unroll
				for (int m = 0; m < T; m++) th[k][m] = (valid && m < K - 1) ? cum[m] * inv : -1.0f;
			}
			unsigned neg[CH][T], ambc = 0;
#pragma unroll
			for (int c = 0; c < CH; c++) {
				const float x4[4] = {X.xs[c].x, X.xs[c].y, X.xs[c + 1].x, X.xs[c + 1].y}; /* positions 2 c .. 2 c + 3 */
				float mn = 3.0e38f;
#pragma unroll
				for (int m = 0; m < T; m++) {
					unsigned n4 = 0;
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const float df = x4[k] - th[k][m];
						n4 += __float_as_uint(df) >> 31;
						if (m < K - 1) mn = __builtin_fminf(mn, __builtin_fabsf(df));
					}
					neg[c][m] = n4;
				}
				ambc |= (mn > 6e-6f) ? 0u : (1u << c);
			}
			if (!okrun) ambc = (1u << CH) - 1u;
			if (valid && ambc) { /* that candidate's four draws at this locus exactly (disc_unif, random.c:403-430) */
				double q[KMAX];
#pragma unroll
				for (int m = 0; m < KMAX; m++) q[m] = (m < K) ? p.qq[(size_t)i * K + m] : 0.0;
#pragma unroll
				for (int c = 0; c < CH; c++) {
					if ((ambc >> c) & 1u) {
						isg_wh s = isg_wh_jump32(&sh.tab, cur, 2u * (unsigned)c + 4u * X.rank);
#pragma unroll
						for (int m = 0; m < T; m++) neg[c][m] = 0;
						for (int k = 0; k < 4; k++) {
							double cumd[KMAX];
							const double tot = weights<KMAX>(p.freq + ((size_t)j * p.Amax + ((X.g >> (8 * k)) & 0xff)) * p.KP, q, cumd, K);
							const int z = bucket_fast<KMAX>(isg_wh_next(&s), cumd, tot, K);
#pragma unroll
							for (int m = 0; m < T; m++) neg[c][m] += (z > m) ? 0u : 1u;
						}
					}
				}
			}
#pragma unroll
			for (int c = 0; c < CH; c++)
#pragma unroll
				for (int m = 0; m < T; m++) cnt[c][m] += neg[c][m];
		};
		Geno g0, g1;
		Data x0, x1;
		load_geno(0, g0);
		load_geno(1, g1);
		load_data(0, g0, x0);
		for (int bb = 0; bb < NB; bb += 2) { /* wave-uniform trip count; two passes of 256 loci in flight */
			load_data(bb + 1, g1, x1);
			load_geno(bb + 2, g0);
			compute(bb, x0);
			if (bb + 1 >= NB) break;
			load_data(bb + 2, g0, x0);
			load_geno(bb + 3, g1);
			compute(bb + 1, x1);
		}
#pragma unroll
		for (int c = 0; c < CH; c++)
#pragma unroll
			for (int m = 0; m < T; m++) {
				if (m < K - 1) {
					const unsigned sct = wave_sum_u32(cnt[c][m]);
					if (lane == 0 && sct) atomicAdd(&red[c][m], (int)sct);
				}
			}
	}
	__syncthreads();
	/* ---- the Dirichlets of the CH candidates, one after the other on the whole workgroup ---- */
	unsigned cres = 0;
	for (int c = 0; c < CH; c++) {
		const int par = c & 1;
		if (t < K) { /* counts per cluster from the cumulative ones: C[m] = draws with Z <= m */
			const int upto = (t < K - 1) ? red[c][t] : 4 * nv, before = (t == 0) ? 0 : red[c][t - 1];
			sh.hist[par][t] = upto - before;
		}
		lds_barrier();
		unsigned cv = ISG_RS_IRR;
		if (covered) {
			const unsigned used = dirichlet_coop<256, KMAX>(d, sh, i, cur, 2ull * (unsigned)c + 4ull * (unsigned)nv, alpha, par, nullptr, false);
			if (!(used & 1u) && used >= 2u * (unsigned)K && (used - 2u * (unsigned)K) / 2u <= 250u) cv = (used - 2u * (unsigned)K) / 2u;
		}
		cres |= cv << (8 * c);
		lds_barrier();
	}
	if (t == 0) ((unsigned *)st->ctab[b & 1])[u] = cres;
}

/* update_P_auto's Dirichlets in the keyed schedule: one lane per (cluster, locus) (rdirich, random.c:264-280); allotetraploid: the first
 * subgenome's Dirichlet and then the second's from the same position on (update_P_allo, poly_geno.c:499-506) */
__global__ void k4_pdirich(PolyDev p, isg_wh base, uint64_t pos0, uint64_t SP)
{
	const int id = blockIdx.x * blockDim.x + threadIdx.x; /* id = k * L + j (reference order) */
	if (id >= p.K * p.L) return;
	const int k = id / p.L, j = id - k * p.L;
	const int A = p.pc[p.lclass[j]].n;
	isg_cursor c;
	c.s = isg_wh_jump(p.tab, base, pos0 + (uint64_t)id * SP);
	c.used = 0;
	c.tape = nullptr;
	for (int sub = 0; sub < (p.allo ? 2 : 1); sub++) {
		const int *cnt = sub ? p.cnt2 : p.cnt;
		double *freq = sub ? p.freq2 : p.freq;
		double sum = 0;
		for (int a = 0; a < A; a++) {
			const double g = isg_rgamma(&c, (double)cnt[((size_t)j * p.Amax + a) * p.K + k] + 1.0);
			freq[((size_t)j * p.Amax + a) * p.KP + k] = g;
			sum += g;
		}
		for (int a = 0; a < A; a++) freq[((size_t)j * p.Amax + a) * p.KP + k] /= sum;
	}
}

/* ------------------------------------------------------------------------------------------ */
/* host side                                                                                   */
/* ------------------------------------------------------------------------------------------ */
static int poly_ctx_create(const isg_config *cfg, const int32_t *allelenum, const int32_t *seq, isg_ctx **out)
{
	if (cfg->K < 1 || cfg->K > ISG_KCAP) return fail("isg_ctx_create_poly: K must be in 1..32 for ploidy 4");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("isg_ctx_create: no HIP device available (the MI355X path has no CPU fallback)");
	if (cfg->device < 0 || cfg->device >= ndev) return fail("isg_ctx_create: bad device ordinal");
	HIPCHK(hipSetDevice(cfg->device));
	const int N = cfg->N, L = cfg->L, K = cfg->K;
	int Amax = 1;
	for (int j = 0; j < L; j++) Amax = allelenum[j] > Amax ? allelenum[j] : Amax;
	if (Amax > ISG_POLY_ACAP_W) return fail("isg_ctx_create: ploidy 4 supports up to 32 alleles per locus in this build");
	const bool wide = Amax > ISG_POLY_ACAP;
	const int allo = cfg->reserved[0] ? 1 : 0; /* isg_config.allo: allotetraploid, -ap 0 */
	for (int j = 0; j < L; j++) /* 0 = nobody typed at this locus: kept, never used (transform_data2 does not drop loci) */
		if (allelenum[j] < 0) return fail("isg_ctx_create: negative allele count");
	{ /* the five tables padded to GS = G(Amax) rows (exfreq, genofreq, genofreqT, tabtmp, ccnt): at most half of what the device has free */
		const int GS = allo ? isg_allo_G(Amax) : isg_poly_G(Amax);
		const size_t tb = sizeof(float) * (size_t)K * (size_t)GS * (4 * (size_t)L + (size_t)((L + 3) & ~3));
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = (size_t)1 << 31;
		if (tb > fr / 2) {
			char msg[256];
			snprintf(msg, sizeof msg, "isg_ctx_create_poly: the genotype tables need %zu bytes (%d genotypes per locus, K %d, L %d): more than half of the free device memory", tb, GS, K, L);
			return fail(msg);
		}
	}
	isg_ctx *c = new isg_ctx();
	PolyCtx *pc = new PolyCtx();
	memset(&pc->p, 0, sizeof(pc->p));
	c->poly = pc;
	pc->wide = wide;
	c->cfg = *cfg;
	ctx_count(c, +1);
	CtxGuard guard(c); /* any early return below releases what has been allocated so far */
	c->Amax = Amax;
	c->allelenum.assign(allelenum, allelenum + L);
	const int Lp = (L + 3) & ~3, KP = (K + 1) & ~1, nwv = (Lp + 63) / 64 + 1;
	/* distinct allele counts and their genotype lists (gen_allele_poly, auto_geno_num/list) */
	for (int j = 0; j < L; j++) {
		bool f = false;
		for (int v : pc->classes) f |= (v == allelenum[j]);
		if (!f) pc->classes.push_back(allelenum[j]);
	}
	std::sort(pc->classes.begin(), pc->classes.end());
	const int ncls = (int)pc->classes.size();
	std::vector<isg_polyclass> cls(ncls);
	std::vector<int> gidoff(ncls), allists;
	std::vector<short> gidmap;
	int GS = 1;
	pc->lists.resize(ncls);
	for (int q = 0; q < ncls; q++) {
		const int n = pc->classes[q];
		pc->lists[q].assign((allo ? isg_allo_G(n) : isg_poly_G(n)) + 1, 0);
		if (allo) isg_allo_build(n, cls[q].g, pc->lists[q].data());
		else isg_poly_build(n, cls[q].g, pc->lists[q].data());
		cls[q].n = n;
		cls[q].G = cls[q].g[0];
		GS = cls[q].G > GS ? cls[q].G : GS;
		if (wide) continue; /* rows in closed form (isg_poly_rank, isg_allo_row): no map */
		gidoff[q] = (int)gidmap.size();
		gidmap.resize(gidmap.size() + (size_t)n * n * n * n, (short)-1);
		for (int g = 0; g < cls[q].G; g++) gidmap[gidoff[q] + pc->lists[q][g]] = (short)g;
	}
	if (wide) gidmap.assign(1, (short)-1);
	pc->lclass_h.resize(L);
	for (int j = 0; j < L; j++)
		for (int q = 0; q < ncls; q++)
			if (pc->classes[q] == allelenum[j]) pc->lclass_h[j] = q;
	/* pack the observation, per-individual counts, stream ranks */
	std::vector<uint8_t> pk((size_t)N * Lp * 4, 0xff);
	std::vector<int> nvalid(N, 0);
	std::vector<unsigned> rw((size_t)N * nwv, 0);
	std::vector<unsigned long long> aw((size_t)N * nwv, 0);
	unsigned long long amb_run = 0;
	for (int i = 0; i < N; i++) {
		unsigned run = 0;
		for (int w = 0; w < nwv; w++) {
			rw[(size_t)i * nwv + w] = run;
			aw[(size_t)i * nwv + w] = amb_run;
			for (int j = 64 * w; j < 64 * (w + 1) && j < L; j++) {
				int na = 0;
				for (int k = 0; k < 4; k++) {
					const int v = seq[((size_t)i * L + j) * 4 + k];
					if (v >= 0) {
						if (v >= allelenum[j] || na != k) return fail("isg_ctx_create: ploidy 4 expects sorted distinct allele codes followed by negative padding");
						pk[((size_t)i * Lp + j) * 4 + na++] = (uint8_t)v;
					}
				}
				if (na) { nvalid[i]++; run++; }
				if (na == 2 || na == 3 || (allo && na == 4)) amb_run++; /* loci whose genotype is drawn: one uniform each */
			}
		}
	}
	pc->total_amb = amb_run;
	PolyDev &p = pc->p;
	memset(&p, 0, sizeof(p));
	p.log4 = isg_log(4.0);
	p.log6 = isg_log(6.0);
	if (isg_exp(0.0) != 1.0) return fail("isg_ctx_create: isg_exp(0) != 1");
	p.N = N; p.L = L; p.Lp = Lp; p.K = K; p.KP = KP; p.Amax = Amax; p.GS = GS; p.nwv = nwv; p.allo = allo;
	DevView &d = c->d;
	memset(&d, 0, sizeof(d));
	d.N = N; d.L = L; d.Lp = Lp; d.K = K; d.KP = KP; d.Amax = Amax; d.mode = 2; d.type_freq = 1;
	HIPCHK(hipStreamCreate(&c->stream));
	const size_t nfreq = (size_t)Lp * Amax * KP, ncnt = (size_t)Lp * Amax * K, ntab = (size_t)K * L * GS;
	HIPCHK(pc->obs.upload(pk));
	HIPCHK(pc->geno.alloc_zero((size_t)N * Lp * 4));
	HIPCHK(pc->z.alloc_zero((size_t)N * Lp * 4));
	HIPCHK(hipMemset(pc->geno, 0xff, (size_t)N * Lp * 4));
	HIPCHK(hipMemset(pc->z, 0xff, (size_t)N * Lp * 4));
	HIPCHK(pc->nvalid.upload(nvalid));
	HIPCHK(pc->rankwave.upload(rw));
	HIPCHK(pc->ambwave.upload(aw));
	HIPCHK(pc->lclass.upload(pc->lclass_h));
	HIPCHK(pc->gidmap.upload(gidmap));
	HIPCHK(pc->gidoff.upload(gidoff));
	pc->dlists.resize(ncls);
	for (int q = 0; q < ncls; q++) {
		HIPCHK(pc->dlists[q].upload(pc->lists[q]));
		cls[q].list = pc->dlists[q];
	}
	HIPCHK(pc->pc.upload(cls));
	HIPCHK(pc->freq.alloc_zero(allo ? 2 * nfreq : nfreq)); /* allotetraploid: freq2 and cnt2 follow freq and cnt, so that a count index beyond ncnt */
	HIPCHK(pc->lfreq.alloc_zero(nfreq));                  /* names the second subgenome's count and frequency (isg_pgroups.h) */
	HIPCHK(pc->cnt.alloc_zero(allo ? 2 * ncnt : ncnt));
	if (allo) {
		HIPCHK(pc->lfreq2.alloc_zero(nfreq));
		HIPCHK(pc->cntmix2.alloc_zero(ncnt));
		pc->freq2_h.assign((size_t)K * L * Amax, 0.0);
		pc->cnt2_h.assign((size_t)L * Amax * K, 0);
	}
	HIPCHK(pc->qq.alloc_zero((size_t)N * K));
	HIPCHK(c->d_qqsave.alloc_zero((size_t)N * K));
	HIPCHK(pc->qqnum.alloc_zero((size_t)N * K));
	HIPCHK(pc->indvlkh.alloc_zero(N));
	HIPCHK(pc->exfreq.alloc_zero(ntab));
	HIPCHK(pc->genofreq.alloc_zero(ntab));
	HIPCHK(pc->genofreqT.alloc_zero((size_t)K * GS * Lp));
	HIPCHK(pc->tabtmp.alloc_zero(ntab));
	HIPCHK(pc->d_self.alloc_zero(2 * ISG_KCAP));
	HIPCHK(pc->ccnt.alloc_zero(ntab));
	HIPCHK(pc->accbuf.alloc_zero(5 * (2 * ISG_KCAP + 2)));
	HIPCHK(pc->d_cntmix.alloc_zero(ncnt));
	HIPCHK(pc->d_catcnt.alloc_zero(8));
	p.obs = pc->obs; p.geno = pc->geno; p.z = pc->z; p.nvalid = pc->nvalid; p.rankwave = pc->rankwave; p.ambwave = pc->ambwave; p.lclass = pc->lclass;
	p.gidmap = pc->gidmap; p.gidoff = pc->gidoff; p.pc = pc->pc; p.freq = pc->freq; p.lfreq = pc->lfreq; p.cnt = pc->cnt;
	p.freq2 = allo ? pc->freq + nfreq : nullptr; p.lfreq2 = pc->lfreq2; p.cnt2 = allo ? pc->cnt + ncnt : nullptr; p.cntmix2 = pc->cntmix2;
	p.qq = pc->qq; p.qqnum = pc->qqnum; p.indvlkh = pc->indvlkh; p.exfreq = pc->exfreq; p.genofreq = pc->genofreq; p.genofreqT = pc->genofreqT;
	p.tabtmp = pc->tabtmp; p.ccnt = pc->ccnt; p.accbuf = pc->accbuf;
	pc->counts_valid = false;
	pc->freq_host = true;
	d.KPF = (K + 3) & ~3;
	/* the genotype draw's single precision pre-decision (geno_one_allo) reads freq2 in float too: its copy follows freq's */
	p.allo_pref = (allo && env_flag(getenv("INSTRUCT_ALLO_PREFILTER"), true)) ? 1 : 0;
	HIPCHK(c->d_freqf.alloc_zero((size_t)Lp * Amax * d.KPF * (p.allo_pref ? 2 : 1)));
	p.freqf = d.freqf = c->d_freqf;
	p.KPF = d.KPF;
	{
		HIPCHK(c->d_coop.alloc_zero(1));
		c->coop = env_flag(getenv("INSTRUCT_ZQ_COOP"), true);
		c->test_abort = (int)env_int(getenv("INSTRUCT_ZQ_TEST_ABORT"), 0);
	}
	{ /* replay update_ZQ with the start positions resolved block-wise (k4_zq_block): opt-in for ploidy 4.  A candidate costs
	   * 4 L draws against K - 1 thresholds and the windows widen with K: at config 5 (K = 10, L = 20000) the resolution takes
	   * 158 ms + 8.6 ms for the sweep, the cooperative chain kernel 105 ms (INSTRUCT_ZQ_RESOLVE_P4=1 to use it anyway) */
		if (env_flag(getenv("INSTRUCT_ZQ_RESOLVE_P4"), false) && resolve_alloc(c, nvalid, 4, 16)) return 1;
		if (c->rs) c->rs->err_bit = 8u;
	}
	if (cfg->rng_sched == ISG_SCHED_REPLAY) {
		/* neither update_P_auto (poly_geno.c:426-434) nor update_P_allo (:491-502) has an allelenum > 1 test; the latter draws two Dirichlets per (k, j) */
		if (allo ? pdev_create_allo(c, &c->pdev, L, K, Amax, allelenum, (long long)ncnt) : pdev_create(c, &c->pdev, L, K, Amax, allelenum, 0)) return 1;
		if (spec_create(c, &c->zspec, nvalid, 4)) return 1;
		if (c->zspec) {
			c->zspec->err_bit = 8u;
			HIPCHK(pc->d_zpart.alloc((size_t)N * K4Z_NRANGE * 2 * K));
		}
	}
	if (ctx_init_common(c, nvalid, Lp, KP, K)) return 1;
	HIPCHK(c->d_total.alloc_zero(1));
	HIPCHK(c->d_S.alloc_zero(ISG_KCAP));
	HIPCHK(c->d_state.alloc_zero(ISG_KCAP));
	p.tab = d.tab; p.err = d.err;
	d.freq = p.freq; d.cnt = p.cnt; d.qq = p.qq; d.qqnum = p.qqnum; d.indvlkh = p.indvlkh; d.nvalid = p.nvalid;
	if (!wide) pc->tab_h.assign((size_t)K * L * GS, 0.f);
	{ /* keyed layout, ploidy 4 (include/instruct_hip.h): the genotype sweeps take one uniform per ambiguous locus */
		const uint64_t N64 = N, L64 = L, K64 = K, amb = pc->total_amb;
		const uint64_t SP = (allo ? 2 : 1) * (16 * (uint64_t)Amax + 16), SZ = 4 * L64 + 16 * K64 + 16, ZI0 = 1 + amb, B0 = ZI0 + N64 * SZ;
		const uint64_t offS = K64 * L64 * SP, offZ = offS + 4 * K64, offGE = offZ + N64 * SZ, BLK = offGE + amb + 4;
		const uint64_t v[9] = {SP, SZ, ZI0, B0, offS, offGE, offZ, offGE, BLK};
		memcpy(c->ky, v, sizeof(v));
	}
	guard.release();
	*out = c;
	return 0;
}

static int poly_check_err(isg_ctx *c)
{
	unsigned e = 0;
	HIPCHK(hipMemcpyAsync(&e, c->d_err, sizeof(e), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (e & 4u) return fail("Genotype frequencies can not be greater than 1!");
	if (e) return fail("device error flag set");
	return 0;
}

static int poly_geno_sweep(isg_ctx *c, int init)
{
	PolyDev &p = c->poly->p;
	/* the sweep's uniforms in stream order, generated 8 per lane (one skip-ahead per 8 instead of one per draw) */
	const uint64_t need = c->poly->total_amb;
	const isg_wh gbase = is_keyed(c) ? isg_wh_jump(&c->tab_h, c->origin, init ? 1 : iter_base(c) + c->ky[KY_OFFG]) : c->rng;
	if (tape_fill(c, gbase, need)) return 1; /* (nothing to fill: no launch) */
	prof_begin(c);
	const int gchunk = p.N >= 2048 ? 256 : (p.N + 7) / 8, nchunk = (p.N + gchunk - 1) / gchunk, ntile = (p.Lp + 255) / 256;
	const dim3 ggrid((unsigned)(((ntile + 7) / 8) * 8 * nchunk));
	const bool wide = c->poly->wide;
	kdispatch(KL_P4_GENO(), p.K, [&](auto km) {
		constexpr int KM = decltype(km)::value;
		if (p.allo) hipLaunchKernelGGL((k4_geno<KM, true>), ggrid, dim3(256), 0, c->stream, p, gbase, init, (const double *)c->d_tape, gchunk, nchunk);
		else if (wide) hipLaunchKernelGGL((k4_geno<KM, false, true>), ggrid, dim3(256), 0, c->stream, p, gbase, init, (const double *)c->d_tape, gchunk, nchunk);
		else hipLaunchKernelGGL((k4_geno<KM, false>), ggrid, dim3(256), 0, c->stream, p, gbase, init, (const double *)c->d_tape, gchunk, nchunk);
	});
	prof_end(c, init ? "k4_geno_init" : "k4_geno");
	HIPCHK(hipGetLastError());
	/* one uniform per locus with 2 or 3 distinct alleles: the consumption is a property of the data */
	if (!is_keyed(c)) host_advance(c, c->poly->total_amb);
	c->poly->counts_valid = false;
	return 0;
}

static int poly_sweep_counts(isg_ctx *c)
{
	PolyCtx *pc = c->poly;
	PolyDev &p = pc->p;
	const int L = p.L, K = p.K, A = p.Amax;
	if (pc->counts_valid) return 0;
	HIPCHK(hipMemsetAsync(p.cnt, 0, sizeof(int) * (size_t)L * A * K, c->stream));
	HIPCHK(hipMemsetAsync(pc->d_cntmix, 0, sizeof(int) * (size_t)L * A * K, c->stream));
	HIPCHK(hipMemsetAsync(p.ccnt, 0, sizeof(int) * (size_t)K * L * p.GS, c->stream));
	HIPCHK(hipMemsetAsync(pc->d_catcnt, 0, sizeof(unsigned long long) * 8, c->stream));
	if (p.allo) {
		HIPCHK(hipMemsetAsync(p.cnt2, 0, sizeof(int) * (size_t)L * A * K, c->stream));
		HIPCHK(hipMemsetAsync(p.cntmix2, 0, sizeof(int) * (size_t)L * A * K, c->stream));
	}
	const size_t lds = p.allo ? (size_t)1 << 30 : sizeof(int) * 2 * (size_t)A * K * 64; /* two subgenomes: the global-atomics form */
	const int chunk = p.N > 4096 ? 1024 : (p.N + 3) / 4;
	const dim3 grid((L + 63) / 64, (p.N + chunk - 1) / chunk);
	prof_begin(c);
	if (pc->wide) {
		if (p.allo) hipLaunchKernelGGL((k4_sweep_counts<false, true, true>), grid, dim3(256), 0, c->stream, p, chunk, pc->d_cntmix, pc->d_catcnt);
		else if (lds <= 60000) hipLaunchKernelGGL((k4_sweep_counts<true, false, true>), grid, dim3(256), lds, c->stream, p, chunk, pc->d_cntmix, pc->d_catcnt);
		else hipLaunchKernelGGL((k4_sweep_counts<false, false, true>), grid, dim3(256), 0, c->stream, p, chunk, pc->d_cntmix, pc->d_catcnt);
	} else if (p.allo) hipLaunchKernelGGL((k4_sweep_counts<false, true, false>), grid, dim3(256), 0, c->stream, p, chunk, pc->d_cntmix, pc->d_catcnt);
	else if (lds <= 60000) hipLaunchKernelGGL((k4_sweep_counts<true, false, false>), grid, dim3(256), lds, c->stream, p, chunk, pc->d_cntmix, pc->d_catcnt);
	else hipLaunchKernelGGL((k4_sweep_counts<false, false, false>), grid, dim3(256), 0, c->stream, p, chunk, pc->d_cntmix, pc->d_catcnt);
	prof_end(c, "k4_sweep_counts");
	HIPCHK(hipGetLastError());
	pc->counts_valid = true;
	return 0;
}

/* calc_exfreq_auto / _allo for every (cluster, locus) table */
static void poly_launch_exfreq(isg_ctx *c)
{
	const PolyDev &p = c->poly->p;
	const int K = p.K, L = p.L;
	if (c->poly->wide) {
		if (p.allo) hipLaunchKernelGGL(k4_exfreq_w<true>, dim3((unsigned)(K * L)), dim3(256), 0, c->stream, p);
		else hipLaunchKernelGGL(k4_exfreq_w<false>, dim3((unsigned)(K * L)), dim3(256), 0, c->stream, p);
		return;
	}
	if (p.allo) hipLaunchKernelGGL(k4_exfreq<true>, dim3((K * L + 127) / 128), dim3(128), 0, c->stream, p);
	else hipLaunchKernelGGL(k4_exfreq<false>, dim3((K * L + 127) / 128), dim3(128), 0, c->stream, p);
}
/* auto_genfreq / allo_genfreq for every table at the rates self[k]: into genofreq (own) or tabtmp */
static void poly_launch_genfreq(isg_ctx *c, const float *self, int own)
{
	const PolyDev &p = c->poly->p;
	const int K = p.K, L = p.L;
	if (c->poly->wide) {
		if (p.allo) hipLaunchKernelGGL(k4_genfreq_w<true>, dim3((unsigned)(K * L)), dim3(256), 0, c->stream, p, self, own);
		else hipLaunchKernelGGL(k4_genfreq_w<false>, dim3((unsigned)(K * L)), dim3(256), 0, c->stream, p, self, own);
		return;
	}
	if (p.allo) hipLaunchKernelGGL(k4_genfreq<true>, dim3((K * L + 63) / 64), dim3(64), 0, c->stream, p, self, own);
	else hipLaunchKernelGGL(k4_genfreq<false>, dim3((K * L + 63) / 64), dim3(64), 0, c->stream, p, self, own);
}

/* What follows a draw of the frequencies, wherever it was made: the single precision rows for the Z pre-filter, then calc_exfreq_auto / _allo
 * (it follows update_P_auto in the chain loop, poly_geno.c:102-103).  on_host: the host mirrors c->freq (and freq2_h) are what the device holds. */
static int poly_after_draw(isg_ctx *c, bool on_host)
{
	if (refresh_freqf(c)) return 1;
	if (c->poly->p.allo_pref) {
		const size_t n = (size_t)c->poly->p.L * c->poly->p.Amax * c->poly->p.KPF;
		prof_begin(c);
		hipLaunchKernelGGL(k4_freq2f, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->poly->p);
		prof_end(c, "k4_freq2f");
	}
	prof_begin(c);
	poly_launch_exfreq(c);
	prof_end(c, c->poly->wide ? "k4_exfreq_w" : "k4_exfreq");
	HIPCHK(hipGetLastError());
	c->poly->freq_host = on_host;
	return 0;
}

static int poly_update_P(isg_ctx *c) /* update_P_auto / update_P_allo */
{
	PolyDev &p = c->poly->p;
	const int L = p.L, K = p.K, A = p.Amax;
	if (poly_sweep_counts(c)) return 1;
	if (is_keyed(c)) { /* every Dirichlet at its own stream position: all on the device */
		prof_begin(c);
		hipLaunchKernelGGL(k4_pdirich, dim3((K * L + 127) / 128), dim3(128), 0, c->stream, p, c->origin, iter_base(c), c->ky[KY_SP]);
		prof_end(c, "k4_pdirich");
		HIPCHK(hipGetLastError());
		return poly_after_draw(c, false);
	}
	if (c->pdev && c->pdev->usable) { /* the Dirichlets' start positions resolved on the device, all of them drawn at once (isg_walk_hip.inc); both variants */
		bool done = false;
		if (pdev_update_P(c, c->pdev, &done)) return 1;
		if (done) return poly_after_draw(c, false);
	}
	/* the host loop (both subgenomes from this stream position); no allelenum > 1 test on this path (poly_geno.c:426-434, 491-502) */
	const HostPSecond second = {p.cnt2, c->poly->cnt2_h.data(), c->poly->freq2_h.data()};
	if (host_update_P(c, HOSTP_REQUEST | HOSTP_DRAW, p.cnt, p.allo ? &second : nullptr, false)) return 1;
	auto ht0 = std::chrono::steady_clock::now();
	if (p.allo) {
		freq_to_device(c->poly->freq2_h.data(), c->freq_stage.data(), K, L, A, p.KP);
		HIPCHK(hipMemcpyAsync(p.freq2, c->freq_stage.data(), sizeof(double) * (size_t)L * A * p.KP, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream)); /* the staging buffer is reused for freq right below */
	}
	freq_to_device(c->freq.data(), c->freq_stage.data(), K, L, A, p.KP);
	HIPCHK(hipMemcpyAsync(p.freq, c->freq_stage.data(), sizeof(double) * (size_t)L * A * p.KP, hipMemcpyHostToDevice, c->stream));
	const int rc = poly_after_draw(c, true);
	HOST_T(c, 5, ht0); /* transpositions + upload launches */
	c->host_n++;
	return rc;
}

static int poly_read_acc(isg_ctx *c, int nslots, std::vector<isg_acc> &out)
{
	std::vector<unsigned long long> raw(5 * (size_t)nslots);
	HIPCHK(hipMemcpyAsync(raw.data(), c->poly->p.accbuf, sizeof(unsigned long long) * raw.size(), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	out.resize(nslots);
	for (int s = 0; s < nslots; s++) {
		unsigned long long t0 = raw[5 * s], t1 = raw[5 * s + 1] + (t0 >> 32), t2 = raw[5 * s + 2] + (t1 >> 32), t3 = raw[5 * s + 3] + (t2 >> 32);
		out[s].lo = (t0 & 0xffffffffULL) | (t1 << 32);
		out[s].hi = (t2 & 0xffffffffULL) | (t3 << 32);
		out[s].flags = (uint32_t)raw[5 * s + 4];
	}
	return 0;
}

static double poly_q_trans(int a, int b) /* mcmc.c:1566-1593 */
{
	if (a == 0) return (b == 0 || b == 1) ? 0.5 : 0.0;
	if (a == 2) return (b == 2 || b == 1) ? 0.5 : 0.0;
	if (a == 1) return (b == 0 || b == 2) ? 0.05 : (b == 1 ? 0.90 : 0.0);
	return 0.0;
}
static int poly_update_S_POP(isg_ctx *c) /* poly_geno.c:584-643 */
{
	/*
	 * The K Metropolis steps are sequential, but what they need from the device is not: a proposal only depends on
	 * the cluster's own current rate (and, for -e 0, state), and the uniforms are consumed in a fixed pattern
	 * (proposal draws, then the acceptance draw of that cluster).  So all proposals are drawn first, ALL tables
	 * (current and proposed rates) and ALL sums are computed in four launches, and the steps are then decided in
	 * order on the host from the exact sums -- same values, same decisions, same consumption as the reference loop.
	 */
	PolyDev &p = c->poly->p;
	const int K = p.K, L = p.L;
	const size_t nt = (size_t)L * p.GS;
	if (ensure_S(c)) return 1;
	if (poly_sweep_counts(c)) return 1;
	if (is_keyed(c)) host_seek(c, iter_base(c) + c->ky[KY_OFFS]);
	std::vector<double> prop(K), uacc(K);
	std::vector<int> pst(K, 0);
	for (int j = 0; j < K; j++) {
		double tmp;
		if (c->cfg.back_refl == 1) {
			tmp = host_next(c) * 2 * 0.05 - 0.05;
			tmp += c->S[j];
			if (tmp <= 0.0) tmp = 0.0 - tmp;
			else if (tmp >= 1.0) tmp = 1.0 - (tmp - 1.0);
		} else { /* adpt_indp (mcmc.c:1461-1520) on the cluster's own state */
			const int st = c->state[j];
			if (st == 0) { if (host_next(c) < 0.50) { tmp = 0.0; pst[j] = 0; } else { tmp = host_next(c); pst[j] = 1; } }
			else if (st == 2) { if (host_next(c) < 0.5) { tmp = 1.0; pst[j] = 2; } else { tmp = host_next(c); pst[j] = 1; } }
			else { const double tt = host_next(c); if (tt <= 0.05) { tmp = 0.0; pst[j] = 0; } else if (tt >= 0.95) { tmp = 1.0; pst[j] = 2; } else { tmp = host_next(c); pst[j] = 1; } }
		}
		prop[j] = tmp;
		uacc[j] = host_next(c); /* the acceptance draw follows the proposal's draws (poly_geno.c:625) */
	}
	float selfs[2 * ISG_KCAP];
	for (int k = 0; k < K; k++) {
		selfs[k] = (float)c->S[k];
		selfs[ISG_KCAP + k] = (float)prop[k];
	}
	HIPCHK(hipMemcpyAsync(c->poly->d_self, selfs, sizeof(selfs), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(p.accbuf, 0, sizeof(unsigned long long) * 5 * (2 * ISG_KCAP + 2), c->stream));
	prof_begin(c);
	poly_launch_genfreq(c, (const float *)c->poly->d_self, 1);
	prof_end(c, c->poly->wide ? "k4_genfreq_w" : "k4_genfreq");
	prof_begin(c);
	poly_launch_genfreq(c, (const float *)(c->poly->d_self + ISG_KCAP), 0);
	prof_end(c, c->poly->wide ? "k4_genfreq_w" : "k4_genfreq");
	{ /* the terms that no selfing rate touches (slot 0), from the counts of the iteration's sweep */
		const size_t ne = (size_t)L * p.Amax * K;
		prof_begin(c);
		hipLaunchKernelGGL(k4_mixsum, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, c->stream, p, (const int *)c->poly->d_cntmix, (const double *)p.freq);
		if (p.allo) hipLaunchKernelGGL(k4_mixsum, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, c->stream, p, (const int *)p.cntmix2, (const double *)p.freq2);
		prof_end(c, "k4_mixsum");
	}
	prof_begin(c);
	if (c->poly->wide) hipLaunchKernelGGL(k4_dsum_w, dim3((unsigned)L, 2 * K), dim3(256), 0, c->stream, p);
	else hipLaunchKernelGGL(k4_dsum, dim3((unsigned)((nt + 255) / 256), 2 * K), dim3(256), 0, c->stream, p);
	prof_end(c, "k4_dsum");
	HIPCHK(hipGetLastError());
	unsigned long long catcnt[8];
	HIPCHK(hipMemcpyAsync(catcnt, c->poly->d_catcnt, sizeof(catcnt), hipMemcpyDeviceToHost, c->stream));
	std::vector<isg_acc> acc; /* [0] fixed terms, [1 + k] current tables, [1 + K + k] proposal tables */
	if (poly_read_acc(c, 2 * K + 1, acc)) return 1;
	if (poly_check_err(c)) return 1;
	{ /* log multinomial coefficients of the mixed loci: log 4, 6, 12, 24 (poly_geno.c:1265-1270), each added count times */
		static const double coef_auto[5] = {1.0, 4.0, 6.0, 12.0, 24.0}, coef_allo[5] = {1.0, 2.0, 2.0, 4.0, 1.0}; /* allo: poly_geno.c:1275-1280 */
		const double *coef = p.allo ? coef_allo : coef_auto;
		for (int q = 1; q < (p.allo ? 4 : 5); q++) {
			unsigned long long left = catcnt[q];
			while (left) {
				const unsigned long long part = left > 0xffffffffULL ? 0xffffffffULL : left;
				acc_add_times(&acc[0], isg_log(coef[q]), part);
				left -= part;
			}
		}
	}
	for (int j = 0; j < K; j++) {
		/* both totals as exact sums over all terms, each rounded once (cal_lkd_props - cal_lkd) */
		isg_acc cur_t = acc[0], new_t = acc[0];
		for (int k = 0; k < K; k++) {
			isg_acc_merge(&cur_t, &acc[1 + k]);
			isg_acc_merge(&new_t, k == j ? &acc[1 + K + j] : &acc[1 + k]);
		}
		double mh = isg_acc_value(&new_t) - isg_acc_value(&cur_t);
		if (c->cfg.back_refl == 0) /* sic: the Hastings factor (only this cluster's state moves) multiplies the log ratio (poly_geno.c:622-623) */
			mh *= poly_q_trans(c->state[j], pst[j]) / poly_q_trans(pst[j], c->state[j]);
		const double m0 = (0 > mh) ? mh : 0; /* MIN2(0, mhratio) */
		if (uacc[j] < isg_exp(m0)) {
			c->S[j] = prop[j];
			if (c->cfg.back_refl == 0) c->state[j] = pst[j];
			acc[1 + j] = acc[1 + K + j];
			HIPCHK(hipMemcpyAsync(p.genofreq + (size_t)j * nt, p.tabtmp + (size_t)j * nt, sizeof(float) * nt, hipMemcpyDeviceToDevice, c->stream));
		}
	}
	HIPCHK(hipMemcpyAsync(c->d_S, c->S.data(), sizeof(double) * K, hipMemcpyHostToDevice, c->stream));
	return 0;
}

#define ISG_POLY_COOP_BLOCK 256 /* 512 (half as many workgroups in the all-to-all exchange) measured slower: two waves per SIMD stretch every phase */
template <int KMAX, int BLOCK>
__global__ void k4_zq_coop(PolyDev p, DevView d, isg_wh base, int init_flag, double alpha, CoopBuf *cb, uint64_t *pos_out);
template <int KMAX>
static bool poly_launch_zq_coop(isg_ctx *c, int init_flag, int G)
{
	if (!fits_resident(k4_zq_coop<KMAX, ISG_POLY_COOP_BLOCK>, ISG_POLY_COOP_BLOCK, G, c->cfg.device)) return false;
	hipLaunchKernelGGL((k4_zq_coop<KMAX, ISG_POLY_COOP_BLOCK>), dim3(G), dim3(ISG_POLY_COOP_BLOCK), 0, c->stream, c->poly->p, c->d, c->rng, init_flag, c->alpha,
			   (CoopBuf *)c->d_coop, c->d_pos);
	return true;
}
template <int KMAX>
static void poly_launch_zq(isg_ctx *c, int init_flag)
{
	if (is_keyed(c)) {
		const uint64_t pos0 = init_flag ? c->ky[KY_ZI0] : iter_base(c) + c->ky[KY_OFFZ];
		hipLaunchKernelGGL((k4_zq<256, KMAX, false>), dim3(c->cfg.N), dim3(256), 0, c->stream, c->poly->p, c->d, c->origin, pos0, c->ky[KY_SZ], init_flag,
				   c->alpha, c->d_pos);
	} else {
		hipLaunchKernelGGL((k4_zq<512, KMAX, true>), dim3(1), dim3(512), 0, c->stream, c->poly->p, c->d, c->rng, (uint64_t)0, (uint64_t)0, init_flag, c->alpha,
				   c->d_pos);
	}
}
static int poly_update_ZQ(isg_ctx *c, int init_flag)
{
	const int K = c->cfg.K;
	c->poly->counts_valid = false;
	c->d.tape = nullptr;
	c->d.tape_len = 0;
	if (c->zspec && !is_keyed(c) && !init_flag) { /* start positions resolved from intervals of shapes, then one parallel sweep (isg_spec_hip.inc) */
		bool done = false;
		SpecCtx *sp = c->zspec;
		const isg_wh base = c->rng;
		const bool zold = sp->zstrip; /* INSTRUCT_ZEXPECT_STRIP=1: the strip-per-wave kernel (k4_zexpect) instead of one lane per individual */
		auto expect = [&](float *alo, float *ahi) {
			kdispatch(KL_P4(), K, [&](auto km) {
				constexpr int KM = decltype(km)::value;
				constexpr int MI = KM <= 8 ? 4 : KM <= 12 ? 3 : KM <= 16 ? 2 : 1; /* individuals per workgroup: 2 MI KM accumulators + MI KM weights per lane */
				const unsigned zg = 8u * (unsigned)((c->cfg.N + MI - 1) / MI);
				int zr = 8;
				if (c->poly->p.Amax * c->d.KPF <= K4Z_SCR_FLOATS && !zold) {
					zr = (c->cfg.L + 63) / 64 < K4Z_NRANGE ? (c->cfg.L + 63) / 64 : K4Z_NRANGE;
					hipLaunchKernelGGL((k4_zexpect_ind<KM>), dim3((unsigned)((c->cfg.N + 255) / 256) * (unsigned)zr), dim3(256), 0, c->stream, c->poly->p, c->d, c->poly->d_zpart, zr);
				} else if (c->poly->p.Amax * c->d.KPF <= K4Z_SCR_FLOATS)
					hipLaunchKernelGGL((k4_zexpect<KM, true, MI>), dim3(zg), dim3(256), 0, c->stream, c->poly->p, c->d, c->poly->d_zpart);
				else
					hipLaunchKernelGGL((k4_zexpect<KM, false, MI>), dim3(zg), dim3(256), 0, c->stream, c->poly->p, c->d, c->poly->d_zpart);
				hipLaunchKernelGGL(k4_zexpect_fin, dim3((unsigned)((c->cfg.N * K + 255) / 256)), dim3(256), 0, c->stream, c->poly->p, (const float *)c->poly->d_zpart, c->alpha, sp->ksig, alo, ahi, zr);
			});
		};
		auto probe = [&](int grid) {
			kdispatch(KL_P4(), K, [&](auto km) {
				hipLaunchKernelGGL((k4_zq_probe<256, decltype(km)::value>), dim3(grid), dim3(256), 0, c->stream, c->poly->p, c->d, base, c->alpha, (const unsigned long long *)sp->d_B,
						   (const SpecProbe *)sp->d_list, sp->d_dev, sp->list_cap, sp->walk.d_table);
			});
		};
		auto at = [&]() {
			kdispatch(KL_P4(), K, [&](auto km) {
				hipLaunchKernelGGL((k4_zq<256, decltype(km)::value, false>), dim3(c->cfg.N), dim3(256), 0, c->stream, c->poly->p, c->d, base, (uint64_t)0, (uint64_t)0, 0, c->alpha, c->d_pos,
						   (const unsigned long long *)sp->d_offs, (const ResolveState *)sp->d_rs);
			});
		};
		if (spec_update_ZQ_with(c, sp, base, &done, expect, probe, at)) return 1;
		if (done) return 0;
	}
	if (c->rs && !is_keyed(c) && !init_flag) { /* start positions resolved block-wise, then one parallel sweep (isg_resolve_hip.inc) */
		bool done = false;
		ResolveCtx *r = c->rs;
		const isg_wh base = c->rng;
		auto block = [&](int b, uint64_t tl) {
			kdispatch(KL_P4_BLOCK(), K, [&](auto km) {
				hipLaunchKernelGGL((k4_zq_block<decltype(km)::value>), dim3(r->plan_h.nunits), dim3(256), 0, c->stream, c->poly->p, c->d, base, c->alpha, (const ResolvePlan *)r->d_plan,
						   r->d_st, (const unsigned long long *)r->d_B, (const float *)r->d_tapef, (unsigned long long)tl, r->d_offs, b);
			});
		};
		auto at = [&]() {
			kdispatch(KL_P4_BLOCK(), K, [&](auto km) {
				hipLaunchKernelGGL((k4_zq<256, decltype(km)::value, false>), dim3(c->cfg.N), dim3(256), 0, c->stream, c->poly->p, c->d, base, (uint64_t)0, (uint64_t)0, 0, c->alpha, c->d_pos,
						   (const unsigned long long *)r->d_offs, (const ResolveState *)r->d_st);
			});
		};
		if (resolve_update_ZQ_with(c, base, &done, block, at, [&](uint64_t) { return false; })) return 1;
		if (done) return 0;
	}
	if (c->coop && !is_keyed(c)) {
		/* the phase's stretch of the stream, generated by the whole chip (see isg_update_ZQ) */
		const uint64_t need = 4 * c->nvalid_total + (16ull * K + 64) * (uint64_t)c->cfg.N + 8192;
		if (tape_fill(c, c->rng, need)) return 1;
		HIPCHK(hipMemsetAsync(c->d_coop, 0, sizeof(CoopBuf), c->stream));
		int G = (c->poly->p.Lp + ISG_POLY_COOP_BLOCK - 1) / ISG_POLY_COOP_BLOCK;
		if (G > ISG_COOP_GMAX) G = ISG_COOP_GMAX;
		HIPCHK(hipMemcpyAsync(c->d_qqsave, c->d.qq, sizeof(double) * (size_t)c->cfg.N * K, hipMemcpyDeviceToDevice, c->stream));
		bool launched = false;
		prof_begin(c);
		kdispatch(KL_P4(), K, [&](auto km) { launched = poly_launch_zq_coop<decltype(km)::value>(c, init_flag, G); });
		prof_end(c, "k4_zq_coop");
		HIPCHK(hipGetLastError());
		bool done = false;
		if (coop_sweep_end(c, launched, &done)) return 1;
		if (done) return 0;
	}
	prof_begin(c);
	kdispatch(KL_P4(), K, [&](auto km) { poly_launch_zq<decltype(km)::value>(c, init_flag); });
	prof_end(c, is_keyed(c) ? "k4_zq_keyed" : "k4_zq");
	HIPCHK(hipGetLastError());
	if (!is_keyed(c) && chain_sweep_end(c)) return 1;
	c->h_qq = false;
	return 0;
}

static int poly_cal_lkh(isg_ctx *c)
{
	PolyDev &p = c->poly->p;
	prof_begin(c);
	hipLaunchKernelGGL(k4_logfreq, dim3((unsigned)(((size_t)p.L * p.Amax * p.KP + (size_t)p.K * p.GS * p.L + 255) / 256)), dim3(256), 0, c->stream, p);
	prof_end(c, "k4_logfreq");
	prof_begin(c);
	if (c->poly->wide) {
		if (p.allo) hipLaunchKernelGGL(k4_lkd_w<true>, dim3(p.N), dim3(256), 0, c->stream, p);
		else hipLaunchKernelGGL(k4_lkd_w<false>, dim3(p.N), dim3(256), 0, c->stream, p);
	} else if (p.allo) hipLaunchKernelGGL(k4_lkd<true>, dim3(p.N), dim3(256), 0, c->stream, p);
	else hipLaunchKernelGGL(k4_lkd<false>, dim3(p.N), dim3(256), 0, c->stream, p);
	prof_end(c, "k4_lkd");
	prof_begin(c);
	hipLaunchKernelGGL(k_lkh_total<1024>, dim3(1), dim3(1024), 0, c->stream, c->d, c->d_total);
	prof_end(c, "k_lkh_total");
	HIPCHK(hipGetLastError());
	c->h_lkh = false;
	return 0;
}

static int poly_chain_init(isg_ctx *c, const float *initd) /* poly_geno.c:85-96 */
{
	const int K = c->cfg.K;
	c->origin = c->rng;
	c->iter = 0;
	c->alpha = host_next(c) * 10; /* initial_chn, poly_geno.c:380 */
	if (poly_geno_sweep(c, 1)) return 1;
	for (int k = 0; k < K; k++) {
		c->S[k] = (double)initd[k];
		if (c->cfg.back_refl == 0) {
			const int st = isg_dt_stat(c->S[k]);
			if (st < 0) return fail("The value of selfing rate or inbreeding coefficient is beyond [0,1]!");
			c->state[k] = st;
		}
	}
	c->h_S = true;
	return poly_update_ZQ(c, 1);
}

static int poly_iteration(isg_ctx *c) /* poly_geno.c:98-116 */
{
	if (poly_update_P(c)) return 1;
	if (poly_update_S_POP(c)) return 1;
	if (poly_update_ZQ(c, 0)) return 1;
	if (poly_geno_sweep(c, 0)) return 1;
	if (poly_cal_lkh(c)) return 1;
	c->iter++;
	return 0;
}

static int poly_count_alleles(isg_ctx *c, int32_t *counts)
{
	PolyDev &p = c->poly->p;
	const int L = p.L, K = p.K, A = p.Amax;
	if (poly_sweep_counts(c)) return 1;
	HIPCHK(hipMemcpyAsync(c->cnt_h.data(), p.cnt, sizeof(int) * c->cnt_h.size(), hipMemcpyDeviceToHost, c->stream));
	if (p.allo) HIPCHK(hipMemcpyAsync(c->poly->cnt2_h.data(), p.cnt2, sizeof(int) * c->poly->cnt2_h.size(), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	counts_from_device(c->cnt_h.data(), p.allo ? c->poly->cnt2_h.data() : nullptr, counts, K, L, A); /* allotetraploid: both subgenomes' copies (seqpop + seqpop2) */
	return 0;
}

/* [N][Lp][4] bytes -> [N][L][4] ints, -1 where the locus is unused */
static int poly_get_bytes(isg_ctx *c, const uint8_t *dev, int32_t *out)
{
	const PolyDev &p = c->poly->p;
	std::vector<uint8_t> h((size_t)p.N * p.Lp * 4);
	HIPCHK(hipMemcpyAsync(h.data(), dev, h.size(), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	bytes_to_ints(h.data(), out, p.N, p.L, p.Lp, 4);
	return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* k4_zq_coop: update_ZQ with several workgroups per individual (see k_zq_coop in               */
/* isg_coop_hip.inc: same exchange of counts, same Dirichlet in every workgroup, same uniform    */
/* tape; one locus = 4 allele copies per lane)                                                   */
/* ------------------------------------------------------------------------------------------ */
template <int KMAX, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k4_zq_coop(PolyDev p, DevView d, isg_wh base, int init_flag, double alpha, CoopBuf *cb, uint64_t *pos_out)
{
	constexpr bool PRE = (KMAX <= 16); /* single precision pre-filter rows in registers */
	__shared__ ZqShared sh;
	const int t = threadIdx.x, g = blockIdx.x, G = gridDim.x, K = p.K;
	{
		const uint16_t *src = (const uint16_t *)p.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += BLOCK) dst[k] = src[k];
		if (t < 2 * ISG_KCAP) {
			(&sh.hist[0][0])[t] = 0;
			(&sh.amask[0][0])[t] = 0;
			(&sh.rmask[0][0])[t] = 0;
			(&sh.ghist[0][0])[t] = 0;
		}
	}
	__syncthreads();
	const isg_wh cur = isg_wh_jump(&sh.tab, base, 0);
	unsigned long long off = 0;
	const int stride = G * BLOCK;
	const size_t rowb = (size_t)p.Lp * 4;
	const bool writer = (g == 0) && (t >= BLOCK - 64);
	const CoopLayout lay = coop_layout(G, BLOCK, K, p.Lp, 4); /* isg_coop_layout.h */
	const bool wmode = lay.wmode;
	const int pack = lay.pack, bits = lay.bits, W = lay.W;
	double icum[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) icum[m] = (m < K) ? (double)(m + 1) / K : 0.0;
	double touch = 0.0, touch2 = 0.0;
	unsigned pg = 0xffffffffu, prw = 0, ng = 0xffffffffu, nrw = 0;
	float pF[4][KMAX];
#pragma unroll
	for (int c = 0; c < 4; c++)
#pragma unroll
		for (int m = 0; m < KMAX; m++) pF[c][m] = 0.f;
	auto fetch_geno = [&](int ni, int nj, unsigned &gw, unsigned &rw) {
		gw = 0xffffffffu;
		rw = 0;
		if (ni < p.N && nj < p.Lp) {
			gw = *(const unsigned *)(p.geno + (size_t)ni * rowb + (size_t)nj * 4);
			rw = p.rankwave[(size_t)ni * p.nwv + (nj >> 6)];
		}
	};
	auto fetch_rows = [&](int nj) {
		if ((pg & 0xff) != 0xff && PRE && !init_flag) {
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const float *R = d.freqf + ((size_t)nj * p.Amax + ((pg >> (8 * c)) & 0xff)) * d.KPF;
#pragma unroll
				for (int m = 0; m < KMAX; m += 4) {
					if (m < K) {
						const float4 f = *(const float4 *)(R + m);
						pF[c][m] = f.x;
						if (m + 1 < KMAX) pF[c][m + 1] = f.y;
						if (m + 2 < KMAX) pF[c][m + 2] = f.z;
						if (m + 3 < KMAX) pF[c][m + 3] = f.w;
					}
				}
			}
		}
	};
	fetch_geno(0, g * BLOCK + t, pg, prw);
	fetch_rows(g * BLOCK + t);
	int pnvalid = p.nvalid[0];
	double pq[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) pq[m] = (m < K && !init_flag) ? p.qq[m] : 0.0;
	for (int i = 0; i < p.N; i++) {
		const unsigned tag = (unsigned)(i % 65535) + 1u;
		const int slot = i & (ISG_COOP_RING - 1), par = i & 1;
		if (touch2 == -1.0 || touch == -1.0) cb->overflow_flag = 2;
		const int nvalid = pnvalid;
		double q[KMAX];
		float qf[KMAX];
#pragma unroll
		for (int m = 0; m < KMAX; m++) {
			q[m] = pq[m];
			qf[m] = (float)q[m];
		}
		int wcnt[KMAX];
#pragma unroll
		for (int m = 0; m < KMAX; m++) wcnt[m] = 0;
		const unsigned long long offi = off;
		const bool covered = offi + 4ull * (unsigned)nvalid + 2048ull <= d.tape_len;
		STAMP(i, 0);
		for (int j = g * BLOCK + t; j - t < p.Lp; j += stride) { /* wave-uniform trip count */
			const unsigned gw = pg;
			const bool valid = ((gw & 0xff) != 0xff);
			const unsigned long long vm = __ballot(valid);
			const unsigned rank = prw + (unsigned)__popcll(vm & ((1ull << lane_id()) - 1ull));
			float F[4][KMAX];
#pragma unroll
			for (int c = 0; c < 4; c++)
#pragma unroll
				for (int m = 0; m < KMAX; m++) F[c][m] = pF[c][m];
			double x[4] = {0, 0, 0, 0};
			if (valid && covered) {
#pragma unroll
				for (int c = 0; c < 4; c++) x[c] = d.tape[offi + 4ull * rank + c];
			}
			if (j - t == g * BLOCK) { /* first pass: everything needed later queues up behind the uniforms */
				if (covered && t < 10) touch = d.tape[offi + 4ull * (unsigned)nvalid + 16u * (unsigned)t];
				fetch_geno(i + 1, g * BLOCK + t, ng, nrw);
				if (i + 1 < p.N) {
					pnvalid = p.nvalid[i + 1];
#pragma unroll
					for (int m = 0; m < KMAX; m++) pq[m] = (m < K && !init_flag) ? p.qq[(size_t)(i + 1) * K + m] : 0.0;
				}
			}
			if (j - t + stride < p.Lp) { /* a further pass of this individual */
				fetch_geno(i, j + stride, pg, prw);
				fetch_rows(j + stride);
			}
			int zz[4] = {0xff, 0xff, 0xff, 0xff};
			if (valid && covered) {
#pragma unroll
				for (int c = 0; c < 4; c++) {
					if (init_flag) {
						zz[c] = bucket_fast<KMAX>(x[c], icum, 1.0, K);
					} else {
						bool amb = true;
						if (PRE) zz[c] = bucket_f32<KMAX>((float)x[c], F[c], qf, K, &amb);
						if (amb) {
							double cum[KMAX];
							const double tot = weights<KMAX>(p.freq + ((size_t)j * p.Amax + ((gw >> (8 * c)) & 0xff)) * p.KP, q, cum, K);
							zz[c] = bucket_fast<KMAX>(x[c], cum, tot, K);
						}
					}
				}
			}
#pragma unroll
			for (int m = 0; m < KMAX; m++)
				if (m < K)
					wcnt[m] += __popcll(__ballot(zz[0] == m)) + __popcll(__ballot(zz[1] == m)) + __popcll(__ballot(zz[2] == m)) +
						   __popcll(__ballot(zz[3] == m));
			if (j < p.Lp)
				*(unsigned *)(p.z + (size_t)i * rowb + (size_t)j * 4) =
					(unsigned)zz[0] | ((unsigned)zz[1] << 8) | ((unsigned)zz[2] << 16) | ((unsigned)zz[3] << 24);
		}
		STAMP(i, 1);
		if (wmode) {
			unsigned long long v = (unsigned long long)tag << 48;
#pragma unroll
			for (int m = 0; m < KMAX; m++)
				if (m < K && (int)lane_id() == m / 3) v |= (unsigned long long)(wcnt[m] & 0xffff) << (16 * (m % 3));
			if ((int)lane_id() < W) st_agent(&cb->gran[slot][(g * (BLOCK / 64) + (t >> 6)) * W + (int)lane_id()], v);
		} else {
			if (lane_id() == 0) {
#pragma unroll
				for (int m = 0; m < KMAX; m++)
					if (m < K && wcnt[m]) atomicAdd(&sh.hist[par][m], wcnt[m]);
			}
			lds_barrier();
			if (t < W) { /* `pack` counts of `bits` bits per word */
				unsigned long long v = (unsigned long long)tag << 48;
				for (int c3 = 0; c3 < pack; c3++)
					if (pack * t + c3 < K) v |= (unsigned long long)(sh.hist[par][pack * t + c3] & ((1 << bits) - 1)) << (bits * c3);
				st_agent(&cb->gran[slot][g * W + t], v);
			}
		}
		STAMP(i, 2);
		/* while they travel: the frequency rows of the next individual's first locus, a touch of its tape lines */
		pg = ng;
		prw = nrw;
		fetch_rows(g * BLOCK + t);
		if (covered && i + 1 < p.N && lane_id() < 18) touch2 = d.tape[offi + 4ull * (unsigned)nvalid + 4ull * prw + 16u * lane_id()];
		if (!covered && t == 0) cb->overflow_flag = 1;
		const int ngran = lay.ngran;
		for (int gi = t; gi - t < ngran; gi += BLOCK) { /* wave-uniform trip count */
			if (gi < ngran && (wmode || gi / W != g)) {
				const unsigned long long v = coop_poll(&cb->gran[slot][gi], tag, cb);
				const int w = gi % W;
				for (int c3 = 0; c3 < pack; c3++) {
					const int m = pack * w + c3;
					const int cc = (int)((v >> (bits * c3)) & ((1 << bits) - 1));
					if (m < K && cc) atomicAdd(&sh.ghist[par][m], cc);
				}
			}
		}
		lds_barrier();
		STAMP(i, 3);
		const unsigned used = 4u * (unsigned)nvalid +
			dirichlet_coop<BLOCK, KMAX>(d, sh, i, cur, offi + 4ull * (unsigned)nvalid, alpha, par,
						    covered ? d.tape + offi + 4ull * (unsigned)nvalid : nullptr, writer);
		off += used;
	}
	if (g == 0 && t == 0) *pos_out = off;
}
