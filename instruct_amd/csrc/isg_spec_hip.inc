/*
 * isg_spec_hip.inc -- replay-schedule update_ZQ (mcmc.c:1122-1203) with the start positions resolved from INTERVALS of shapes.
 *
 * Individual i + 1 starts where individual i's Dirichlet (mcmc.c:1196-1198, random.c:264-280) stopped, and that Dirichlet's
 * shapes are the cluster counts of i's own Z draws + alpha: nobody knows them before the draws are made, and the draws need
 * the start position.  The block resolver (isg_resolve_hip.inc) therefore makes the draws for EVERY candidate position of a
 * window (33 per individual at config 3).  But the accept / reject decision of an rgamma2 attempt (random.c:195-231) hardly
 * depends on a large shape: with  lambda_m = sum over the allele copies of P(Z = m)  and  sigma_m^2 = sum of P (1 - P)  (one
 * pass over the individual's loci, no random numbers) the count of cluster m lies in  lambda_m +- k sigma_m  whatever the
 * start position, and for such an interval of shapes most attempts have the SAME outcome at both ends: their accept bit is
 * CERTAIN without a single draw.  The walk engine (isg_walk.h, interval mode) builds its tables from those bits and flags the
 * bytes whose path touched an uncertain attempt; then
 *
 *   1. a walk in which an uncertain byte counts as guessed gives a trajectory that is right up to its first wrong guess;
 *   2. the uncertain bytes ON that trajectory (3 % of the individuals) are PROBED: the individual's draws at that very start
 *      position, counts, the Dirichlet's consumption -- exactly, by the sweep kernel's own code (zq_one, nothing written) -- and
 *      patched into the tables;
 *   3. the walk again over the patched tables.  Where a guess was wrong the trajectory leaves the old one -- and joins it again
 *      a few individuals later (two walks that land on the same offset stay together, and neighbouring offsets do so within a few
 *      steps): only the stretch in between brings new uncertain bytes.  2. and 3. repeat until the trajectory holds none: three
 *      rounds and 330 probes at N = 10000, L = 5000, K = 5 (a window of candidates around a guessed trajectory does not work: once
 *      apart, two trajectories drift like independent random walks, 120 offsets in that sweep);
 *   4. k_zq_at runs the sweep at the resolved positions and checks every Dirichlet's consumption, as for the block resolver.
 *
 * Certain bits are speculation in two places -- the count interval is a k-sigma bound and the bounds on a margin's movement
 * inside an interval are first order -- so step 4's check is what makes the result exact: any mismatch (or a window that was
 * missed, rounds that do not settle) restores qq and hands the sweep to the block resolver / the chain kernels.  Early in a chain (all clusters large) about 2 % of the candidates are uncertain at N = 10000, L = 5000, K = 5; when
 * clusters with a handful of draws appear every candidate is, the probes outnumber the block resolver's work, and this path
 * stands back (it looks again every few sweeps).
 */
struct SpecProbe {
	int i;
	unsigned x;                /* absolute pair offset of the candidate */
	unsigned long long taddr;  /* its table byte */
};
struct SpecDev {
	unsigned nlist, overflow;     /* uncertain bytes on the current trajectory (zeroed before every round) */
	unsigned nprobes, rounds;     /* probes answered in all; rounds that found something to probe */
};
struct SpecCtx {
	WalkRun walk;
	int N = 0, K = 0, copies = 2;
	std::vector<int> gam0_h;
	DevBuf<int> d_gam0;
	DevBuf<unsigned long long> d_gpos, d_B, d_offs;
	DevBuf<float> d_alo, d_ahi;
	bool zstrip = false;      /* ploidy 4, INSTRUCT_ZEXPECT_STRIP=1: the strip-per-wave kernel k4_zexpect instead of one lane per individual.  (The diploid
	                           * k_zexpect gains nothing from a lane per individual: 0.196 against 0.190 ms at config 3, measured.) */
	DevBuf<SpecProbe> d_list;
	DevBuf<SpecDev> d_dev;
	DevBuf<ResolveState> d_rs;
	int list_cap = 0, band = 0, rounds = 2; /* rounds launched without looking (two settle 9 sweeps in 10 at config 3; more, one by one, if not) */
	float ksig = 4.5f;
	unsigned err_bit = 4u;
	/* policy */
	int cooldown = 0;           /* sweeps to sit out after a sweep this path lost */
	int backoff = 0;
	long retried = 0; /* sweeps redone at once with wider windows after a missed one */
	long sweeps = 0, done = 0, lost = 0;
	unsigned last_probes = 0, last_fail = 0, last_rounds = 0, lost_fail = 0; /* lost_fail: the fail bits of all lost sweeps */
	int test_abort = 0;
};

/* lambda, sigma of the cluster counts of an individual and from them the interval of each gamma's shape.
 * P(Z = m) for an allele copy = qq[m] freq[m][locus][allele] / sum (mcmc.c:1146-1147, normalised as disc_unif does, random.c:412-413)
 * A workgroup takes MI individuals: a lane fetches its locus' rows ONCE and uses them for all MI (one individual per workgroup reads the
 * whole table, L x Amax x KPF floats, from the L2 again: 3.2 GB per sweep at config 3, the kernel ran at the L2's bandwidth); clusters in
 * pairs (v_pk_mul_f32 / v_pk_add_f32 do two per lane and cycle). */
typedef float zx_f2 __attribute__((ext_vector_type(2)));
template <int KMAX, int MI>
__global__ void __launch_bounds__(256) k_zexpect(DevView d, double alpha, float ksig, float *alo, float *ahi)
{
	constexpr int KH = (KMAX + 1) / 2, Q4 = (KMAX + 3) / 4;
	__shared__ float red[MI][4][2 * KMAX];
	const int i0 = blockIdx.x * MI, t = threadIdx.x, K = d.K, lane = (int)lane_id();
	zx_f2 qf[MI][KH], lam[MI][KH], var[MI][KH];
#pragma unroll
	for (int m = 0; m < MI; m++)
#pragma unroll
		for (int h = 0; h < KH; h++) {
			const int i = (i0 + m < d.N) ? i0 + m : d.N - 1;
			qf[m][h].x = (2 * h < K) ? (float)d.qq[(size_t)i * K + 2 * h] : 0.f;
			qf[m][h].y = (2 * h + 1 < K) ? (float)d.qq[(size_t)i * K + 2 * h + 1] : 0.f;
			lam[m][h] = (zx_f2)(0.f);
			var[m][h] = (zx_f2)(0.f);
		}
	const unsigned short *grow = (const unsigned short *)(d.geno + (size_t)i0 * d.Lp * 2);
	const bool two = (d.Amax == 2);
	for (int j = t; j < d.Lp; j += 256) {
		/* two alleles (the usual case): the locus' two rows are one contiguous block -- fetched whole by every lane (coalesced: a gathered
		 * 32-byte row costs a 128-byte L2 line per lane), the copies' rows picked in registers */
		float4 B0[Q4], B1[Q4];
		if (two) {
			const float4 *src = (const float4 *)(d.freqf + (size_t)j * 2 * d.KPF);
#pragma unroll
			for (int q = 0; q < Q4; q++) {
				B0[q] = (4 * q < d.KPF) ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);
				B1[q] = (4 * q < d.KPF) ? src[d.KPF / 4 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
			}
		}
		unsigned gs[MI];
#pragma unroll
		for (int m = 0; m < MI; m++) gs[m] = (i0 + m < d.N) ? grow[(size_t)m * d.Lp + j] : 0xffffu;
#pragma unroll
		for (int m = 0; m < MI; m++) {
			const unsigned g = gs[m];
			const unsigned a0 = g & 0xff, a1 = g >> 8;
			if (a0 == 0xff) continue;
#pragma unroll
			for (int cp = 0; cp < 2; cp++) {
				const unsigned al = cp ? a1 : a0;
				const float *F = d.freqf + ((size_t)j * d.Amax + al) * d.KPF;
				zx_f2 w[KH], tot2 = (zx_f2)(0.f);
#pragma unroll
				for (int q = 0; q < Q4; q++) {
					float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
					if (4 * q < K) {
						if (two) {
							const float4 r0 = B0[q], r1 = B1[q];
							f = al ? r1 : r0;
						} else {
							f = *(const float4 *)(F + 4 * q);
						}
					}
					w[2 * q] = qf[m][2 * q] * (zx_f2){f.x, f.y};
					if (2 * q + 1 < KH) w[2 * q + 1] = qf[m][2 * q + 1] * (zx_f2){f.z, f.w};
				}
#pragma unroll
				for (int h = 0; h < KH; h++) tot2 += w[h];
				const float tot = tot2.x + tot2.y;
				const float inv = (tot > 0.f) ? 1.0f / tot : 0.f;
				const zx_f2 inv2 = (zx_f2)(inv), one2 = (zx_f2)(1.0f);
#pragma unroll
				for (int h = 0; h < KH; h++) {
					const zx_f2 pr = w[h] * inv2;
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
		if (i >= d.N) break;
		const float l = red[m][0][k] + red[m][1][k] + red[m][2][k] + red[m][3][k];
		float v = red[m][0][KMAX + k] + red[m][1][KMAX + k] + red[m][2][KMAX + k] + red[m][3][KMAX + k];
		v = v > 0.f ? v : 0.f;
		/* single precision sums of up to 2 L terms: allow for their rounding as well */
		const float h = ksig * __builtin_sqrtf(v) + 1.0f + 1e-5f * l;
		float lo = __builtin_floorf(l - h), hi = __builtin_ceilf(l + h);
		const float tot = 2.0f * (float)d.nvalid[i];
		if (lo < 0.f) lo = 0.f;
		if (hi > tot) hi = tot;
		if (d.nvalid[i] == 0) lo = hi = 0.f;
		alo[(size_t)i * K + k] = (float)((double)lo + alpha);
		ahi[(size_t)i * K + k] = (float)((double)hi + alpha);
	}
}

/* the uncertain bytes within +-band offsets of the lenient trajectory: one thread per (individual, offset) */
__global__ void __launch_bounds__(256) k_zs_band(const WkBlock *blk, const WkSeg *segs, int nseg, const unsigned char *table, const WkState *st, const unsigned long long *T, int N, int band,
						 SpecProbe *list, int cap, SpecDev *dev)
{
	const long id = (long)blockIdx.x * 256 + threadIdx.x;
	const int span = 2 * band + 1;
	const int i = (int)(id / span), j = (int)(id - (long)i * span) - band;
	if (i >= N || st->fail) return;
	int s = 0;
	while (s + 1 < nseg && i >= segs[s].g1) s++;
	const WkSeg S = segs[s];
	const WkBlock B = blk[S.b0 + (i - S.g0) / S.bg];
	const long long x = (long long)T[i] + j;
	const long long col = x - (long long)st->xin[s] - B.wlo;
	if (x < 0 || col < 0 || col >= B.W) return;
	const unsigned long long addr = B.toff + (unsigned long long)(i - B.g0) * (unsigned long long)B.W + (unsigned long long)col;
	const unsigned v = table[addr];
	if (v == WK_IRR || !(v & WK_UFLAG)) return;
	const unsigned slot = atomicAdd(&dev->nlist, 1u);
	if (slot < (unsigned)cap) {
		list[slot].i = i;
		list[slot].x = (unsigned)x;
		list[slot].taddr = addr;
	} else {
		dev->overflow = 1u;
	}
}

/* K > ISG_KCAP: the same intervals, one workgroup per (individual, ISG_ZX_WCH clusters).  Each copy's total is formed anew from the qq
 * row in LDS (K terms) so that a lane holds ISG_ZX_WCH accumulator pairs whatever K is. */
#define ISG_ZX_WCH 16
__global__ void __launch_bounds__(256) k_zexpect_w(DevView d, double alpha, float ksig, float *alo, float *ahi)
{
	__shared__ float qs[ISG_KWIDE];
	__shared__ float red[4][2 * ISG_ZX_WCH];
	const int i = blockIdx.x, k0 = blockIdx.y * ISG_ZX_WCH, t = threadIdx.x, K = d.K, lane = (int)lane_id();
	if (t < K) qs[t] = (float)d.qq[(size_t)i * K + t];
	__syncthreads();
	float lam[ISG_ZX_WCH], var[ISG_ZX_WCH];
#pragma unroll
	for (int h = 0; h < ISG_ZX_WCH; h++) lam[h] = var[h] = 0.f;
	const unsigned short *grow = (const unsigned short *)(d.geno + (size_t)i * d.Lp * 2);
	for (int j = t; j < d.Lp; j += 256) {
		const unsigned g = grow[j];
		const unsigned a0 = g & 0xff, a1 = g >> 8;
		if (a0 == 0xff) continue;
		for (int cp = 0; cp < 2; cp++) {
			const float *F = d.freqf + ((size_t)j * d.Amax + (cp ? a1 : a0)) * d.KPF;
			float tot = 0.f;
			for (int m = 0; m < K; m++) tot += qs[m] * F[m];
			const float inv = (tot > 0.f) ? 1.0f / tot : 0.f;
#pragma unroll
			for (int h = 0; h < ISG_ZX_WCH; h++) {
				const bool in = (k0 + h < K);
				const int k = in ? k0 + h : 0;
				const float pr = in ? qs[k] * F[k] * inv : 0.f;
				lam[h] += pr;
				var[h] += pr * (1.0f - pr);
			}
		}
	}
#pragma unroll
	for (int h = 0; h < ISG_ZX_WCH; h++) {
		float l = lam[h], v = var[h];
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			l += __shfl_down(l, o, 64);
			v += __shfl_down(v, o, 64);
		}
		if (lane == 0) {
			red[t >> 6][h] = l;
			red[t >> 6][ISG_ZX_WCH + h] = v;
		}
	}
	__syncthreads();
	const int k = k0 + t;
	if (t < ISG_ZX_WCH && k < K) { /* as k_zexpect */
		const float l = red[0][t] + red[1][t] + red[2][t] + red[3][t];
		float v = red[0][ISG_ZX_WCH + t] + red[1][ISG_ZX_WCH + t] + red[2][ISG_ZX_WCH + t] + red[3][ISG_ZX_WCH + t];
		v = v > 0.f ? v : 0.f;
		const float h = ksig * __builtin_sqrtf(v) + 1.0f + 1e-5f * l;
		float lo = __builtin_floorf(l - h), hi = __builtin_ceilf(l + h);
		const float tot = 2.0f * (float)d.nvalid[i];
		if (lo < 0.f) lo = 0.f;
		if (hi > tot) hi = tot;
		if (d.nvalid[i] == 0) lo = hi = 0.f;
		alo[(size_t)i * K + k] = (float)((double)lo + alpha);
		ahi[(size_t)i * K + k] = (float)((double)hi + alpha);
	}
}

/* a probe: individual i started at B[i] + 2 x -- its Z draws, counts and the Dirichlet's consumption, exactly as the sweep takes them
 * (zq_one), nothing written but the table byte.  Workgroups take probes in turn. */
template <int BLOCK, int KMAX>
__global__ void __launch_bounds__(BLOCK) k_zq_probe(DevView d, isg_wh base, double alpha, const unsigned long long *Bpre, const SpecProbe *list, SpecDev *dev, int cap, unsigned char *table)
{
	__shared__ ZqSh<KMAX> sh;
	const int t = threadIdx.x;
	{
		const uint16_t *src = (const uint16_t *)d.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += BLOCK) dst[k] = src[k];
	}
	__syncthreads();
	const isg_wh mult0 = isg_wh_power(&sh.tab, 8u * (unsigned)t);
	const isg_wh mult_pass = isg_wh_power(&sh.tab, 8u * (unsigned)BLOCK);
	const unsigned n = dev->nlist < (unsigned)cap ? dev->nlist : (unsigned)cap;
	if (blockIdx.x == 0 && t == 0 && n) { dev->nprobes += n; dev->rounds += 1u; }
	for (unsigned p = blockIdx.x; p < n; p += gridDim.x) {
		if (t < 2 * ZqSh<KMAX>::KC) (&sh.hist[0][0])[t] = 0;
		__syncthreads();
		const int i = list[p].i;
		const unsigned long long o = Bpre[i] + 2ull * list[p].x;
		const isg_wh cur = isg_wh_jump(&sh.tab, base, o);
		ZqPrefetch<KMAX> pf;
		zq_prefetch<KMAX>(d, i, 0, pf);
		const unsigned used = zq_one<BLOCK, KMAX, false, false>(d, sh, i, cur, 0, 0, alpha, mult0, mult_pass, pf);
		if (t == 0) {
			const unsigned minimal = 2u * (unsigned)d.nvalid[i] + 2u * (unsigned)d.K;
			unsigned char v = (unsigned char)WK_IRR;
			if (used >= minimal && !((used - minimal) & 1u) && (used - minimal) / 2u <= 126u) v = (unsigned char)((used - minimal) / 2u);
			table[list[p].taddr] = v;
		}
		__syncthreads();
	}
}

/* the strict walk's offsets as the sweep kernel wants them: stream positions from the phase's base, and the go / no-go record */
__global__ void __launch_bounds__(256) k_zs_offs(const unsigned long long *T, const unsigned long long *Bpre, int N, const WkState *st, const SpecDev *dev, unsigned long long *offs, ResolveState *rs)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	const bool bad = st->fail != 0u || dev->overflow != 0u || dev->nlist != 0u; /* (nlist: uncertain bytes left on the trajectory) */
	if (i <= N) offs[i] = bad ? 0ull : Bpre[i] + 2ull * T[i];
	if (i == 0) {
		rs->fail = bad ? 1u : 0u;
		rs->total = bad ? 0ull : Bpre[N] + 2ull * T[N];
		rs->done = 1u;
	}
}

/* nvalid: used loci per individual (host); copies: allele copies per locus = uniforms per used locus */
static int spec_create(isg_ctx *c, SpecCtx **out, const std::vector<int> &nvalid, int copies)
{
	*out = nullptr;
	if (!env_flag(getenv("INSTRUCT_ZQ_SPEC_RESOLVE"), true)) return 0;
	const int N = c->cfg.N, K = c->cfg.K;
	if (K > WK_NGMAX) return 0;
	SpecCtx *sp = new SpecCtx();
	sp->N = N;
	sp->K = K;
	sp->copies = copies;
	sp->gam0_h.resize((size_t)N + 1);
	std::vector<unsigned long long> B((size_t)N + 1, 0), gpos((size_t)N * K + 1, 0);
	for (int i = 0; i < N; i++) {
		sp->gam0_h[i] = i * K;
		B[i + 1] = B[i] + (unsigned long long)copies * (unsigned)nvalid[i] + 2ull * (unsigned)K;
		for (int m = 0; m < K; m++) gpos[(size_t)i * K + m] = B[i] + (unsigned long long)copies * (unsigned)nvalid[i] + 2ull * (unsigned)m;
	}
	sp->gam0_h[N] = N * K;
	gpos[(size_t)N * K] = B[N];
	sp->band = (int)env_int(getenv("INSTRUCT_ZQ_SPEC_BAND"), sp->band, 0, 512);
	sp->rounds = (int)env_int(getenv("INSTRUCT_ZQ_SPEC_ROUNDS"), sp->rounds, 0, 16);
	sp->ksig = (float)env_double(getenv("INSTRUCT_ZQ_SPEC_KSIG"), sp->ksig, 1.0);
	sp->walk.seg_groups = (int)env_int(getenv("INSTRUCT_ZQ_SPEC_SEG"), 16384, 64, INT_MAX);
	sp->walk.kwin = env_double(getenv("INSTRUCT_WALK_K"), sp->walk.kwin, 1.0);
	walk_read_trim_env(sp->walk);
	sp->test_abort = (int)env_int(getenv("INSTRUCT_ZQ_SPEC_TEST_ABORT"), 0);
	sp->list_cap = 6 * N + 1024;
	*out = sp; /* the context owns it from here on, whatever fails below */
	HIPCHK(sp->d_gam0.alloc((size_t)N + 1));
	HIPCHK(sp->d_gpos.alloc((size_t)N * K + 1));
	HIPCHK(sp->d_B.alloc((size_t)N + 1));
	HIPCHK(sp->d_offs.alloc((size_t)N + 1));
	HIPCHK(sp->d_alo.alloc((size_t)N * K));
	HIPCHK(sp->d_ahi.alloc((size_t)N * K));
	sp->zstrip = env_flag(getenv("INSTRUCT_ZEXPECT_STRIP"), false);
	HIPCHK(sp->d_list.alloc((size_t)sp->list_cap));
	HIPCHK(sp->d_dev.alloc(1));
	HIPCHK(sp->d_rs.alloc(1));
	HIPCHK(hipMemcpy(sp->d_gam0, sp->gam0_h.data(), sizeof(int) * ((size_t)N + 1), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(sp->d_gpos, gpos.data(), sizeof(unsigned long long) * gpos.size(), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(sp->d_B, B.data(), sizeof(unsigned long long) * B.size(), hipMemcpyHostToDevice));
	return 0;
}

/* what update_ZQ's look brings back (the mailbox's slot MAIL_ZQ) */
struct MailZQ {
	struct { unsigned done, fail; unsigned long long total; } r;
	WkState st;
	SpecDev dev;
	unsigned err[4];
};
static_assert(sizeof(MailZQ) <= MAIL_RATIOS - MAIL_ZQ, "update_ZQ's slot of the mailbox");

static WalkInputs spec_inputs(const SpecCtx *sp, isg_wh base)
{
	WalkInputs in;
	in.gam0 = sp->d_gam0; in.gpos = sp->d_gpos; in.gcnt = nullptr; in.alo = sp->d_alo; in.ahi = sp->d_ahi; in.base = base;
	return in;
}
/* The part of a sweep that takes no stream position: whether the path runs at all this sweep, the plan, the state words zeroed, qq saved,
 * the intervals of shapes and the windows' centres (WkCenterArgs has no base).  It is valid for the coming sweep only.  *ready = false: the
 * interval path sits this sweep out.  update_G's look runs it ahead (spec_ZQ_prologue_ahead); walk_prepare may wait for the stream. */
template <class LE>
static int spec_ZQ_prologue(isg_ctx *c, SpecCtx *sp, LE launch_expect, bool second, bool *ready)
{
	*ready = false;
	if (!second && sp->cooldown > 0) { sp->cooldown--; return 0; }
	const int N = sp->N, K = sp->K;
	WalkRun &w = sp->walk;
	bool ok = false;
	if (walk_prepare(c, w, sp->gam0_h.data(), N, WK_MODE_INTERVAL, false, &ok, 160)) return 1; /* (a later round may enter a segment this far from where the first walk did) */
	if (!ok) { sp->cooldown = 1 << 30; return 0; }
	if (!second) sp->sweeps++;
	HIPCHK(hipMemsetAsync(w.d_st, 0, sizeof(WkState), c->stream));
	HIPCHK(hipMemsetAsync(sp->d_dev, 0, sizeof(SpecDev), c->stream));
	HIPCHK(hipMemsetAsync(sp->d_rs, 0, sizeof(ResolveState), c->stream));
	HIPCHK(hipMemcpyAsync(c->d_qqsave, c->d.qq, sizeof(double) * (size_t)N * K, hipMemcpyDeviceToDevice, c->stream));
	prof_begin(c);
	launch_expect(sp->d_alo, sp->d_ahi);
	prof_end(c, "k_zexpect");
	isg_wh nobase;
	nobase.s1 = nobase.s2 = nobase.s3 = 0;
	walk_launch_centers(c, w, spec_inputs(sp, nobase), "k_wk_centers_Z");
	HIPCHK(hipGetLastError());
	*ready = true;
	return 0;
}

/* launch_expect(alo, ahi) / launch_probe(grid) / launch_at(): the ploidy's kernels.  *done = false: nothing is changed (qq restored),
 * the caller takes its other paths.  pro_done: the prologue of this sweep ran ahead (c->zq_pro_ready: what it found). */
template <class LE, class LP, class LA>
static int spec_update_ZQ_once(isg_ctx *c, SpecCtx *sp, isg_wh base, bool *done, LE launch_expect, LP launch_probe, LA launch_at, bool second, bool *again, bool pro_done)
{
	*done = false;
	*again = false;
	if (!sp) return 0;
	bool ready = pro_done && c->zq_pro_ready;
	if (!pro_done && spec_ZQ_prologue(c, sp, launch_expect, second, &ready)) return 1;
	if (!ready) return 0;
	const int N = sp->N, K = sp->K;
	WalkRun &w = sp->walk;
	const WalkInputs in = spec_inputs(sp, base);
	const int nseg = (int)w.plan.seg.size();
	for (int s = 0; s < nseg; s++) {
		walk_launch_tables(c, w, in, s, "k_wk_table_Z");
		walk_launch_walk(c, w, in, s, 0, 0, "k_wk_walk_Z");
	}
	/* three-launch walk: the first launch of a second walk zeroes the list counters and the state's per-walk tail itself (it runs behind
	 * k_zq_probe, which reads the counters, and ahead of k_wk_down and k_zs_band, which add to both); before the sweep's first k_zs_band the
	 * prologue's memset of all of SpecDev still holds, nothing has written it since */
	const bool fused = walk_fused(w);
	WalkZero zero;
	zero.words = (unsigned *)sp->d_dev.get(); zero.n = 2; zero.tail = true;
	auto list_on_path = [&]() { /* the uncertain bytes on the current trajectory (band = 0) */
		if (!fused) (void)hipMemsetAsync(sp->d_dev, 0, 2 * sizeof(unsigned), c->stream);
		const long nthr = (long)N * (2 * sp->band + 1);
		prof_begin(c);
		hipLaunchKernelGGL(k_zs_band, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, c->stream, (const WkBlock *)w.d_blk, (const WkSeg *)w.d_seg, nseg, (const unsigned char *)w.d_table,
				   (const WkState *)w.d_st, (const unsigned long long *)w.d_T, N, sp->band, sp->d_list, sp->list_cap, sp->d_dev);
		prof_end(c, "k_zs_band");
	};
	auto round = [&]() { /* probe them, walk again over the patched tables (origins kept) */
		prof_begin(c);
		launch_probe(1024);
		prof_end(c, "k_zq_probe");
		if (!fused) (void)hipMemsetAsync((char *)w.d_st.get() + offsetof(WkState, sum_d), 0, sizeof(WkState) - offsetof(WkState, sum_d), c->stream);
		for (int s = 0; s < nseg; s++) walk_launch_walk(c, w, in, s, 0, 1, "k_wk_walk_Z", (fused && s == 0) ? &zero : nullptr);
		list_on_path();
	};
	auto finish = [&]() {
		prof_begin(c);
		hipLaunchKernelGGL(k_zs_offs, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long *)w.d_T, (const unsigned long long *)sp->d_B, N, (const WkState *)w.d_st,
				   (const SpecDev *)sp->d_dev, sp->d_offs, sp->d_rs);
		prof_end(c, "k_zs_offs");
		prof_begin(c);
		launch_at();
		prof_end(c, "k_zq_at");
	};
	list_on_path();
	for (int r = 0; r < sp->rounds; r++) round();
	finish(); /* (does nothing if the trajectory still holds uncertain bytes) */
	HIPCHK(hipGetLastError());
	MailZQ *m = mail_slot<MailZQ>(c, MAIL_ZQ);
	auto look = [&]() -> int { /* the four answers into the look's slot, its event behind them */
		HIPCHK(hipMemcpyAsync(&m->r, &sp->d_rs.get()->done, sizeof(m->r), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipMemcpyAsync(&m->st, w.d_st, sizeof(m->st), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipMemcpyAsync(&m->dev, sp->d_dev, sizeof(m->dev), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipMemcpyAsync(m->err, c->d_err, sizeof(m->err), hipMemcpyDeviceToHost, c->stream));
		return look_record(c, AH_LOOK_ZQ);
	};
	if (look()) return 1;
	/* launch-ahead: if the blind rounds settled it, Z is final behind k_zq_at and cal_lkh's sweep (it does not read alpha) may as well run now */
	bool lkh_early = false;
	if (c->la_on && lkh_sweep_is_generic(c)) {
		if (launch_lkh_sweep(c)) return 1;
		lkh_early = true;
	}
	if (look_wait(c, AH_LOOK_ZQ)) return 1;
	for (int extra = 0; extra < 12 && !m->st.fail && !m->dev.overflow && m->dev.nlist != 0u; extra++) { /* not settled yet: round by round, looking each time */
		lkh_early = false; /* (it saw a Z that k_zq_at had not written) */
		round();
		finish();
		HIPCHK(hipGetLastError());
		if (look() || look_wait(c, AH_LOOK_ZQ)) return 1;
	}
	const auto hr = m->r;
	const WkState hs = m->st;
	const SpecDev hd = m->dev;
	unsigned err[4] = {m->err[0], m->err[1], m->err[2], m->err[3]};
	sp->last_probes = hd.nprobes;
	sp->last_rounds = hd.rounds;
	sp->last_fail = hs.fail | (hd.overflow ? 16u : 0u) | ((err[0] & sp->err_bit) ? 32u : 0u) | (hd.nlist ? 64u : 0u);
	bool good = hr.done && !hr.fail && !(err[0] & sp->err_bit);
	if (sp->test_abort > 0 && --sp->test_abort == 0) good = false; /* (tests: INSTRUCT_ZQ_SPEC_TEST_ABORT=n loses the n-th sweep) */
	walk_adapt(w, hs);
	if (!good) {
		if (err[0] & sp->err_bit) { /* only this path's bit: whatever else is pending stays */
			err[0] &= ~sp->err_bit;
			HIPCHK(hipMemcpyAsync(c->d_err, err, sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
		}
		HIPCHK(hipMemcpyAsync(c->d.qq, c->d_qqsave, sizeof(double) * (size_t)N * K, hipMemcpyDeviceToDevice, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		sp->lost_fail |= sp->last_fail;
		if (!second && (hs.fail & 1u) && !(hs.fail & ~1u)) { /* only a window was missed: once more with the wider windows walk_adapt has just set */
			*again = true;
			return 0;
		}
		sp->lost++;
		/* a first loss after a clean stretch costs nothing more; losses in a row: sit out 1, 2, 4 .. 64 sweeps */
		sp->cooldown = sp->backoff;
		sp->backoff = sp->backoff ? (sp->backoff < 64 ? sp->backoff * 2 : 64) : 1;
		return 0;
	}
	if (hd.nprobes > (unsigned)(2 * N)) sp->cooldown = 2; /* it worked, but the probes cost more than the block resolver would have */
	sp->backoff = 0;
	sp->done++;
	host_advance(c, hr.total);
	c->h_qq = false;
	if (lkh_early) ahead_set(&c->ah, AH_LKH);
	*done = true;
	return 0;
}

template <class LE, class LP, class LA>
static int spec_update_ZQ_with(isg_ctx *c, SpecCtx *sp, isg_wh base, bool *done, LE launch_expect, LP launch_probe, LA launch_at, bool pro_done = false)
{
	bool again = false;
	if (spec_update_ZQ_once(c, sp, base, done, launch_expect, launch_probe, launch_at, false, &again, pro_done)) return 1;
	if (!again) return 0;
	sp->retried++;
	return spec_update_ZQ_once(c, sp, base, done, launch_expect, launch_probe, launch_at, true, &again, false);
}

template <int KMAX>
static void spec_launch_expect(isg_ctx *c, SpecCtx *sp, float *alo, float *ahi)
{
	if constexpr (KMAX > ISG_KCAP) {
		hipLaunchKernelGGL(k_zexpect_w, dim3((unsigned)c->cfg.N, (unsigned)((c->cfg.K + ISG_ZX_WCH - 1) / ISG_ZX_WCH)), dim3(256), 0, c->stream, c->d, c->alpha, sp->ksig, alo, ahi);
	} else {
		constexpr int MI = KMAX <= 8 ? 4 : KMAX <= 16 ? 2 : 1; /* individuals per workgroup: 2 MI KMAX accumulators + MI KMAX weights per lane */
		hipLaunchKernelGGL((k_zexpect<KMAX, MI>), dim3((unsigned)((c->cfg.N + MI - 1) / MI)), dim3(256), 0, c->stream, c->d, c->alpha, sp->ksig, alo, ahi);
	}
}
template <int KMAX>
static void spec_launch_probe(isg_ctx *c, SpecCtx *sp, isg_wh base, int grid)
{
	hipLaunchKernelGGL((k_zq_probe<256, KMAX>), dim3(grid), dim3(256), 0, c->stream, c->d, base, c->alpha, (const unsigned long long *)sp->d_B, (const SpecProbe *)sp->d_list,
			   sp->d_dev, sp->list_cap, sp->walk.d_table);
}
template <int KMAX>
static void spec_launch_at(isg_ctx *c, SpecCtx *sp, isg_wh base)
{
	hipLaunchKernelGGL((k_zq_at<256, KMAX>), dim3(c->cfg.N), dim3(256), 0, c->stream, c->d, base, c->alpha, (const ResolveState *)sp->d_rs, (const unsigned long long *)sp->d_offs);
}
static int spec_update_ZQ(isg_ctx *c, SpecCtx *sp, isg_wh base, bool *done, bool pro_done)
{
	const int K = c->cfg.K;
	return spec_update_ZQ_with(c, sp, base, done,
				   [&](float *alo, float *ahi) { kdispatch(KL_ZQ(), K, [&](auto km) { spec_launch_expect<decltype(km)::value>(c, sp, alo, ahi); }); },
				   [&](int grid) { kdispatch(KL_ZQ(), K, [&](auto km) { spec_launch_probe<decltype(km)::value>(c, sp, base, grid); }); },
				   [&]() { kdispatch(KL_ZQ(), K, [&](auto km) { spec_launch_at<decltype(km)::value>(c, sp, base); }); }, pro_done);
}
/* launch-ahead behind update_G's look (isg_iteration, diploid replay chains): the coming sweep's prologue, enqueued before the stream position
 * of update_ZQ is known.  isg_update_ZQ takes AH_EXPECT and starts at the tables. */
static int spec_ZQ_prologue_ahead(isg_ctx *c, SpecCtx *sp)
{
	const int K = c->cfg.K;
	c->d.tape = nullptr; /* (as isg_update_ZQ leaves the view before it comes here) */
	c->d.tape_len = 0;
	bool ready = false;
	if (spec_ZQ_prologue(c, sp, [&](float *alo, float *ahi) { kdispatch(KL_ZQ(), K, [&](auto km) { spec_launch_expect<decltype(km)::value>(c, sp, alo, ahi); }); }, false, &ready)) return 1;
	c->zq_pro_ready = ready;
	ahead_set(&c->ah, AH_EXPECT);
	return 0;
}
