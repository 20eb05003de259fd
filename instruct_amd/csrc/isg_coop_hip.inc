/* ------------------------------------------------------------------------------------------ */
/* k_zq_coop: update_ZQ, replay schedule, several workgroups per individual                      */
/* ------------------------------------------------------------------------------------------ */
/*
 * In the replay schedule individual i+1 starts where individual i's Dirichlet stopped, so the
 * individuals are processed in order; what CAN be spread out is one individual's loci.  G workgroups
 * (one locus per lane) all work on the same individual: each draws the Z of its loci from the uniform
 * tape at the individual's start offset, counts its buckets and publishes the counts; every workgroup
 * collects all of them and draws the Dirichlet itself (same inputs, same consumption), so each knows where
 * the next individual starts without being told: one exchange per individual.
 *
 * Hand-offs are single naturally aligned 8-byte words that carry their own tag (16 bits derived from
 * the individual's index), written with one agent-scope store and polled with agent-scope loads
 * (MI355X_MICROARCH.md, "data-tagged granules"): no separate flag, no fence ordering to get wrong.
 *   gran[slot][g][w] = counts 3w..3w+2 (16 bits each) | tag(16)  workgroup (or wave) g -> everybody
 * Nobody runs more than one individual ahead of anybody else (the next offset needs everybody's
 * counts), so a ring of 4 slots suffices.  Every spin is bounded and watches a common abort word.
 */
#include "isg_coop_layout.h"
struct CoopBuf {
	unsigned long long gran[ISG_COOP_RING][ISG_COOP_GMAX * ISG_COOP_WMAX];
	unsigned abort_flag;
	unsigned overflow_flag;
	unsigned long long xcc[ISG_COOP_GMAX]; /* which XCD each workgroup runs on (tagged), for the same-XCD fast path */
};
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p)
{
	return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned long long *p, unsigned long long v)
{
	__hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
/* store that stays in the XCD's L2 (no write-through to the memory side): visible to agent-scope loads of
 * workgroups on the SAME XCD only -- used after the workgroups have established that they share one */
__device__ __forceinline__ void st_xcd(unsigned long long *p, unsigned long long v)
{
	__hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ unsigned xcc_id()
{
	unsigned x;
	asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
	return x & 0xfu;
}
/*
 * isg_rgamma2_try (random.c:195-231) for the cooperative kernels' critical path.  The two logarithms only feed the
 * accept / reject decision  c3 log(u1) - log(w) + w >= 1 ; evaluated with single precision logarithms the sign of
 * (that - 1) is certain outside a band of 2e-6 (1 + |terms|) -- v_log_f32 is good to 1 ulp, the float image of the
 * argument to 6e-8 -- and inside the band (or for non-finite intermediates) the double precision expression
 * decides.  Same return value, same consumption as isg_rgamma2_try in every case.
 */
__device__ __forceinline__ double rgamma1_try_pre(double u0, double u1, double alpha) /* isg_rgamma1_try, uniforms drawn */
{
	double r, x;
	if (u0 > ISG_E / (alpha + ISG_E)) {
		r = -isg_log((alpha + ISG_E) * (1 - u0) / (alpha * ISG_E));
		if (u1 > isg_pow(r, alpha - 1)) return -1;
		return r;
	}
	x = (alpha + ISG_E) * u0 / ISG_E;
	r = isg_pow(x, 1 / alpha);
	if (u1 > isg_exp(-r)) return -1;
	return r;
}
/* pu0, pu1: the first two uniforms, already drawn from *c */
__device__ __forceinline__ double rgamma2_try_dev(isg_cursor *c, double pu0, double pu1, double alpha)
{
	double u1, u2, c1, c2, c3, c4, c5, w;
	c1 = alpha - 1;
	c2 = (alpha - 1 / (6 * alpha)) / c1;
	c3 = 2 / c1;
	c4 = c3 + 2;
	c5 = 1 / isg_sqrt(alpha);
	u1 = pu0;
	u2 = pu1;
	if (alpha > 2.5) u1 = u2 + c5 * (1 - 1.86 * u1);
	while ((u1 >= 1) || (u1 <= 0)) {
		u1 = isg_cur_next(c);
		u2 = isg_cur_next(c);
		if (alpha > 2.5) u1 = u2 + c5 * (1 - 1.86 * u1);
	}
	w = c2 * u2 / u1;
	if ((c3 * u1 + w + 1 / w) > c4) {
		const float l1 = __builtin_amdgcn_logf((float)u1) * 0.693147180559945f, lw = __builtin_amdgcn_logf((float)w) * 0.693147180559945f;
		const double al1 = __builtin_fabs((double)l1), alw = __builtin_fabs((double)lw);
		const double dlt = (c3 * (double)l1 - (double)lw + w) - 1;
		const double tol = 2e-6 * (__builtin_fabs(c3) * (1.0 + al1) + 1.0 + alw) + 1e-12 * __builtin_fabs(w);
		bool rej;
		if (dlt > tol) rej = true;
		else if (dlt < -tol) rej = false;
		else rej = (c3 * isg_log(u1) - isg_log(w) + w) >= 1;
		if (rej) return -1;
	}
	return c1 * w;
}

/* the calling lane polls granule *p until it carries `tag`; every spin is bounded and watches the common abort word */
__device__ __forceinline__ unsigned long long coop_poll(const unsigned long long *p, unsigned tag, CoopBuf *cb)
{
	unsigned long long v = 0;
	for (unsigned spin = 0;; spin++) {
		v = ld_agent(p);
		if ((unsigned)(v >> 48) == tag) break;
		if ((spin & 1023u) == 1023u) {
			if (__hip_atomic_load(&cb->abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
			if (spin > (1u << 24)) {
				__hip_atomic_store(&cb->abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				break;
			}
		}
		__builtin_amdgcn_s_sleep(1);
	}
	return v;
}

/*
 * Do all G workgroups of this launch run on one XCD?  (Blocks are dealt round-robin over the 8 XCDs, so the
 * launcher starts 8 G blocks of which every 8th works; this only makes it likely -- the answer comes from the
 * hardware register.)  One tagged agent-scope word per workgroup, everybody reads all of them.
 */
__device__ __forceinline__ bool coop_same_xcd(CoopBuf *cb, int g, int G, unsigned *lds_flag)
{
	const int t = threadIdx.x;
	if (t == 0) {
		*lds_flag = 1u;
		st_agent(&cb->xcc[g], (1ull << 48) | xcc_id());
	}
	__syncthreads();
	if (t < G) {
		const unsigned long long v = coop_poll(&cb->xcc[t], 1u, cb);
		if ((unsigned)(v >> 48) != 1u || (unsigned)(v & 0xfu) != xcc_id()) atomicAnd(lds_flag, 0u);
	}
	__syncthreads();
	return *lds_flag != 0u;
}

/*
 * The Dirichlet of the cooperative kernels.  Every workgroup runs it on the same counts and gets the same
 * consumption, so nobody has to be told where the next individual starts: ONE exchange (the counts) per
 * individual.  Attempts are evaluated as in dirichlet_block; the walk over the attempt table is scalar: per gamma
 * a 32-bit mask of accepted attempts and one of attempts that did not consume exactly two uniforms (a retry inside
 * the attempt, random.c:213-216), so a step is shift / find-first-set / add on SGPRs.  Shape 1 (odd consumption)
 * or a walk that leaves the table continue with the plain sequential loop from that point.
 * Called by all threads after the counts are complete in sh.hist[par]; returns the uniforms consumed.
 * `writer`: this wave stores qq[i] / qqnum[i].
 */
struct NoHook { __device__ __forceinline__ void operator()() const {} };
template <int BLOCK, int KMAX, class Hook = NoHook>
__device__ __forceinline__ unsigned dirichlet_coop(const DevView &d, ZqShared &sh, int i, const isg_wh &cur, unsigned long long dstart_off,
						  double alpha, int par, const double *dtape, bool writer, Hook hook = Hook())
{
	const int K = d.K, t = threadIdx.x, lane = (int)lane_id();
	const int *hist = sh.hist[par], *ghist = sh.ghist[par]; /* own + collected counts */
	int noff = BLOCK / K;
	if (noff > 32) noff = 32;
	if (t < K * noff) {
		const int m = t / noff, o = t - m * noff;
		const double a = (double)(hist[m] + ghist[m]) + alpha;
		isg_cursor c;
		c.used = 0;
		c.tape = dtape ? dtape + 2 * o : nullptr;
		if (!dtape) c.s = isg_wh_jump(&sh.tab, cur, dstart_off + 2ull * (unsigned)o);
		/* the attempt's first two uniforms, then whatever the caller wants in flight behind them (loads return in
		 * issue order: nothing issued from here on delays these two) */
		const double pu0 = isg_cur_next(&c), pu1 = isg_cur_next(&c);
		hook();
		double r = -1;
		if (a < 1) r = rgamma1_try_pre(pu0, pu1, a);
		else if (a > 1) r = rgamma2_try_dev(&c, pu0, pu1, a);
		else c.used = 255;
		sh.at_val[t] = r;
		sh.at_used[t] = (unsigned char)(c.used > 255 ? 255 : c.used);
		if (!(r < 0)) atomicOr(&sh.amask[par][m], 1u << o);
		if (c.used != 2) atomicOr(&sh.rmask[par][m], 1u << o);
	}
	else hook();
	if (t < KMAX) { /* the other parity's buffers: last read before the previous two barriers */
		sh.hist[par ^ 1][t] = 0;
		sh.ghist[par ^ 1][t] = 0;
		sh.amask[par ^ 1][t] = 0;
		sh.rmask[par ^ 1][t] = 0;
	}
	lds_barrier();
	STAMP(i, 4);
	/* every wave walks for itself (wave-uniform state) */
	const unsigned am = (lane < K) ? sh.amask[par][lane] : 0u, rm = (lane < K) ? sh.rmask[par][lane] : 0u;
	unsigned o = 0, my_o = 0;
	int m = 0;
	{ /* the common case straight-line: per gamma the first attempt at or after o that is accepted, none irregular */
		unsigned fo = 0, fmy = 0;
		bool bad = false;
#pragma unroll
		for (int mm = 0; mm < KMAX; mm++) {
			if (mm < K) {
				const unsigned A = (unsigned)__builtin_amdgcn_readlane((int)am, mm), I = (unsigned)__builtin_amdgcn_readlane((int)rm, mm);
				const unsigned rest = (fo < 32u) ? ((A | I) >> fo) : 0u;
				const unsigned e = fo + (rest ? (unsigned)__builtin_ctz(rest) : 0u);
				bad |= (rest == 0u) || (((I >> (e & 31u)) & 1u) != 0u) || (e >= (unsigned)noff);
				fmy = (lane == mm) ? e : fmy;
				fo = e + 1u;
			}
		}
		if (!bad) {
			o = fo;
			my_o = fmy;
			m = K;
		}
	}
	while (m < K) {
		const unsigned A = (unsigned)__builtin_amdgcn_readlane((int)am, m), I = (unsigned)__builtin_amdgcn_readlane((int)rm, m);
		if (o >= (unsigned)noff) break;
		const unsigned rest = (A | I) >> o; /* the attempts before the first set bit are plain rejections: 2 uniforms each */
		if (rest == 0) break;
		const unsigned e = o + (unsigned)__builtin_ctz(rest);
		unsigned step = 1;
		if ((I >> e) & 1u) { /* a retry inside the attempt (random.c:213-216) or shape 1: consumption from the table */
			const unsigned u = sh.at_used[m * noff + (int)e];
			if (u == 255u || (u & 1u)) break;
			step = u >> 1;
		}
		o = e + step;
		if ((A >> e) & 1u) {
			my_o = (lane == m) ? e : my_o;
			m++;
		}
	}
	unsigned used = 2u * o;
	const bool ok = (m == K);
	double v = (lane < m) ? sh.at_val[lane * noff + (int)my_o] : 0.0;
	if (!ok) { /* wave-uniform and the same in every wave: continue sequentially from (gamma m, offset 2 o) */
		if (t < 64) {
			if (lane < m) sh.gval[lane] = v;
			if (t == 0) {
				isg_cursor c;
				c.s = isg_wh_jump(&sh.tab, cur, dstart_off + 2ull * o);
				c.used = 0;
				c.tape = nullptr;
				for (int mm = m; mm < K; mm++) sh.gval[mm] = isg_rgamma(&c, (double)(hist[mm] + ghist[mm]) + alpha);
				sh.used_total = 2ull * o + c.used;
			}
		}
		lds_barrier();
		used = (unsigned)sh.used_total;
		if (lane < K) v = sh.gval[lane];
		lds_barrier(); /* gval / used_total are rewritten by the next fallback only after this */
	}
	STAMP(i, 5);
	if (writer) { /* qq[i] = g / sum with the sum taken in stream order (random.c:272-279) */
		double sum = 0;
		for (int k2 = 0; k2 < K; k2++) sum += readlane_f64(v, k2);
		if (lane < K) {
			d.qq[(size_t)i * K + lane] = v / sum;
			d.qqnum[(size_t)i * K + lane] = hist[lane] + ghist[lane];
		}
	}
	return used;
}

template <int KMAX>
__global__ void __launch_bounds__(256) k_zq_coop(DevView d, isg_wh base, int init_flag, double alpha, CoopBuf *cb, uint64_t *pos_out, int xcd_pack)
{
	constexpr int BLOCK = 256;
	constexpr bool PRE = (KMAX <= 8);
	__shared__ ZqShared sh;
	__shared__ unsigned same_xcd;
	if (xcd_pack && (blockIdx.x & 7)) return; /* every 8th block works: one XCD under round-robin placement */
	const int t = threadIdx.x, g = xcd_pack ? blockIdx.x >> 3 : blockIdx.x, G = xcd_pack ? gridDim.x >> 3 : gridDim.x, K = d.K;
	{
		const uint16_t *src = (const uint16_t *)d.tab;
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
	const bool local = xcd_pack && coop_same_xcd(cb, g, G, &same_xcd);
	const isg_wh cur = isg_wh_jump(&sh.tab, base, 0);
	unsigned long long off = 0; /* offset of the current individual: every workgroup derives it for itself */
	const int stride = G * BLOCK;
	const size_t rowb = (size_t)d.Lp * 2;
	const bool writer = (g == 0) && (t >= BLOCK - 64);
	const CoopLayout lay = coop_layout(G, BLOCK, K, d.Lp, 2); /* isg_coop_layout.h */
	const bool wmode = lay.wmode;
	const int pack = lay.pack, bits = lay.bits, W = lay.W;
	double icum[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) icum[m] = (m < K) ? (double)(m + 1) / K : 0.0; /* mcmc.c:1144 */
	double touch = 0.0, touch2 = 0.0;
	/* position independent data of the lane's upcoming locus, loaded one step ahead */
	unsigned pa0 = 0xff, pa1 = 0xff, prw = 0;
	float pF0[KMAX], pF1[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) pF0[m] = pF1[m] = 0.f;
	unsigned na0 = 0xff, na1 = 0xff, nrw = 0; /* the NEXT individual's first locus (one step further ahead) */
	auto fetch_geno = [&](int ni, int nj, unsigned &b0, unsigned &b1, unsigned &rw) {
		b0 = b1 = 0xff;
		rw = 0;
		if (ni < d.N && nj < d.Lp) {
			const unsigned short gg = *(const unsigned short *)(d.geno + (size_t)ni * rowb + (size_t)nj * 2);
			b0 = gg & 0xff;
			b1 = gg >> 8;
			rw = d.rankwave[(size_t)ni * d.nwv + (nj >> 6)];
		}
	};
	auto fetch_rows = [&](int nj) {
		if (pa0 != 0xff && PRE && !init_flag) {
			const float *P0 = d.freqf + ((size_t)nj * d.Amax + pa0) * d.KPF, *P1 = d.freqf + ((size_t)nj * d.Amax + pa1) * d.KPF;
#pragma unroll
			for (int m = 0; m < KMAX; m += 4) {
				if (m < K) {
					const float4 f0 = *(const float4 *)(P0 + m), f1 = *(const float4 *)(P1 + m);
					pF0[m] = f0.x; pF1[m] = f1.x;
					if (m + 1 < KMAX) { pF0[m + 1] = f0.y; pF1[m + 1] = f1.y; }
					if (m + 2 < KMAX) { pF0[m + 2] = f0.z; pF1[m + 2] = f1.z; }
					if (m + 3 < KMAX) { pF0[m + 3] = f0.w; pF1[m + 3] = f1.w; }
				}
			}
		}
	};
	fetch_geno(0, g * BLOCK + t, pa0, pa1, prw);
	fetch_rows(g * BLOCK + t);
	int pnvalid = d.nvalid[0];
	double pq[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) pq[m] = (m < K && !init_flag) ? d.qq[m] : 0.0;
	for (int i = 0; i < d.N; i++) {
		const unsigned tag = (unsigned)(i % 65535) + 1u;
		const int slot = i & (ISG_COOP_RING - 1), par = i & 1;
		if (touch2 == -1.0 || touch == -1.0) cb->overflow_flag = 2; /* consumes last individual's cache warming loads */
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
		STAMP(i, 0);
		const unsigned long long offi = off;
		const bool covered = offi + 2ull * (unsigned)nvalid + 1024ull <= d.tape_len;
		/* Loads return in issue order, so everything that is only needed later is issued BEHIND the loads the
		 * critical path waits for: the uniforms first, then the warm-up of the Dirichlet's stretch and the next
		 * individual's data. */
		for (int j = g * BLOCK + t; j - t < d.Lp; j += stride) { /* wave-uniform trip count */
			const unsigned a0 = pa0, a1 = pa1;
			const bool valid = (a0 != 0xff);
			const unsigned long long vm = __ballot(valid);
			const unsigned rank = prw + (unsigned)__popcll(vm & ((1ull << lane_id()) - 1ull));
			float F0[KMAX], F1[KMAX];
#pragma unroll
			for (int m = 0; m < KMAX; m++) { F0[m] = pF0[m]; F1[m] = pF1[m]; }
			double x0 = 0, x1 = 0;
			if (valid && covered) {
				x0 = d.tape[offi + 2ull * rank];
				x1 = d.tape[offi + 2ull * rank + 1];
			}
#ifdef ISG_EXP_XWAIT
			STAMP(i, 2);
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			STAMP(i, 3);
#endif
			if (j - t == g * BLOCK) { /* first pass */
				if (covered && t < 10) touch = d.tape[offi + 2ull * (unsigned)nvalid + 16u * (unsigned)t]; /* one lane per 128-byte line */
				fetch_geno(i + 1, g * BLOCK + t, na0, na1, nrw);
				if (i + 1 < d.N) {
					pnvalid = d.nvalid[i + 1];
#pragma unroll
					for (int m = 0; m < KMAX; m++) pq[m] = (m < K && !init_flag) ? d.qq[(size_t)(i + 1) * K + m] : 0.0;
				}
			}
			const bool more = (j - t + stride < d.Lp);
			if (more) { /* a further pass of this individual */
				fetch_geno(i, j + stride, pa0, pa1, prw);
				fetch_rows(j + stride);
			}
			int z0 = 0xff, z1 = 0xff;
			STAMP(i, 6);
			if (valid && covered) {
				if (init_flag) {
					z0 = bucket_fast<KMAX>(x0, icum, 1.0, K);
					z1 = bucket_fast<KMAX>(x1, icum, 1.0, K);
				} else {
					bool amb0 = true, amb1 = true;
					if (PRE) {
						z0 = bucket_f32<KMAX>((float)x0, F0, qf, K, &amb0);
						z1 = bucket_f32<KMAX>((float)x1, F1, qf, K, &amb1);
					}
					if (amb0) {
						double cum[KMAX];
						double tot = weights<KMAX>(d.freq + ((size_t)j * d.Amax + a0) * d.KP, q, cum, K);
						z0 = bucket_fast<KMAX>(x0, cum, tot, K);
					}
					if (amb1) {
						double cum[KMAX];
						double tot = weights<KMAX>(d.freq + ((size_t)j * d.Amax + a1) * d.KP, q, cum, K);
						z1 = bucket_fast<KMAX>(x1, cum, tot, K);
					}
				}
			}
			STAMP(i, 7);
#pragma unroll
			for (int m = 0; m < KMAX; m++)
				if (m < K) wcnt[m] += __popcll(__ballot(z0 == m)) + __popcll(__ballot(z1 == m));
			if (j < d.Lp) *(unsigned short *)(d.z + (size_t)i * rowb + (size_t)j * 2) = (unsigned short)(z0 | (z1 << 8));
		}
		STAMP(i, 1);
		if (wmode) { /* few workgroups: every wave hands its counts over itself, no reduction inside the workgroup first */
			unsigned long long v = (unsigned long long)tag << 48;
#pragma unroll
			for (int m = 0; m < KMAX; m++)
				if (m < K && (int)lane_id() == m / 3) v |= (unsigned long long)(wcnt[m] & 0xffff) << (16 * (m % 3));
			if ((int)lane_id() < W) { if (local) st_xcd(&cb->gran[slot][(g * (BLOCK / 64) + (t >> 6)) * W + (int)lane_id()], v); else st_agent(&cb->gran[slot][(g * (BLOCK / 64) + (t >> 6)) * W + (int)lane_id()], v); }
		} else {
			if (lane_id() == 0) {
#pragma unroll
				for (int m = 0; m < KMAX; m++)
					if (m < K && wcnt[m]) atomicAdd(&sh.hist[par][m], wcnt[m]);
			}
			lds_barrier();
			/* this workgroup's counts leave; everybody else's are collected */
			if (t < W) { /* `pack` counts of `bits` bits per word */
				unsigned long long v = (unsigned long long)tag << 48;
				for (int c3 = 0; c3 < pack; c3++)
					if (pack * t + c3 < K) v |= (unsigned long long)(sh.hist[par][pack * t + c3] & ((1 << bits) - 1)) << (bits * c3);
				if (local) st_xcd(&cb->gran[slot][g * W + t], v); else st_agent(&cb->gran[slot][g * W + t], v);
			}
		}
#ifndef ISG_EXP_XWAIT
		STAMP(i, 2);
#endif
		/* while they travel: the frequency rows of the next individual's first locus (its genotype bytes arrived
		 * during the draws) and a touch of the tape lines it will read */
		pa0 = na0; pa1 = na1; prw = nrw;
		fetch_rows(g * BLOCK + t);
		if (covered && i + 1 < d.N && lane_id() < 10) touch2 = d.tape[offi + 2ull * (unsigned)nvalid + 2ull * prw + 16u * lane_id()];
		if (!covered && t == 0) cb->overflow_flag = 1;
		const int ngran = lay.ngran;
		for (int gi = t; gi - t < ngran; gi += BLOCK) { /* wave-uniform trip count */
			if (gi < ngran && (wmode || gi / W != g)) {
				const unsigned long long v = coop_poll(&cb->gran[slot][gi], tag, cb);
				const int w = gi % W;
				for (int c3 = 0; c3 < pack; c3++) {
					const int m = pack * w + c3;
					const int c = (int)((v >> (bits * c3)) & ((1 << bits) - 1));
					if (m < K && c) atomicAdd(&sh.ghist[par][m], c);
				}
			}
		}
		lds_barrier();
#ifndef ISG_EXP_XWAIT
		STAMP(i, 3);
#endif
		const unsigned used = 2u * (unsigned)nvalid +
			dirichlet_coop<BLOCK, KMAX>(d, sh, i, cur, offi + 2ull * (unsigned)nvalid, alpha, par,
						    covered ? d.tape + offi + 2ull * (unsigned)nvalid : nullptr, writer);
		off += used;
	}
	if (g == 0 && t == 0) *pos_out = off;
}

/*
 * The Dirichlet of k_zq_spec (K <= 8): every WAVE evaluates the attempt table for itself -- lane (m, d) the attempt of
 * gamma m at stream offset m + d (gamma m cannot start before m earlier gammas took an attempt each; 64 / K offsets
 * per gamma) -- and gets the accepted / irregular masks from two ballots, so the walk needs no LDS round trip and no
 * barrier.  Walks that leave the table (1 % at K = 5) are redone sequentially by lane 0 of each wave.
 * Counts: sh.hist3[buf] + sh.ghist3[buf]; the caller's barrier made them complete.
 */
/* cntf(m) = the individual's count of cluster m; tab = the skip-ahead tables (LDS) */
template <int KMAX, class CntF>
__device__ __forceinline__ unsigned dirichlet_wave_f(const DevView &d, const isg_wh_tables *tab, CntF cntf, int i, const isg_wh &cur, unsigned long long dstart_off,
						    double alpha, const double *dtape, bool writer, bool pre = false, double ppu0 = 0.0, double ppu1 = 0.0)
{
	const int K = d.K, lane = (int)lane_id(), D = 64 / K;
	const int m = (lane < K * D) ? lane / D : K - 1, dd = lane - m * D;
	const bool act = lane < K * D;
	const int cnt = cntf(m);
	const double a = (double)cnt + alpha;
	isg_cursor c;
	c.used = 0;
	c.tape = dtape ? dtape + 2 * (m + dd) : nullptr;
	if (!dtape) c.s = isg_wh_jump(tab, cur, dstart_off + 2ull * (unsigned)(m + dd));
	double r = -1;
	if (act) {
		double pu0, pu1;
		if (pre && dtape) { /* the caller fetched this lane's first two uniforms (dtape[2 (m + dd)], [.. + 1]) ahead of time */
			pu0 = ppu0;
			pu1 = ppu1;
			c.used = 2;
		} else {
			pu0 = isg_cur_next(&c);
			pu1 = isg_cur_next(&c);
		}
		if (a < 1) r = rgamma1_try_pre(pu0, pu1, a);
		else if (a > 1) r = rgamma2_try_dev(&c, pu0, pu1, a);
		else c.used = 255; /* shape 1: odd consumption */
	}
	const unsigned long long A = __ballot(act && !(r < 0)), I = __ballot(act && c.used != 2);
	const unsigned dmask = (D >= 32) ? 0xffffffffu : ((1u << D) - 1u);
	unsigned fo = 0; /* attempts consumed so far = stream offset / 2 */
	bool bad = false;
	double v = 0.0;  /* lane mm < K ends up with gamma mm's value */
#pragma unroll
	for (int mm = 0; mm < KMAX; mm++) {
		if (mm < K) {
			const unsigned Am = (unsigned)(A >> (mm * D)) & dmask, Im = (unsigned)(I >> (mm * D)) & dmask;
			const unsigned rel = fo - (unsigned)mm; /* fo >= mm always */
			const unsigned rest = (rel < (unsigned)D) ? ((Am | Im) >> rel) : 0u;
			const unsigned e = rel + (rest ? (unsigned)__builtin_ctz(rest) : 0u);
			bad |= (rest == 0u) || (((Im >> (e & 31u)) & 1u) != 0u);
			const double val = readlane_f64(r, (mm * D + (int)(e < (unsigned)D ? e : 0u)) & 63);
			v = (lane == mm) ? val : v;
			fo = (unsigned)mm + e + 1u;
		}
	}
	unsigned used = 2u * fo;
	if (bad) { /* an irregular attempt on the path (a retry inside it: more than two uniforms): the general walk */
		const unsigned ul = (unsigned)c.used;
		unsigned go = 0;
		int gm = 0;
		bool ok = true;
		while (gm < K) {
			const unsigned Am = (unsigned)(A >> (gm * D)) & dmask, Im = (unsigned)(I >> (gm * D)) & dmask;
			const unsigned rel = go - (unsigned)gm;
			if (rel >= (unsigned)D) { ok = false; break; }
			const unsigned rest = (Am | Im) >> rel;
			if (rest == 0u) { ok = false; break; }
			const unsigned e = rel + (unsigned)__builtin_ctz(rest);
			const int idx = gm * D + (int)e;
			unsigned step = 1;
			if ((Im >> e) & 1u) {
				const unsigned u = (unsigned)__builtin_amdgcn_readlane((int)ul, idx);
				if (u == 255u || (u & 1u)) { ok = false; break; }
				step = u >> 1;
			}
			go = (unsigned)gm + e + step;
			if ((Am >> e) & 1u) {
				const double val = readlane_f64(r, idx);
				v = (lane == gm) ? val : v;
				gm++;
			}
		}
		bad = !ok;
		used = 2u * go;
	}
	if (bad) { /* wave-uniform: the plain loop from the Dirichlet's first position */
		double g[KMAX];
		unsigned u = 0;
		if (lane == 0) {
			isg_cursor q;
			q.used = 0;
			q.tape = nullptr;
			q.s = isg_wh_jump(tab, cur, dstart_off);
#pragma unroll
			for (int mm = 0; mm < KMAX; mm++) g[mm] = (mm < K) ? isg_rgamma(&q, (double)cntf(mm) + alpha) : 0.0;
			u = q.used;
		} else {
#pragma unroll
			for (int mm = 0; mm < KMAX; mm++) g[mm] = 0.0;
		}
		used = (unsigned)__builtin_amdgcn_readfirstlane((int)u);
#pragma unroll
		for (int mm = 0; mm < KMAX; mm++) {
			const double val = readlane_f64(g[mm], 0);
			v = (lane == mm) ? val : v;
		}
	}
	if (writer) { /* qq[i] = g / sum with the sum taken in stream order (random.c:272-279) */
		double sum = 0;
		for (int k2 = 0; k2 < K; k2++) sum += readlane_f64(v, k2);
		if (lane < K) {
			d.qq[(size_t)i * K + lane] = v / sum;
			d.qqnum[(size_t)i * K + lane] = cntf(lane);
		}
	}
	return used;
}
template <int KMAX>
__device__ __forceinline__ unsigned dirichlet_wave(const DevView &d, ZqShared &sh, int i, const isg_wh &cur, unsigned long long dstart_off,
						  double alpha, int buf, const double *dtape, bool writer, bool pre = false, double ppu0 = 0.0, double ppu1 = 0.0)
{
	return dirichlet_wave_f<KMAX>(d, &sh.tab, [&](int m) { return sh.hist3[buf][m] + sh.ghist3[buf][m]; }, i, cur, dstart_off, alpha, dtape, writer, pre, ppu0, ppu1);
}

/*
 * k_zq_spec: k_zq_coop with the Z draws taken off the critical path (single pass: one locus per lane, K <= 8).
 * Individual i+1 starts used_i uniforms behind the end of individual i's draws, and used_i = 2 K + 2 c where c is
 * the number of rejected gamma attempts of i's Dirichlet -- almost always 0..3.  While the counts of individual i
 * travel between the workgroups, every lane draws its two Z of individual i+1 for each of these ISG_SPEC_C start
 * positions (the running sums are shared, a candidate costs a multiply and K-1 compares per copy).  When the
 * Dirichlet of i is done the matching candidate is picked; any other consumption takes the plain path of
 * k_zq_coop for that individual.  Same Z, same counts, same consumption in every case.
 */
#ifndef ISG_SPEC_C
#define ISG_SPEC_C 6
#endif
template <int KMAX>
__global__ void __launch_bounds__(256) k_zq_spec(DevView d, isg_wh base, double alpha, CoopBuf *cb, uint64_t *pos_out, int xcd_pack)
{
	constexpr int BLOCK = 256, C = ISG_SPEC_C;
	static_assert(KMAX <= 8 && C <= 8, "pre-filter rows in registers; candidates packed 4 bits each");
	__shared__ ZqShared sh;
	__shared__ unsigned same_xcd;
	if (xcd_pack && (blockIdx.x & 7)) return; /* every 8th block works: one XCD under round-robin placement */
	const int t = threadIdx.x, g = xcd_pack ? blockIdx.x >> 3 : blockIdx.x, G = xcd_pack ? gridDim.x >> 3 : gridDim.x, K = d.K, lane = (int)lane_id();
	{
		const uint16_t *src = (const uint16_t *)d.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += BLOCK) dst[k] = src[k];
		if (t < 2 * ISG_KCAP) {
			(&sh.hist[0][0])[t] = 0;
			(&sh.amask[0][0])[t] = 0;
			(&sh.rmask[0][0])[t] = 0;
			(&sh.ghist[0][0])[t] = 0;
		}
		if (t < 3 * ISG_KCAP) {
			(&sh.hist3[0][0])[t] = 0;
			(&sh.ghist3[0][0])[t] = 0;
		}
	}
	__syncthreads();
	const bool local = xcd_pack && coop_same_xcd(cb, g, G, &same_xcd);
	const isg_wh cur = isg_wh_jump(&sh.tab, base, 0);
	unsigned long long off = 0;
	const size_t rowb = (size_t)d.Lp * 2;
	const bool writer = (g == 0) && (t >= BLOCK - 64);
	const CoopLayout lay = coop_layout(G, BLOCK, K, d.Lp, 2); /* isg_coop_layout.h */
	const bool wmode = lay.wmode;
	const int pack = lay.pack, bits = lay.bits, W = lay.W;
	const int j = g * BLOCK + t; /* this lane's locus */
	double touch = 0.0;
	/* three individuals in flight per lane: cl = the one being finished, nl = the one whose candidates are drawn,
	 * ml = the one whose data is being fetched */
	/* the individual's qq row and locus count travel as ONE vector load each (lane m holds qq[m]; they are spread
	 * with v_readlane when used): a scalar load here would sit in the same counter as the LDS traffic and stall the
	 * next LDS wait for a cold HBM access */
	struct Loc {
		unsigned a0, a1, rw;
		float F0[KMAX], F1[KMAX];
		double qv;
		int nvv;
	};
	Loc cl, nl, ml;
	auto fetch_geno = [&](int ni, Loc &L) {
		L.a0 = L.a1 = 0xff;
		L.rw = 0;
		L.nvv = 0;
		L.qv = 0.0;
		if (ni < d.N) {
			L.nvv = d.nvalid[min(ni + lane, d.N - 1)];
			if (lane < K) L.qv = d.qq[(size_t)ni * K + lane];
			if (j < d.Lp) {
				const unsigned short gg = *(const unsigned short *)(d.geno + (size_t)ni * rowb + (size_t)j * 2);
				L.a0 = gg & 0xff;
				L.a1 = gg >> 8;
				L.rw = d.rankwave[(size_t)ni * d.nwv + (j >> 6)];
			}
		}
	};
	auto fetch_rows = [&](Loc &L) {
#pragma unroll
		for (int m = 0; m < KMAX; m++) L.F0[m] = L.F1[m] = 0.f;
		if (L.a0 != 0xff) {
			const float *P0 = d.freqf + ((size_t)j * d.Amax + L.a0) * d.KPF, *P1 = d.freqf + ((size_t)j * d.Amax + L.a1) * d.KPF;
#pragma unroll
			for (int m = 0; m < KMAX; m += 4) {
				if (m < K) {
					const float4 f0 = *(const float4 *)(P0 + m), f1 = *(const float4 *)(P1 + m);
					L.F0[m] = f0.x; L.F1[m] = f1.x;
					if (m + 1 < KMAX) { L.F0[m + 1] = f0.y; L.F1[m + 1] = f1.y; }
					if (m + 2 < KMAX) { L.F0[m + 2] = f0.z; L.F1[m + 2] = f1.z; }
					if (m + 3 < KMAX) { L.F0[m + 3] = f0.w; L.F1[m + 3] = f1.w; }
				}
			}
		}
	};
	fetch_geno(0, cl);
	fetch_rows(cl);
	fetch_geno(1, nl);
	ml = nl;
	/* candidates of the individual about to be finished: buckets packed 4 bits each, ambiguity bits, base offset */
	unsigned cz0 = 0, cz1 = 0, camb = 0;
	unsigned long long cbase = 0;
	bool cvalid = false;
	for (int i = 0; i < d.N; i++) {
		const unsigned tag = (unsigned)(i % 65535) + 1u;
		const int slot = i & (ISG_COOP_RING - 1), buf = i % 3;
		if (touch == -1.0) cb->overflow_flag = 2;
		const int nvalid = __builtin_amdgcn_readfirstlane(cl.nvv), nnvalid = __builtin_amdgcn_readfirstlane(nl.nvv);
		const unsigned long long offi = off;
		const bool covered = offi + 2ull * (unsigned)nvalid + 1024ull <= d.tape_len;
		const bool valid = (cl.a0 != 0xff);
		const unsigned rank = cl.rw + (unsigned)__popcll(__ballot(valid) & ((1ull << lane) - 1ull));
		STAMP(i, 0);
		/* ---- first in the queue: the uniforms of the NEXT individual's candidates and its frequency rows ---- */
		const unsigned long long nbase = offi + 2ull * (unsigned)nvalid + 2ull * (unsigned)K; /* every gamma: >= one attempt of two uniforms */
		const bool nvalidc = (i + 1 < d.N) && (nbase + 2ull * (C - 1) + 2ull * (unsigned)nnvalid + 1024ull <= d.tape_len);
		const bool nvalidl = (nl.a0 != 0xff);
		const unsigned nrank = nl.rw + (unsigned)__popcll(__ballot(nvalidl) & ((1ull << lane) - 1ull));
		double xs[2 * C];
#pragma unroll
		for (int k = 0; k < 2 * C; k++) xs[k] = 0.5;
		if (nvalidc && nvalidl) {
			const double *tp = d.tape + nbase + 2ull * nrank;
#pragma unroll
			for (int k = 0; k < 2 * C; k++) xs[k] = tp[k];
		}
		fetch_rows(nl);
		if (covered && lane < 10) touch = d.tape[offi + 2ull * (unsigned)nvalid + 16u * (unsigned)lane]; /* this Dirichlet's stretch */
		/* ---- this individual's Z: a candidate drawn earlier, or the plain path ---- */
		const unsigned long long dc = offi - cbase;
		const bool hit = cvalid && offi >= cbase && !(dc & 1ull) && dc < 2ull * C;
		int z0 = 0xff, z1 = 0xff;
		bool amb0 = false, amb1 = false;
		if (hit) {
			const unsigned c = (unsigned)(dc >> 1);
			if (valid) {
				z0 = (int)((cz0 >> (4 * c)) & 0xfu);
				z1 = (int)((cz1 >> (4 * c)) & 0xfu);
				amb0 = (camb >> c) & 1u;
				amb1 = (camb >> (8 + c)) & 1u;
			}
		} else if (valid && covered) {
			float qf[KMAX];
#pragma unroll
			for (int m = 0; m < KMAX; m++) qf[m] = (m < K) ? (float)readlane_f64(cl.qv, m) : 0.f;
			const double x0 = d.tape[offi + 2ull * rank], x1 = d.tape[offi + 2ull * rank + 1];
			z0 = bucket_f32<KMAX>((float)x0, cl.F0, qf, K, &amb0);
			z1 = bucket_f32<KMAX>((float)x1, cl.F1, qf, K, &amb1);
		}
		if (__ballot(valid && covered && (amb0 || amb1))) { /* rare: the draw in double */
			double cum[KMAX], q[KMAX];
#pragma unroll
			for (int m = 0; m < KMAX; m++) q[m] = (m < K) ? readlane_f64(cl.qv, m) : 0.0;
			if (valid && covered && amb0) {
				const double tot = weights<KMAX>(d.freq + ((size_t)j * d.Amax + cl.a0) * d.KP, q, cum, K);
				z0 = bucket_fast<KMAX>(d.tape[offi + 2ull * rank], cum, tot, K);
			}
			if (valid && covered && amb1) {
				const double tot = weights<KMAX>(d.freq + ((size_t)j * d.Amax + cl.a1) * d.KP, q, cum, K);
				z1 = bucket_fast<KMAX>(d.tape[offi + 2ull * rank + 1], cum, tot, K);
			}
		}
		if (!covered) { z0 = z1 = 0xff; }
		int wcnt[KMAX];
#pragma unroll
		for (int m = 0; m < KMAX; m++) wcnt[m] = (m < K) ? __popcll(__ballot(z0 == m)) + __popcll(__ballot(z1 == m)) : 0;
		STAMP(i, 1);
		/* ---- counts leave ---- */
		if (wmode) {
			unsigned long long v = (unsigned long long)tag << 48;
#pragma unroll
			for (int m = 0; m < KMAX; m++)
				if (m < K && lane == m / 3) v |= (unsigned long long)(wcnt[m] & 0xffff) << (16 * (m % 3));
			if (lane < W) { if (local) st_xcd(&cb->gran[slot][(g * (BLOCK / 64) + (t >> 6)) * W + lane], v); else st_agent(&cb->gran[slot][(g * (BLOCK / 64) + (t >> 6)) * W + lane], v); }
		} else {
			if (lane == 0) {
#pragma unroll
				for (int m = 0; m < KMAX; m++)
					if (m < K && wcnt[m]) atomicAdd(&sh.hist3[buf][m], wcnt[m]);
			}
			lds_barrier();
			if (t < W) { /* `pack` counts of `bits` bits per word */
				unsigned long long v = (unsigned long long)tag << 48;
				for (int c3 = 0; c3 < pack; c3++)
					if (pack * t + c3 < K) v |= (unsigned long long)(sh.hist3[buf][pack * t + c3] & ((1 << bits) - 1)) << (bits * c3);
				if (local) st_xcd(&cb->gran[slot][g * W + t], v); else st_agent(&cb->gran[slot][g * W + t], v);
			}
		}
		if (j < d.Lp) *(unsigned short *)(d.z + (size_t)i * rowb + (size_t)j * 2) = (unsigned short)(z0 | (z1 << 8));
		STAMP(i, 2);
		if (!covered && t == 0) cb->overflow_flag = 1;
		/* ---- while they travel: the data of the individual after the next is requested (cold: it arrives under
		 * the arithmetic below, before the polling loads queue up behind it), then the next one's candidates ---- */
		fetch_geno(i + 2, ml);
		cbase = nbase;
		cvalid = nvalidc;
		cz0 = cz1 = camb = 0;
		if (nvalidc && nvalidl) {
			float qf[KMAX], cum0[KMAX], cum1[KMAX];
#pragma unroll
			for (int m = 0; m < KMAX; m++) qf[m] = (m < K) ? (float)readlane_f64(nl.qv, m) : 0.f;
			const float run0 = prefix_f32<KMAX>(nl.F0, qf, K, cum0), run1 = prefix_f32<KMAX>(nl.F1, qf, K, cum1);
#pragma unroll
			for (int c = 0; c < C; c++) {
				bool a0, a1;
				const int b0 = bucket_from_cum<KMAX>((float)xs[2 * c], cum0, run0, K, &a0);
				const int b1 = bucket_from_cum<KMAX>((float)xs[2 * c + 1], cum1, run1, K, &a1);
				cz0 |= (unsigned)b0 << (4 * c);
				cz1 |= (unsigned)b1 << (4 * c);
				camb |= (a0 ? 1u : 0u) << c;
				camb |= (a1 ? 1u : 0u) << (8 + c);
			}
		}
		STAMP(i, 6);
		/* ---- everybody's counts ---- */
		const int ngran = lay.ngran;
		for (int gi = t; gi - t < ngran; gi += BLOCK) { /* wave-uniform trip count */
			if (gi < ngran && (wmode || gi / W != g)) {
				const unsigned long long v = coop_poll(&cb->gran[slot][gi], tag, cb);
				const int w = gi % W;
				for (int c3 = 0; c3 < pack; c3++) {
					const int m = pack * w + c3;
					const int c = (int)((v >> (bits * c3)) & ((1 << bits) - 1));
					if (m < K && c) atomicAdd(&sh.ghist3[buf][m], c);
				}
			}
		}
		lds_barrier();
		STAMP(i, 3);
		/* the buffer of individual i + 2 (last read before this barrier, next written after the next one) */
		if (t < KMAX) {
			sh.hist3[(i + 2) % 3][t] = 0;
			sh.ghist3[(i + 2) % 3][t] = 0;
		}
		const unsigned used = 2u * (unsigned)nvalid +
			dirichlet_wave<KMAX>(d, sh, i, cur, offi + 2ull * (unsigned)nvalid, alpha, buf,
					     covered ? d.tape + offi + 2ull * (unsigned)nvalid : nullptr, writer);
		STAMP(i, 5);
		off += used;
		cl = nl;
		nl = ml;
	}
	if (g == 0 && t == 0) *pos_out = off;
}

/* the same sum in every lane: rotations inside the rows of 16 lanes, then the rows through two cross-lane exchanges */
__device__ __forceinline__ unsigned wave_allsum_u32(unsigned x)
{
	x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x121, 0xf, 0xf, false); /* row_ror:1 */
	x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x122, 0xf, 0xf, false); /* row_ror:2 */
	x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xf, 0xf, false); /* row_ror:4 */
	x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, false); /* row_ror:8 */
	x += (unsigned)__shfl_xor((int)x, 16, 64);
	x += (unsigned)__shfl_xor((int)x, 32, 64);
	return x;
}

/*
 * k_zq_pipe: the replay update_ZQ chain with the exchange of an individual's counts taken off the critical path.
 * Every workgroup has DW draw waves (one locus per lane) and ONE control wave; nothing but LDS words joins them.
 *   draw waves:   individual i starts where the control wave says (LDS).  Its Z is the candidate drawn earlier for
 *                 that start position (92 %), or the plain path.  Then the C candidates of individual i+1 are drawn
 *                 (start = end of i's draws + 2 K + 2 c, c = rejected attempts of i's Dirichlet), the few draws the
 *                 single precision filter could not decide are redone in double, and the wave's counts of EVERY
 *                 candidate leave as tagged words -- before anybody knows which candidate it will be.
 *   control wave: knows c when its Dirichlet of i-1 is done; the counts of individual i for that candidate were
 *                 published while that Dirichlet and the exchange before it ran, so they have arrived or are about
 *                 to; it sums them (packed 16-bit fields add without carries: a total stays below 2 Lp < 65536), runs
 *                 the Dirichlet of i (dirichlet_wave) and posts the next start position.
 * A start position no candidate was drawn for (8 %: c >= C, a shape of exactly 1, the first individual) takes the
 * plain path: the draw waves draw Z then, publish the counts in a set of their own, and the control wave waits for
 * those.  Same Z, same counts, same consumption as k_zq_spec / k_zq_coop in every case.
 * Granules: pipe_gran(slot of the individual, publishing wave, set * W + w); set = candidate, or C for the plain path.
 */
#ifndef ISG_PIPE_DW
#define ISG_PIPE_DW 3
#endif
#define ISG_PIPE_RMAX 6
#ifndef ISG_PIPE_C
#define ISG_PIPE_C 5 /* candidates per individual: 4 / 5 / 6 / 7 measured 9.78 / 9.52 / 9.70 / 9.96 k cycles per individual at config 3 */
#endif
#ifdef ISG_STAMPS
#define STAMPC(i, k) do { if (threadIdx.x == 64 * DW && blockIdx.x == 0 && (i) < 4096) g_stamps[(i) * 8 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define STAMPC(i, k) do { } while (0)
#endif
/* granules of k_zq_pipe: every publishing wave has lines of its own, 4352 bytes from the next wave's (4 KiB + 256 B:
 * consecutive publishers fall on different HBM stacks AND channels). */
#define ISG_PIPE_STRIDE 544 /* 8-byte words */
__device__ __forceinline__ unsigned long long *pipe_gran(unsigned long long *pg, int slot, int NP, int p, int w)
{
	return pg + ((size_t)slot * NP + p) * ISG_PIPE_STRIDE + w;
}
template <int KMAX, int DW>
__global__ void __launch_bounds__(64 * (DW + 1)) k_zq_pipe(DevView d, isg_wh base, double alpha, CoopBuf *cb, unsigned long long *pg, uint64_t *pos_out, int xcd_pack)
{
	constexpr int BLOCK = 64 * (DW + 1), C = ISG_PIPE_C, LW = 64 * DW;
	static_assert(KMAX <= 8 && C <= 8, "pre-filter rows in registers; candidates packed 4 bits each");
	__shared__ ZqShared sh;
	__shared__ unsigned long long off_sh[4]; /* start position of individual i in off_sh[i & 3] ... */
	__shared__ unsigned seq_sh;              /* ... valid once seq_sh >= i */
	__shared__ unsigned same_xcd;
	if (xcd_pack && (blockIdx.x & 7)) return; /* every 8th block works: one XCD under round-robin placement */
	const int t = threadIdx.x, g = xcd_pack ? blockIdx.x >> 3 : blockIdx.x, G = xcd_pack ? gridDim.x >> 3 : gridDim.x, K = d.K, lane = (int)lane_id();
	const bool ctrl = (t >= LW);
	{
		const uint16_t *src = (const uint16_t *)d.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += BLOCK) dst[k] = src[k];
		if (t < 3 * ISG_KCAP) {
			(&sh.hist3[0][0])[t] = 0;
			(&sh.ghist3[0][0])[t] = 0;
		}
		if (t < 4) off_sh[t] = 0;
		if (t == 4) seq_sh = 0;
	}
	__syncthreads();
	/* all workgroups on one XCD (checked through the hardware register): the counts are handed over in its L2 */
	const bool local = xcd_pack && coop_same_xcd(cb, g, G, &same_xcd);
	const isg_wh cur = isg_wh_jump(&sh.tab, base, 0);
	const int W = (K + 2) / 3, NP = G * DW;
	const size_t rowb = (size_t)d.Lp * 2;
	if (ctrl) {
		/* ------------------------------- control wave ------------------------------- */
		const bool writer = (g == 0);
		unsigned long long off = 0, pcbase = 0;
		bool pcvalid = false;
		int nvv = d.nvalid[min(lane, d.N - 1)], nvn = d.nvalid[min(64 + lane, d.N - 1)];
		for (int i = 0; i < d.N; i++) {
			if (i && !(i & 63)) {
				nvv = nvn;
				nvn = d.nvalid[min(i + 64 + lane, d.N - 1)];
			}
			const int nvalid = __builtin_amdgcn_readlane(nvv, i & 63);
			const int nvnext = ((i + 1) & 63) ? __builtin_amdgcn_readlane(nvv, (i + 1) & 63) : __builtin_amdgcn_readlane(nvn, 0);
			const unsigned tag = (unsigned)(i % 65535) + 1u;
			const int slot = i & (ISG_COOP_RING - 1);
			const unsigned long long offi = off, dpos = offi + 2ull * (unsigned)nvalid;
			const bool covered = dpos + 1024ull <= d.tape_len;
			/* which set of counts: the draw waves decide the same way from the same numbers */
			const unsigned long long dc = offi - pcbase;
			const bool hit = pcvalid && offi >= pcbase && !(dc & 1ull) && dc < 2ull * C;
			const int set = hit ? (int)(dc >> 1) : C;
			STAMPC(i, 4);
			/* this lane's attempt of the Dirichlet (gamma m at offset m + dd, as dirichlet_wave lays them out): its two
			 * uniforms are fetched now, under the exchange (the draw waves touched these lines an individual ago) */
			double ppu0 = 0.0, ppu1 = 0.0;
			if (covered) {
				const int D = 64 / K, m = (lane < K * D) ? lane / D : K - 1, dd = lane - m * D;
				ppu0 = d.tape[dpos + 2 * (m + dd)]; /* (a shape of exactly 1 makes the position odd: no 16-byte load) */
				ppu1 = d.tape[dpos + 2 * (m + dd) + 1];
			}
			/* everybody's counts: the probes of all missing granules go out together; every spin is bounded and watches
			 * the common abort word */
			unsigned long long v[3][ISG_PIPE_RMAX];
#pragma unroll
			for (int w = 0; w < 3; w++)
#pragma unroll
				for (int r = 0; r < ISG_PIPE_RMAX; r++) {
					const int p = r * 64 + lane;
					v[w][r] = (w < W && r * 64 < NP && p < NP) ? 0ull : ((unsigned long long)tag << 48);
				}
			for (unsigned spin = 0;; spin++) {
#pragma unroll
				for (int w = 0; w < 3; w++)
#pragma unroll
					for (int r = 0; r < ISG_PIPE_RMAX; r++) {
						const int p = r * 64 + lane;
						if (w < W && r * 64 < NP && p < NP && (unsigned)(v[w][r] >> 48) != tag) v[w][r] = ld_agent(pipe_gran(pg, slot, NP, p, set * W + w));
					}
				bool miss = false;
#pragma unroll
				for (int w = 0; w < 3; w++)
#pragma unroll
					for (int r = 0; r < ISG_PIPE_RMAX; r++)
						miss |= ((unsigned)(v[w][r] >> 48) != tag);
				if (!__ballot(miss)) break;
				if ((spin & 1023u) == 1023u) {
					if (__hip_atomic_load(&cb->abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
					if (spin > (1u << 22)) {
						__hip_atomic_store(&cb->abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						break;
					}
				}
			}
			unsigned lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
#pragma unroll
			for (int w = 0; w < 3; w++)
#pragma unroll
				for (int r = 0; r < ISG_PIPE_RMAX; r++)
					if (w < W && r * 64 < NP) {
						lo[w] += (unsigned)v[w][r];
						hi[w] += (unsigned)(v[w][r] >> 32) & 0xffffu;
					}
			unsigned cnt = 0;
#pragma unroll
			for (int w = 0; w < 3; w++)
				if (w < W) {
					const unsigned Ls = wave_sum_u32(lo[w]), Hs = wave_sum_u32(hi[w]);
					cnt = (lane == 3 * w) ? (Ls & 0xffffu) : (lane == 3 * w + 1) ? (Ls >> 16) : (lane == 3 * w + 2) ? Hs : cnt;
				}
			if (lane < K) sh.ghist3[0][lane] = (int)cnt;
			STAMPC(i, 3);
			const unsigned used = 2u * (unsigned)nvalid +
				dirichlet_wave<KMAX>(d, sh, i, cur, dpos, alpha, 0, covered ? d.tape + dpos : nullptr, writer, true, ppu0, ppu1);
			off += used;
			if (lane == 0) {
				off_sh[(i + 1) & 3] = off;
				__hip_atomic_store(&seq_sh, (unsigned)(i + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
			}
			/* the candidates the draw waves are drawing for individual i + 1 */
			pcbase = dpos + 2ull * (unsigned)K;
			pcvalid = (i + 1 < d.N) && (pcbase + 2ull * (C - 1) + 2ull * (unsigned)nvnext + 1024ull <= d.tape_len);
			STAMPC(i, 5);
		}
		if (g == 0 && lane == 0) *pos_out = off;
#ifdef ISG_STAMPS
		if (g == 0 && lane == 0) g_stamps[4095 * 8 + 4] = (local ? 1ull : 0ull) | ((unsigned long long)xcc_id() << 8) | ((unsigned long long)G << 16);
#endif
		return;
	}
	/* --------------------------------- draw waves --------------------------------- */
	const int j = g * LW + t; /* this lane's locus */
	const int pub = g * DW + (t >> 6);
	const int myc = lane / W, myw = lane % W; /* the candidate and the word this lane publishes */
	struct Loc {
		unsigned a0, a1, rw;
		float F0[KMAX], F1[KMAX];
		double qv;
		int nvv;
	};
	Loc cl, nl, ml;
	auto fetch_geno = [&](int ni, Loc &L) {
		L.a0 = L.a1 = 0xff;
		L.rw = 0;
		L.nvv = 0;
		L.qv = 0.0;
		if (ni < d.N) {
			L.nvv = d.nvalid[min(ni + lane, d.N - 1)];
			if (lane < K) L.qv = d.qq[(size_t)ni * K + lane];
			if (j < d.Lp) {
				const unsigned short gg = *(const unsigned short *)(d.geno + (size_t)ni * rowb + (size_t)j * 2);
				L.a0 = gg & 0xff;
				L.a1 = gg >> 8;
				L.rw = d.rankwave[(size_t)ni * d.nwv + (j >> 6)];
			}
		}
	};
	auto fetch_rows = [&](Loc &L) {
#pragma unroll
		for (int m = 0; m < KMAX; m++) L.F0[m] = L.F1[m] = 0.f;
		if (L.a0 != 0xff) {
			const float *P0 = d.freqf + ((size_t)j * d.Amax + L.a0) * d.KPF, *P1 = d.freqf + ((size_t)j * d.Amax + L.a1) * d.KPF;
#pragma unroll
			for (int m = 0; m < KMAX; m += 4) {
				if (m < K) {
					const float4 f0 = *(const float4 *)(P0 + m), f1 = *(const float4 *)(P1 + m);
					L.F0[m] = f0.x; L.F1[m] = f1.x;
					if (m + 1 < KMAX) { L.F0[m + 1] = f0.y; L.F1[m + 1] = f1.y; }
					if (m + 2 < KMAX) { L.F0[m + 2] = f0.z; L.F1[m + 2] = f1.z; }
					if (m + 3 < KMAX) { L.F0[m + 3] = f0.w; L.F1[m + 3] = f1.w; }
				}
			}
		}
	};
	fetch_geno(0, cl);
	fetch_rows(cl);
	fetch_geno(1, nl);
	ml = nl;
	unsigned cz0 = 0, cz1 = 0;
	unsigned long long cbase = 0;
	bool cvalid = false;
	double touch = 0.0;
	for (int i = 0; i < d.N; i++) {
		const unsigned tag = (unsigned)(i % 65535) + 1u, ntag = (unsigned)((i + 1) % 65535) + 1u;
		const int slot = i & (ISG_COOP_RING - 1), nslot = (i + 1) & (ISG_COOP_RING - 1);
		/* the start position, posted by the control wave when its Dirichlet of individual i - 1 was done */
		while (__hip_atomic_load(&seq_sh, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < (unsigned)i) __builtin_amdgcn_s_sleep(1);
		const unsigned long long offi = off_sh[i & 3];
		const int nvalid = __builtin_amdgcn_readfirstlane(cl.nvv), nnvalid = __builtin_amdgcn_readfirstlane(nl.nvv);
		const bool covered = offi + 2ull * (unsigned)nvalid + 1024ull <= d.tape_len;
		const bool valid = (cl.a0 != 0xff);
		STAMP(i, 0);
		/* ---- first in the queue: the uniforms of the next individual's candidates and its frequency rows ---- */
		const unsigned long long nbase = offi + 2ull * (unsigned)nvalid + 2ull * (unsigned)K; /* every gamma: >= one attempt of two uniforms */
		const bool nvalidc = (i + 1 < d.N) && (nbase + 2ull * (C - 1) + 2ull * (unsigned)nnvalid + 1024ull <= d.tape_len);
		const bool nvalidl = (nl.a0 != 0xff);
		const unsigned nrank = nl.rw + (unsigned)__popcll(__ballot(nvalidl) & ((1ull << lane) - 1ull));
		double xs[2 * C];
#pragma unroll
		for (int k = 0; k < 2 * C; k++) xs[k] = 0.5;
		if (nvalidc && nvalidl) {
			const double *tp = d.tape + nbase + 2ull * nrank;
#pragma unroll
			for (int k = 0; k < 2 * C; k++) xs[k] = tp[k];
		}
		fetch_rows(nl);
		/* ---- this individual's Z: a candidate drawn earlier (its counts left then), or the plain path ---- */
		const unsigned long long dc = offi - cbase;
		const bool hit = cvalid && offi >= cbase && !(dc & 1ull) && dc < 2ull * C;
		int z0 = 0xff, z1 = 0xff;
		if (hit) {
			const unsigned c = (unsigned)(dc >> 1);
			if (valid) {
				z0 = (int)((cz0 >> (4 * c)) & 0xfu);
				z1 = (int)((cz1 >> (4 * c)) & 0xfu);
			}
		} else {
			const unsigned rank = cl.rw + (unsigned)__popcll(__ballot(valid) & ((1ull << lane) - 1ull));
			bool amb0 = false, amb1 = false;
			if (valid && covered) {
				float qf[KMAX];
#pragma unroll
				for (int m = 0; m < KMAX; m++) qf[m] = (m < K) ? (float)readlane_f64(cl.qv, m) : 0.f;
				const double x0 = d.tape[offi + 2ull * rank], x1 = d.tape[offi + 2ull * rank + 1];
				z0 = bucket_f32<KMAX>((float)x0, cl.F0, qf, K, &amb0);
				z1 = bucket_f32<KMAX>((float)x1, cl.F1, qf, K, &amb1);
			}
			if (__ballot(valid && covered && (amb0 || amb1))) { /* rare: the draw in double */
				double cum[KMAX], q[KMAX];
#pragma unroll
				for (int m = 0; m < KMAX; m++) q[m] = (m < K) ? readlane_f64(cl.qv, m) : 0.0;
				if (valid && covered && amb0) {
					const double tot = weights<KMAX>(d.freq + ((size_t)j * d.Amax + cl.a0) * d.KP, q, cum, K);
					z0 = bucket_fast<KMAX>(d.tape[offi + 2ull * rank], cum, tot, K);
				}
				if (valid && covered && amb1) {
					const double tot = weights<KMAX>(d.freq + ((size_t)j * d.Amax + cl.a1) * d.KP, q, cum, K);
					z1 = bucket_fast<KMAX>(d.tape[offi + 2ull * rank + 1], cum, tot, K);
				}
			}
			if (!covered) { z0 = z1 = 0xff; }
			/* the plain path's counts: set C */
			unsigned long long v = (unsigned long long)tag << 48;
#pragma unroll
			for (int m = 0; m < KMAX; m++)
				if (m < K) {
					const int wc = __popcll(__ballot(z0 == m)) + __popcll(__ballot(z1 == m));
					if (lane == m / 3) v |= (unsigned long long)(wc & 0xffff) << (16 * (m % 3));
				}
			if (lane < W) { if (local) st_xcd(pipe_gran(pg, slot, NP, pub, C * W + lane), v); else st_agent(pipe_gran(pg, slot, NP, pub, C * W + lane), v); }
		}
		STAMP(i, 1);
		if (j < d.Lp) *(unsigned short *)(d.z + (size_t)i * rowb + (size_t)j * 2) = (unsigned short)(z0 | (z1 << 8));
		if (!covered && t == 0) cb->overflow_flag = 1;
		STAMP(i, 2);
		/* ---- the next individual's candidates ---- */
		fetch_geno(i + 2, ml);
		/* the next Dirichlet's stretch of the tape (its start is known up to this Dirichlet's rejected attempts: 160
		 * uniforms cover that), so that the control wave finds it in L2 */
		if (touch == -1.0) cb->overflow_flag = 2;
		if (t < 10 && nvalidc) touch = d.tape[nbase + 2ull * (unsigned)nnvalid + 16u * (unsigned)t];
		cbase = nbase;
		cvalid = nvalidc;
		cz0 = cz1 = 0;
		if (nvalidc) { /* wave-uniform */
			unsigned camb = 0;
			if (nvalidl) {
				float qf[KMAX], cum0[KMAX], cum1[KMAX];
#pragma unroll
				for (int m = 0; m < KMAX; m++) qf[m] = (m < K) ? (float)readlane_f64(nl.qv, m) : 0.f;
				const float run0 = prefix_f32<KMAX>(nl.F0, qf, K, cum0), run1 = prefix_f32<KMAX>(nl.F1, qf, K, cum1);
#pragma unroll
				for (int c = 0; c < C; c++) {
					bool a0, a1;
					const int b0 = bucket_from_cum<KMAX>((float)xs[2 * c], cum0, run0, K, &a0);
					const int b1 = bucket_from_cum<KMAX>((float)xs[2 * c + 1], cum1, run1, K, &a1);
					cz0 |= (unsigned)b0 << (4 * c);
					cz1 |= (unsigned)b1 << (4 * c);
					camb |= (a0 ? 1u : 0u) << c;
					camb |= (a1 ? 1u : 0u) << (8 + c);
				}
			}
			STAMP(i, 6);
			if (__ballot(camb != 0u)) { /* rare (about 4 % of the waves): the draws the filter could not decide, in double */
				double cum[KMAX], q[KMAX];
#pragma unroll
				for (int m = 0; m < KMAX; m++) q[m] = (m < K) ? readlane_f64(nl.qv, m) : 0.0;
				if (camb & 0xffu) {
					const double tot = weights<KMAX>(d.freq + ((size_t)j * d.Amax + nl.a0) * d.KP, q, cum, K);
#pragma unroll
					for (int c = 0; c < C; c++)
						if ((camb >> c) & 1u) cz0 = (cz0 & ~(0xfu << (4 * c))) | ((unsigned)bucket_fast<KMAX>(xs[2 * c], cum, tot, K) << (4 * c));
				}
				if (camb >> 8) {
					const double tot = weights<KMAX>(d.freq + ((size_t)j * d.Amax + nl.a1) * d.KP, q, cum, K);
#pragma unroll
					for (int c = 0; c < C; c++)
						if ((camb >> (8 + c)) & 1u) cz1 = (cz1 & ~(0xfu << (4 * c))) | ((unsigned)bucket_fast<KMAX>(xs[2 * c + 1], cum, tot, K) << (4 * c));
				}
			}
			/* the wave's counts of every candidate: lane c * W + w carries word w of candidate c.  A lane's two draws as
			 * 8-bit fields (one per cluster), summed over the wave with DPP adds (a field stays <= 128: no carries) --
			 * 2 K ballots and scalar popcounts per candidate took 5 k cycles here */
			unsigned mylo = 0, myhi = 0;
#pragma unroll
			for (int c = 0; c < C; c++) {
				unsigned long long P = 0;
				if (nvalidl) P = (1ull << (8 * ((cz0 >> (4 * c)) & 0xfu))) + (1ull << (8 * ((cz1 >> (4 * c)) & 0xfu)));
				const unsigned plo = wave_allsum_u32((unsigned)P), phi = (KMAX > 4) ? wave_allsum_u32((unsigned)(P >> 32)) : 0u;
				if (myc == c) {
					mylo = plo;
					myhi = phi;
				}
			}
			const unsigned long long my = ((unsigned long long)myhi << 32) | mylo;
			unsigned long long v = (unsigned long long)ntag << 48;
#pragma unroll
			for (int k = 0; k < 3; k++)
				if (3 * myw + k < 8) v |= ((my >> (8 * (3 * myw + k))) & 0xffull) << (16 * k);
			if (lane < C * W) { if (local) st_xcd(pipe_gran(pg, nslot, NP, pub, lane), v); else st_agent(pipe_gran(pg, nslot, NP, pub, lane), v); }
		}
		STAMP(i, 7);
		cl = nl;
		nl = ml;
	}
}
