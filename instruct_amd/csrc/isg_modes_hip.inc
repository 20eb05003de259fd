/*
 * isg_modes_hip.inc -- the diploid modes besides 1 and 2 (mcmc_updating's switch, mcmc.c:63-87); update_P, update_ZQ,
 * update_alpha and the table-driven likelihood sweeps are the kernels of isg_hip.hip.  Included by isg_hip.hip behind
 * isg_poly_hip.inc (shares its exact-accumulator helpers).
 *
 *   mode 4 (-v 4)  mcmc_POP_inbreedcoff   mcmc.c:242-295   update_inbreedcoff_POP :986-1051, log_ld_F_pop :1776-1809
 *   mode 3 (-v 3)  mcmc_INDV_selfing      mcmc.c:297-385   update_S_IND :864-884 (uniform prior), update_G with the individual's rate
 *   mode 5 (-v 5)  mcmc_INDV_inbreedcoff  mcmc.c:386-470   update_F_IND :888-910 (uniform prior), log_ld_F_indv :1812-1847
 *   mode 0 (-v 0)  mcmc_POP_no_admixture  mcmc.c:90-132    update_Z :1094-1120, log_ld_indv_K :1893-1914
 *
 * Mode 4.  update_inbreedcoff_POP compares log_ld_F_total (mcmc.c:1850-1868) at the proposed and at the current
 * coefficients for each cluster in turn: 2 K passes over N x L in the reference.  A coefficient only enters the
 * terms of loci whose two copies sit in that cluster, and such a term depends on (locus, allele pair, cluster)
 * only, so ONE count sweep (pair counts + allele counts of the other loci) turns every total into a sum over
 * K L Amax^2 table entries, exact and integer weighted:
 *     total(F) = sum cntmix log freq + nhet log 2 + sum_k sum_(j,a0,a1) npair[k][j][a0][a1] log genofreq_F(f0, f1, F_k)
 * As for ploidy 4 all proposals are drawn first (a proposal depends on the cluster's own coefficient and state), all
 * 2 K cluster sums come from one launch and the Metropolis steps are decided in order on the host.
 */
struct InbreedCtx {
	DevBuf<int> d_npair;   /* [L][Amax][Amax][K] loci with both copies in cluster k, by allele pair (a0, a1) as stored */
	DevBuf<int> d_cntmix;  /* [L][Amax][K] allele copies of the other loci */
	DevBuf<unsigned long long> d_nhet; /* [1] heterozygous loci among those */
	DevBuf<unsigned long long> d_acc;  /* exact accumulators: slot 0 fixed terms, 1 + k current, 1 + K + k proposed */
	DevBuf<double> d_F;    /* [2][KCAP] current and proposed coefficients */
};

/* genofreq_inbreedcoff (mcmc.c:1705-1723) */
__device__ __forceinline__ double genofreq_F(bool hom, double f0, double f1, double inbreed)
{
	if (hom) return isg_pow(f0, 2.0) * (1 - inbreed) + f0 * inbreed;
	return 2 * f0 * f1 * (1 - inbreed);
}

/* the count sweep: 64 loci x a chunk of individuals per workgroup, tiles in LDS when they fit */
template <bool TILE>
__global__ void __launch_bounds__(256) k_paircount(DevView d, int chunk, int *npair, int *cntmix, unsigned long long *nhet)
{
	extern __shared__ int tile[]; /* [A*A*K + A*K][64] */
	const int A = d.Amax, K = d.K, NP = A * A * K, NM = A * K, lane = (int)lane_id(), wave = threadIdx.x >> 6;
	const int j = blockIdx.x * 64 + lane, i0 = blockIdx.y * chunk, i1 = min(d.N, i0 + chunk);
	if (TILE) {
		for (int e = threadIdx.x; e < (NP + NM) * 64; e += 256) tile[e] = 0;
		__syncthreads();
	}
	unsigned het = 0;
	if (j < d.L) {
		for (int i = i0 + wave; i < i1; i += 4) {
			const size_t id = (size_t)i * d.Lp + j;
			const unsigned short g = *(const unsigned short *)(d.geno + id * 2);
			const unsigned a0 = g & 0xff, a1 = g >> 8;
			if (a0 == 0xff) continue;
			const unsigned short zz = *(const unsigned short *)(d.z + id * 2);
			const unsigned z0 = zz & 0xff, z1 = zz >> 8;
			if (z0 == z1) {
				if (TILE) atomicAdd(&tile[((a0 * A + a1) * K + z0) * 64 + lane], 1);
				else atomicAdd(&npair[(((size_t)j * A + a0) * A + a1) * K + z0], 1);
			} else {
				if (TILE) {
					atomicAdd(&tile[(NP + a0 * K + z0) * 64 + lane], 1);
					atomicAdd(&tile[(NP + a1 * K + z1) * 64 + lane], 1);
				} else {
					atomicAdd(&cntmix[((size_t)j * A + a0) * K + z0], 1);
					atomicAdd(&cntmix[((size_t)j * A + a1) * K + z1], 1);
				}
				het += (a0 != a1);
			}
		}
	}
	if (TILE) {
		__syncthreads();
		for (int e = threadIdx.x; e < (NP + NM) * 64; e += 256) {
			const int v = tile[e], l = e & 63, r = e >> 6, jj = blockIdx.x * 64 + l;
			if (v && jj < d.L) {
				if (r < NP) atomicAdd(&npair[(size_t)jj * NP + r], v);
				else atomicAdd(&cntmix[(size_t)jj * NM + (r - NP)], v);
			}
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) het += __shfl_down(het, o, 64);
	if (lane == 0 && het) atomicAdd(nhet, (unsigned long long)het);
}

/* blockIdx.y = accumulator slot: 0 sum cntmix log freq; 1 + k / 1 + K + k the pair terms of cluster k at the current /
 * proposed coefficient.  One block reduction, one set of atomics per block. */
template <int FS> /* F: [2][FS], current and proposed coefficients */
__device__ __forceinline__ void Fsums_body(DevView d, const int *npair, const int *cntmix, const double *F, unsigned long long *acc)
{
	__shared__ unsigned long long sm[4 * 5];
	const int A = d.Amax, K = d.K, slot = blockIdx.y;
	const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
	isg_acc a;
	isg_acc_zero(&a);
	if (slot == 0) {
		if (id < (size_t)d.L * A * K) {
			const unsigned c = (unsigned)cntmix[id];
			if (c) {
				const size_t r = id / K;
				acc_add_times(&a, isg_log(d.freq[r * d.KP + (id - r * K)]), c);
			}
		}
	} else if (id < (size_t)d.L * A * A) { /* id = (j A + a0) A + a1 */
		const int prop = (slot - 1) >= K, k = (slot - 1) - (prop ? K : 0);
		const unsigned c = (unsigned)npair[id * K + k];
		if (c) {
			const int a1 = (int)(id % A), a0 = (int)((id / A) % A), j = (int)(id / A / A);
			const double f0 = d.freq[((size_t)j * A + a0) * d.KP + k], f1 = d.freq[((size_t)j * A + a1) * d.KP + k];
			acc_add_times(&a, isg_log(genofreq_F(a0 == a1, f0, f1, F[prop * FS + k])), c);
		}
	}
	const isg_acc r = block_reduce_acc<256>(a, sm);
	if (threadIdx.x == 0) acc_global_add(acc + 5 * slot, r);
}
__global__ void __launch_bounds__(256) k_Fsums(DevView d, const int *npair, const int *cntmix, const double *F, unsigned long long *acc) { Fsums_body<ISG_KCAP>(d, npair, cntmix, F, acc); }
/* K > ISG_KCAP */
__global__ void __launch_bounds__(256) k_Fsums_w(DevView d, const int *npair, const int *cntmix, const double *F, unsigned long long *acc) { Fsums_body<ISG_KWIDE>(d, npair, cntmix, F, acc); }

/* lltab slot 0 = log genofreq_F(f0, f1, F_k): cal_lkh's same-cluster terms (k_loglik_tab reads it with generation 1) */
__global__ void k_lltabF(DevView d, const double *F)
{
	const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const size_t per = (size_t)d.L * d.Amax * d.Amax * d.K;
	if (id >= per) return;
	const int k = (int)(id % d.K);
	const int a1 = (int)((id / d.K) % d.Amax), a0 = (int)((id / d.K / d.Amax) % d.Amax), j = (int)(id / d.K / d.Amax / d.Amax);
	const double f0 = d.freq[((size_t)j * d.Amax + a0) * d.KP + k], f1 = d.freq[((size_t)j * d.Amax + a1) * d.KP + k];
	d.lltab[id] = isg_log(genofreq_F(a0 == a1, f0, f1, F[k]));
}

static int inbreed_alloc(isg_ctx *c)
{
	const int L = c->cfg.L, K = c->cfg.K, A = c->Amax;
	InbreedCtx *ib = new InbreedCtx();
	c->inb = ib;
	HIPCHK(ib->d_npair.alloc_zero((size_t)L * A * A * K));
	HIPCHK(ib->d_cntmix.alloc_zero((size_t)L * A * K));
	HIPCHK(ib->d_nhet.alloc_zero(1));
	HIPCHK(ib->d_acc.alloc_zero(5 * (2 * ISG_KWIDE + 2)));
	HIPCHK(ib->d_F.alloc_zero(2 * ISG_KWIDE));
	return 0;
}

static int inbreed_update_F_POP(isg_ctx *c) /* update_inbreedcoff_POP, mcmc.c:986-1051 */
{
	InbreedCtx *ib = c->inb;
	DevView &d = c->d;
	const int K = c->cfg.K, L = c->cfg.L, A = c->Amax;
	if (ensure_S(c)) return 1;
	/* counts of the current (z, genotype) */
	HIPCHK(hipMemsetAsync(ib->d_npair, 0, sizeof(int) * (size_t)L * A * A * K, c->stream));
	HIPCHK(hipMemsetAsync(ib->d_cntmix, 0, sizeof(int) * (size_t)L * A * K, c->stream));
	HIPCHK(hipMemsetAsync(ib->d_nhet, 0, sizeof(unsigned long long), c->stream));
	{
		const size_t lds = sizeof(int) * (size_t)(A * A * K + A * K) * 64;
		const int chunk = d.N > 4096 ? 1024 : (d.N + 3) / 4;
		const dim3 grid((L + 63) / 64, (d.N + chunk - 1) / chunk);
		prof_begin(c);
		if (lds <= 60000) hipLaunchKernelGGL(k_paircount<true>, grid, dim3(256), lds, c->stream, d, chunk, ib->d_npair, ib->d_cntmix, ib->d_nhet);
		else hipLaunchKernelGGL(k_paircount<false>, grid, dim3(256), 0, c->stream, d, chunk, ib->d_npair, ib->d_cntmix, ib->d_nhet);
		prof_end(c, "k_paircount");
	}
	/* proposals and acceptance draws in the reference's order */
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
		} else {
			const int st = c->state[j];
			if (st == 0) { if (host_next(c) < 0.50) { tmp = 0.0; pst[j] = 0; } else { tmp = host_next(c); pst[j] = 1; } }
			else if (st == 2) { if (host_next(c) < 0.5) { tmp = 1.0; pst[j] = 2; } else { tmp = host_next(c); pst[j] = 1; } }
			else { const double tt = host_next(c); if (tt <= 0.05) { tmp = 0.0; pst[j] = 0; } else if (tt >= 0.95) { tmp = 1.0; pst[j] = 2; } else { tmp = host_next(c); pst[j] = 1; } }
		}
		prop[j] = tmp;
		uacc[j] = host_next(c);
	}
	const int FS = (K > ISG_KCAP) ? ISG_KWIDE : ISG_KCAP; /* k_Fsums / k_Fsums_w: [2][FS] */
	double Fs[2 * ISG_KWIDE];
	for (int k = 0; k < K; k++) {
		Fs[k] = c->S[k];
		Fs[FS + k] = prop[k];
	}
	HIPCHK(hipMemcpyAsync(ib->d_F, Fs, sizeof(double) * 2 * FS, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(ib->d_acc, 0, sizeof(unsigned long long) * 5 * (2 * FS + 2), c->stream));
	{
		const size_t ne = (size_t)L * A * (A > K ? A : K);
		prof_begin(c);
		if (K > ISG_KCAP)
			hipLaunchKernelGGL(k_Fsums_w, dim3((unsigned)((ne + 255) / 256), 2 * K + 1), dim3(256), 0, c->stream, d, (const int *)ib->d_npair, (const int *)ib->d_cntmix,
					   (const double *)ib->d_F, ib->d_acc);
		else
			hipLaunchKernelGGL(k_Fsums, dim3((unsigned)((ne + 255) / 256), 2 * K + 1), dim3(256), 0, c->stream, d, (const int *)ib->d_npair, (const int *)ib->d_cntmix,
					   (const double *)ib->d_F, ib->d_acc);
		prof_end(c, "k_Fsums");
	}
	HIPCHK(hipGetLastError());
	unsigned long long nhet = 0;
	std::vector<unsigned long long> raw(5 * (size_t)(2 * K + 1));
	HIPCHK(hipMemcpyAsync(&nhet, ib->d_nhet, sizeof(nhet), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(raw.data(), ib->d_acc, sizeof(unsigned long long) * raw.size(), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	std::vector<isg_acc> acc(2 * K + 1);
	for (int s = 0; s < 2 * K + 1; s++) {
		unsigned long long t0 = raw[5 * s], t1 = raw[5 * s + 1] + (t0 >> 32), t2 = raw[5 * s + 2] + (t1 >> 32), t3 = raw[5 * s + 3] + (t2 >> 32);
		acc[s].lo = (t0 & 0xffffffffULL) | (t1 << 32);
		acc[s].hi = (t2 & 0xffffffffULL) | (t3 << 32);
		acc[s].flags = (uint32_t)raw[5 * s + 4];
	}
	while (nhet) { /* log 2 once per heterozygous locus with copies in two clusters (mcmc.c:1802-1803) */
		const unsigned long long part = nhet > 0xffffffffULL ? 0xffffffffULL : nhet;
		acc_add_times(&acc[0], isg_log(2.0), part);
		nhet -= part;
	}
	for (int j = 0; j < K; j++) {
		isg_acc cur_t = acc[0], new_t = acc[0];
		for (int k = 0; k < K; k++) {
			isg_acc_merge(&cur_t, &acc[1 + k]);
			isg_acc_merge(&new_t, k == j ? &acc[1 + K + j] : &acc[1 + k]);
		}
		double mh = isg_acc_value(&new_t) - isg_acc_value(&cur_t);
		if (c->cfg.back_refl == 0) mh *= poly_q_trans(c->state[j], pst[j]) / poly_q_trans(pst[j], c->state[j]);
		const double m1 = (1 > mh) ? mh : 1; /* sic: MIN2(1, mhratio) on the log ratio (mcmc.c:1040) */
		if (uacc[j] < isg_exp(m1)) {
			c->S[j] = prop[j];
			if (c->cfg.back_refl == 0) c->state[j] = pst[j];
			acc[1 + j] = acc[1 + K + j];
		}
	}
	HIPCHK(hipMemcpyAsync(c->d_S, c->S.data(), sizeof(double) * K, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->d_state, c->state.data(), sizeof(int) * K, hipMemcpyHostToDevice, c->stream));
	return 0;
}

/* cal_lkh, mode 4: the table of same-cluster terms at the current coefficients, then the table sweep */
static int inbreed_cal_lkh(isg_ctx *c)
{
	DevView &d = c->d;
	const size_t per = (size_t)d.L * d.Amax * d.Amax * d.K;
	prof_begin(c);
	hipLaunchKernelGGL(k_lltabF, dim3((unsigned)((per + 127) / 128)), dim3(128), 0, c->stream, d, (const double *)c->d_S);
	prof_end(c, "k_lltabF");
	prof_begin(c);
	hipLaunchKernelGGL((k_loglik_tab<256, false>), dim3(d.N), dim3(256), 0, c->stream, d);
	prof_end(c, "k_loglik_lkh");
	prof_begin(c);
	hipLaunchKernelGGL(k_lkh_total<1024>, dim3(1), dim3(1024), 0, c->stream, d, c->d_total);
	prof_end(c, "k_lkh_total");
	HIPCHK(hipGetLastError());
	c->h_lkh = false;
	return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* mode 3 (`-v 3`, mcmc_INDV_selfing, mcmc.c:297-385, uniform prior): one selfing rate per individual.        */
/* update_S_IND (mcmc.c:864-884) consumes exactly two uniforms per individual: one lane each.                 */
/* ------------------------------------------------------------------------------------------ */
__global__ void k_sind(DevView d, double *S, isg_wh base)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= d.N) return;
	isg_wh s = isg_wh_jump(d.tab, base, 2ull * (unsigned)j);
	const double cur = S[j];
	const int g = d.gen[j];
	double tmp = isg_wh_next(&s) * 2 * 0.05 - 0.05;
	tmp += cur;
	if (tmp <= 0.0) tmp = 0.0 - tmp;
	if (tmp >= 1.0) tmp = 1.0 - (tmp - 1);
	/* dgeom (mcmc.c:1596-1604) */
	const double dn = isg_pow(tmp, (double)(g - 1)) * (1 - tmp), dc = isg_pow(cur, (double)(g - 1)) * (1 - cur);
	const double mh = isg_exp(isg_log(dn) - isg_log(dc));
	const double thr = (1 > mh) ? mh : 1;
	S[j] = (isg_wh_next(&s) < thr) ? tmp : cur;
}

static int indiv_update_S_IND(isg_ctx *c)
{
	const int N = c->cfg.N;
	const isg_wh base = is_keyed(c) ? isg_wh_jump(&c->tab_h, c->origin, iter_base(c) + c->ky[KY_OFFA] + 4) : c->rng;
	prof_begin(c);
	hipLaunchKernelGGL(k_sind, dim3((N + 255) / 256), dim3(256), 0, c->stream, c->d, c->d_S, base);
	prof_end(c, "k_sind");
	HIPCHK(hipGetLastError());
	if (!is_keyed(c)) host_advance(c, 2ull * (unsigned)N);
	c->h_S = false;
	return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* mode 5 (`-v 5`, mcmc_INDV_inbreedcoff, mcmc.c:386-470, uniform prior): one inbreeding coefficient per individual */
/* (kept in the N selfing-rate slots).  update_F_IND (mcmc.c:888-910) = proposals (two uniforms per individual at   */
/* static positions) + ONE pass that evaluates log_ld_F_indv (mcmc.c:1812-1847) at the proposed and the current     */
/* coefficient; cal_lkh is the same pass at the current one.                                                        */
/* ------------------------------------------------------------------------------------------ */
__global__ void k_find_prop(DevView d, const double *F, double *Fprop, isg_wh base)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= d.N) return;
	isg_wh s = isg_wh_jump(d.tab, base, 2ull * (unsigned)j);
	double tmp = isg_wh_next(&s) * 2 * 0.05 - 0.05;
	tmp += F[j];
	if (tmp <= 0.0) tmp = 0.0 - tmp;
	if (tmp >= 1.0) tmp = 1.0 - (tmp - 1);
	Fprop[j] = tmp;
	d.uacc[j] = isg_wh_next(&s);
}

template <int BLOCK, bool PAIR>
__global__ void __launch_bounds__(BLOCK) k_loglikF(DevView d, double *F, const double *Fprop)
{
	__shared__ long long sm[(BLOCK / 64) * 3];
	const int i = blockIdx.x;
	const double fc = F[i], fp = PAIR ? Fprop[i] : 0.0;
	const double log2c = isg_log(2.0);
	isg_acc2 accC, accP, accX; /* same-cluster terms at the current / proposed coefficient, coefficient-free terms */
	isg_acc2_zero(&accC);
	isg_acc2_zero(&accP);
	isg_acc2_zero(&accX);
	const size_t rowb = (size_t)d.Lp * 2;
	const uint8_t *grow = d.geno + (size_t)i * rowb;
	const uint8_t *zrow = d.z + (size_t)i * rowb;
	for (int j0 = threadIdx.x * ISG_LPT; j0 < d.Lp; j0 += BLOCK * ISG_LPT) {
		const uint2 g = *(const uint2 *)(grow + (size_t)j0 * 2);
		const uint2 zz = *(const uint2 *)(zrow + (size_t)j0 * 2);
		unsigned long long gb = ((unsigned long long)g.y << 32) | g.x, zb = ((unsigned long long)zz.y << 32) | zz.x;
#pragma unroll
		for (int l = 0; l < ISG_LPT; l++) {
			unsigned a0 = (unsigned)(gb >> (16 * l)) & 0xff, a1 = (unsigned)(gb >> (16 * l + 8)) & 0xff;
			unsigned z0 = (unsigned)(zb >> (16 * l)) & 0xff, z1 = (unsigned)(zb >> (16 * l + 8)) & 0xff;
			const bool valid = (a0 != 0xff);
			if (!valid) { a0 = a1 = 0; z0 = z1 = 0; }
			const int j = (j0 + l < d.L) ? j0 + l : 0;
			const double f0 = d.freq[((size_t)j * d.Amax + a0) * d.KP + z0], f1 = d.freq[((size_t)j * d.Amax + a1) * d.KP + z1];
			const bool same = (z0 == z1), hom = (a0 == a1);
			const double v0 = same ? genofreq_F(hom, f0, f1, fc) : f0, v1 = same ? (PAIR ? genofreq_F(hom, f0, f1, fp) : 1.0) : f1;
			const double L0 = isg_log(v0), L1 = isg_log(v1);
			isg_acc2_add(&accC, (valid && same) ? L0 : 0.0);
			if (PAIR) isg_acc2_add(&accP, (valid && same) ? L1 : 0.0);
			isg_acc2_add(&accX, (valid && !same) ? L0 : 0.0);
			isg_acc2_add(&accX, (valid && !same) ? L1 : 0.0);
			isg_acc2_add(&accX, (valid && !same && !hom) ? log2c : 0.0);
		}
	}
	isg_acc2 rc, rp, rx;
	rc = block_reduce_acc2<BLOCK>(accC, sm);
	rx = block_reduce_acc2<BLOCK>(accX, sm);
	if (PAIR) rp = block_reduce_acc2<BLOCK>(accP, sm);
	if (threadIdx.x == 0) {
		isg_acc2 tc = rc;
		isg_acc2_merge(&tc, &rx);
		const double lc = isg_acc2_value(&tc);
		if (PAIR) {
			isg_acc2 tp = rp;
			isg_acc2_merge(&tp, &rx);
			const double lp = isg_acc2_value(&tp);
			const double mh = isg_exp(lp - lc);
			const double thr = (1 > mh) ? mh : 1;
			if (d.uacc[i] < thr) F[i] = fp;
		} else {
			d.indvlkh[i] = lc;
		}
	}
}

static int indiv_update_F_IND(isg_ctx *c)
{
	const int N = c->cfg.N;
	const isg_wh base = is_keyed(c) ? isg_wh_jump(&c->tab_h, c->origin, iter_base(c) + c->ky[KY_OFFG]) : c->rng;
	prof_begin(c);
	hipLaunchKernelGGL(k_find_prop, dim3((N + 255) / 256), dim3(256), 0, c->stream, c->d, (const double *)c->d_S, c->d_Fprop, base);
	prof_end(c, "k_find_prop");
	prof_begin(c);
	hipLaunchKernelGGL((k_loglikF<256, true>), dim3(N), dim3(256), 0, c->stream, c->d, c->d_S, (const double *)c->d_Fprop);
	prof_end(c, "k_loglikF_pair");
	HIPCHK(hipGetLastError());
	if (!is_keyed(c)) host_advance(c, 2ull * (unsigned)N);
	c->h_S = false;
	return 0;
}

static int indiv_cal_lkh_F(isg_ctx *c)
{
	prof_begin(c);
	hipLaunchKernelGGL((k_loglikF<256, false>), dim3(c->cfg.N), dim3(256), 0, c->stream, c->d, c->d_S, (const double *)nullptr);
	prof_end(c, "k_loglik_lkh");
	prof_begin(c);
	hipLaunchKernelGGL(k_lkh_total<1024>, dim3(1), dim3(1024), 0, c->stream, c->d, c->d_total);
	prof_end(c, "k_lkh_total");
	HIPCHK(hipGetLastError());
	c->h_lkh = false;
	return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* mode 0 (`-v 0`, mcmc_POP_no_admixture, mcmc.c:90-132): no admixture, a whole individual belongs to one cluster.  */
/* update_Z (mcmc.c:1094-1120): K log-likelihoods of the individual (log_ld_indv_K, mcmc.c:1893-1914: sums of      */
/* log freq over its allele copies -> the lftab table), exp-normalised, one uniform.  One workgroup per individual; */
/* zz[i] is kept in gen[i] (this mode has no generations) and mirrored into the individual's z bytes so that       */
/* update_P's allele counts (mcmc.c:825-829) are k_count's.  what: 0 initial draw, 1 update, 2 log-likelihood only. */
/* ------------------------------------------------------------------------------------------ */
template <int BLOCK, int KC>
__device__ __forceinline__ void z0_body(DevView d, isg_wh base, unsigned long long stride, int what)
{
	__shared__ long long sm[(BLOCK / 64) * 3];
	__shared__ double ld[KC];
	__shared__ int zsh;
	const int i = blockIdx.x, K = d.K, t = threadIdx.x;
	const size_t rowb = (size_t)d.Lp * 2;
	const uint8_t *grow = d.geno + (size_t)i * rowb;
	if (what != 0) {
		const double log2c = isg_log(2.0);
		for (int m = 0; m < K; m++) { /* one exact sum per cluster (K passes over the row: it stays in L1/L2) */
			if (what == 2 && m != d.gen[i]) continue;
			isg_acc2 a;
			isg_acc2_zero(&a);
			for (int j = t; j < d.L; j += BLOCK) {
				const unsigned short g = *(const unsigned short *)(grow + (size_t)j * 2);
				const unsigned a0 = g & 0xff, a1 = g >> 8;
				if (a0 == 0xff) continue;
				isg_acc2_add(&a, d.lftab[((size_t)j * d.Amax + a0) * K + m]);
				isg_acc2_add(&a, d.lftab[((size_t)j * d.Amax + a1) * K + m]);
				if (a0 != a1) isg_acc2_add(&a, log2c);
			}
			const isg_acc2 r = block_reduce_acc2<BLOCK>(a, sm);
			if (t == 0) ld[m] = isg_acc2_value(&r);
			__syncthreads();
		}
	}
	if (t == 0) {
		int zz = d.gen[i];
		if (what != 2) {
			double cum[KC];
			for (int m = 0; m < K; m++) {
				if (what == 0) cum[m] = (double)(m + 1) / K;
				else {
					cum[m] = isg_exp(ld[m] - ld[0]);
					if (m >= 1) cum[m] += cum[m - 1];
				}
			}
			isg_wh s = isg_wh_jump(d.tab, base, stride * (unsigned)i);
			zz = isg_bucket(isg_wh_next(&s), cum, K);
			d.gen[i] = zz;
		}
		if (what != 0) d.indvlkh[i] = ld[zz];
		zsh = zz;
	}
	__syncthreads();
	if (what != 2) {
		const unsigned short zw = (unsigned short)(zsh | (zsh << 8));
		for (int j = t; j < d.L; j += BLOCK)
			if (grow[(size_t)j * 2] != 0xff) *(unsigned short *)(d.z + (size_t)i * rowb + (size_t)j * 2) = zw;
	}
}
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_z0(DevView d, isg_wh base, unsigned long long stride, int what) { z0_body<BLOCK, ISG_KCAP>(d, base, stride, what); }
template <int BLOCK> /* K > ISG_KCAP */
__global__ void __launch_bounds__(BLOCK) k_z0_w(DevView d, isg_wh base, unsigned long long stride, int what) { z0_body<BLOCK, ISG_KWIDE>(d, base, stride, what); }

static int noadm_update_Z(isg_ctx *c, int init_flag)
{
	const int N = c->cfg.N;
	isg_wh base;
	unsigned long long stride;
	if (is_keyed(c)) {
		base = isg_wh_jump(&c->tab_h, c->origin, init_flag ? 1 : iter_base(c) + c->ky[KY_OFFG]);
		stride = 2;
	} else {
		base = c->rng;
		stride = 1;
	}
	prof_begin(c);
	if (c->cfg.K > ISG_KCAP) hipLaunchKernelGGL(k_z0_w<256>, dim3(N), dim3(256), 0, c->stream, c->d, base, stride, init_flag ? 0 : 1);
	else hipLaunchKernelGGL(k_z0<256>, dim3(N), dim3(256), 0, c->stream, c->d, base, stride, init_flag ? 0 : 1);
	prof_end(c, "k_z0");
	HIPCHK(hipGetLastError());
	if (!is_keyed(c)) host_advance(c, (uint64_t)N);
	c->h_gen = false;
	c->h_lkh = false;
	return 0;
}

static int noadm_cal_lkh(isg_ctx *c)
{
	prof_begin(c);
	if (c->cfg.K > ISG_KCAP) hipLaunchKernelGGL(k_z0_w<256>, dim3(c->cfg.N), dim3(256), 0, c->stream, c->d, c->rng, 0ull, 2);
	else hipLaunchKernelGGL(k_z0<256>, dim3(c->cfg.N), dim3(256), 0, c->stream, c->d, c->rng, 0ull, 2);
	prof_end(c, "k_z0_lkh");
	prof_begin(c);
	hipLaunchKernelGGL(k_lkh_total<1024>, dim3(1), dim3(1024), 0, c->stream, c->d, c->d_total);
	prof_end(c, "k_lkh_total");
	HIPCHK(hipGetLastError());
	c->h_lkh = false;
	return 0;
}
