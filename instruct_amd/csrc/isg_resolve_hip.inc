/*
 * isg_resolve_hip.inc -- replay-schedule update_ZQ (mcmc.c:1122-1203) without a serial chain over the individuals.
 *
 * In the replay schedule individual i+1 starts where individual i's Dirichlet (random.c:264-280, rejection samplers
 * :167-250) stopped, so the start positions form a recurrence  off[i+1] = off[i] + 2 nvalid[i] + used_i(off[i]).  The
 * kernels in isg_coop_hip.inc walk that recurrence one individual per inter-workgroup hand-off (3.9 us each at config 3).
 * Here the recurrence is RESOLVED first, a block of individuals at a time on the whole chip, and the sweep itself
 * (Z draws, counts, qq) is then one parallel pass over all individuals at their known positions:
 *
 *   off[i] = B[i] + 2 e[i],   B[i] = sum_{i' < i} (2 nvalid[i'] + 2 K)   (every gamma takes at least one attempt of two
 *                                                                         uniforms; B is a property of the data)
 *   e[i+1] = e[i] + c_i(e[i]), c_i(e) = rejected attempts of individual i's Dirichlet when it starts at B[i] + 2 e.
 *
 * c_i(e) only depends on (i, e): for a block of D consecutive individuals whose first one has a known e = E, individual
 * r of the block can only have e in a window  E + [lo_r, lo_r + w_r)  (a random walk: mean mu r, spread sigma sqrt r;
 * mu, sigma measured on the previous sweep).  k_zq_block evaluates c for EVERY (individual, candidate e) of the block
 * -- one workgroup (a UNIT) per (individual, 4 candidates): all its loci's Z draws for the 4 start positions (single precision
 * filter against normalised running sums; the few undecidable draws are noted and taken exactly in double after the loop),
 * counts, then the Dirichlet's consumption, one wave per candidate -- and every workgroup then walks the table for itself:
 * e -> e + c[r][e] for r = 0, 1, ...  A walk that leaves a window ends the block there (the next block starts at that individual
 * with its known e).
 *
 * k_zq_blocks does all blocks in ONE launch: the workgroups stay, a block's table travels as one tagged 8-byte granule per unit
 * (agent-scope store, polled; bounded waits, common abort word); all workgroups must be resident together (two per compute unit).
 * k_zq_block is the same block as one launch (the table travels through the kernel boundary: no polling, no co-residency
 * requirement) -- used when the device carries other contexts of this process, after a timed-out wait, or on request
 * (INSTRUCT_ZQ_RESOLVE_PERSIST=0).
 *
 * k_zq_at then runs the sweep proper, one workgroup per individual at off[i] (the keyed schedule's kernel body), and checks
 * that every Dirichlet consumed exactly what the resolution said.  Anything irregular -- a shape of exactly 1 (odd
 * consumption), more than 250 rejections, a check that fails, a wait that timed out -- makes the host redo the sweep with the
 * chain kernels (isg_coop_hip.inc; the chain form of k_zq in isg_hip.hip) from the saved state.  Same Z, counts, qq and
 * stream position in every case.
 */
#define ISG_RS_CH 4     /* candidates per unit = waves per workgroup (one Dirichlet per wave) */
#define ISG_RS_UMAX 512 /* units per block (workgroups of the launch) */
#define ISG_RS_DMAX 64  /* individuals per block */
#ifndef ISG_RS_PB
#define ISG_RS_PB 2     /* passes of 256 loci per batch */
#endif
#ifndef ISG_RS_OCC
#define ISG_RS_OCC 2    /* workgroups per compute unit the block kernels' register budget allows (waves per SIMD) */
#endif
#define ISG_RS_WMAX 128 /* candidates per individual the walk can look at (plan windows are cut to this) */
#define ISG_RS_EVMAX 256 /* notes of undecided draws per unit (about 0.6 on average) */
#define ISG_RS_IRR 255u /* table entry: consumption not representable (odd, or more than 250 rejections) */

struct ResolvePlan {
	int D, nunits;
	short lo[ISG_RS_DMAX];    /* first candidate of individual r, relative to the block's E */
	short w[ISG_RS_DMAX];     /* candidates of individual r (a multiple of ISG_RS_CH) */
	short cbase[ISG_RS_DMAX]; /* its first table slot */
	short ur[ISG_RS_UMAX];    /* unit -> individual of the block */
	short uo[ISG_RS_UMAX];    /* unit -> its first candidate, relative to E */
	short cslot[ISG_RS_UMAX]; /* unit -> where its first table byte goes in the walk's LDS image (the next three: + 4, + 8, + 12):
	                           * byte r % 4 of dword (r / 4) * ISG_RS_WMAX + (uo - lo[r]) */
};
/* rec[b & 3]: what launch b worked on; done / fail / total for the host */
struct ResolveState {
	unsigned long long d0[4], E[4];
	unsigned done, fail;
	unsigned long long total;     /* uniforms consumed by the whole phase */
	unsigned long long nblocks, nmiss, sumc, sumc2, nind;
	unsigned long long nexact; /* (locus, candidate) pairs redone exactly */
	unsigned char ctab[2][ISG_RS_UMAX * ISG_RS_CH];
};

/* the phase's uniforms as floats, stream order: the pre-filter's input (8 per lane: one skip-ahead, then stepping) */
__global__ void __launch_bounds__(256) k_tapef(const isg_wh_tables *tab, isg_wh base, unsigned long long n, float *tape)
{
	const unsigned long long p0 = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 8ull;
	if (p0 >= n) return;
	isg_wh s = isg_wh_jump(tab, base, p0);
	float v[8];
#pragma unroll
	for (int k = 0; k < 8; k++) v[k] = (float)isg_wh_next(&s);
	if (p0 + 8 <= n) {
		float4 *o = (float4 *)(tape + p0);
		o[0] = make_float4(v[0], v[1], v[2], v[3]);
		o[1] = make_float4(v[4], v[5], v[6], v[7]);
	} else {
		for (int k = 0; k < 8 && p0 + k < n; k++) tape[p0 + k] = v[k];
	}
}

#ifdef ISG_STAMPS
#define STAMPB(b, k) do { if (threadIdx.x == 0 && blockIdx.x == ISG_STAMP_UNIT && (b) < 2048) g_stamps[(b) * 8 + (k)] = __builtin_readcyclecounter(); \
	if (threadIdx.x == 0 && (b) == 50 && blockIdx.x < 1024) g_stamps[(2048 + blockIdx.x) * 8 + (k)] = __builtin_readcyclecounter(); } while (0)
#ifndef ISG_STAMP_UNIT
#define ISG_STAMP_UNIT 40
#endif
#define STAMPW(b, k) do { if (threadIdx.x == 0 && blockIdx.x == ISG_STAMP_UNIT && (b) < 2048) g_stamps2[(b) * 8 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define STAMPB(b, k) do { } while (0)
#define STAMPW(b, k) do { } while (0)
#endif
/*
 * Start of a block, shared by the diploid and the ploidy-4 block kernels.  Walks the previous block's table (every workgroup
 * for itself: wave 0 holds the plan -- lane r: window of individual r -- and the table -- lane x: column x of every row -- in
 * registers; a step is a few scalar operations and v_readlane, no memory access on the chain), lets workgroup 0 record the
 * resolved positions and the statistics, and tells this unit its individual.  Contains a workgroup barrier: call from all 256
 * threads.
 */
/* Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8); the units of one individual are consecutive, and they all read
 * that individual's genotype row and stretch of the uniform tape.  Unit of block b = the b/8-th unit of XCD (b % 8)'s contiguous share:
 * an individual's units then sit on one XCD (or two) and its tape stretch is fetched into one L2 instead of eight (measured: 12.8 MB of
 * HBM reads per launch without this, for 1.5 MB of distinct data).  Placement-independent for correctness: it is a bijection. */
__device__ __forceinline__ int rs_unit_of_block(int bid, int nu)
{
	const int x = bid & 7, idx = bid >> 3, q = nu >> 3, rem = nu & 7;
	return x * q + (x < rem ? x : rem) + idx;
}
/* returns 0: evaluate individual *i_out; 1: nothing for this workgroup in this block; 2: the phase is over (resolved, or failed).
 * PERSIST (k_zq_blocks, one launch for the whole phase): the previous block's table arrives as one tagged 8-byte granule per unit
 * (low word: the unit's 4 table bytes, high word: block number + 1), polled with agent-scope loads; the previous block's (d0, E)
 * are the workgroup's own (blk_s).  Otherwise (k_zq_block, one launch per block) both come from ResolveState. */
#define RS_CONTINUE 0
#define RS_IDLE 1
#define RS_OVER 2
template <bool PERSIST>
__device__ __forceinline__ int rs_block_start(int u, int N, const ResolvePlan *plan, ResolveState *st, const unsigned long long *Bpre, unsigned long long *offs, int b,
					      unsigned *e_s /* [DMAX] LDS */, unsigned long long *blk_s /* [5] LDS */, unsigned char *cs /* [DMAX * WMAX] LDS */,
					      int *i_out, unsigned long long *E_out, const unsigned long long *gran_prev, unsigned *abort_flag)
{
	constexpr int CH = ISG_RS_CH;
	const int t = threadIdx.x, lane = (int)lane_id();
	const int D = plan->D, NUC = plan->nunits * CH;
	if (t < 64) {
		unsigned long long nd0 = 0, nE = 0, pd0 = 0, pE = 0;
		int rr = 0;
		unsigned stop = 0;
		if (!PERSIST) /* an earlier launch failed or finished: nothing to do (one wave reads the flags: workgroup 0 of this very launch may be setting them) */
			stop = __builtin_amdgcn_readfirstlane(st->fail | st->done);
		if (stop) {
			nd0 = ~0ull;
		} else if (b > 0) {
			/* The previous block's table goes through LDS into wave 0's REGISTERS: cs as dwords [row / 4][rel], byte row % 4 = the table
			 * byte of (individual `row` of the block, candidate lo[row] + rel), 255 = not evaluated / irregular; lane x then holds
			 * column rel = x (ta) and x + 64 (tb, only for windows wider than 64) of every row.  A step of the walk is two scalar
			 * compares and one v_readlane with a static register and a scalar lane number -- no memory access on the chain (a
			 * dependent LDS read per step made it 430 cycles a step: 14 k cycles for a block of 33 individuals). */
			constexpr int G = ISG_RS_DMAX / 4;
			const int plo = (lane < D) ? plan->lo[lane] : 0, pw = (lane < D) ? plan->w[lane] : 0;
			const int nun = NUC / CH, ng = (D + 3) / 4;
			const bool wide = __any(pw > 64);
			for (int k = lane; k < ng * ISG_RS_WMAX; k += 64) ((unsigned *)cs)[k] = 0xffffffffu;
			bool timed_out = false;
			if (PERSIST) {
				/* all of this lane's granules requested together, again until every one carries this block's tag (bounded; a
				 * common abort word ends everybody's wait) */
				constexpr int Q = ISG_RS_UMAX / 64;
				unsigned long long v[Q];
				int slot[Q]; /* (read before the wait, not after it) */
#pragma unroll
				for (int q = 0; q < Q; q++) slot[q] = (lane + 64 * q < nun) ? plan->cslot[lane + 64 * q] : 0;
				for (unsigned spin = 0;; spin++) {
					bool all = true;
#pragma unroll
					for (int q = 0; q < Q; q++) {
						const int un = lane + 64 * q;
						if (un < nun) {
							v[q] = ld_agent(gran_prev + un);
							all = all && ((unsigned)(v[q] >> 32) == (unsigned)b);
						}
					}
					if (__all(all)) break;
					if ((spin & 255u) == 255u) {
						if (__hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { timed_out = true; break; }
						if (spin > (1u << 18)) { /* about a second; a block takes 30 us */
							__hip_atomic_store(abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							timed_out = true;
							break;
						}
					}
					__builtin_amdgcn_s_sleep(1);
				}
#ifndef ISG_STAMPS_EV
				STAMPB(b, 1); /* all granules of the previous block have arrived */
#endif
#pragma unroll
				for (int q = 0; q < Q; q++) {
					const int un = lane + 64 * q;
					if (un < nun) {
						unsigned char *dst = cs + slot[q];
						const unsigned tv = (unsigned)v[q];
						dst[0] = (unsigned char)tv; dst[4] = (unsigned char)(tv >> 8); dst[8] = (unsigned char)(tv >> 16); dst[12] = (unsigned char)(tv >> 24);
					}
				}
				STAMPW(b, 0);
				pd0 = __builtin_amdgcn_readfirstlane((unsigned)blk_s[0]) | ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(blk_s[0] >> 32)) << 32);
				pE = __builtin_amdgcn_readfirstlane((unsigned)blk_s[1]) | ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(blk_s[1] >> 32)) << 32);
			} else {
				const unsigned *src4 = (const unsigned *)st->ctab[(b - 1) & 1];
				for (int un = lane; un < nun; un += 64) {
					unsigned char *dst = cs + plan->cslot[un];
					const unsigned tv = src4[un];
					dst[0] = (unsigned char)tv; dst[4] = (unsigned char)(tv >> 8); dst[8] = (unsigned char)(tv >> 16); dst[12] = (unsigned char)(tv >> 24);
				}
				pd0 = st->d0[(b - 1) & 3];
				pE = st->E[(b - 1) & 3];
			}
			STAMPW(b, 1);
			__builtin_amdgcn_wave_barrier();
			unsigned ta[G], tb[G];
#pragma unroll
			for (int g = 0; g < G; g++) {
				ta[g] = ((const unsigned *)cs)[g * ISG_RS_WMAX + lane];
				tb[g] = 0xffffffffu;
			}
			if (wide) {
#pragma unroll
				for (int g = 0; g < G; g++) tb[g] = ((const unsigned *)cs)[g * ISG_RS_WMAX + 64 + lane];
			}
			const int nleft = (pd0 + (unsigned long long)D <= (unsigned long long)N) ? D : (int)((unsigned long long)N - pd0);
			unsigned e = 0, my_e = 0; /* relative to pE */
			bool irr = timed_out;
#ifdef ISG_STAMPS
			if (ta[0] + ta[G - 1] + tb[G - 1] == 0x12345u) irr = true; /* (never; makes the stamp wait for the loads) */
			STAMPW(b, 2);
#endif
			if (!wide && !timed_out) {
				/* Ten instructions a step (a lone wave issues one every 4 cycles; nested conditions took 60 and taken branches):
				 *   rel = e - lo[r];  lane r of my_e = e;  cv = byte r % 4 of lane rel of row group r / 4;  rr = min(rr, rel < w[r] ? 64 : r);  e += cv
				 * Nothing is masked after the first step that leaves its window (w = 0 from the end of the data on): later steps can
				 * only propose a larger rr, and the e to continue from is the one the failing step recorded in its lane.  An
				 * irregular entry (255; regular ones are <= 250) throws the next step out of any window (w <= 128, lo moves by a
				 * few), so only the LAST accepted step can have read one: checked after the loop. */
				const int pwl = (lane < nleft) ? pw : 0;
				rr = 64;
#define RS_STEP(r) do { \
		const int lo_ = __builtin_amdgcn_readlane(plo, r), w_ = __builtin_amdgcn_readlane(pwl, r); \
		const unsigned rel_ = e - (unsigned)lo_; \
		asm("v_writelane_b32 %0, %1, " #r : "+v"(my_e) : "s"(e)); \
		const unsigned cv_ = ((unsigned)__builtin_amdgcn_readlane((int)ta[(r) >> 2], (int)(rel_ & 63u)) >> (8 * ((r) & 3))) & 0xffu; \
		const int stop_ = (rel_ < (unsigned)w_) ? 64 : (r); \
		rr = (stop_ < rr) ? stop_ : rr; \
		e += cv_; \
	} while (0)
				if (rr >= 0) { RS_STEP(0); RS_STEP(1); RS_STEP(2); RS_STEP(3); RS_STEP(4); RS_STEP(5); RS_STEP(6); RS_STEP(7); }
				if (rr >= 8) { RS_STEP(8); RS_STEP(9); RS_STEP(10); RS_STEP(11); RS_STEP(12); RS_STEP(13); RS_STEP(14); RS_STEP(15); }
				if (rr >= 16) { RS_STEP(16); RS_STEP(17); RS_STEP(18); RS_STEP(19); RS_STEP(20); RS_STEP(21); RS_STEP(22); RS_STEP(23); }
				if (rr >= 24) { RS_STEP(24); RS_STEP(25); RS_STEP(26); RS_STEP(27); RS_STEP(28); RS_STEP(29); RS_STEP(30); RS_STEP(31); }
				if (rr >= 32) { RS_STEP(32); RS_STEP(33); RS_STEP(34); RS_STEP(35); RS_STEP(36); RS_STEP(37); RS_STEP(38); RS_STEP(39); }
				if (rr >= 40) { RS_STEP(40); RS_STEP(41); RS_STEP(42); RS_STEP(43); RS_STEP(44); RS_STEP(45); RS_STEP(46); RS_STEP(47); }
				if (rr >= 48) { RS_STEP(48); RS_STEP(49); RS_STEP(50); RS_STEP(51); RS_STEP(52); RS_STEP(53); RS_STEP(54); RS_STEP(55); }
				if (rr >= 56) { RS_STEP(56); RS_STEP(57); RS_STEP(58); RS_STEP(59); RS_STEP(60); RS_STEP(61); RS_STEP(62); RS_STEP(63); }
#undef RS_STEP
				if (rr < 64) e = (unsigned)__builtin_amdgcn_readlane((int)my_e, rr); /* where the walk stopped */
				if (rr > 0 && e - (unsigned)__builtin_amdgcn_readlane((int)my_e, rr - 1) == ISG_RS_IRR) irr = true;
			} else if (!timed_out) {
				/* windows wider than 64 candidates (second register set): the same walk with every condition spelled out */
				unsigned alive = 1u, hit_irr = 0u;
#pragma unroll
				for (int r8 = 0; r8 < ISG_RS_DMAX; r8 += 8) {
					if (alive && r8 < nleft) {
#pragma unroll
						for (int r = r8; r < r8 + 8; r++) {
							const int lo = __builtin_amdgcn_readlane(plo, r), w = __builtin_amdgcn_readlane(pw, r);
							const int rel = (int)e - lo;
							const unsigned wa = (unsigned)__builtin_amdgcn_readlane((int)ta[r >> 2], rel & 63), wb = (unsigned)__builtin_amdgcn_readlane((int)tb[r >> 2], rel & 63);
							const unsigned cv = (((rel & 64) ? wb : wa) >> (8 * (r & 3))) & 0xffu;
							const unsigned inwin = (unsigned)(r < nleft) & (unsigned)(rel >= 0) & (unsigned)(rel < w);
							const unsigned reg = (unsigned)(cv != ISG_RS_IRR);
							hit_irr |= alive & inwin & (reg ^ 1u);
							alive &= inwin & reg;
							my_e = (lane == r && alive) ? e : my_e;
							e += cv & (0u - alive);
							rr += (int)alive;
						}
					}
				}
				irr = irr || hit_irr;
			}
			STAMPW(b, 3);
			if (lane < rr) e_s[lane] = my_e;
			if (irr || rr == 0) { /* rr == 0 cannot happen (candidate 0 of individual 0 is always evaluated) unless irregular */
				if ((u == 0 || timed_out) && lane == 0) st->fail = 1;
				nd0 = ~0ull;
			} else {
				nd0 = pd0 + (unsigned long long)rr;
				nE = pE + e;
			}
		}
		if (lane == 0) {
			blk_s[0] = nd0;
			blk_s[1] = nE;
			blk_s[2] = (unsigned long long)rr;
			blk_s[3] = pd0;
			blk_s[4] = pE;
		}
	}
	STAMPW(b, 4);
	__syncthreads();
	const unsigned long long d0 = blk_s[0], E = blk_s[1];
	STAMPB(b, 2);
	if (d0 == ~0ull) return RS_OVER;
	if (u == 0) { /* the record of this block, the resolved positions of the previous block, statistics */
		const int r = (int)blk_s[2];
		if (b > 0) {
			const unsigned long long pd0 = blk_s[3], pE = blk_s[4];
			if (t < r) offs[pd0 + t] = Bpre[pd0 + t] + 2ull * (pE + e_s[t]);
			if (t == 0) {
				unsigned long long sc = 0, sc2 = 0;
				for (int k = 0; k < r; k++) {
					const unsigned long long cv = (k + 1 < r ? e_s[k + 1] : (unsigned)(E - pE)) - e_s[k];
					sc += cv;
					sc2 += cv * cv;
				}
				st->sumc += sc;
				st->sumc2 += sc2;
				st->nind += (unsigned long long)r;
				st->nblocks += 1;
				if (r < D && pd0 + r < (unsigned long long)N) st->nmiss += 1;
			}
		}
		if (t == 0) {
			st->d0[b & 3] = d0;
			st->E[b & 3] = E;
			if (d0 >= (unsigned long long)N) {
				offs[N] = Bpre[N] + 2ull * E;
				st->total = Bpre[N] + 2ull * E;
				__threadfence();
				st->done = 1;
			}
		}
	}
	if (d0 >= (unsigned long long)N) return RS_OVER;
	if (u >= plan->nunits) return RS_IDLE;
	const long long di = (long long)d0 + plan->ur[u];
	if (di >= N) return RS_IDLE;
	*i_out = (int)di;
	*E_out = E;
	return RS_CONTINUE;
}

template <int KMAX>
struct RsShared {
	isg_wh_tables tab;
	unsigned e_s[ISG_RS_DMAX];
	unsigned long long blk_s[5]; /* d0, E, individuals of the previous block the walk resolved, the previous block's d0, E */
	__attribute__((aligned(16))) unsigned char cs[ISG_RS_DMAX * ISG_RS_WMAX];
	int red[ISG_RS_CH][KMAX];
	unsigned cres[ISG_RS_CH];
	struct { unsigned j, rank, info, pad; unsigned long long fneg; } ev[ISG_RS_EVMAX]; /* draws to be taken exactly after the loop */
	unsigned nev, ovf_s;
};
/* one unit of one block: individual i, candidates E + uo[u] .. + CH - 1; returns the unit's 4 table bytes (all 256 threads call;
 * sh.red, sh.nev, sh.ovf_s zeroed by the caller before the workgroup's last barrier) */
template <int KMAX>
__device__ __forceinline__ unsigned rs_eval_unit(const DevView &d, RsShared<KMAX> &sh, const isg_wh &base, double alpha, const ResolvePlan *plan, ResolveState *st,
						 const unsigned long long *Bpre, const float *tapef, unsigned long long tape_len, int u, int i, unsigned long long E, int b)
{
	constexpr int CH = ISG_RS_CH, T = (KMAX > 1) ? KMAX - 1 : 1, KPFC = (KMAX + 3) & ~3; /* KPFC == d.KPF: the host dispatches K == KMAX (K = 1: KMAX = 2) */
	const int t = threadIdx.x, K = (KMAX == 2) ? d.K : KMAX, lane = (int)lane_id(), wv = t >> 6;
	/* ---- this unit: individual i, candidates E + uo .. + CH - 1 ---- */
	const int nv = d.nvalid[i];
	const unsigned long long off0 = Bpre[i] + 2ull * (E + (unsigned long long)plan->uo[u]); /* first candidate's start, from the phase base */
	const bool covered = off0 + 2ull * (CH - 1) + 2ull * (unsigned)nv + 8ull <= tape_len;
	float qf[KMAX];
#pragma unroll
	for (int m = 0; m < KMAX; m++) qf[m] = (m < K) ? (float)d.qq[(size_t)i * K + m] : 0.f;
	const isg_wh cur = isg_wh_jump(&sh.tab, base, off0); /* the stream at the first candidate's start: offsets from here fit 32 bits */
	/* How far the single precision threshold can be from the exact one: each of the (up to K) products q f carries three
	 * roundings, each of the K - 1 additions one more on a partial sum <= tot, the same again for the normaliser, v_rcp_f32 is
	 * good to 1 ulp, the final product and the float image of the uniform round once each: (2 K + 8) 2^-24 in all on values
	 * <= 1.  The band is TWICE that bound (K = 5: 2.1e-6, K = 8: 2.9e-6; 6e-6 redid 3.1 times as many draws). */
	const float band = (float)(2 * K + 8) * 1.1920929e-7f;
	/* cnt[c][m] = draws of candidate c that fall below threshold m = draws with Z <= m */
	unsigned cnt[CH][T];
#pragma unroll
	for (int c = 0; c < CH; c++)
#pragma unroll
		for (int m = 0; m < T; m++) cnt[c][m] = 0;
	double touch = 0.0;
	STAMPB(b, 3);
	if (covered) {
		/* The loci in batches of PB passes of 256.  cnt[c][m] counts the draws of candidate c that fall BELOW threshold m (sign
		 * bits of x - t).
		 * Addresses: a uniform base per unit (scalar registers) + a 32-bit byte offset per lane (the host checks that the
		 * tables stay below 4 GB): no 64-bit vector arithmetic, no 32-bit vector multiplies in the loop. */
		constexpr int PB = ISG_RS_PB, Q4 = (KMAX + 3) / 4;
		struct Geno { unsigned short gg[PB]; unsigned rw[PB]; };
		struct Data { unsigned a0[PB], a1[PB], rank[PB]; float2 xs[PB][CH]; float4 R[PB][2][Q4]; };
		const int NB = (d.Lp + 256 * PB - 1) / (256 * PB);
		const char *gbase = (const char *)d.geno + (size_t)i * (size_t)d.Lp * 2, *rwbase = (const char *)(d.rankwave + (size_t)i * d.nwv);
		const char *tbase = (const char *)(tapef + off0), *fbase = (const char *)d.freqf;
		const unsigned lastj = (unsigned)d.Lp - 1u, amax = (unsigned)d.Amax;
		/* every load is issued by every lane (a lane without a locus reads the last locus and ignores the result): straight-line code */
		auto load_geno = [&](int bb, Geno &G) {
#pragma unroll
			for (int p = 0; p < PB; p++) {
				const unsigned j = (unsigned)((bb * PB + p) * 256 + t), jc = (j < lastj) ? j : lastj;
				const unsigned short g = *(const unsigned short *)(gbase + jc * 2u);
				G.gg[p] = (j <= lastj) ? g : (unsigned short)0xffff;
				G.rw[p] = *(const unsigned *)(rwbase + (jc >> 6) * 4u);
			}
		};
		auto load_data = [&](int bb, const Geno &G, Data &X) {
#pragma unroll
			for (int p = 0; p < PB; p++) {
				const unsigned j = (unsigned)((bb * PB + p) * 256 + t), jc = (j < lastj) ? j : lastj;
				X.a0[p] = G.gg[p] & 0xff;
				X.a1[p] = G.gg[p] >> 8;
				const bool valid = (X.a0[p] != 0xff);
				X.rank[p] = G.rw[p] + (unsigned)__popcll(__ballot(valid) & ((1ull << lane) - 1ull));
				/* the uniforms of the CH candidates: copy k of candidate c at off0 + 2 c + 2 rank + k (rank <= nv: inside the tape) */
				const float2 *tp = (const float2 *)(tbase + X.rank[p] * 8u);
#pragma unroll
				for (int c = 0; c < CH; c++) X.xs[p][c] = tp[c];
				const unsigned row = __umul24(jc, amax); /* Lp, Amax < 2^24 */
				const char *P0 = fbase + (row + (valid ? X.a0[p] : 0u)) * (unsigned)(KPFC * 4), *P1 = fbase + (row + (valid ? X.a1[p] : 0u)) * (unsigned)(KPFC * 4);
#pragma unroll
				for (int q4 = 0; q4 < Q4; q4++) {
					X.R[p][0][q4] = *(const float4 *)(P0 + 16 * q4);
					X.R[p][1][q4] = *(const float4 *)(P1 + 16 * q4);
				}
			}
		};
		auto compute = [&](int bb, const Data &X) {
#pragma unroll
			for (int p = 0; p < PB; p++) {
				const int j = (bb * PB + p) * 256 + t;
				const bool valid = (X.a0[p] != 0xff);
				float th[2][T], minrun = 3.0e38f;
#pragma unroll
				for (int k = 0; k < 2; k++) { /* normalised running sums: Z = #{m <= K-2 : cum[m] / tot < x} */
					float F[KMAX], cum[KMAX];
#pragma unroll
					for (int m = 0; m < KMAX; m++) {
						const float4 v = X.R[p][k][m >> 2];
						F[m] = ((m & 3) == 0) ? v.x : ((m & 3) == 1) ? v.y : ((m & 3) == 2) ? v.z : v.w;
					}
					const float run = prefix_f32<KMAX>(F, qf, K, cum);
					minrun = __builtin_fminf(minrun, run);
					/* 1 ulp: inside the band's allowance.  A lane without a used locus gets thresholds <= 0: nothing below */
					const float inv = valid ? __builtin_amdgcn_rcpf(run) : -1.0f;
#pragma unroll
					for (int m = 0; m < T; m++) th[k][m] = (m < K - 1) ? cum[m] * inv : -1.0f;
				}
				/* sign bits of x - t counted; the smallest |x - t| of all candidates and thresholds decides whether anything here
				 * needs the exact treatment (which candidates: worked out in the rare branch) */
				float mn = 3.0e38f;
#pragma unroll
				for (int c = 0; c < CH; c++) {
#pragma unroll
					for (int m = 0; m < T; m++) {
						const float d0f = X.xs[p][c].x - th[0][m], d1f = X.xs[p][c].y - th[1][m];
						cnt[c][m] += (__float_as_uint(d0f) >> 31) + (__float_as_uint(d1f) >> 31);
						if (m < K - 1) mn = __builtin_fminf(__builtin_fminf(mn, __builtin_fabsf(d0f)), __builtin_fabsf(d1f));
					}
				}
				/* sums q f are at most K; one that is not comfortably normal (or a NaN) sends the locus to the exact path */
				const bool amb = !(mn > band) || !(minrun > 1e-30f);
				/* a draw within `band` of a threshold: that candidate's two draws at this locus are noted (locus, stream rank, alleles,
				 * candidates, what the filter counted for them) and taken exactly after the loop, which also takes the filter's counts
				 * back: the loop stays straight-line and nobody in the workgroup waits for a neighbour's double precision detour */
				if (valid && amb) {
					unsigned ambc = 0;
					if (!(minrun > 1e-30f)) {
						ambc = (1u << CH) - 1u;
					} else {
#pragma unroll
						for (int c = 0; c < CH; c++) {
							float x0 = X.xs[p][c].x, x1 = X.xs[p][c].y, mc = 3.0e38f;
							asm volatile("" : "+v"(x0), "+v"(x1));
#pragma unroll
							for (int m = 0; m < T; m++)
								if (m < K - 1) mc = __builtin_fminf(__builtin_fminf(mc, __builtin_fabsf(x0 - th[0][m])), __builtin_fabsf(x1 - th[1][m]));
							ambc |= (mc > band) ? 0u : (1u << c);
						}
					}
					const unsigned slot = atomicAdd(&sh.nev, 1u);
					if (slot < ISG_RS_EVMAX) {
						/* (the empty asm statements keep this rare path's arithmetic inside the branch: hoisted, the packing of the
						 * filter's counts and the address of the double precision rows cost every pass 30 instructions) */
						unsigned long long fn = 0;
#pragma unroll
						for (int c = 0; c < CH; c++) {
							float x0 = X.xs[p][c].x, x1 = X.xs[p][c].y;
							asm volatile("" : "+v"(x0), "+v"(x1));
#pragma unroll
							for (int m = 0; m < T; m++) {
								const unsigned ng = (__float_as_uint(x0 - th[0][m]) >> 31) + (__float_as_uint(x1 - th[1][m]) >> 31); /* as counted above */
								fn |= (unsigned long long)ng << (2 * (c * T + m));
							}
						}
						unsigned jj = (unsigned)j;
						asm volatile("" : "+v"(jj));
						sh.ev[slot].j = jj;
						sh.ev[slot].rank = X.rank[p];
						sh.ev[slot].info = X.a0[p] | (X.a1[p] << 8) | (ambc << 16);
						sh.ev[slot].fneg = fn;
						/* the double precision rows the exact draw will read: requested now, used after the loop */
						touch = d.freq[((size_t)jj * d.Amax + X.a0[p]) * d.KP] + d.freq[((size_t)jj * d.Amax + X.a1[p]) * d.KP + (K > 4 ? 4 : 0)];
					}
				}
			}
		};
		Geno g0;
		Data x0;
#ifdef ISG_LOOP_TWICE /* diagnostic: the loop once with cold, once with warm caches (the first run's counts and notes are dropped) */
		for (int bb = 0; bb < NB; bb++) { load_geno(bb, g0); load_data(bb, g0, x0); compute(bb, x0); }
		for (int c = 0; c < CH; c++) for (int m = 0; m < T; m++) cnt[c][m] = 0;
		__syncthreads();
		if (t == 0) sh.nev = 0;
		__syncthreads();
		STAMPW(b, 5);
#endif
		/* the next batch's genotype bytes are requested before this batch is evaluated; its rows and uniforms (whose addresses need
		 * those bytes) after.  The second workgroup on the compute unit fills the wait.  (Measured: two batches of four passes in
		 * flight per wave need all 256 + 91 registers -- one workgroup per compute unit -- and took 9.4 ms per sweep at config 3;
		 * this loop 8.8 ms at one workgroup per compute unit, 7.5 ms at two.) */
		load_geno(0, g0);
		for (int bb = 0; bb < NB; bb++) { /* wave-uniform trip count */
			load_data(bb, g0, x0);
			load_geno(bb + 1, g0);
			compute(bb, x0);
		}
#pragma unroll
		for (int c = 0; c < CH; c++)
#pragma unroll
			for (int m = 0; m < T; m++) {
				if (m < K - 1) {
					const unsigned s = wave_sum_u32(cnt[c][m]);
					if (lane == 0 && s) atomicAdd(&sh.red[c][m], (int)s);
				}
			}
	}
	STAMPB(b, 4);
	__syncthreads();
	if (covered) { /* the noted draws exactly, as the reference takes them (disc_unif, random.c:403-430) */
		const unsigned n = sh.nev < ISG_RS_EVMAX ? sh.nev : ISG_RS_EVMAX;
		for (unsigned e = (unsigned)wv; e < n && lane == 0; e += 4) { /* one note per WAVE at a time: lanes of one wave would take their notes' candidates one after the other */
			const unsigned j = sh.ev[e].j, rank = sh.ev[e].rank, a0 = sh.ev[e].info & 0xff, a1 = (sh.ev[e].info >> 8) & 0xff, cm = sh.ev[e].info >> 16;
			const unsigned long long fneg = sh.ev[e].fneg;
			double q[KMAX], cumd[2][KMAX], tot[2];
#pragma unroll
			for (int m = 0; m < KMAX; m++) q[m] = (m < K) ? d.qq[(size_t)i * K + m] : 0.0;
			tot[0] = weights<KMAX>(d.freq + ((size_t)j * d.Amax + a0) * d.KP, q, cumd[0], K);
			tot[1] = weights<KMAX>(d.freq + ((size_t)j * d.Amax + a1) * d.KP, q, cumd[1], K);
#ifdef ISG_STAMPS_EV
			if (tot[0] + tot[1] == -1.0) sh.ovf_s = 1u; /* (diagnostic build: make the stamp below wait for the loads) */
			STAMPB(b, 1);
#endif
			for (int c = 0; c < CH; c++) {
				if ((cm >> c) & 1u) {
#ifdef ISG_STAMPS
					atomicAdd(&st->nexact, 1ull);
#endif
					isg_wh s = isg_wh_jump32(&sh.tab, cur, 2u * (unsigned)c + 2u * rank);
					const int z0 = bucket_fast<KMAX>(isg_wh_next(&s), cumd[0], tot[0], K);
					const int z1 = bucket_fast<KMAX>(isg_wh_next(&s), cumd[1], tot[1], K);
					for (int m = 0; m < K - 1; m++) { /* the exact count in place of the filter's */
						const int v = ((z0 > m) ? 0 : 1) + ((z1 > m) ? 0 : 1) - (int)((fneg >> (2 * (c * T + m))) & 3ull);
						if (v) atomicAdd(&sh.red[c][m], v);
					}
				}
			}
		}
		if (touch == -1.0) sh.ovf_s = 1u; /* (consumes the warming loads; a frequency is never negative) */
		if (sh.nev > ISG_RS_EVMAX && t == 0) sh.ovf_s = 1u; /* more notes than slots (never at a 2e-6 band): report the unit as irregular */
	}
	__syncthreads();
	STAMPB(b, 5);
	/* ---- the Dirichlet of candidate wv: its consumption ---- */
	{
		const int c = wv;
		const int *C = sh.red[c];
		auto cntf = [&](int m) -> int { /* counts per cluster from the cumulative ones: C[m] = draws with Z <= m */
			const int upto = (m < K - 1) ? C[m] : 2 * nv, before = (m == 0) ? 0 : C[m - 1];
			return upto - before;
		};
		const unsigned long long dpos = 2ull * (unsigned)c + 2ull * (unsigned)nv; /* from `cur` */
		unsigned cv = ISG_RS_IRR;
		if (covered && !sh.ovf_s) {
			const unsigned used = dirichlet_wave_f<KMAX>(d, &sh.tab, cntf, i, cur, dpos, alpha, nullptr, false);
			if (!(used & 1u) && used >= 2u * (unsigned)K && (used - 2u * (unsigned)K) / 2u <= 250u) cv = (used - 2u * (unsigned)K) / 2u;
		}
		if (lane == 0) sh.cres[c] = cv;
	}
	STAMPB(b, 6);
	__syncthreads();
	return sh.cres[0] | (sh.cres[1] << 8) | (sh.cres[2] << 16) | (sh.cres[3] << 24);
}

template <int KMAX>
__global__ void __launch_bounds__(256, ISG_RS_OCC) k_zq_block(DevView d, isg_wh base, double alpha, const ResolvePlan *plan, ResolveState *st, const unsigned long long *Bpre,
						  const float *tapef, unsigned long long tape_len, unsigned long long *offs, int b)
{
	__shared__ RsShared<KMAX> sh;
	const int t = threadIdx.x, u = rs_unit_of_block((int)blockIdx.x, (int)gridDim.x);
	STAMPB(b, 0);
	{
		const uint16_t *src = (const uint16_t *)d.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += 256) dst[k] = src[k];
		if (t < ISG_RS_CH * KMAX) (&sh.red[0][0])[t] = 0;
		if (t == 0) { sh.nev = 0; sh.ovf_s = 0; }
	}
	int i = 0;
	unsigned long long E = 0;
	if (rs_block_start<false>(u, d.N, plan, st, Bpre, offs, b, sh.e_s, sh.blk_s, sh.cs, &i, &E, nullptr, nullptr) != RS_CONTINUE) return;
	const unsigned packed = rs_eval_unit<KMAX>(d, sh, base, alpha, plan, st, Bpre, tapef, tape_len, u, i, E, b);
	if (t == 0) ((unsigned *)st->ctab[b & 1])[u] = packed;
	STAMPB(b, 7);
}

/* The whole resolution in ONE launch: every workgroup stays, block after block; a block's table travels as tagged granules
 * (rs_block_start<true>) instead of through a kernel boundary.  All gridDim.x workgroups must be resident together (the host
 * checks the occupancy); every wait is bounded and watches *abort_flag.  Every workgroup walks the same tables, so all of them
 * see the same (d0, E) and leave the loop in the same block. */
template <int KMAX>
__global__ void __launch_bounds__(256, ISG_RS_OCC) k_zq_blocks(DevView d, isg_wh base, double alpha, const ResolvePlan *plan, ResolveState *st, const unsigned long long *Bpre,
						   const float *tapef, unsigned long long tape_len, unsigned long long *offs, unsigned long long *gran /* [2][ISG_RS_UMAX] */,
						   unsigned *abort_flag)
{
	__shared__ RsShared<KMAX> sh;
	const int t = threadIdx.x, u = rs_unit_of_block((int)blockIdx.x, (int)gridDim.x);
	{
		const uint16_t *src = (const uint16_t *)d.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += 256) dst[k] = src[k];
	}
	for (int b = 0; b <= d.N + 1; b++) { /* a block resolves at least one individual */
		STAMPB(b, 0);
		__syncthreads(); /* (a workgroup that sat the previous block out took none of its barriers: its waves must be done reading blk_s before wave 0 writes it again) */
		if (t < ISG_RS_CH * KMAX) (&sh.red[0][0])[t] = 0;
		if (t == 0) { sh.nev = 0; sh.ovf_s = 0; }
		int i = 0;
		unsigned long long E = 0;
		const int what = rs_block_start<true>(u, d.N, plan, st, Bpre, offs, b, sh.e_s, sh.blk_s, sh.cs, &i, &E, gran + (size_t)((b - 1) & 1) * ISG_RS_UMAX, abort_flag);
		if (what == RS_OVER) break;
		unsigned packed = 0xffffffffu; /* ISG_RS_IRR four times */
		if (what == RS_CONTINUE) packed = rs_eval_unit<KMAX>(d, sh, base, alpha, plan, st, Bpre, tapef, tape_len, u, i, E, b);
		if (t == 0) st_agent(&gran[(size_t)(b & 1) * ISG_RS_UMAX + u], ((unsigned long long)(unsigned)(b + 1) << 32) | packed);
		STAMPB(b, 7);
	}
}

/* the sweep at the resolved positions: Z, qqnum, qq of individual i = blockIdx.x, and the check that its Dirichlet
 * consumed what the resolution said */
template <int BLOCK, int KMAX>
__global__ void __launch_bounds__(BLOCK) k_zq_at(DevView d, isg_wh base, double alpha, const ResolveState *st, const unsigned long long *offs)
{
	__shared__ ZqSh<KMAX> sh;
	if (!st->done || st->fail) return;
	const int t = threadIdx.x, i = blockIdx.x;
	{
		const uint16_t *src = (const uint16_t *)d.tab;
		uint16_t *dst = (uint16_t *)&sh.tab;
		for (int k = t; k < (int)(sizeof(isg_wh_tables) / 2); k += BLOCK) dst[k] = src[k];
		if (t < 2 * ZqSh<KMAX>::KC) (&sh.hist[0][0])[t] = 0;
	}
	__syncthreads();
	const isg_wh mult0 = isg_wh_power(&sh.tab, 8u * (unsigned)t);
	const isg_wh mult_pass = isg_wh_power(&sh.tab, 8u * (unsigned)BLOCK);
	ZqPrefetch<KMAX> pf;
	const unsigned long long o = offs[i], o1 = offs[i + 1];
	const isg_wh cur = isg_wh_jump(&sh.tab, base, o);
	zq_prefetch<KMAX>(d, i, 0, pf);
	const unsigned used = zq_one<BLOCK, KMAX, false>(d, sh, i, cur, 0, 0, alpha, mult0, mult_pass, pf);
	if (t == 0 && (unsigned long long)used != o1 - o) atomicOr(d.err, 4u);
}

/* ---- host ---- */
static void resolve_plan_build(ResolvePlan &p, int K, int nunits_max, double mu, double sigma, double a0, double shape)
{
	memset(&p, 0, sizeof(p));
	int units = 0, r = 0;
	for (; r < ISG_RS_DMAX; r++) {
		const double sr = sqrt((double)r);
		/* wider windows early in the block, narrower late: a walk that leaves a window at individual r wastes the block's other
		 * D - r individuals */
		const double a = a0 * (1.0 + shape * (0.5 - (double)r / ISG_RS_DMAX));
		long lo = (long)floor(mu * r - a * sigma * sr - (r ? 1.0 : 0.0)), hi = (long)ceil(mu * r + a * sigma * sr + (r ? 1.0 : 0.0));
		if (lo < 0) lo = 0;
		if (r == 0) hi = 0;
		int w = (int)(hi - lo + 1);
		w = (w + ISG_RS_CH - 1) / ISG_RS_CH * ISG_RS_CH;
		const int nu = w / ISG_RS_CH;
		if (units + nu > nunits_max || lo + w > 30000 || w > ISG_RS_WMAX) break;
		if (r > 0 && lo - p.lo[r - 1] > 100) break; /* (the walk relies on an irregular entry, 255, leaving the next window) */
		p.lo[r] = (short)lo;
		p.w[r] = (short)w;
		units += nu;
	}
	/* Unit numbers: rs_unit_of_block gives XCD x the x-th eighth of them.  Window widths differ along the block (few candidates for the
	 * first individuals, most in the middle), so numbered in block order the XCDs would hold different numbers of distinct individuals
	 * (genotype rows, tape stretches) for the same number of units.  The individuals are dealt to eight groups in snake order (0..7,
	 * 7..0, ...) and numbered group by group: every eighth gets the same mix (measured: 0.5 % of the block kernel's time). */
	int n = 0;
	for (int x = 0; x < 8; x++)
		for (int q = 0; q < r; q++) {
			const int round = q / 8, pos = q % 8;
			if (((round & 1) ? 7 - pos : pos) != x) continue;
			const int nu = p.w[q] / ISG_RS_CH;
			p.cbase[q] = (short)(n * ISG_RS_CH);
			for (int k = 0; k < nu; k++) {
				p.ur[n + k] = (short)q;
				p.uo[n + k] = (short)(p.lo[q] + k * ISG_RS_CH);
				p.cslot[n + k] = (short)((((q >> 2) * ISG_RS_WMAX + k * ISG_RS_CH) << 2) + (q & 3));
			}
			n += nu;
		}
	p.D = r;
	p.nunits = units;
	(void)K;
}

struct ResolveCtx {
	DevBuf<unsigned long long> d_B, d_offs;
	DevBuf<float> d_tapef;
	ResolvePlan plan_h;
	DevBuf<ResolvePlan> d_plan;
	DevBuf<ResolveState> d_st;
	DevBuf<unsigned long long> d_gran; /* k_zq_blocks: [2][ISG_RS_UMAX] tagged granules, then the abort word */
	bool persist = true;                  /* the whole resolution in one launch (INSTRUCT_ZQ_RESOLVE_PERSIST=0: one launch per block) */
	/* Windows: individual r of a block gets  mu r +- a_r sigma sqrt(r),  a_r = a (1 + shape (1/2 - r / 64)):  wide early, narrow late (a
	 * walk that leaves its window at individual r wastes the block's remaining D - r).  Measured at config 3, update_ZQ's block kernel
	 * per sweep: (a, shape) = (1.8, 0) 7.34 ms, (2.0, 0) 7.41, (1.6, 0) 7.50, (1.8, 0.4) 7.01, (1.8, 0.8) 6.96, (1.6, 0.8) 6.85,
	 * (1.5, 0.8) 6.73, (1.5, 1.2) 6.64, (1.6, 1.5) 6.66, (1.4, 1.2) 6.78.  INSTRUCT_ZQ_RESOLVE_A / _SHAPE override. */
	double shape = 1.2;
	double mu = 0, sigma = 0, a = 1.5;
	int units = 256;
	long est_blocks = 0;
	bool plan_valid = false;
	unsigned err_bit = 4u; /* bit of the device error word the sweep kernel raises on a consumption mismatch */
	int copies = 2; /* allele copies per locus = uniforms per used locus (2; ploidy 4: 4) */
	/* diagnostics of the last sweep */
	unsigned long long last_blocks = 0, last_miss = 0, last_launches = 0, last_exact = 0;
};

/* nvalid: loci used per individual (host copy); called once per context */
static int resolve_alloc(isg_ctx *c, const std::vector<int> &nvalid, int copies = 2, int kmax = 8)
{
	if (!env_flag(getenv("INSTRUCT_ZQ_RESOLVE"), true)) return 0;
	const int N = c->cfg.N, K = c->cfg.K;
	if (K > kmax || (copies == 2 && c->cfg.mode == 0)) return 0; /* pre-filter rows in registers; mode 0 has no update_ZQ */
	if (copies == 2 && ((uint64_t)c->d.Lp * (uint64_t)c->d.Amax * 32ull >= (1ull << 32) || c->d.Lp >= (1 << 24) || c->d.Amax >= (1 << 24))) return 0; /* 32-bit byte offsets into the float frequency table */
	ResolveCtx *r = new ResolveCtx();
	c->rs = r;
	r->copies = copies;
	std::vector<unsigned long long> B((size_t)N + 1, 0);
	for (int i = 0; i < N; i++) B[i + 1] = B[i] + (unsigned long long)copies * (unsigned)nvalid[i] + 2ull * (unsigned)K;
	HIPCHK(r->d_B.alloc((size_t)N + 1));
	HIPCHK(hipMemcpy(r->d_B, B.data(), sizeof(unsigned long long) * ((size_t)N + 1), hipMemcpyHostToDevice));
	HIPCHK(r->d_offs.alloc((size_t)N + 1));
	HIPCHK(r->d_plan.alloc(1));
	HIPCHK(r->d_st.alloc(1));
	HIPCHK(r->d_gran.alloc(2 * ISG_RS_UMAX + 1));
	r->persist = env_flag(getenv("INSTRUCT_ZQ_RESOLVE_PERSIST"), true);
	/* rejected attempts per individual: about 0.46 per gamma with a spread of 0.8 sqrt(K) (measured at K = 5: 2.3, 1.8);
	 * replaced by the previous sweep's own statistics from the second sweep on */
	r->mu = 0.46 * K;
	r->sigma = 0.8 * sqrt((double)K);
	const double a = env_double(getenv("INSTRUCT_ZQ_RESOLVE_A"), r->a, 0.5);
	if (a > 0.5) r->a = a; /* (0.5 itself is not taken) */
	r->shape = env_double(getenv("INSTRUCT_ZQ_RESOLVE_SHAPE"), r->shape, 0.0, 1.5);
	{ /* ISG_RS_OCC units (workgroups of 4 waves) per compute unit, all resident together.  Measured at config 3 on 256 CUs, update_ZQ's
	   * block kernel per sweep: 256 / 384 / 512 units -> 8.9 / 8.5 / 7.5 ms (a block's fixed costs -- hand-over, walk, Dirichlet --
	   * are shared by more individuals: 33 / 44 / 54 per block); ploidy 4's block kernel holds one workgroup per compute unit */
		int cus = 0;
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->cfg.device) == hipSuccess && cus >= 8) {
			const int want = (copies == 2 ? ISG_RS_OCC : 1) * cus;
			r->units = want > ISG_RS_UMAX ? ISG_RS_UMAX : want;
		}
	}
	const int units = (int)env_int(getenv("INSTRUCT_ZQ_RESOLVE_UNITS"), r->units, 8, INT_MAX);
	r->units = units > ISG_RS_UMAX ? ISG_RS_UMAX : units;
	return 0;
}

template <int KMAX>
static void resolve_launch_block(isg_ctx *c, isg_wh base, uint64_t tape_len, int b)
{
	ResolveCtx *r = c->rs;
	hipLaunchKernelGGL((k_zq_block<KMAX>), dim3(r->plan_h.nunits), dim3(256), 0, c->stream, c->d, base, c->alpha, (const ResolvePlan *)r->d_plan, r->d_st,
			   (const unsigned long long *)r->d_B, (const float *)r->d_tapef, (unsigned long long)tape_len, r->d_offs, b);
}
/* false: the workgroups would not all be resident together -- the caller launches block by block */
template <int KMAX>
static bool resolve_launch_persist(isg_ctx *c, isg_wh base, uint64_t tape_len)
{
	ResolveCtx *r = c->rs;
	if (!r->persist || g_live_ctx[c->cfg.device & 63].load() > 1) return false; /* (another chain on this GPU: per-block launches interleave) */
	if (!fits_resident(k_zq_blocks<KMAX>, 256, r->plan_h.nunits, c->cfg.device)) return false;
	if (hipMemsetAsync(r->d_gran, 0, sizeof(unsigned long long) * (2 * ISG_RS_UMAX + 1), c->stream) != hipSuccess) return false;
	hipLaunchKernelGGL((k_zq_blocks<KMAX>), dim3(r->plan_h.nunits), dim3(256), 0, c->stream, c->d, base, c->alpha, (const ResolvePlan *)r->d_plan, r->d_st,
			   (const unsigned long long *)r->d_B, (const float *)r->d_tapef, (unsigned long long)tape_len, r->d_offs, r->d_gran,
			   (unsigned *)(r->d_gran + 2 * ISG_RS_UMAX));
	return true;
}
template <int KMAX>
static void resolve_launch_at(isg_ctx *c, isg_wh base)
{
	ResolveCtx *r = c->rs;
	hipLaunchKernelGGL((k_zq_at<256, KMAX>), dim3(c->cfg.N), dim3(256), 0, c->stream, c->d, base, c->alpha, (const ResolveState *)r->d_st,
			   (const unsigned long long *)r->d_offs);
}

/* returns 0 and *done = true when the sweep is complete; *done = false: nothing is changed (qq restored), the caller
 * takes the chain kernels */
/* launch_block(b, tape_len) / launch_at() / launch_persist(tape_len): the ploidy's kernels */
template <class LB, class LA, class LP>
static int resolve_update_ZQ_with(isg_ctx *c, isg_wh base, bool *done, LB launch_block, LA launch_at, LP launch_persist)
{
	ResolveCtx *r = c->rs;
	*done = false;
	const int N = c->cfg.N, K = c->cfg.K;
	/* the float image of the phase's stretch of the stream (Z draws of all individuals + Dirichlet allowance) */
	const uint64_t need = (uint64_t)r->copies * c->nvalid_total + (uint64_t)(8 * K + 32 > 96 ? 8 * K + 32 : 96) * (uint64_t)N + 4096;
	HIPCHK(r->d_tapef.grow(need));
	prof_begin(c);
	hipLaunchKernelGGL(k_tapef, dim3((unsigned)((need + 2047) / 2048)), dim3(256), 0, c->stream, c->d.tab, base, (unsigned long long)need, r->d_tapef);
	prof_end(c, "k_tapef");
	/* plan from the current estimate of the rejection statistics */
	ResolvePlan np;
	resolve_plan_build(np, K, r->units, r->mu, r->sigma, r->a, r->shape);
	if (!r->plan_valid || memcmp(&np, &r->plan_h, sizeof(np)) != 0) {
		if (r->plan_valid && np.D > 0) r->est_blocks = r->est_blocks * r->plan_h.D / np.D + 1; /* blocks scale with 1 / D */
		r->plan_h = np;
		HIPCHK(hipMemcpyAsync(r->d_plan, &r->plan_h, sizeof(ResolvePlan), hipMemcpyHostToDevice, c->stream));
		r->plan_valid = true;
	}
	if (r->plan_h.D < 1) return 0;
	HIPCHK(hipMemsetAsync(r->d_st, 0, sizeof(ResolveState), c->stream));
	HIPCHK(hipMemcpyAsync(c->d_qqsave, c->d.qq, sizeof(double) * (size_t)N * K, hipMemcpyDeviceToDevice, c->stream));
	long est = r->est_blocks > 0 ? r->est_blocks + r->est_blocks / 16 + 4 : (long)((double)N / r->plan_h.D * 1.4) + 8;
	int b = 0;
	struct { unsigned done, fail; unsigned long long total, nblocks, nmiss, sumc, sumc2, nind, nexact; } hs;
	unsigned err[4] = {0, 0, 0, 0};
	r->last_launches = 0;
	bool launch_failed = false;
	for (int round = 0; round < 64; round++) {
		prof_begin(c);
		const bool one = (round == 0) && launch_persist(need);
		if (!one)
			for (long k = 0; k < est; k++, b++) launch_block(b, need);
		prof_end(c, one ? "k_zq_blocks" : "k_zq_block");
		r->last_launches += one ? 1ull : (unsigned long long)est;
		prof_begin(c);
		launch_at();
		prof_end(c, "k_zq_at");
		if (hipGetLastError() != hipSuccess) launch_failed = true; /* (resources, an occupancy other than fits_resident saw): the chain kernels take the sweep */
		HIPCHK(hipMemcpyAsync(&hs, &r->d_st.get()->done, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipMemcpyAsync(err, c->d_err, sizeof(err), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		if (hs.fail || hs.done || one || launch_failed) break; /* (k_zq_blocks ends resolved or failed) */
		est = est / 4 + 8; /* the estimate fell short: some more launches, then look again */
	}
	bool ok = hs.done && !hs.fail && !(err[0] & r->err_bit) && !launch_failed;
	if (c->test_abort > 0 && --c->test_abort == 0) ok = false;
	if (!ok && r->last_launches == 1) { /* k_zq_blocks: a wait that timed out means its workgroups were not resident together (the GPU is
					     * shared): from now on one launch per block, which needs no co-residency */
		unsigned ab = 0;
		HIPCHK(hipMemcpy(&ab, r->d_gran + 2 * ISG_RS_UMAX, sizeof(ab), hipMemcpyDeviceToHost));
		if (ab) r->persist = false;
	}
	if (!ok) { /* irregular consumption somewhere, or the check failed: qq back, the caller redoes the sweep with the chain kernels */
		if (err[0] & r->err_bit) { /* only this path's bit: whatever else is pending (dt_stat's flag and value) stays */
			err[0] &= ~r->err_bit;
			HIPCHK(hipMemcpyAsync(c->d_err, err, sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
			HIPCHK(hipStreamSynchronize(c->stream));
		}
		HIPCHK(hipMemcpyAsync(c->d.qq, c->d_qqsave, sizeof(double) * (size_t)N * K, hipMemcpyDeviceToDevice, c->stream));
		c->zq_fallbacks++;
		return 0;
	}
	r->last_blocks = hs.nblocks;
	r->last_miss = hs.nmiss;
	r->last_exact = hs.nexact;
	r->est_blocks = (long)hs.nblocks + 1;
	if (hs.nind > 64) { /* next sweep's windows from this sweep's rejection statistics */
		const double m = (double)hs.sumc / (double)hs.nind, v = (double)hs.sumc2 / (double)hs.nind - m * m;
		r->mu = 0.5 * r->mu + 0.5 * m;
		r->sigma = 0.5 * r->sigma + 0.5 * sqrt(v > 0.01 ? v : 0.01);
	}
	host_advance(c, hs.total);
	c->h_qq = false;
	*done = true;
	return 0;
}

static int resolve_update_ZQ(isg_ctx *c, isg_wh base, bool *done)
{
	const int K = c->cfg.K;
	/* the block kernels take K as a compile-time constant (KL_ZQ_EXACT) */
	return resolve_update_ZQ_with(c, base, done,
				      [&](int b, uint64_t tl) { kdispatch(KL_ZQ_EXACT(), K, [&](auto km) { resolve_launch_block<decltype(km)::value>(c, base, tl, b); }); },
				      [&]() { kdispatch(KL_ZQ_8(), K, [&](auto km) { resolve_launch_at<decltype(km)::value>(c, base); }); },
				      [&](uint64_t tl) {
					      bool ok = false;
					      kdispatch(KL_ZQ_EXACT(), K, [&](auto km) { ok = resolve_launch_persist<decltype(km)::value>(c, base, tl); });
					      return ok;
				      });
}

extern "C" int isg_zq_resolve_stats(isg_ctx *c, long out[8])
{
	for (int k = 0; k < 8; k++) out[k] = 0;
	if (!c->rs) return 0;
	out[0] = (long)c->rs->last_blocks;
	out[1] = (long)c->rs->last_miss;
	out[2] = (long)c->rs->last_launches;
	out[3] = c->rs->plan_h.D;
	out[4] = c->rs->plan_h.nunits;
	out[5] = (long)(c->rs->mu * 1000.0);
	out[6] = (long)(c->rs->sigma * 1000.0);
	out[7] = (long)c->rs->last_exact; /* ISG_STAMPS builds only */
	return 0;
}

extern "C" int isg_zq_resolve_plan(int units, double mu, double sigma, double a, double shape, short *lo, short *w, short *ur, short *uo, short *cslot, int *nunits)
{
	ResolvePlan p;
	if (units > ISG_RS_UMAX) units = ISG_RS_UMAX;
	resolve_plan_build(p, 0, units, mu, sigma, a, shape);
	memcpy(lo, p.lo, sizeof(p.lo));
	memcpy(w, p.w, sizeof(p.w));
	memcpy(ur, p.ur, sizeof(p.ur));
	memcpy(uo, p.uo, sizeof(p.uo));
	memcpy(cslot, p.cslot, sizeof(p.cslot));
	*nunits = p.nunits;
	return p.D;
}
