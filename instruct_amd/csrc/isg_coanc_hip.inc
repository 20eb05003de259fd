/* ---- posterior co-ancestry on the device (isg_coanc_*; DESIGN.md "Posterior co-ancestry") ----
 * C[i][j] = (1/S) sum over the S stored steps of sum_k q_ik q_jk: the probability that an allele copy of i and one of j come from the
 * same cluster, unchanged when the clusters are relabelled.  A stored step copies Q into a slot of the history ([batch][Np][Kp],
 * zero padded; mode 0: the unit vector of zz[i]); when `batch` slots are held, k_coanc_syrk adds sum_t Q_t Q_t^T to the lower
 * tile triangle of the dense [N][N] accumulator with the f64 matrix instruction.  Nothing here writes chain state or draws. */

typedef double coanc_v4d __attribute__((ext_vector_type(4)));

/* slot <- Q (gen == nullptr) or the unit vectors of gen (mode 0); only [N][K] of the slot is written, its padding stays zero */
__global__ void __launch_bounds__(256) k_coanc_snap(const double *__restrict__ qq, const int *__restrict__ gen, double *__restrict__ slot, int N, int K, int Kp)
{
	const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (e >= (size_t)N * K) return;
	const int i = (int)(e / K), k = (int)(e % K);
	slot[(size_t)i * Kp + k] = gen ? (gen[i] == k ? 1.0 : 0.0) : qq[e];
}

/* One workgroup per tile pair (ti, tj), tj <= ti; wave w owns sub-row w of the tile and chains the inner dimension (nb snapshots x Kp
 * columns, 4 per instruction) into its NSUB accumulators, which share the A operand and are independent of each other.  Operand
 * rows are below Np (zero padding), accumulator elements are guarded at N. */
__global__ void __launch_bounds__(ISG_COANC_BLOCK, 2) k_coanc_syrk(const double *__restrict__ hist, int nb, int N, int Np, int Kp, double *__restrict__ acc)
{
	int ti, tj;
	isg_coanc_decode(blockIdx.x, &ti, &tj);
	const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
	coanc_v4d c[ISG_COANC_NSUB];
#pragma unroll
	for (int s = 0; s < ISG_COANC_NSUB; s++) {
		const int j = isg_coanc_c_col(tj, s, lane);
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int i = isg_coanc_c_row(ti, wave, lane, r);
			c[s][r] = (i < N && j < N) ? acc[(size_t)i * N + j] : 0.0;
		}
	}
	/* both operands from one base each: the sub-columns' rows of Q lie SUB rows apart */
	const int kq = isg_coanc_ab_k(lane);
	const double *pa = hist + isg_coanc_hist_index(0, isg_coanc_a_row(ti, wave, lane), kq, Np, Kp);
	const double *pb = hist + isg_coanc_hist_index(0, isg_coanc_b_row(tj, 0, lane), kq, Np, Kp);
	const int sb = ISG_COANC_SUB * Kp;
	const size_t slot = (size_t)Np * Kp;
	for (int t = 0; t < nb; t++, pa += slot, pb += slot) {
		for (int k0 = 0; k0 < Kp; k0 += ISG_COANC_KSTEP) {
			const double a = pa[k0];
			double b[ISG_COANC_NSUB];
#pragma unroll
			for (int s = 0; s < ISG_COANC_NSUB; s++) b[s] = pb[s * sb + k0];
#pragma unroll
			for (int s = 0; s < ISG_COANC_NSUB; s++) c[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[s], c[s], 0, 0, 0);
		}
	}
#pragma unroll
	for (int s = 0; s < ISG_COANC_NSUB; s++) {
		const int j = isg_coanc_c_col(tj, s, lane);
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int i = isg_coanc_c_row(ti, wave, lane, r);
			if (i < N && j < N) acc[(size_t)i * N + j] = c[s][r];
		}
	}
}

static void coanc_free(isg_ctx *c)
{
	c->co_hist.reset();
	c->co_acc.reset();
	c->co_on = false;
	c->co_batch = c->co_held = 0;
	c->co_steps = 0;
}
/* the held snapshots into the accumulator */
static int coanc_flush(isg_ctx *c)
{
	if (!c->co_held) return 0;
	const int N = c->cfg.N;
	prof_begin(c);
	hipLaunchKernelGGL(k_coanc_syrk, dim3((unsigned)isg_coanc_groups(N)), dim3(ISG_COANC_BLOCK), 0, c->stream, (const double *)c->co_hist, c->co_held, N,
			   isg_coanc_np(N), isg_coanc_kp(c->cfg.K), c->co_acc.get());
	prof_end(c, "k_coanc_syrk");
	HIPCHK(hipGetLastError());
	c->co_held = 0;
	return 0;
}
extern "C" int isg_coanc_begin(isg_ctx *c, int batch)
{
	HIPCHK(hipSetDevice(c->cfg.device));
	if (batch < 0) return fail("isg_coanc_begin: batch must be >= 0 (0: the default)");
	if (batch == 0) batch = ISG_COANC_BATCH;
	coanc_free(c);
	const int N = c->cfg.N, K = c->cfg.K;
	const size_t need = isg_coanc_bytes(N, K, batch);
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = (size_t)1 << 31;
	if (need > fr / 2) {
		char msg[256];
		snprintf(msg, sizeof msg, "isg_coanc_begin: the co-ancestry accumulator and %d snapshots need %zu bytes (N %d, K %d): more than half of the free device memory", batch, need, N, K);
		return fail(msg);
	}
	/* zeroed on the launch stream: the null-stream memset of alloc_zero would do as well, this keeps the order explicit */
	HIPCHK(c->co_acc.alloc((size_t)N * N));
	HIPCHK(c->co_hist.alloc((size_t)batch * isg_coanc_hist_stride(N, K)));
	HIPCHK(hipMemsetAsync(c->co_acc, 0, sizeof(double) * (size_t)N * N, c->stream));
	HIPCHK(hipMemsetAsync(c->co_hist, 0, sizeof(double) * (size_t)batch * isg_coanc_hist_stride(N, K), c->stream));
	c->co_batch = batch;
	c->co_on = true;
	return 0;
}
extern "C" int isg_coanc_step(isg_ctx *c)
{
	HIPCHK(hipSetDevice(c->cfg.device));
	if (!c->co_on) return fail("isg_coanc_step: isg_coanc_begin first");
	const int N = c->cfg.N, K = c->cfg.K;
	const bool noadm = !c->poly && c->cfg.mode == 0;
	const size_t n = (size_t)N * K;
	prof_begin(c);
	hipLaunchKernelGGL(k_coanc_snap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double *)c->d.qq, noadm ? (const int *)c->d.gen : (const int *)nullptr,
			   c->co_hist.get() + (size_t)c->co_held * isg_coanc_hist_stride(N, K), N, K, isg_coanc_kp(K));
	prof_end(c, "k_coanc_snap");
	HIPCHK(hipGetLastError());
	c->co_held++;
	c->co_steps++;
	return c->co_held == c->co_batch ? coanc_flush(c) : 0;
}
/* mean [N][N]: the accumulator's lower triangle divided by the steps, mirrored; accumulation goes on afterwards */
extern "C" int isg_coanc_fetch(isg_ctx *c, double *mean, long *steps)
{
	HIPCHK(hipSetDevice(c->cfg.device));
	if (!c->co_on) return fail("isg_coanc_fetch: isg_coanc_begin first");
	if (c->co_steps == 0) return fail("isg_coanc_fetch: no step has been accumulated yet");
	if (coanc_flush(c)) return 1;
	const size_t N = (size_t)c->cfg.N;
	HIPCHK(hipMemcpyAsync(mean, c->co_acc, sizeof(double) * N * N, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	const double s = (double)c->co_steps;
	for (size_t i = 0; i < N; i++)
		for (size_t j = 0; j <= i; j++) mean[j * N + i] = mean[i * N + j] = mean[i * N + j] / s;
	if (steps) *steps = c->co_steps;
	return 0;
}
extern "C" int isg_coanc_end(isg_ctx *c)
{
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipStreamSynchronize(c->stream)); /* a flush may still be reading the buffers */
	coanc_free(c);
	return 0;
}
