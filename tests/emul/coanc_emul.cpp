/* Runs the tiling, padding and lane maps of instruct_amd/csrc/isg_coanc.h on the host (tests/test_coanc_layout.py reads the lines):
 *   DECODE N T groups bad    bad = tile pairs with tj <= ti not visited exactly once + workgroups decoded to anything else
 *   PAD K Kp                 K = 1 .. 64
 *   NP N Np T                N = 1 .. 300 and 10000
 *   MFMA bad                 one 16 x 16 x 4 product of asymmetric integer matrices through the lane maps against the triple loop
 *   SYRK N K nb bad          k_coanc_syrk's walk over a 3-tile N emulated lane by lane against the plain loop
 * The matrix instruction itself is emulated as documented: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] and receives
 * D[(l >> 4) + 4 reg][l & 15], written out in mfma_emul; what the kernel puts into a lane and takes out of it goes through the
 * header's functions, so a header that disagrees with the instruction (the f32 forms' row 4 (l >> 4) + reg, say) shows. */
#include <stdio.h>
#include <vector>
#include "../../instruct_amd/csrc/isg_coanc.h"

/* D = A B + C for one wave: a[l], b[l] the lanes' operands, c[l][reg] their accumulators */
static void mfma_emul(const double a[64], const double b[64], double c[64][4])
{
	double A[16][4], B[4][16];
	for (int l = 0; l < 64; l++) { /* the instruction's own maps, written out: not the header's functions */
		A[l & 15][l >> 4] = a[l];
		B[l >> 4][l & 15] = b[l];
	}
	for (int l = 0; l < 64; l++)
		for (int r = 0; r < 4; r++) {
			const int i = (l >> 4) + 4 * r, j = l & 15;
			double s = c[l][r];
			for (int k = 0; k < 4; k++) s += A[i][k] * B[k][j];
			c[l][r] = s;
		}
}

static long decode_bad(int N)
{
	const int T = isg_coanc_tiles(N);
	const long G = isg_coanc_groups(N);
	std::vector<int> seen((size_t)T * T, 0);
	long bad = 0;
	for (long w = 0; w < G; w++) {
		int ti, tj;
		isg_coanc_decode((unsigned)w, &ti, &tj);
		if (ti < 0 || ti >= T || tj < 0 || tj > ti) { bad++; continue; }
		seen[(size_t)ti * T + tj]++;
	}
	for (int ti = 0; ti < T; ti++)
		for (int tj = 0; tj < T; tj++) bad += seen[(size_t)ti * T + tj] != (tj <= ti ? 1 : 0);
	return bad;
}

static long mfma_bad()
{
	double A[16][4], B[4][16], C[16][16], a[64], b[64], c[64][4];
	for (int i = 0; i < 16; i++)
		for (int k = 0; k < 4; k++) A[i][k] = 3 * i + 7 * k + 1;
	for (int k = 0; k < 4; k++)
		for (int j = 0; j < 16; j++) B[k][j] = 5 * j * j - 2 * k + 11;
	for (int i = 0; i < 16; i++)
		for (int j = 0; j < 16; j++) C[i][j] = 100 * i - 9 * j;
	/* the lanes as the kernel fills them: operand rows / columns and accumulator elements by the header's maps */
	for (int l = 0; l < 64; l++) {
		a[l] = A[isg_coanc_ab_idx(l)][isg_coanc_ab_k(l)];
		b[l] = B[isg_coanc_ab_k(l)][isg_coanc_ab_idx(l)];
		for (int r = 0; r < 4; r++) c[l][r] = C[isg_coanc_cd_row(l, r)][isg_coanc_cd_col(l)];
	}
	mfma_emul(a, b, c);
	long bad = 0;
	int hit[16][16] = {};
	for (int l = 0; l < 64; l++)
		for (int r = 0; r < 4; r++) {
			const int i = isg_coanc_cd_row(l, r), j = isg_coanc_cd_col(l);
			double s = C[i][j];
			for (int k = 0; k < 4; k++) s += A[i][k] * B[k][j];
			bad += c[l][r] != s;
			hit[i][j]++;
		}
	for (int i = 0; i < 16; i++)
		for (int j = 0; j < 16; j++) bad += hit[i][j] != 1; /* the result map covers the 16 x 16 block once */
	return bad;
}

/* the kernel's walk: history [nb][Np][Kp], accumulator [N][N], every workgroup, wave and lane in turn */
static long syrk_bad(int N, int K, int nb)
{
	const int Np = isg_coanc_np(N), Kp = isg_coanc_kp(K);
	std::vector<double> hist((size_t)nb * isg_coanc_hist_stride(N, K), 0.0), acc((size_t)N * N), want((size_t)N * N, 0.0);
	for (int t = 0; t < nb; t++)
		for (int i = 0; i < N; i++)
			for (int k = 0; k < K; k++) hist[isg_coanc_hist_index(t, i, k, Np, Kp)] = (double)((i * 7 + k * 13 + t * 5 + i * k) % 23) - 4.0;
	for (int i = 0; i < N; i++)
		for (int j = 0; j < N; j++) acc[(size_t)i * N + j] = want[(size_t)i * N + j] = (double)(i * 3 - j); /* what earlier flushes left */
	for (int i = 0; i < N; i++)
		for (int j = 0; j <= i; j++)
			for (int t = 0; t < nb; t++)
				for (int k = 0; k < K; k++) want[(size_t)i * N + j] += hist[isg_coanc_hist_index(t, i, k, Np, Kp)] * hist[isg_coanc_hist_index(t, j, k, Np, Kp)];
	long bad = 0;
	for (long w = 0; w < isg_coanc_groups(N); w++) {
		int ti, tj;
		isg_coanc_decode((unsigned)w, &ti, &tj);
		for (int wave = 0; wave < ISG_COANC_WAVES; wave++) {
			double c[ISG_COANC_NSUB][64][4], a[64], b[64];
			for (int s = 0; s < ISG_COANC_NSUB; s++)
				for (int l = 0; l < 64; l++)
					for (int r = 0; r < 4; r++) {
						const int i = isg_coanc_c_row(ti, wave, l, r), j = isg_coanc_c_col(tj, s, l);
						c[s][l][r] = (i < N && j < N) ? acc[(size_t)i * N + j] : 0.0;
					}
			for (int t = 0; t < nb; t++)
				for (int k0 = 0; k0 < Kp; k0 += ISG_COANC_KSTEP)
					for (int s = 0; s < ISG_COANC_NSUB; s++) {
						for (int l = 0; l < 64; l++) {
							const int ra = isg_coanc_a_row(ti, wave, l), rb = isg_coanc_b_row(tj, s, l), k = k0 + isg_coanc_ab_k(l);
							if (ra >= Np || rb >= Np || k >= Kp) { bad++; a[l] = b[l] = 0; continue; } /* a read outside the history */
							a[l] = hist[isg_coanc_hist_index(t, ra, k, Np, Kp)];
							b[l] = hist[isg_coanc_hist_index(t, rb, k, Np, Kp)];
						}
						mfma_emul(a, b, c[s]);
					}
			for (int s = 0; s < ISG_COANC_NSUB; s++)
				for (int l = 0; l < 64; l++)
					for (int r = 0; r < 4; r++) {
						const int i = isg_coanc_c_row(ti, wave, l, r), j = isg_coanc_c_col(tj, s, l);
						if (i < N && j < N) acc[(size_t)i * N + j] = c[s][l][r];
					}
		}
	}
	for (int i = 0; i < N; i++)
		for (int j = 0; j <= i; j++) bad += acc[(size_t)i * N + j] != want[(size_t)i * N + j];
	return bad;
}

int main()
{
	for (int N = 1; N <= 301; N++) {
		const int n = N == 301 ? 10000 : N;
		printf("NP %d %d %d\n", n, isg_coanc_np(n), isg_coanc_tiles(n));
		printf("DECODE %d %d %ld %ld\n", n, isg_coanc_tiles(n), isg_coanc_groups(n), decode_bad(n));
	}
	for (int K = 1; K <= 64; K++) printf("PAD %d %d\n", K, isg_coanc_kp(K));
	printf("TILE %d %d %d %d\n", ISG_COANC_TILE, ISG_COANC_SUB, ISG_COANC_KSTEP, ISG_COANC_NSUB);
	printf("MFMA %ld\n", mfma_bad());
	printf("SYRK %d %d %d %ld\n", 130, 5, 2, syrk_bad(130, 5, 2));
	printf("SYRK %d %d %d %ld\n", 129, 4, 2, syrk_bad(129, 4, 2));
	return 0;
}
