/*
 * isg_poly_tables.h -- genotype-class tables of the autotetraploid sampler (reference poly_geno.c).
 *
 * For a locus with n alleles a tetraploid genotype falls in one of five classes (iiii, iiij, iijj, iijk,
 * ijkl; poly_geno.c:1698-1713); all G(n) genotypes are listed in a fixed order, encoded as base-n
 * numbers (auto_geno_list, poly_geno.c:1716-1800).  Two float tables per (cluster, locus) drive the
 * sampler:
 *   exfreq   log expected (panmictic) genotype frequency          calc_exfreq_auto  poly_geno.c:1515-1590
 *   genfreq  log genotype frequency at selfing rate s, solved class by class from quadri-allelic down
 *            to mono-allelic genotypes (3x3 float Gauss-Jordan for the tri-allelic triples)
 *                                                                   auto_genfreq      poly_geno.c:1803-2028
 * The arithmetic keeps the reference's float/double promotion pattern (the tables are float,
 * poly_geno.h:19-20; libm calls are double), including its quirks (the repeated test at :1990-1996).
 *
 * This is a TEMPLATE header: include it with PT_NAME(x), PT_LOG(x), PT_EXP(x) defined.  The product
 * (host and device) instantiates it with the bit-reproducible isg_math.h functions; the CPU oracle
 * instantiates it a second time with glibc's log/exp, and THAT instance is pinned byte-for-byte to the
 * reference's golden trajectories (tests/golden/t*.golden), which is what validates this code.
 */
#include "isg_math.h"

#ifndef ISG_POLY_COMMON
#define ISG_POLY_COMMON
typedef struct {
	int n;        /* alleles at the locus */
	int G;        /* genotypes in total */
	int g[6];     /* g[1..5]: mono, simplex, duplex, tri, quadri (genonum row, poly_geno.c:1706-1713) */
	const int *list; /* [G] base-n codes in table order */
} isg_polyclass;

ISG_HD int isg_poly_G(int i) { return i + i * (i - 1) * 3 / 2 + i * (i - 1) * (i - 2) / 2 + i * (i - 1) * (i - 2) * (i - 3) / 24; }

/* auto_geno_num + auto_geno_list for one allele count (host side table construction) */
static inline void isg_poly_build(int i, int g[6], int *list)
{
	int j, k, m, n, cnt, tmp;
	g[1] = i;
	g[2] = i * (i - 1);
	g[3] = i * (i - 1) / 2;
	g[4] = i * (i - 1) * (i - 2) / 2;
	g[5] = i * (i - 1) * (i - 2) * (i - 3) / 24;
	g[0] = isg_poly_G(i);
	for (j = 0; j < g[1]; j++) list[j] = j * (i * i * i + i * i + i + 1);
	tmp = g[1];
	cnt = 0;
	for (j = 0; j < i - 1; j++)
		for (k = j + 1; k < i; k++) {
			list[tmp + 2 * cnt] = j * (i * i * i + i * i + i) + k;
			list[tmp + 2 * cnt + 1] = i * (i * i + i + 1) * k + j;
			cnt++;
		}
	tmp += g[2];
	cnt = 0;
	for (j = 0; j < i - 1; j++)
		for (k = j + 1; k < i; k++) list[tmp + cnt++] = j * (i * i * i + i * i) + k * (i + 1);
	tmp += g[3];
	cnt = 0;
	for (j = 0; j < i - 2; j++)
		for (k = j + 1; k < i - 1; k++)
			for (m = k + 1; m < i; m++) {
				list[tmp + 3 * cnt] = j * (i * i * i + i * i) + k * i + m;
				list[tmp + 3 * cnt + 1] = k * (i * i * i + i * i) + j * i + m;
				list[tmp + 3 * cnt + 2] = m * (i * i * i + i * i) + j * i + k;
				cnt++;
			}
	tmp += g[4];
	cnt = 0;
	for (j = 0; j < i - 3; j++)
		for (k = j + 1; k < i - 2; k++)
			for (m = k + 1; m < i - 1; m++)
				for (n = m + 1; n < i; n++) list[tmp + cnt++] = j * i * i * i + k * i * i + i * m + n;
}

/*
 * Closed-form row of an autotetraploid genotype in isg_poly_build's order, from the multiset of its four allele codes (any order,
 * each < n).  With C(m, r) the binomial and rank_r(c_0 < .. < c_{r-1}) = C(n, r) - 1 - sum_i C(n - 1 - c_i, r - i) the rank of a
 * combination in lexicographic order:
 *   iiii  a | iiij  g1 + 2 rank_2(min, max) + (triple allele is the larger) | iijj  g1 + g2 + rank_2 | iijk  g1 + g2 + g3 + 3 rank_3(i, j, k)
 *   + (position of the doubled allele among the three) | ijkl  g1 + g2 + g3 + g4 + rank_4.  The table rows below find every row with it
 * (the reference searches the list: find_id, poly_geno.c:2367-2381; same rows), and so do the sweeps above 16 alleles, where a
 * code -> row map (n^4 entries, rows beyond a short) no longer fits.
 */
ISG_HD int isg_poly_binom(int m, int r)
{
	return r == 1 ? m : r == 2 ? m * (m - 1) / 2 : r == 3 ? m * (m - 1) * (m - 2) / 6 : m * (m - 1) * (m - 2) * (m - 3) / 24;
}
ISG_HD int isg_poly_rank(int n, int a, int b, int c, int d)
{
	int t;
#define ISG_CSWAP(x, y) if (x > y) { t = x; x = y; y = t; }
	ISG_CSWAP(a, b) ISG_CSWAP(c, d) ISG_CSWAP(a, c) ISG_CSWAP(b, d) ISG_CSWAP(b, c) /* a <= b <= c <= d */
#undef ISG_CSWAP
	const int g2 = n * (n - 1), g3 = g2 / 2, g4 = n * (n - 1) * (n - 2) / 2, C2 = g3, C3 = g4 / 3;
	if (a == d) return a;
	if (a == c || b == d) { /* simplex: the triple allele is a (a a a d) or d (a d d d) */
		const int r2 = C2 - 1 - isg_poly_binom(n - 1 - a, 2) - isg_poly_binom(n - 1 - d, 1);
		return n + 2 * r2 + (a == c ? 0 : 1);
	}
	if (a == b && c == d) return n + g2 + C2 - 1 - isg_poly_binom(n - 1 - a, 2) - isg_poly_binom(n - 1 - c, 1);
	if (a == b || b == c || c == d) { /* tri: the three distinct alleles x < y < z, the doubled one at position q */
		const int x = a, y = (a == b) ? c : b, z = d, q = (a == b) ? 0 : (b == c) ? 1 : 2;
		const int r3 = C3 - 1 - isg_poly_binom(n - 1 - x, 3) - isg_poly_binom(n - 1 - y, 2) - isg_poly_binom(n - 1 - z, 1);
		return n + g2 + g3 + 3 * r3 + q;
	}
	return n + g2 + g3 + g4 + isg_poly_binom(n, 4) - 1 - isg_poly_binom(n - 1 - a, 4) - isg_poly_binom(n - 1 - b, 3) - isg_poly_binom(n - 1 - c, 2) -
	       isg_poly_binom(n - 1 - d, 1);
}

ISG_HD int isg_poly_exists(int value, const int *vec, int leng) /* data_interface.c:865-877 */
{
	int i, flag = 0;
	for (i = 0; i < leng; i++)
		if (value == vec[i]) flag = 1;
	return flag;
}
/* gaussj (poly_geno.c:2384-2435) for the 3x3 system with one right-hand side, float, 1-based */
ISG_HD void isg_poly_gaussj3(float a[4][4], float b[4], int *err)
{
	int indxc[4], indxr[4], ipiv[4], i, icol = 1, irow = 1, j, k, l, ll;
	const int n = 3;
	float big, dum, pivinv, temp;
	for (j = 1; j <= n; j++) ipiv[j] = 0;
	for (i = 1; i <= n; i++) {
		big = 0.0f;
		for (j = 1; j <= n; j++)
			if (ipiv[j] != 1)
				for (k = 1; k <= n; k++)
					if (ipiv[k] == 0) {
						const float av = a[j][k] < 0 ? -a[j][k] : a[j][k];
						if (av >= big) { big = av; irow = j; icol = k; }
					}
		++(ipiv[icol]);
		if (irow != icol) {
			for (l = 1; l <= n; l++) { temp = a[irow][l]; a[irow][l] = a[icol][l]; a[icol][l] = temp; }
			temp = b[irow]; b[irow] = b[icol]; b[icol] = temp;
		}
		indxr[i] = irow;
		indxc[i] = icol;
		if (a[icol][icol] == 0.0f) { *err |= 2; return; }
		pivinv = (float)(1.0 / a[icol][icol]);
		a[icol][icol] = 1.0f;
		for (l = 1; l <= n; l++) a[icol][l] *= pivinv;
		b[icol] *= pivinv;
		for (ll = 1; ll <= n; ll++)
			if (ll != icol) {
				dum = a[ll][icol];
				a[ll][icol] = 0.0f;
				for (l = 1; l <= n; l++) a[ll][l] -= a[icol][l] * dum;
				b[ll] -= b[icol] * dum;
			}
	}
	for (l = n; l >= 1; l--)
		if (indxr[l] != indxc[l])
			for (k = 1; k <= n; k++) { temp = a[k][indxr[l]]; a[k][indxr[l]] = a[k][indxc[l]]; a[k][indxc[l]] = temp; }
}

/* genotype category of a 4-copy genotype (get_cat_auto, poly_geno.c:1313-1339): 0 iiii, 1 iiij, 2 iijj, 3 iijk, 4 ijkl */
ISG_HD int isg_poly_cat(const int *g)
{
	int i, cnt = 0, tmp[4], c0 = 0;
	tmp[cnt++] = g[0];
	for (i = 1; i < 4; i++)
		if (!isg_poly_exists(g[i], tmp, cnt)) tmp[cnt++] = g[i];
	if (cnt == 1) return 0;
	if (cnt == 3) return 3;
	if (cnt == 4) return 4;
	for (i = 0; i < 4; i++) c0 += (g[i] == tmp[0]);
	return c0 == 2 ? 2 : 1;
}

/*
 * Allotetraploid (-ap 0): a genotype is a pair of diploid genotypes, one per subgenome -- copies 0, 1 from the first
 * (allele frequencies freq), copies 2, 3 from the second (freq2).  Four classes for a locus with n alleles, in table order
 * (allo_geno_num / allo_geno_list, poly_geno.c:2031-2119):  0 iikk (both homozygous), 1 iikl (second heterozygous),
 * 2 ijkk (first heterozygous), 3 ijkl (both).  A canonical genotype (g0 <= g1, g2 <= g3) has a closed-form row:
 * with C = n (n - 1) / 2 and pair(a, b) = the rank of a < b among the pairs in lexicographic order,
 *   iikk  g0 n + g2 | iikl  n^2 + g0 C + pair(g2, g3) | ijkk  n^2 + n C + pair(g0, g1) n + g2 | ijkl  n^2 + 2 n C + pair(g0, g1) C + pair(g2, g3)
 * -- the reference finds rows by linear search of the base-n code (find_id, poly_geno.c:2367-2381); same rows.
 */
ISG_HD int isg_allo_G(int n) { return n * n + n * (n - 1) * n + n * (n - 1) * n * (n - 1) / 4; }
ISG_HD int isg_allo_pair(int a, int b, int n) { return a * n - a * (a + 1) / 2 + (b - a - 1); } /* a < b */
ISG_HD int isg_allo_row(int n, int g0, int g1, int g2, int g3) /* canonical genotype -> table row */
{
	const int C = n * (n - 1) / 2, hetA = g0 != g1, hetB = g2 != g3;
	if (!hetA && !hetB) return g0 * n + g2;
	if (!hetA) return n * n + g0 * C + isg_allo_pair(g2, g3, n);
	if (!hetB) return n * n + n * C + isg_allo_pair(g0, g1, n) * n + g2;
	return n * n + 2 * n * C + isg_allo_pair(g0, g1, n) * C + isg_allo_pair(g2, g3, n);
}
ISG_HD int isg_allo_row_any(int n, int a, int b, int c, int d) /* each pair in either order */
{
	return isg_allo_row(n, a < b ? a : b, a < b ? b : a, c < d ? c : d, c < d ? d : c);
}
/* get_cat_allo (poly_geno.c:1341-1372) */
ISG_HD int isg_allo_cat(const int *g) { return (g[0] != g[1] ? 2 : 0) + (g[2] != g[3] ? 1 : 0); }
/* class sizes and the base-n codes in table order (g[1..4]; g[5] = 0) */
static inline void isg_allo_build(int n, int g[6], int *list)
{
	int a, b, c, d, r = 0;
	const int C = n * (n - 1) / 2;
	g[1] = n * n; g[2] = n * C; g[3] = n * C; g[4] = C * C; g[5] = 0;
	g[0] = isg_allo_G(n);
	for (a = 0; a < n; a++)
		for (c = 0; c < n; c++) list[r++] = ((a * n + a) * n + c) * n + c;
	for (a = 0; a < n; a++)
		for (c = 0; c < n - 1; c++)
			for (d = c + 1; d < n; d++) list[r++] = ((a * n + a) * n + c) * n + d;
	for (a = 0; a < n - 1; a++)
		for (b = a + 1; b < n; b++)
			for (c = 0; c < n; c++) list[r++] = ((a * n + b) * n + c) * n + c;
	for (a = 0; a < n - 1; a++)
		for (b = a + 1; b < n; b++)
			for (c = 0; c < n - 1; c++)
				for (d = c + 1; d < n; d++) list[r++] = ((a * n + b) * n + c) * n + d;
}
#endif /* ISG_POLY_COMMON */

/* ---- instantiated part: needs PT_NAME, PT_LOG, PT_EXP ----
 *
 * One function per table ROW; each expression of the tables is written here once.  A row function reads the code of its own row
 * from pc->list, finds every other row in closed form (isg_poly_rank, isg_allo_row_any) and, for genfreq, reads only rows of fr
 * that belong to classes solved BEFORE its own -- autotetraploid: quadri -> tri -> duplex -> simplex -> mono; allotetraploid:
 * ijkl -> {iikl, ijkk} -> iikk.  So the rows of one class can be computed in any order or side by side, as long as the classes
 * come in that order (tests/test_poly_tables.py checks exactly this on the CPU).  The whole-row functions further down are the
 * serial schedule (the oracle, the one-lane-per-table kernels); the wide-allele kernels spread a class over a workgroup's lanes.
 * *err |= 4 when a log frequency comes out positive (the reference aborts: "Genotype frequencies can not be greater than 1!"),
 * |= 2 from the 3x3 solve.
 */

/* calc_exfreq_auto (poly_geno.c:1515-1590), row r: f = allele frequencies of the cluster at the locus */
ISG_HD float PT_NAME(exfreq_at)(const isg_polyclass *pc, const double *f, int r)
{
	const int n = pc->n, P = 4;
	int tmp = pc->list[r], digit[4], m, b = pc->g[1];
	float ex;
	if (r < b) return (float)PT_LOG(f[tmp % n]) * (float)P;
	if (r < (b += pc->g[2])) {
		digit[0] = tmp % n;
		tmp /= n;
		digit[1] = tmp % n;
		return (float)(PT_LOG(4.0) + PT_LOG(f[digit[1]]) * (float)(P - 1) + PT_LOG(f[digit[0]]));
	}
	if (r < (b += pc->g[3])) {
		digit[0] = tmp % n;
		tmp /= (n * n);
		digit[1] = tmp % n;
		return (float)(PT_LOG(6.0) + (PT_LOG(f[digit[1]]) + PT_LOG(f[digit[0]])) * (P / 2));
	}
	if (r < (b += pc->g[4])) {
		for (m = 0; m < P - 1; m++) { digit[m] = tmp % n; tmp /= n; }
		return (float)(PT_LOG(12.0) + PT_LOG(f[digit[2]]) * (P / 2) + PT_LOG(f[digit[0]]) + PT_LOG(f[digit[1]]));
	}
	for (m = 0; m < P; m++) { digit[m] = tmp % n; tmp /= n; }
	ex = (float)PT_LOG(24.0);
	for (m = 0; m < P; m++) ex += (float)PT_LOG(f[digit[m]]);
	return ex;
}

/* auto_genfreq (poly_geno.c:1803-2028) at selfing rate self, row by row: ex = the table's exfreq row, fr = its output row */
ISG_HD void PT_NAME(genfreq_quadri_at)(float self, const float *ex, float *fr, int r, int *err) /* ijkl */
{
	fr[r] = (float)(PT_LOG((double)(1 - self)) + ex[r] - PT_LOG((double)(1 - self / 6)));
	if (fr[r] > 0) *err |= 4;
}
/* iijk: the three rows r0, r0 + 1, r0 + 2 of one allele triple (each allele doubled in turn) come out of one 3x3 system */
ISG_HD void PT_NAME(genfreq_tri_at)(float self, const isg_polyclass *pc, const float *ex, float *fr, int r0, int *err)
{
	const int n = pc->n, tri = 3;
	int num = pc->list[r0], digit[3], j, k, l;
	float temp = 0, matr[4][4], vec[4];
	for (j = tri - 1; j >= 0; j--) { digit[j] = num % n; num /= n; }
	if (n >= 4) {
		for (l = 0; l < n; l++)
			if (l != digit[0] && l != digit[1] && l != digit[2])
				temp = (float)(temp + PT_EXP((double)fr[isg_poly_rank(n, digit[0], digit[1], digit[2], l)]));
		if (temp > 1) *err |= 4;
	}
	for (j = 1; j <= tri; j++) {
		for (k = 1; k <= tri; k++) {
			if (j == k) matr[j][k] = (float)(1 - self * 10.0 / 36.0);
			else matr[j][k] = (float)(-self / 9.0);
		}
		vec[j] = (float)(self / 18.0 * temp + (1.0 - self) * PT_EXP((double)ex[r0 + j - 1]));
	}
	temp = vec[1];
	for (j = 1; j <= tri; j++) vec[j] /= temp;
	isg_poly_gaussj3(matr, vec, err);
	for (j = 0; j < tri; j++) {
		fr[r0 + j] = (float)(PT_LOG((double)vec[j + 1]) + PT_LOG((double)temp));
		if (fr[r0 + j] > 0) *err |= 4;
	}
}
ISG_HD void PT_NAME(genfreq_duplex_at)(float self, const isg_polyclass *pc, const float *ex, float *fr, int r, int *err) /* iijj */
{
	const int n = pc->n, d0 = pc->list[r] % n, d1 = (pc->list[r] / (n * n)) % n;
	int x, y;
	float temp = 0;
	if (n >= 3)
		for (x = 0; x < n; x++)
			if (x != d0 && x != d1) {
				temp = (float)(temp + PT_EXP((double)fr[isg_poly_rank(n, d1, d1, d0, x)]) / 9.0 * self);
				temp = (float)(temp + PT_EXP((double)fr[isg_poly_rank(n, d0, d0, d1, x)]) / 9.0 * self);
				temp = (float)(temp + PT_EXP((double)fr[isg_poly_rank(n, x, x, d1, d0)]) / 36.0 * self);
				if (n >= 4)
					for (y = x + 1; y < n; y++)
						if (y != d0 && y != d1) temp = (float)(temp + PT_EXP((double)fr[isg_poly_rank(n, d0, d1, x, y)]) / 36.0 * self);
			}
	fr[r] = (float)(PT_LOG((1 - self) * PT_EXP((double)ex[r]) + temp) - PT_LOG(1 - self / 2.0));
	if (fr[r] > 0) *err |= 4;
}
ISG_HD void PT_NAME(genfreq_simplex_at)(float self, const isg_polyclass *pc, const float *ex, float *fr, int r, int *err) /* iiij */
{
	const int n = pc->n, d0 = pc->list[r] % n, d1 = (pc->list[r] / n) % n; /* d1 is the tripled allele */
	int x;
	float temp = (float)(8.0 / 36.0 * PT_EXP((double)fr[isg_poly_rank(n, d0, d0, d1, d1)]) * self);
	if (n >= 3)
		for (x = 0; x < n; x++)
			if (x != d0 && x != d1) temp = (float)(temp + PT_EXP((double)fr[isg_poly_rank(n, d1, d1, d0, x)]) / 9.0 * self);
	fr[r] = (float)(PT_LOG((1 - self) * PT_EXP((double)ex[r]) + temp) - PT_LOG(1 - self / 2.0));
	if (fr[r] > 0) *err |= 4;
}
ISG_HD void PT_NAME(genfreq_mono_at)(float self, const isg_polyclass *pc, const float *ex, float *fr, int r, int *err) /* iiii */
{
	const int n = pc->n, a = pc->list[r] % n;
	int x, y, row;
	float temp = 0;
	for (x = 0; x < n; x++)
		if (x != a) {
			row = isg_poly_rank(n, a, a, a, x);
			temp = (float)(temp + PT_EXP((double)fr[row]) / 4.0 * self);
			/* sic: for a > x the reference repeats the a < x test in its else branch, so the duplex term reuses the
			 * simplex row found above (poly_geno.c:1990-1996) */
			if (a < x) row = isg_poly_rank(n, a, a, x, x);
			temp = (float)(temp + PT_EXP((double)fr[row]) / 36.0 * self);
			if (n >= 3)
				for (y = x + 1; y < n; y++)
					if (y != a) temp = (float)(temp + PT_EXP((double)fr[isg_poly_rank(n, a, a, x, y)]) / 36.0 * self);
		}
	fr[r] = (float)(PT_LOG((1 - self) * PT_EXP((double)ex[r]) + temp) - PT_LOG((double)(1 - self)));
	if (fr[r] > 0) *err |= 4;
}

/* calc_exfreq_allo (poly_geno.c:1592-1670), row r: f / f2 = the cluster's allele frequencies in the two subgenomes.  Copies 0, 1
 * (digits 3, 2 of the code) take f, copies 2, 3 take f2; float / double exactly as the reference. */
ISG_HD float PT_NAME(exfreq_allo_at)(const isg_polyclass *pc, const double *f, const double *f2, int r)
{
	const int n = pc->n, code = pc->list[r], d0 = code % n, d1 = (code / n) % n, d2 = (code / n / n) % n, d3 = code / n / n / n;
	float ex;
	if (r < pc->g[1]) return (float)((PT_LOG(f[d2]) + PT_LOG(f2[d0])) * 2);
	if (r < pc->g[1] + pc->g[2]) return (float)(PT_LOG(2.0) + PT_LOG(f[d2]) * 2 + PT_LOG(f2[d0]) + PT_LOG(f2[d1]));
	if (r < pc->g[1] + pc->g[2] + pc->g[3]) return (float)(PT_LOG(2.0) + PT_LOG(f2[d1]) * 2 + PT_LOG(f[d3]) + PT_LOG(f[d2]));
	ex = (float)PT_LOG(4.0);
	ex += (float)PT_LOG(f2[d0]);
	ex += (float)PT_LOG(f2[d1]);
	ex += (float)PT_LOG(f[d2]);
	ex += (float)PT_LOG(f[d3]);
	return ex;
}

/* allo_genfreq (poly_geno.c:2122-2304) at selfing rate self, row by row */
ISG_HD void PT_NAME(genfreq_allo_ijkl_at)(float self, const float *ex, float *fr, int r, int *err)
{
	fr[r] = (float)(PT_LOG((double)(1 - self)) + ex[r] - PT_LOG((double)(1 - self / 4)));
	if (fr[r] > 0) *err |= 4;
}
/* iikl (r below the ijkk rows) and ijkk: the homozygous subgenome comes from selfed heterozygotes a v / k v -- ijkl rows only */
ISG_HD void PT_NAME(genfreq_allo_het_at)(float self, const isg_polyclass *pc, const float *ex, float *fr, int r, int *err)
{
	const int n = pc->n, code = pc->list[r];
	int v;
	float temp = 0;
	if (r >= pc->g[1] + pc->g[2]) { /* ijkk */
		const int k = code % n, b = (code / n / n) % n, a = code / n / n / n;
		for (v = 0; v < n; v++)
			if (v != k) temp = (float)(temp + PT_EXP((double)fr[isg_allo_row_any(n, a, b, k, v)]) * self / 8.0);
	} else { /* iikl */
		const int d = code % n, c = (code / n) % n, a = (code / n / n) % n;
		for (v = 0; v < n; v++)
			if (v != a) temp = (float)(temp + PT_EXP((double)fr[isg_allo_row_any(n, a, v, c, d)]) * self / 8.0);
	}
	fr[r] = (float)(PT_LOG((1 - self) * PT_EXP((double)ex[r]) + temp) - PT_LOG(1 - self / 2.0));
	if (fr[r] > 0) *err |= 4;
}
ISG_HD void PT_NAME(genfreq_allo_iikk_at)(float self, const isg_polyclass *pc, const float *ex, float *fr, int r, int *err)
{
	const int n = pc->n, code = pc->list[r], k = code % n, a = (code / n / n) % n;
	int v, w;
	float temp = 0;
	for (v = 0; v < n; v++)
		if (v != k) temp = (float)(temp + PT_EXP((double)fr[isg_allo_row_any(n, a, a, k, v)]) * self / 4.0);
	for (v = 0; v < n; v++)
		if (v != a) temp = (float)(temp + PT_EXP((double)fr[isg_allo_row_any(n, a, v, k, k)]) * self / 4.0);
	for (v = 0; v < n; v++)
		for (w = 0; w < n; w++)
			if (v != a && w != k) temp = (float)(temp + PT_EXP((double)fr[isg_allo_row_any(n, a, v, k, w)]) * self / 16.0);
	fr[r] = (float)(PT_LOG((1 - self) * PT_EXP((double)ex[r]) + temp) - PT_LOG((double)(1 - self)));
	if (fr[r] > 0) *err |= 4;
}

/* ---- whole tables for one (cluster, locus), serially: every row, the genfreq classes in dependency order ---- */
ISG_HD void PT_NAME(exfreq_row)(const isg_polyclass *pc, const double *f, float *ex)
{
	int r;
	for (r = 0; r < pc->G; r++) ex[r] = PT_NAME(exfreq_at)(pc, f, r);
}
ISG_HD void PT_NAME(genfreq_row)(float self, const isg_polyclass *pc, const float *ex, float *fr, int *err)
{
	const int b1 = pc->g[1], b2 = b1 + pc->g[2], b3 = b2 + pc->g[3], b4 = b3 + pc->g[4];
	int r;
	for (r = b4; r < pc->G; r++) PT_NAME(genfreq_quadri_at)(self, ex, fr, r, err);
	for (r = b3; r < b4; r += 3) PT_NAME(genfreq_tri_at)(self, pc, ex, fr, r, err);
	for (r = b2; r < b3; r++) PT_NAME(genfreq_duplex_at)(self, pc, ex, fr, r, err);
	for (r = b1; r < b2; r++) PT_NAME(genfreq_simplex_at)(self, pc, ex, fr, r, err);
	for (r = 0; r < b1; r++) PT_NAME(genfreq_mono_at)(self, pc, ex, fr, r, err);
}
ISG_HD void PT_NAME(exfreq_row_allo)(const isg_polyclass *pc, const double *f, const double *f2, float *ex)
{
	int r;
	for (r = 0; r < pc->G; r++) ex[r] = PT_NAME(exfreq_allo_at)(pc, f, f2, r);
}
ISG_HD void PT_NAME(genfreq_row_allo)(float self, const isg_polyclass *pc, const float *ex, float *fr, int *err)
{
	const int b1 = pc->g[1], b3 = b1 + pc->g[2] + pc->g[3];
	int r;
	for (r = b3; r < pc->G; r++) PT_NAME(genfreq_allo_ijkl_at)(self, ex, fr, r, err);
	for (r = b1; r < b3; r++) PT_NAME(genfreq_allo_het_at)(self, pc, ex, fr, r, err);
	for (r = 0; r < b1; r++) PT_NAME(genfreq_allo_iikk_at)(self, pc, ex, fr, r, err);
}
