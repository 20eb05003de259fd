/* The per-row table functions of instruct_amd/csrc/isg_poly_tables.h on the CPU, for tests/test_poly_tables.py.  The header is
 * instantiated with the canonical math (isg_math.h) and with glibc, as the oracle does, and a third time with isg_poly_rank /
 * isg_allo_row_any replaced by versions that check every row they hand out.  For every allele count argv[1] .. argv[2] (default 1 .. 32;
 * a count's lines do not depend on the range, so the test runs several ranges side by side), both tetraploid variants and the selfing
 * rates 0, 0.05, 0.5, 0.95, 1 (ploidy 4 with -e 0 reaches exactly 0 and 1):
 *   EX    variant n G rows bad       exfreq_row against the _at function called in descending r
 *   GEN   variant n G runs bad odd   k4_genfreq_w's schedule (lanes t = 0..255 over each class, ascending and descending, the rows not
 *                                    yet solved poisoned with 0.0f and with a quiet NaN before every class) against genfreq_row;
 *                                    odd = rows of genfreq_row that are not finite (compared by bit pattern like all others)
 *   NEG   variant n differing        the same with two classes swapped: has to differ, or the poison proves nothing
 *   READS variant n reads bad        n <= 6: rows a per-row function looked up that lie outside [end of its class, G)
 * Everything is compared as uint32 images of the floats and of the err word, without a tolerance. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define PT_NAME(x) pti_##x
#define PT_LOG(x) isg_log(x)
#define PT_EXP(x) isg_exp(x)
#include "../../instruct_amd/csrc/isg_poly_tables.h"
#undef PT_NAME
#undef PT_LOG
#undef PT_EXP
#define PT_NAME(x) ptl_##x
#define PT_LOG(x) log(x)
#define PT_EXP(x) exp(x)
#include "../../instruct_amd/csrc/isg_poly_tables.h"
#undef PT_NAME

/* third instance: every row a row function finds has to belong to a class solved before the one being computed */
static int g_lo, g_hi;
static long g_reads, g_bad_reads;
static int note(int row)
{
	g_reads++;
	if (row < g_lo || row >= g_hi) g_bad_reads++;
	return row < 0 || row >= g_hi ? 0 : row;
}
static int rec_poly_rank(int n, int a, int b, int c, int d) { return note(isg_poly_rank(n, a, b, c, d)); }
static int rec_allo_row_any(int n, int a, int b, int c, int d) { return note(isg_allo_row_any(n, a, b, c, d)); }
#define isg_poly_rank rec_poly_rank
#define isg_allo_row_any rec_allo_row_any
#define PT_NAME(x) ptr_##x
#include "../../instruct_amd/csrc/isg_poly_tables.h"
#undef PT_NAME
#undef isg_poly_rank
#undef isg_allo_row_any

typedef void (*RowAt0)(float, const float *, float *, int, int *);
typedef void (*RowAt)(float, const isg_polyclass *, const float *, float *, int, int *);
struct Inst {
	float (*exfreq_at)(const isg_polyclass *, const double *, int);
	float (*exfreq_allo_at)(const isg_polyclass *, const double *, const double *, int);
	void (*exfreq_row)(const isg_polyclass *, const double *, float *);
	void (*exfreq_row_allo)(const isg_polyclass *, const double *, const double *, float *);
	void (*genfreq_row)(float, const isg_polyclass *, const float *, float *, int *);
	void (*genfreq_row_allo)(float, const isg_polyclass *, const float *, float *, int *);
	RowAt0 quadri, allo_ijkl;
	RowAt tri, duplex, simplex, mono, allo_het, allo_iikk;
};
#define INST(p) {p##exfreq_at, p##exfreq_allo_at, p##exfreq_row, p##exfreq_row_allo, p##genfreq_row, p##genfreq_row_allo, p##genfreq_quadri_at, \
	p##genfreq_allo_ijkl_at, p##genfreq_tri_at, p##genfreq_duplex_at, p##genfreq_simplex_at, p##genfreq_mono_at, p##genfreq_allo_het_at, p##genfreq_allo_iikk_at}
static const Inst CANON = INST(pti_), GLIBC = INST(ptl_), RECORD = INST(ptr_);

/* the classes in the order k4_genfreq_w takes them: rows first .. end - 1, one lane per `step` rows (a tri lane solves a triple) */
struct Class { int first, end, step; RowAt0 f0; RowAt f; };
static int classes(const Inst &I, bool allo, const isg_polyclass &pc, Class cl[5])
{
	const int b1 = pc.g[1], b2 = b1 + pc.g[2], b3 = b2 + pc.g[3], b4 = b3 + pc.g[4];
	if (allo) {
		cl[0] = {b3, pc.G, 1, I.allo_ijkl, 0}; cl[1] = {b1, b3, 1, 0, I.allo_het}; cl[2] = {0, b1, 1, 0, I.allo_iikk};
		return 3;
	}
	cl[0] = {b4, pc.G, 1, I.quadri, 0}; cl[1] = {b3, b4, 3, 0, I.tri}; cl[2] = {b2, b3, 1, 0, I.duplex};
	cl[3] = {b1, b2, 1, 0, I.simplex}; cl[4] = {0, b1, 1, 0, I.mono};
	return 5;
}

/* a workgroup of 256 lanes, one after the other: per class, lane t takes rows first + step t, first + step (t + 256), ...; what a
 * barrier separates on the device is separated by the class loop here.  Before a class its own rows and those of all classes still
 * to come are overwritten with `poison`. */
static void schedule(const Class *cl, const int *order, int ncl, float s, const isg_polyclass &pc, const float *ex, float *fr, int *err, bool descending, float poison)
{
	for (int c = 0; c < ncl; c++) {
		const Class &k = cl[order[c]];
		for (int d = c; d < ncl; d++)
			for (int r = cl[order[d]].first; r < cl[order[d]].end; r++) fr[r] = poison;
		g_lo = k.end;
		g_hi = pc.G;
		for (int i = 0; i < 256; i++) {
			const int t = descending ? 255 - i : i;
			for (int r = k.first + k.step * t; r < k.end; r += k.step * 256) {
				if (k.f0) k.f0(s, ex, fr, r, err);
				else k.f(s, &pc, ex, fr, r, err);
			}
		}
	}
}

static uint64_t lcg;
static double uni() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0; }
static void frequencies(int n, double *f)
{
	double sum = 0;
	for (int a = 0; a < n; a++) sum += (f[a] = 0.01 + uni());
	if (n == 1) { f[0] = 1.0; return; }
	const int tiny = (int)(uni() * n);
	sum -= f[tiny];
	for (int a = 0; a < n; a++) f[a] = a == tiny ? 1e-12 : f[a] / sum * (1.0 - 1e-12);
}
static long differing(const std::vector<float> &a, const std::vector<float> &b, int ea, int eb)
{
	long bad = ea != eb;
	for (size_t r = 0; r < a.size(); r++) {
		uint32_t x, y;
		memcpy(&x, &a[r], 4);
		memcpy(&y, &b[r], 4);
		bad += x != y;
	}
	return bad;
}

int main(int argc, char **argv)
{
	const int nmin = argc > 2 ? atoi(argv[1]) : 1, nmax = argc > 2 ? atoi(argv[2]) : 32;
	const float rates[5] = {0.0f, 0.05f, 0.5f, 0.95f, 1.0f}, poisons[2] = {0.0f, NAN};
	const int straight[5] = {0, 1, 2, 3, 4};
	for (int allo = 0; allo < 2; allo++)
		for (int n = nmin; n <= nmax; n++) {
			const char *name = allo ? "allo" : "auto";
			const int G = allo ? isg_allo_G(n) : isg_poly_G(n);
			std::vector<int> list(G + 1);
			isg_polyclass pc;
			pc.n = n;
			allo ? isg_allo_build(n, pc.g, list.data()) : isg_poly_build(n, pc.g, list.data());
			pc.G = pc.g[0];
			pc.list = list.data();
			if (pc.G != G) return 2;
			double f[32], f2[32];
			lcg = 20261018 + 100 * allo + n;
			frequencies(n, f);
			frequencies(n, f2);
			std::vector<float> ex(G), ref(G), got(G);
			long ex_rows = 0, ex_bad = 0, gen_runs = 0, gen_bad = 0, odd = 0, neg = 0;
			for (const Inst *I : {&CANON, &GLIBC}) {
				allo ? I->exfreq_row_allo(&pc, f, f2, ex.data()) : I->exfreq_row(&pc, f, ex.data());
				for (int r = G - 1; r >= 0; r--) {
					const float v = allo ? I->exfreq_allo_at(&pc, f, f2, r) : I->exfreq_at(&pc, f, r);
					ex_rows++;
					ex_bad += memcmp(&v, &ex[r], 4) != 0;
				}
				Class cl[5];
				const int ncl = classes(*I, allo, pc, cl);
				for (float s : rates) {
					int eref = 0;
					ref.assign(G, NAN);
					allo ? I->genfreq_row_allo(s, &pc, ex.data(), ref.data(), &eref) : I->genfreq_row(s, &pc, ex.data(), ref.data(), &eref);
					for (float v : ref) odd += !(v - v == 0);
					for (float poison : poisons)
						for (int descending = 0; descending < 2; descending++) {
							int e = 0;
							got.assign(G, poison);
							schedule(cl, straight, ncl, s, pc, ex.data(), got.data(), &e, descending, poison);
							gen_runs++;
							gen_bad += differing(got, ref, e, eref);
						}
					if (n == 5 && s == 0.5f) { /* swapped: (auto) simplex before duplex, (allo) iikk before iikl / ijkk */
						const int swapped[5] = {0, allo ? 2 : 1, allo ? 1 : 3, 2, 4};
						long differ = 0;
						for (float poison : poisons) {
							int e = 0;
							got.assign(G, poison);
							schedule(cl, swapped, ncl, s, pc, ex.data(), got.data(), &e, false, poison);
							differ += differing(got, ref, e, eref) != 0;
						}
						neg += differ;
					}
				}
			}
			printf("EX %s %d %d %ld %ld\n", name, n, G, ex_rows, ex_bad);
			printf("GEN %s %d %d %ld %ld %ld\n", name, n, G, gen_runs, gen_bad, odd);
			if (n == 5) printf("NEG %s %d %ld\n", name, n, neg);
			if (n <= 6) {
				Class cl[5];
				const int ncl = classes(RECORD, allo, pc, cl);
				g_reads = g_bad_reads = 0;
				for (float s : rates) {
					int e = 0;
					got.assign(G, NAN);
					schedule(cl, straight, ncl, s, pc, ex.data(), got.data(), &e, false, NAN);
				}
				printf("READS %s %d %ld %ld\n", name, n, g_reads, g_bad_reads);
			}
		}
	return 0;
}
