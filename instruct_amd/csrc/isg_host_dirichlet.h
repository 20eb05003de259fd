/*
 * isg_host_dirichlet.h -- the host side of update_P in the replay schedule, without any HIP in it (tests/emul/host_dirichlet_emul.cpp
 * runs it on the CPU): the K L Dirichlets drawn in stream order from the counts, the uniform tape they may read, and the layout
 * conversions between the reference's arrays and the device's.
 *
 *   host_gamma_coef(s), host_rgamma2_try_pre, host_rdirich_pre   rdirich with rgamma2's accept test pre-decided in single precision
 *   HostTape, host_tape_need / _attach / _guard / _end            the uniforms generated beforehand, and leaving them when they run short
 *   HostDirichletPass, ngamma_of, host_pass_shapes / _draw       one pass over all Dirichlets of a sweep
 *   freq_to_device / freq_from_device / counts_from_device / bytes_to_ints
 */
#ifndef ISG_HOST_DIRICHLET_H
#define ISG_HOST_DIRICHLET_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <thread>
#include <vector>
#include "isg_math.h"
#include "isg_wh.h"
#include "isg_sampler.h"

/*
 * rdirich (random.c:264-280) with the accept / reject test of rgamma2 (random.c:195-231) pre-decided in single precision,
 * exactly as rgamma2_try_dev does on the device -- the two logarithms only feed the comparison
 * c3 log(u1) - log(w) + w >= 1; outside a band of 2e-6 (1 + |terms|) the float value decides, inside it the double
 * expression.  Same values, same consumption as isg_rdirich.
 *
 * rgamma2's constants only depend on the shape (random.c:199-203): the sequential loop has three divisions and a square root
 * less per attempt when they are formed beforehand -- for all gammas of the sweep at once, by a few threads (the shapes are
 * the counts + 1, known before the first draw).  Same expressions, same values.
 */
struct HostGammaCoef { double c1, c2, c3, c4, c5; };
static inline void host_gamma_coef(double alpha, HostGammaCoef *o)
{
	o->c1 = alpha - 1;
	o->c2 = (alpha - 1 / (6 * alpha)) / o->c1;
	o->c3 = 2 / o->c1;
	o->c4 = o->c3 + 2;
	o->c5 = 1 / isg_sqrt(alpha);
}
static inline void host_gamma_coefs(const double *shape, size_t n, HostGammaCoef *out)
{
	unsigned nt = std::thread::hardware_concurrency();
	nt = nt > 4 ? 4 : (nt < 1 ? 1 : nt);
	if (n < 16384) nt = 1;
	auto work = [&](size_t a, size_t b) { for (size_t g = a; g < b; g++) host_gamma_coef(shape[g], &out[g]); };
	std::vector<std::thread> th;
	const size_t per = (n + nt - 1) / nt;
	for (unsigned k = 1; k < nt; k++) th.emplace_back(work, k * per < n ? k * per : n, (k + 1) * per < n ? (k + 1) * per : n);
	work(0, per < n ? per : n);
	for (auto &t : th) t.join();
}
static inline double host_rgamma2_try_pre(isg_cursor *c, double alpha, const HostGammaCoef &k)
{
	double u1, u2, w;
	do {
		u1 = isg_cur_next(c);
		u2 = isg_cur_next(c);
		if (alpha > 2.5) u1 = u2 + k.c5 * (1 - 1.86 * u1);
	} while ((u1 >= 1) || (u1 <= 0));
	w = k.c2 * u2 / u1;
	if ((k.c3 * u1 + w + 1 / w) > k.c4) {
		const float l1 = logf((float)u1), lw = logf((float)w);
		const double al1 = fabs((double)l1), alw = fabs((double)lw);
		const double dlt = (k.c3 * (double)l1 - (double)lw + w) - 1;
		const double tol = 2e-6 * (fabs(k.c3) * (1.0 + al1) + 1.0 + alw) + 1e-12 * fabs(w);
		bool rej;
		if (dlt > tol) rej = true;
		else if (dlt < -tol) rej = false;
		else rej = (k.c3 * isg_log(u1) - isg_log(w) + w) >= 1;
		if (rej) return -1;
	}
	return k.c1 * w;
}
/* rdirich over shapes given directly (count + 1 already formed) with their constants */
static inline void host_rdirich_pre(isg_cursor *c, const double *shape, const HostGammaCoef *coef, int n, double *out)
{
	double sum = 0;
	for (int k = 0; k < n; k++) {
		const double a = shape[k];
		double g = 0;
		if (a > 1) {
			do { g = host_rgamma2_try_pre(c, a, coef[k]); } while (g < 0);
		} else {
			g = isg_rgamma(c, a);
		}
		out[k] = g;
		sum += g;
	}
	for (int k = 0; k < n; k++) out[k] /= sum;
}

/*
 * The uniforms of the loop may have been generated beforehand (on the device: half of the loop's time was the generator, 21 ns per
 * uniform, ~3 per gamma of ~118 ns): `tape` holds the next `len` uniforms of the stream that is in state `base` at the tape's start.
 * They are budgeted at 3 per gamma; if they run short the loop continues with the generator from the position reached -- same values
 * either way.  len == 0: no tape, the generator from `base`.
 */
struct HostTape {
	const double *tape;
	uint64_t len;
	isg_wh base;
	const isg_wh_tables *tab; /* skip-ahead */
};
/* uniforms to generate for a sweep of ngamma gammas; 0: the sweep is too small to gain from a tape (or tapes are switched off) */
static inline uint64_t host_tape_need(uint64_t ngamma, bool enabled) { return (!enabled || ngamma < 4096) ? 0 : 3 * ngamma + 65536; }
/* once the tape has arrived, before the loop */
static inline void host_tape_attach(const HostTape &t, isg_cursor *cur)
{
	cur->s = t.base;
	cur->used = 0;
	cur->tape = t.len ? t.tape : nullptr;
}
/* before each Dirichlet of n gammas: leave the tape while a comfortable margin remains (32 attempts per gamma) */
static inline void host_tape_guard(const HostTape &t, isg_cursor *cur, int n)
{
	if (cur->tape && (uint64_t)cur->used + 64ull * (unsigned)n + 64 > t.len) {
		cur->s = isg_wh_jump(t.tab, t.base, cur->used);
		cur->tape = nullptr;
	}
}
/* the generator's state after the loop */
static inline isg_wh host_tape_end(const HostTape &t, const isg_cursor *cur) { return cur->tape ? isg_wh_jump(t.tab, t.base, cur->used) : cur->s; }

/*
 * One pass over the Dirichlets of a sweep in stream order: (cluster, locus) outermost; with two subgenomes (allotetraploid) the first
 * subgenome's Dirichlet of a (cluster, locus), then the second's (poly_geno.c:499-506).  The diploid update_P passes over loci with a
 * single allele without drawing (its allelenum > 1 test); the ploidy 4 ones draw their one gamma (poly_geno.c:426-434).
 */
struct HostDirichletPass {
	const int *allelenum; /* [L] */
	int K, L, A;          /* A: the arrays' allele stride (Amax) */
	bool skip_single;
	int nsub;             /* subgenomes: 1 or 2 */
	const int *cnt[2];    /* counts in device order [L][A][K], one array per subgenome */
	double *out[2];       /* frequencies in the reference's order [K][L][A] */
};
static inline uint64_t ngamma_of(const int *allelenum, int L, int K, int subgenomes, bool skip_single)
{
	uint64_t n = 0;
	for (int j = 0; j < L; j++) n += (skip_single && allelenum[j] <= 1) ? 0 : (uint64_t)allelenum[j] * K * subgenomes;
	return n;
}
static inline uint64_t ngamma_of(const HostDirichletPass &p) { return ngamma_of(p.allelenum, p.L, p.K, p.nsub, p.skip_single); }
/* the shapes (count + 1.0, rdirich's `add`) of all gammas in stream order: shape[ngamma_of(p)] */
static inline void host_pass_shapes(const HostDirichletPass &p, double *shape)
{
	size_t g = 0;
	for (int k = 0; k < p.K; k++)
		for (int j = 0; j < p.L; j++) {
			const int Aj = p.allelenum[j];
			if (p.skip_single && Aj <= 1) continue;
			for (int s = 0; s < p.nsub; s++)
				for (int a = 0; a < Aj; a++) shape[g++] = (double)p.cnt[s][((size_t)j * p.A + a) * p.K + k] + 1.0;
		}
}
/* the draws, from shapes and their constants (host_gamma_coefs); returns the generator's state after the last one */
static inline isg_wh host_pass_draw(const HostDirichletPass &p, const double *shape, const HostGammaCoef *coef, const HostTape &tape)
{
	isg_cursor cur;
	host_tape_attach(tape, &cur);
	size_t g = 0;
	for (int k = 0; k < p.K; k++)
		for (int j = 0; j < p.L; j++) {
			const int Aj = p.allelenum[j];
			if (p.skip_single && Aj <= 1) continue;
			for (int s = 0; s < p.nsub; s++) {
				host_tape_guard(tape, &cur, Aj);
				host_rdirich_pre(&cur, shape + g, coef + g, Aj, p.out[s] + ((size_t)k * p.L + j) * p.A);
				g += (size_t)Aj;
			}
		}
	return host_tape_end(tape, &cur);
}

/* ---- layouts: the reference keeps [K][L][A], the device [L][A][KP] (frequencies, KP >= K) and [L][A][K] (counts) ---- */
static inline void freq_to_device(const double *ref, double *dev, int K, int L, int A, int KP)
{
	for (int k = 0; k < K; k++)
		for (int j = 0; j < L; j++)
			for (int a = 0; a < A; a++) dev[((size_t)j * A + a) * KP + k] = ref[((size_t)k * L + j) * A + a];
}
static inline void freq_from_device(const double *dev, double *ref, int K, int L, int A, int KP)
{
	for (int k = 0; k < K; k++)
		for (int j = 0; j < L; j++)
			for (int a = 0; a < A; a++) ref[((size_t)k * L + j) * A + a] = dev[((size_t)j * A + a) * KP + k];
}
/* dev2 (may be null): a second subgenome's counts, added in */
static inline void counts_from_device(const int *dev, const int *dev2, int32_t *ref, int K, int L, int A)
{
	for (int k = 0; k < K; k++)
		for (int j = 0; j < L; j++)
			for (int a = 0; a < A; a++) {
				const size_t s = ((size_t)j * A + a) * K + k;
				ref[((size_t)k * L + j) * A + a] = dev[s] + (dev2 ? dev2[s] : 0);
			}
}
/* [N][Lp][copies] bytes, 0xFF where the locus is unused -> [N][L][copies] ints, -1 there */
static inline void bytes_to_ints(const uint8_t *rows, int32_t *out, int N, int L, int Lp, int copies)
{
	for (int i = 0; i < N; i++)
		for (int j = 0; j < L; j++)
			for (int k = 0; k < copies; k++) {
				const uint8_t v = rows[((size_t)i * Lp + j) * copies + k];
				out[((size_t)i * L + j) * copies + k] = (v == 0xff) ? -1 : (int)v;
			}
}

#endif
