/* Host checks of the float-resident Wichmann-Hill state (instruct_amd/csrc/isg_wh.h: isg_whf_*), the code the device runs.
 * Built by tests/test_whf_step.py with gcc -ffp-contract=off; every function returns the number of disagreements it found. */
#include <stdint.h>
#include <string.h>
#include "../../instruct_amd/csrc/isg_wh.h"

static const uint32_t M[3] = {ISG_M1, ISG_M2, ISG_M3}, A[3] = {ISG_A1, ISG_A2, ISG_A3};

static float comp(const isg_whf *f, int g) { return g == 0 ? f->s1 : (g == 1 ? f->s2 : f->s3); }

/* every state s < limit[g] of generator g, through isg_whf_step itself: the result is (a*s) % m and an integer-valued float */
long whf_step_exhaustive(int extra)
{
	long bad = 0;
	for (int g = 0; g < 3; g++) {
		for (uint32_t s = 0; s < M[g] + (uint32_t)extra; s++) {
			isg_whf f = {0.f, 0.f, 0.f};
			if (g == 0) f.s1 = (float)s;
			else if (g == 1) f.s2 = (float)s;
			else f.s3 = (float)s;
			isg_whf_step(&f);
			const float r = comp(&f, g);
			const uint32_t want = (A[g] * s) % M[g];
			if (!(r == (float)want) || (float)(uint32_t)r != r || isg_f2u(r) != isg_f2u((float)want)) bad++;
		}
	}
	return bad;
}

/* isg_whf_from reduces states at or above the modulus; isg_whf_to gives the integers back */
long whf_from_reduces(void)
{
	long bad = 0;
	for (uint32_t s = 0; s < 200000; s += 7) {
		isg_wh w = {s, s + 1, s + 2};
		const isg_whf f = isg_whf_from(w);
		const isg_wh b = isg_whf_to(f);
		if (f.s1 != (float)(s % ISG_M1) || f.s2 != (float)((s + 1) % ISG_M2) || f.s3 != (float)((s + 2) % ISG_M3)) bad++;
		if (b.s1 != s % ISG_M1 || b.s2 != (s + 1) % ISG_M2 || b.s3 != (s + 2) % ISG_M3) bad++;
	}
	return bad;
}

/* n steps from the seeds: the float state equals the integer one at every step, value_f32 as bits, the exact value as bits */
long whf_walk(uint32_t s1, uint32_t s2, uint32_t s3, long n)
{
	isg_wh w = {s1, s2, s3};
	isg_whf f = isg_whf_from(w);
	long bad = 0;
	w.s1 %= ISG_M1; w.s2 %= ISG_M2; w.s3 %= ISG_M3;
	for (long k = 0; k < n; k++) {
		/* the plain formulas of the generator, not a shortcut of the header's */
		w.s1 = (ISG_A1 * w.s1) % ISG_M1;
		w.s2 = (ISG_A2 * w.s2) % ISG_M2;
		w.s3 = (ISG_A3 * w.s3) % ISG_M3;
		isg_whf_step(&f);
		const isg_wh b = isg_whf_to(f);
		if (b.s1 != w.s1 || b.s2 != w.s2 || b.s3 != w.s3) bad++;
		if (isg_f2u(isg_whf_value_f32(&f)) != isg_f2u(isg_wh_value_f32(&w))) bad++;
		if (isg_d2u(isg_whf_value(&f)) != isg_d2u(isg_wh_value(&w))) bad++;
	}
	return bad;
}

/* the redo path: the state of copy c8 of a pass, re-derived from the lane's pass-start state and the validity mask of its loci, is the
 * state the pass itself reached for that copy (stepping twice per locus, an unused locus handing its predecessor's state on) */
long whf_rederive(uint32_t s1, uint32_t s2, uint32_t s3, unsigned vmask)
{
	const isg_wh w = {s1, s2, s3};
	const isg_whf start = isg_whf_from(w);
	isg_wh s = isg_whf_to(start);
	long bad = 0;
	for (int l = 0; l < 4; l++) { /* four loci per lane and pass, as in zq_one */
		isg_wh s2w = s;
		for (int cp = 0; cp < 2; cp++) {
			isg_wh_step(&s2w);
			if ((vmask >> l) & 1u) {
				const isg_whf r = isg_whf_copy_state(start, vmask, 2 * l + cp);
				const isg_wh b = isg_whf_to(r);
				if (b.s1 != s2w.s1 || b.s2 != s2w.s2 || b.s3 != s2w.s3) bad++;
			}
		}
		if ((vmask >> l) & 1u) s = s2w;
	}
	return bad;
}
