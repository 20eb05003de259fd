/* Runs the host side of replay update_P (instruct_amd/csrc/isg_host_dirichlet.h) on the CPU and prints what tests/test_host_dirichlet.py
 * asserts on.  Comparisons of doubles and generator states are made here, bit for bit (memcmp); the layout helpers' outputs are printed
 * and compared with the index formulas written out in Python.
 *
 *   RDIRICH total equal shape_eq_1 shape_le_2.5 shape_gt_2.5
 *   PASS name ngamma formula_ngamma used outputs_equal state_equal
 *   TAPE consumed lengths equal never_on_tape left_midway on_tape_to_the_end
 *   NEED ngamma enabled need
 *   LAYOUT name dims... : values...
 */
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../instruct_amd/csrc/isg_host_dirichlet.h"

static uint64_t g_lcg = 88172645463325252ull; /* the test's own source of counts: xorshift64 */
static uint32_t rnd(uint32_t n)
{
	g_lcg ^= g_lcg << 13;
	g_lcg ^= g_lcg >> 7;
	g_lcg ^= g_lcg << 17;
	return (uint32_t)((g_lcg >> 11) % n);
}
static bool same_state(isg_wh a, isg_wh b) { return a.s1 == b.s1 && a.s2 == b.s2 && a.s3 == b.s3; }
static isg_cursor cursor_at(isg_wh s)
{
	isg_cursor c;
	c.s = s;
	c.used = 0;
	c.tape = nullptr;
	return c;
}

/* host_rdirich_pre against isg_rdirich(..., add = 1.0): 21 000 Dirichlets of 2 .. 32 components, counts from three ranges */
static void check_rdirich()
{
	const uint32_t ranges[3] = {4, 60, 20000};
	isg_wh s = {13, 4, 1972};
	long total = 0, equal = 0, one = 0, low = 0, high = 0;
	for (int r = 0; r < 3; r++)
		for (int d = 0; d < 7000; d++) {
			const int n = 2 + d % 31;
			double count[32], shape[32], want[32], got[32];
			HostGammaCoef coef[32];
			for (int k = 0; k < n; k++) {
				count[k] = (double)rnd(ranges[r]);
				shape[k] = count[k] + 1.0;
				one += shape[k] == 1.0;
				low += shape[k] > 1.0 && shape[k] <= 2.5;
				high += shape[k] > 2.5;
			}
			host_gamma_coefs(shape, (size_t)n, coef);
			isg_cursor a = cursor_at(s), b = cursor_at(s);
			isg_rdirich(&a, count, n, want, 1.0);
			host_rdirich_pre(&b, shape, coef, n, got);
			total++;
			equal += memcmp(want, got, sizeof(double) * n) == 0 && same_state(a.s, b.s) && a.used == b.used;
			s = a.s;
		}
	printf("RDIRICH %ld %ld %ld %ld %ld\n", total, equal, one, low, high);
}

struct Case {
	int K, L, A, nsub;
	bool skip;
	std::vector<int> allelenum, cnt[2];
	std::vector<double> out[2];
	HostDirichletPass pass() { return {allelenum.data(), K, L, A, skip, nsub, {cnt[0].data(), nsub > 1 ? cnt[1].data() : nullptr}, {out[0].data(), nsub > 1 ? out[1].data() : nullptr}}; }
};
static Case make_case(int K, int L, int A, int nsub, bool skip, uint32_t range)
{
	Case c;
	c.K = K; c.L = L; c.A = A; c.nsub = nsub; c.skip = skip;
	for (int j = 0; j < L; j++) c.allelenum.push_back(j % 4 == 1 ? 1 : 2 + (j * 7) % (A - 1)); /* every fourth locus has a single allele */
	for (int s = 0; s < nsub; s++) {
		c.cnt[s].assign((size_t)L * A * K, 0);
		for (int j = 0; j < L; j++)
			for (int a = 0; a < c.allelenum[j]; a++)
				for (int k = 0; k < K; k++) c.cnt[s][((size_t)j * A + a) * K + k] = (c.allelenum[j] == 1 && skip) ? 0 : (int)rnd(range);
		c.out[s].assign((size_t)K * L * A, -7.0);
	}
	return c;
}
/* the plain triple loop over isg_rdirich in the reference's order */
static isg_wh reference_pass(const Case &c, std::vector<double> out[2], uint32_t *used)
{
	isg_cursor cur = cursor_at({13, 4, 1972});
	for (int s = 0; s < c.nsub; s++) out[s].assign((size_t)c.K * c.L * c.A, -7.0);
	for (int k = 0; k < c.K; k++)
		for (int j = 0; j < c.L; j++) {
			const int Aj = c.allelenum[j];
			if (c.skip && Aj <= 1) continue;
			for (int s = 0; s < c.nsub; s++) {
				double count[64];
				for (int a = 0; a < Aj; a++) count[a] = (double)c.cnt[s][((size_t)j * c.A + a) * c.K + k];
				isg_rdirich(&cur, count, Aj, &out[s][((size_t)k * c.L + j) * c.A], 1.0);
			}
		}
	*used = cur.used;
	return cur.s;
}
static isg_wh run_pass(Case &c, const HostTape &tape)
{
	const HostDirichletPass p = c.pass();
	const uint64_t n = ngamma_of(p);
	std::vector<double> shape(n);
	std::vector<HostGammaCoef> coef(n);
	for (int s = 0; s < c.nsub; s++) c.out[s].assign((size_t)c.K * c.L * c.A, -7.0);
	host_pass_shapes(p, shape.data());
	host_gamma_coefs(shape.data(), (size_t)n, coef.data());
	return host_pass_draw(p, shape.data(), coef.data(), tape);
}
static bool same_outputs(const Case &c, const std::vector<double> want[2])
{
	for (int s = 0; s < c.nsub; s++)
		if (memcmp(c.out[s].data(), want[s].data(), sizeof(double) * want[s].size()) != 0) return false;
	return true;
}

static void check_pass(const char *name, int K, int L, int A, int nsub, bool skip, uint32_t range)
{
	static isg_wh_tables tab;
	isg_wh_tables_init(&tab);
	Case c = make_case(K, L, A, nsub, skip, range);
	std::vector<double> want[2];
	uint32_t used = 0;
	const isg_wh end = reference_pass(c, want, &used);
	const HostTape none = {nullptr, 0, {13, 4, 1972}, &tab};
	const isg_wh got = run_pass(c, none);
	uint64_t formula = 0;
	for (int j = 0; j < L; j++) formula += (skip && c.allelenum[j] <= 1) ? 0 : (uint64_t)c.allelenum[j] * K * nsub;
	printf("PASS %s %llu %llu %u %d %d\n", name, (unsigned long long)ngamma_of(c.allelenum.data(), L, K, nsub, skip), (unsigned long long)formula, used,
	       same_outputs(c, want) ? 1 : 0, same_state(end, got) ? 1 : 0);
}

/* a tape of the stream's own uniforms cut to every length from 0 to a little past what the pass consumes */
static void check_tape()
{
	static isg_wh_tables tab;
	isg_wh_tables_init(&tab);
	const isg_wh base = {13, 4, 1972};
	Case c = make_case(3, 60, 5, 2, false, 40);
	std::vector<double> want[2];
	uint32_t used = 0;
	const isg_wh end = reference_pass(c, want, &used);
	const uint32_t past = 64 * 5 + 64 + 8; /* the guard's margin for the widest Dirichlet, and a few more */
	std::vector<double> uniforms(used + past);
	isg_wh g = base;
	for (double &u : uniforms) u = isg_wh_next(&g);
	long lengths = 0, equal = 0, never = 0, midway = 0, to_end = 0;
	for (uint32_t len = 0; len <= used + past; len++) {
		/* a copy that ends where the tape does: reading past the end is an error the sanitizer build reports */
		const std::vector<double> cut(uniforms.begin(), uniforms.begin() + len);
		const HostTape tape = {cut.data(), len, base, &tab};
		const isg_wh got = run_pass(c, tape);
		lengths++;
		equal += same_outputs(c, want) && same_state(end, got);
		/* what the guard does with this length, from its own rule */
		const uint32_t first = 64 * (uint32_t)c.allelenum[0] + 64;
		if (len < first) never++;
		else if (len >= used + 64 * 5 + 64) to_end++;
		else midway++;
	}
	printf("TAPE %u %ld %ld %ld %ld %ld\n", used, lengths, equal, never, midway, to_end);
	const uint64_t ns[] = {0, 4095, 4096, 100000};
	for (uint64_t n : ns)
		for (int en = 0; en < 2; en++) printf("NEED %llu %d %llu\n", (unsigned long long)n, en, (unsigned long long)host_tape_need(n, en != 0));
}

static void print_ints(const char *head, const std::vector<int32_t> &v)
{
	printf("%s :", head);
	for (int32_t x : v) printf(" %d", x);
	printf("\n");
}
static void check_layouts()
{
	const int shapes[][4] = {{3, 7, 2, 4}, {5, 4, 5, 8}, {6, 3, 2, 6}, {1, 5, 5, 2}}; /* K, L, A, KP: KP > K except in the third */
	char head[96];
	for (const auto &sh : shapes) {
		const int K = sh[0], L = sh[1], A = sh[2], KP = sh[3], Lp = (L + 7) & ~7;
		std::vector<double> ref((size_t)K * L * A), dev((size_t)Lp * A * KP, -1.0), back((size_t)K * L * A, -2.0);
		for (size_t i = 0; i < ref.size(); i++) ref[i] = (double)(100 + i);
		freq_to_device(ref.data(), dev.data(), K, L, A, KP);
		freq_from_device(dev.data(), back.data(), K, L, A, KP);
		snprintf(head, sizeof(head), "LAYOUT freq_to_device %d %d %d %d %d %d", K, L, A, KP, Lp, back == ref ? 1 : 0);
		print_ints(head, std::vector<int32_t>(dev.begin(), dev.end()));
		std::vector<double> dev_in((size_t)Lp * A * KP);
		for (size_t i = 0; i < dev_in.size(); i++) dev_in[i] = (double)(500 + i);
		std::vector<double> out((size_t)K * L * A, -2.0), dev_back(dev_in);
		freq_from_device(dev_in.data(), out.data(), K, L, A, KP);
		freq_to_device(out.data(), dev_back.data(), K, L, A, KP); /* writes back exactly what was read: the padding stays */
		snprintf(head, sizeof(head), "LAYOUT freq_from_device %d %d %d %d %d %d", K, L, A, KP, Lp, dev_back == dev_in ? 1 : 0);
		print_ints(head, std::vector<int32_t>(out.begin(), out.end()));
		std::vector<int> c1((size_t)L * A * K), c2((size_t)L * A * K);
		for (size_t i = 0; i < c1.size(); i++) { c1[i] = (int)(10 + i); c2[i] = (int)(7000 + 3 * i); }
		std::vector<int32_t> one((size_t)K * L * A, -2), both((size_t)K * L * A, -2);
		counts_from_device(c1.data(), nullptr, one.data(), K, L, A);
		counts_from_device(c1.data(), c2.data(), both.data(), K, L, A);
		snprintf(head, sizeof(head), "LAYOUT counts_one %d %d %d", K, L, A);
		print_ints(head, one);
		snprintf(head, sizeof(head), "LAYOUT counts_both %d %d %d", K, L, A);
		print_ints(head, both);
	}
	for (int copies = 2; copies <= 4; copies += 2) {
		const int N = 3, L = 5, Lp = 8;
		std::vector<uint8_t> rows((size_t)N * Lp * copies, 0xff);
		for (int i = 0; i < N; i++)
			for (int j = 0; j < L; j++)
				for (int k = 0; k < copies; k++)
					if ((i + j) % 3 != 0 && k <= j) rows[((size_t)i * Lp + j) * copies + k] = (uint8_t)((i * 31 + j * 7 + k) % 255);
		std::vector<int32_t> out((size_t)N * L * copies, -2);
		bytes_to_ints(rows.data(), out.data(), N, L, Lp, copies);
		snprintf(head, sizeof(head), "LAYOUT bytes_in %d %d %d %d", N, L, Lp, copies);
		print_ints(head, std::vector<int32_t>(rows.begin(), rows.end()));
		snprintf(head, sizeof(head), "LAYOUT bytes_out %d %d %d %d", N, L, Lp, copies);
		print_ints(head, out);
	}
}

int main()
{
	check_rdirich();
	check_pass("skip_on", 3, 9, 5, 1, true, 60);
	check_pass("skip_off", 3, 9, 5, 1, false, 60);
	check_pass("two_subgenomes", 2, 6, 4, 2, false, 4);
	check_pass("two_subgenomes_large", 4, 11, 6, 2, false, 20000);
	check_tape();
	check_layouts();
	return 0;
}
