/*
 * isg_pgroups.h -- replay update_P's Dirichlets as the walk engine's groups (isg_walk_hip.inc), in the reference's stream order.
 * Plain host code: tests/emul/pgroups_emul.cpp prints it for tests/test_pgroups.py.  The allotetraploid chain's list is built here
 * (pdev_create_allo, isg_poly_hip.inc); with sub = 1 the function gives the lists pdev_create (isg_walk_hip.inc) builds for the other two.
 *
 *   ploidy 2          mcmc.c:846-857       for k < K, for j < L with allelenum[j] > 1: the alleles of (k, j)          (min_alleles = 1, sub = 1)
 *   autotetraploid    poly_geno.c:426-434  the same without the allelenum > 1 test: a one-allele locus is a group of one (min_alleles = 0, sub = 1)
 *   allotetraploid    poly_geno.c:491-502  for k < K, for j < L: the alleles of (k, j) in the first subgenome (counts in cnt, result in freq), then
 *                                          the same alleles in the second (cnt2 -> freq2): two groups, each normalised on its own
 *                                                                                                                     (min_alleles = 0, sub = 2)
 *
 * The second subgenome's arrays follow the first's in one allocation: cnt2 = cnt + sub_stride, sub_stride a multiple of K, and freq2 = freq +
 * (sub_stride / K) KP.  A gamma of the second subgenome is then just a count index beyond sub_stride, and k_pd_gather / k_pdirich_at
 * (isg_walk_hip.inc: count at cnt[gidx], frequency at freq[(gidx / K) KP + gidx % K]) take the list as they take any other.
 */
#ifndef ISG_PGROUPS_H
#define ISG_PGROUPS_H
#include <vector>

struct PGroups {
	std::vector<int> gam0;           /* [G + 1] first gamma of every group */
	std::vector<int> gidx;           /* [NG] a gamma's count: index into cnt ([L][Amax][K]); second subgenome: + sub_stride, i.e. into cnt2 */
	std::vector<unsigned char> gsub; /* [G] the group's subgenome: 0 (cnt -> freq), 1 (cnt2 -> freq2) */
};

/* false: a locus has more than ngmax alleles (more than a group of the engine holds), or the indices do not fit an int */
static bool pgroups_build(PGroups &P, int L, int K, int Amax, const int *allelenum, int min_alleles, int sub, long long sub_stride, int ngmax)
{
	P = PGroups();
	P.gam0.push_back(0);
	if ((long long)L * Amax * K + (sub - 1) * sub_stride > 0x7fffffffLL) return false;
	for (int k = 0; k < K; k++)
		for (int j = 0; j < L; j++) {
			const int Aj = allelenum[j];
			if (Aj <= min_alleles) continue;
			if (Aj > ngmax) return false;
			for (int s = 0; s < sub; s++) {
				for (int a = 0; a < Aj; a++) P.gidx.push_back((int)(s * sub_stride) + (j * Amax + a) * K + k);
				P.gam0.push_back((int)P.gidx.size());
				P.gsub.push_back((unsigned char)s);
			}
		}
	return true;
}

#endif
