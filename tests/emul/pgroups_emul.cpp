/* Prints pgroups_build (instruct_amd/csrc/isg_pgroups.h) for the panel given on the command line:
 *   pgroups_emul K Amax min_alleles sub sub_stride ngmax allelenum[0] allelenum[1] ...
 * "OK 0|1", then "G NG", one line "g gam0 n sub" per group, and the count indices of all gammas in one line
 * (tests/test_pgroups.py computes the expected values in numpy). */
#include <stdio.h>
#include <stdlib.h>
#include "../../instruct_amd/csrc/isg_pgroups.h"

int main(int argc, char **argv)
{
	if (argc < 8) return 2;
	const int K = atoi(argv[1]), Amax = atoi(argv[2]), min_alleles = atoi(argv[3]), sub = atoi(argv[4]), ngmax = atoi(argv[6]);
	const long long sub_stride = atoll(argv[5]);
	std::vector<int> an;
	for (int k = 7; k < argc; k++) an.push_back(atoi(argv[k]));
	PGroups P;
	const bool ok = pgroups_build(P, (int)an.size(), K, Amax, an.data(), min_alleles, sub, sub_stride, ngmax);
	printf("OK %d\n", ok ? 1 : 0);
	if (!ok) return 0;
	const int G = (int)P.gam0.size() - 1;
	printf("%d %d\n", G, (int)P.gidx.size());
	for (int g = 0; g < G; g++) printf("%d %d %d %d\n", g, P.gam0[g], P.gam0[g + 1] - P.gam0[g], (int)P.gsub[g]);
	for (int v : P.gidx) printf("%d ", v);
	printf("\n");
	return 0;
}
