/* Prints, for every ladder of instruct_amd/csrc/isg_kdispatch.h and K = 1 .. 64, the rung kdispatch chooses:
 * one line "NAME r1 r2 ... r64" per ladder (tests/test_kdispatch.py holds the expected rows). */
#include <stdio.h>
#include "../../instruct_amd/csrc/isg_kdispatch.h"

template <class L>
static void row(const char *name)
{
	printf("%s", name);
	for (int K = 1; K <= 64; K++) {
		int got = 0, calls = 0;
		kdispatch(L(), K, [&](auto km) { got = decltype(km)::value; calls++; });
		printf(" %d", calls == 1 ? got : -1);
	}
	printf("\n");
}

int main()
{
	row<KL_ZQ>("KL_ZQ");
	row<KL_ZQ_COOP>("KL_ZQ_COOP");
	row<KL_ZQ_8>("KL_ZQ_8");
	row<KL_ZQ_EXACT>("KL_ZQ_EXACT");
	row<KL_P4>("KL_P4");
	row<KL_P4_BLOCK>("KL_P4_BLOCK");
	row<KL_P4_GENO>("KL_P4_GENO");
	return 0;
}
