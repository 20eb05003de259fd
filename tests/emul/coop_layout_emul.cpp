/* Prints coop_layout (instruct_amd/csrc/isg_coop_layout.h) over the grid below: one line
 * "copies G K Lp wmode pack bits W ngran" per case, then "LIMITS ring gmax wmax" (tests/test_coop_layout.py computes
 * the expected values from the formulas the kernels used to carry). */
#include <stdio.h>
#include "../../instruct_amd/csrc/isg_coop_layout.h"

int main()
{
	const int BLOCK = 256, Gs[] = {1, 2, 3, 11, 32, 128}, passes[] = {1, 3, 8}, copies[] = {2, 4};
	for (int cp : copies)
		for (int G : Gs)
			for (int np : passes)
				for (int tail = 0; tail < 2; tail++) { /* a full last pass, and one that holds a single locus */
					const int Lp = tail ? (np - 1) * G * BLOCK + 1 : np * G * BLOCK;
					for (int K = 1; K <= 32; K++) {
						const CoopLayout l = coop_layout(G, BLOCK, K, Lp, cp);
						printf("%d %d %d %d %d %d %d %d %d\n", cp, G, K, Lp, l.wmode ? 1 : 0, l.pack, l.bits, l.W, l.ngran);
					}
				}
	printf("LIMITS %d %d %d\n", ISG_COOP_RING, ISG_COOP_GMAX, ISG_COOP_WMAX);
	return 0;
}
