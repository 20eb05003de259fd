"""CPU: the closed-form genotype rows of the wide-allele ploidy-4 path (isg_poly_rank, isg_allo_row in
instruct_amd/csrc/isg_poly_tables.h) against the table order isg_poly_build / isg_allo_build list, for every allele count
1..32 and every genotype; up to 16 alleles also against the code -> row map the narrow kernels read (gidmap)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "instruct_amd", "csrc")

HARNESS = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#define PT_NAME(x) tst_##x
#define PT_LOG(x) log(x)
#define PT_EXP(x) exp(x)
#include "isg_poly_tables.h"

/* every genotype of the list, its four digits in every order: rank == position; n <= 16: the short map the narrow path builds */
static int check_auto(int n)
{
	int g[6], bad = 0;
	const int G = isg_poly_G(n);
	int *list = (int *)malloc(sizeof(int) * (G + 1));
	isg_poly_build(n, g, list);
	short *map = NULL;
	if (n <= 16) {
		map = (short *)malloc(sizeof(short) * n * n * n * n);
		for (int c = 0; c < n * n * n * n; c++) map[c] = -1;
		for (int r = 0; r < G; r++) map[list[r]] = (short)r;
	}
	static const int perm[24][4] = {{0,1,2,3},{0,1,3,2},{0,2,1,3},{0,2,3,1},{0,3,1,2},{0,3,2,1},{1,0,2,3},{1,0,3,2},{1,2,0,3},{1,2,3,0},
		{1,3,0,2},{1,3,2,0},{2,0,1,3},{2,0,3,1},{2,1,0,3},{2,1,3,0},{2,3,0,1},{2,3,1,0},{3,0,1,2},{3,0,2,1},{3,1,0,2},{3,1,2,0},{3,2,0,1},{3,2,1,0}};
	for (int r = 0; r < G; r++) {
		const int code = list[r], d[4] = {code / (n * n * n), (code / (n * n)) % n, (code / n) % n, code % n};
		for (int p = 0; p < 24; p++)
			if (isg_poly_rank(n, d[perm[p][0]], d[perm[p][1]], d[perm[p][2]], d[perm[p][3]]) != r) bad++;
		if (map && map[((d[0] * n + d[1]) * n + d[2]) * n + d[3]] != isg_poly_rank(n, d[0], d[1], d[2], d[3])) bad++;
	}
	free(list);
	free(map);
	return bad;
}
static int check_allo(int n)
{
	int g[6], bad = 0;
	const int G = isg_allo_G(n);
	int *list = (int *)malloc(sizeof(int) * (G + 1));
	isg_allo_build(n, g, list);
	for (int r = 0; r < G; r++) {
		const int code = list[r], d0 = code / (n * n * n), d1 = (code / (n * n)) % n, d2 = (code / n) % n, d3 = code % n;
		if (isg_allo_row(n, d0, d1, d2, d3) != r || isg_allo_row_any(n, d1, d0, d3, d2) != r) bad++;
	}
	free(list);
	return bad;
}
int main(void)
{
	for (int n = 1; n <= 32; n++) {
		const int a = check_auto(n), b = check_allo(n);
		printf("%d %d %d %d %d\n", n, isg_poly_G(n), a, isg_allo_G(n), b);
	}
	return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank")
    src, exe = str(d / "rank.c"), str(d / "rank")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-I", CSRC, "-o", exe, src, "-lm"])
    out = subprocess.check_output([exe], text=True)
    return {int(t[0]): tuple(int(x) for x in t[1:]) for t in (l.split() for l in out.splitlines())}


@pytest.mark.parametrize("n", range(1, 33))
def test_autotetraploid_rank_is_the_list_position(rows, n):
    G, bad, _, _ = rows[n]
    assert G == n + n * (n - 1) * 3 // 2 + n * (n - 1) * (n - 2) // 2 + n * (n - 1) * (n - 2) * (n - 3) // 24
    assert bad == 0


@pytest.mark.parametrize("n", range(1, 33))
def test_allotetraploid_row_is_the_list_position(rows, n):
    _, _, G, bad = rows[n]
    assert G == n * n + n * (n - 1) * n + (n * (n - 1) // 2) ** 2
    assert bad == 0


def test_thirty_two_alleles_overflow_a_short_row():
    """why the wide path cannot keep the map: 52 360 / 278 784 rows at 32 alleles"""
    assert (52360, 278784) == (32 + 32 * 31 * 3 // 2 + 32 * 31 * 30 // 2 + 32 * 31 * 30 * 29 // 24, 32 * 32 + 32 * 31 * 32 + (32 * 31 // 2) ** 2)
