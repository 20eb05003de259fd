"""Fixtures for ploidy 4 with more than 16 alleles per locus (tests/test_oracle_poly_alleles.py, tests/test_gpu_poly_alleles.py),
written by the reference's own code.

    python -m instruct_amd.build --oracle && python tests/golden/make_golden_alleles.py

tw_auto.txt / .golden    oracle/_ref/ref_dump_poly (the reference's poly_geno.c sweeps), -ap 1: loci of 17..24 alleles and of 1..4
tw_allo.txt / .golden    the same, -ap 0: loci of 17 and 18 alleles (29 241 genotypes) and of 2..3
tw_cli_output.txt        the reference program, -p 4 -ap 1, on tw_auto.txt
"""
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (also puts the repository on sys.path)
from instruct_amd import synth  # noqa: E402

# name: (N, L, K, allele counts per locus, missing, u, b, t, e, r, j, seeds, allo) -- every listed allele is observed
CASES = {
    "tw_auto": (60, 8, 2, (17, 19, 20, 24, 1, 2, 3, 4), 0.03, 2, 1, 1, 1, 1, 1, (41, 7, 1999), False),
    "tw_allo": (60, 4, 2, (17, 18, 2, 3), 0.03, 2, 1, 1, 0, 1, 1, (42, 8, 2000), True),
}
TW_CLI = ["-K", "2", "-L", "8", "-N", "60", "-p", "4", "-ap", "1", "-af", "1", "-u", "6", "-b", "3", "-t", "1", "-c", "1",
          "-v", "2", "-g", "1", "-r", "1", "-j", "1", "-lb", "0", "-a", "0", "-s", "13", "4", "1972", "-pi", "0", "-pf", "0"]


def panel(N, sizes, K, missing, seed):
    """Raw tetraploid alleles [N][L][4] (1-based labels, synth.MISSING for a missing locus) with exactly sizes[j] distinct alleles
    observed at locus j: K clusters (individual i in cluster i % K) with their own Dirichlet(1..1) allele frequencies, and the first
    individuals' copies cycling through all labels so that every allele occurs."""
    rng = np.random.default_rng(seed)
    L = len(sizes)
    raw = np.empty((N, L, 4), dtype=np.int32)
    for j, A in enumerate(sizes):
        f = rng.dirichlet(np.ones(A), size=K)
        for i in range(N):
            raw[i, j] = 1 + rng.choice(A, size=4, p=f[i % K])
        cover = np.arange(A) + 1
        ncov = (A + 3) // 4
        raw[:ncov, j] = np.resize(cover, 4 * ncov).reshape(ncov, 4)
        miss = rng.random(N) < missing
        miss[:ncov] = False
        raw[miss, j] = synth.MISSING
    return raw


def data_for(name):
    N, L, K, sizes, miss = CASES[name][:5]
    return panel(N, sizes, K, miss, 20261020 + sorted(CASES).index(name))


def dump_args(name, txt, out):
    N, L, K, sizes, miss, u, b, t, e, r, j, seeds, allo = CASES[name]
    return [txt, out] + [str(x) for x in (K, N, L, u, b, t, e, r, j) + tuple(seeds)] + (["0"] if allo else [])


def main():
    for name in sorted(CASES):
        txt = os.path.join(HERE, name + ".txt")
        synth.write_text_polyploid(txt, data_for(name))
        t0 = time.time()
        with open(os.devnull, "w") as devnull:
            subprocess.check_call([os.path.join(mg.REF, "ref_dump_poly")] + dump_args(name, txt, os.path.join(HERE, name + ".golden")), stdout=devnull)
        print(name, "%.1f s" % (time.time() - t0), os.path.getsize(os.path.join(HERE, name + ".golden")), "bytes")
    out = os.path.join(HERE, "tw_cli_output.txt")
    if os.path.exists(out):
        os.unlink(out)
    t0 = time.time()
    with open(os.devnull, "w") as devnull:
        subprocess.check_call([mg.CLI_REF, "-d", "tw_auto.txt", "-o", "tw_cli_output.txt"] + TW_CLI, stdout=devnull, cwd=HERE)
    print("tw_cli_output.txt", "%.1f s" % (time.time() - t0), os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
