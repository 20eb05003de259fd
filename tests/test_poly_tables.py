"""The per-row genotype-frequency tables of ploidy 4 (instruct_amd/csrc/isg_poly_tables.h) on the CPU: tests/emul/poly_tables_emul.cpp
runs, for every allele count 1..32, both tetraploid variants, the selfing rates 0, 0.05, 0.5, 0.95 and 1 and both instances of the header
(canonical math and glibc), the whole-row functions against the per-row ones in the order the wide kernels call them, and prints the counts
asserted here.  Floats and the err word are compared as bit patterns, without a tolerance.  An allotetraploid table of n alleles costs about
50 n^4 exponentials (n^2 iikk rows of n^2 terms, 5 rates, 2 instances, 5 passes), 350 million up to 32 alleles, so the allele counts are
run as four ranges of equal cost side by side.  The program is also built with the address and undefined-behaviour sanitizers and run on
its own; that build is about twice as slow and runs 1..20 alleles (a tenth of the work), which covers every branch on n and class sizes on
both sides of the 256 lanes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "poly_tables_emul.cpp")
CSRC = os.path.join(ROOT, "instruct_amd", "csrc")
RATES, INSTANCES = 5, 2


RANGES = [(1, 24), (25, 28), (29, 30), (31, 32)]   # sums of n^4 within 15 % of each other


def _build_and_run(tmp, name, extra, ranges):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function"] + extra + ["-o", exe, SRC])
    procs = [subprocess.Popen([exe, str(a), str(b)], stdout=subprocess.PIPE, text=True) for a, b in ranges]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0] * len(procs)
    return "".join(outs)


def auto_G(n):
    return n + n * (n - 1) * 3 // 2 + n * (n - 1) * (n - 2) // 2 + n * (n - 1) * (n - 2) * (n - 3) // 24


def allo_G(n):
    return n * n + n * (n - 1) * n + (n * (n - 1) // 2) ** 2


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("poly_tables")


@pytest.fixture(scope="module")
def emul(tmp):
    text = _build_and_run(tmp, "poly_tables_emul", [], RANGES)
    rows = {}
    for line in text.splitlines():
        f = line.split()
        rows.setdefault(f[0], {})[(f[1], int(f[2]))] = [int(x) for x in f[3:]]
    return text, rows


def test_sanitizer_build_runs_clean_and_prints_the_same(emul, tmp):
    """the stand-alone program under -fsanitize=address,undefined, 1..20 alleles: no report (either would end it with a non-zero status),
    the same lines"""
    text = _build_and_run(tmp, "poly_tables_emul_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [(1, 16), (17, 20)])
    want = [l for l in emul[0].splitlines() if int(l.split()[2]) <= 20]
    assert len(want) == 2 * (2 * 20 + 1 + 6) and sorted(text.splitlines()) == sorted(want)


@pytest.mark.parametrize("variant", ["auto", "allo"])
def test_exfreq_row_is_the_row_function_in_any_order(emul, variant):
    for n in range(1, 33):
        G, rows, bad = emul[1]["EX"][(variant, n)]
        assert G == (auto_G(n) if variant == "auto" else allo_G(n))
        assert rows == INSTANCES * G and bad == 0, n


@pytest.mark.parametrize("variant", ["auto", "allo"])
def test_wide_kernel_schedule_equals_genfreq_row_whatever_the_unsolved_rows_hold(emul, variant):
    """lanes ascending and descending, the rows of the class at hand and of all later classes set to 0.0f and to a quiet NaN before each
    class: 4 runs per rate and instance, all equal to genfreq_row -- so no row function reads a row that is not solved yet"""
    odd_total = 0
    for n in range(1, 33):
        G, runs, bad, odd = emul[1]["GEN"][(variant, n)]
        assert runs == INSTANCES * RATES * 4 and bad == 0, n
        odd_total += odd
    assert odd_total > 0   # selfing rate 1 (and 0 frequencies' logs) do give -inf / NaN rows, compared like the others
    # the comparison can fail: with two classes swapped every poisoned run differs from genfreq_row
    assert emul[1]["NEG"][(variant, 5)] == [INSTANCES * 2]


@pytest.mark.parametrize("variant", ["auto", "allo"])
def test_row_functions_read_earlier_classes_only(emul, variant):
    """n <= 6: every row found through isg_poly_rank / isg_allo_row_any lies in [end of the class being solved, G)"""
    for n in range(1, 7):
        reads, bad = emul[1]["READS"][(variant, n)]
        assert bad == 0 and (reads > 0 or n == 1), n
    assert sorted(k[1] for k in emul[1]["READS"] if k[0] == variant) == list(range(1, 7))


def test_sources_state_the_table_arithmetic_once():
    """each table expression occurs in isg_poly_tables.h only, and there once: the kernels' second copy stays gone"""
    texts = {f: open(os.path.join(CSRC, f), errors="replace").read() for f in os.listdir(CSRC)}
    for word in ("10.0 / 36.0", "8.0 / 36.0", "isg_poly_gaussj3(matr", "/ 16.0"):
        assert {f: t.count(word) for f, t in texts.items() if word in t} == {"isg_poly_tables.h": 1}, word
