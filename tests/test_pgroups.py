"""The group list of replay update_P on the walk engine (instruct_amd/csrc/isg_pgroups.h) against the order of the reference's loops, written
out again here in numpy: update_P_allo (poly_geno.c:491-502) draws, for every cluster and every locus, the first subgenome's Dirichlet
(counts seqpop -> freq) and then the second's (seqpop2 -> freq2); update_P_auto (:426-434) one Dirichlet per (cluster, locus); neither tests
allelenum > 1, the diploid update_P (mcmc.c:846-857) does.  The panel has 0-, 1- and many-allele loci."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "pgroups_emul.cpp")
STRIDE = 3000   # cnt2 = cnt + STRIDE (a multiple of every K used here, at least L * Amax * K)
PANEL = [4, 1, 0, 9, 2, 1, 24, 0, 3, 5, 1, 2]
AMAX = 24
NGMAX = 64


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgroups") / "pgroups_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-o", out, SRC])
    return out


def run(exe, K, Amax, min_alleles, sub, ngmax, panel, stride=STRIDE):
    lines = subprocess.check_output([exe] + [str(x) for x in [K, Amax, min_alleles, sub, stride, ngmax] + list(panel)], text=True).splitlines()
    if lines[0] != "OK 1":
        assert lines == ["OK 0"]
        return None
    G, NG = (int(x) for x in lines[1].split())
    rows = np.array([[int(x) for x in l.split()] for l in lines[2:2 + G]]).reshape(G, 4)
    assert np.array_equal(rows[:, 0], np.arange(G))
    gidx = np.array(lines[2 + G].split(), dtype=np.int64)
    assert len(gidx) == NG
    return rows[:, 1], rows[:, 2], rows[:, 3], gidx


def expected(K, Amax, min_alleles, sub, panel):
    """the reference's loop nest: cluster, locus, subgenome, allele; a count lives at [locus][allele][cluster] of cnt (subgenome 0) or of cnt2 =
    cnt + STRIDE; returns group starts, sizes, subgenomes, and every gamma's index into its own array and its subgenome"""
    panel = np.asarray(panel)
    L = len(panel)
    kk, jj, ss = np.meshgrid(np.arange(K), np.arange(L), np.arange(sub), indexing="ij")
    keep = panel[jj] > min_alleles
    kk, jj, ss = kk[keep], jj[keep], ss[keep]          # C order of the mesh = the nest's order
    n = panel[jj]
    start = np.concatenate([[0], np.cumsum(n)[:-1]]) if len(n) else np.zeros(0, dtype=np.int64)
    gk, gj, gs = np.repeat(kk, n), np.repeat(jj, n), np.repeat(ss, n)
    a = np.arange(int(n.sum())) - np.repeat(start, n)
    return start, n, ss, (gj * Amax + a) * K + gk, gs


@pytest.mark.parametrize("K", [1, 3])
def test_allotetraploid_groups_are_the_reference_stream_order(exe, K):
    start, n, sub, gidx = run(exe, K, AMAX, 0, 2, NGMAX, PANEL)
    w_start, w_n, w_sub, w_gidx, w_gsub = expected(K, AMAX, 0, 2, PANEL)
    assert STRIDE % K == 0 and STRIDE >= len(PANEL) * AMAX * K
    used = sum(1 for x in PANEL if x > 0)
    assert len(start) == 2 * K * used and len(gidx) == 2 * K * sum(PANEL)   # 2 K sum(A) gammas; a one-allele locus is a group of one
    assert np.array_equal(start, w_start) and np.array_equal(n, w_n) and np.array_equal(sub, w_sub)
    assert np.array_equal(gidx, w_gidx + STRIDE * w_gsub)
    # what k_pd_gather / k_pdirich_at make of an index: row = gidx // K of [2][L][Amax] rows, cluster = gidx % K
    assert np.array_equal(gidx % K, w_gidx % K) and np.array_equal(gidx // K, w_gidx // K + (STRIDE // K) * w_gsub)
    assert (n == 1).sum() == 2 * K * PANEL.count(1) and sub[0] == 0 and sub[1] == 1
    # the two Dirichlets of one (cluster, locus) read the same indices, of cnt and of cnt2
    g0, g1 = start[0::2], start[1::2]
    for a, b, m in zip(g0, g1, n[0::2]):
        assert np.array_equal(gidx[a:a + m] + STRIDE, gidx[b:b + m])


@pytest.mark.parametrize("min_alleles", [0, 1])
def test_one_subgenome_keeps_the_order_it_had(exe, min_alleles):
    """the autotetraploid (min_alleles = 0) and diploid (1) lists: one group per (cluster, used locus), every index into cnt itself"""
    start, n, sub, gidx = run(exe, 3, AMAX, min_alleles, 1, NGMAX, PANEL)
    w_start, w_n, w_sub, w_gidx, _ = expected(3, AMAX, min_alleles, 1, PANEL)
    assert np.array_equal(start, w_start) and np.array_equal(n, w_n) and not sub.any()
    assert np.array_equal(gidx, w_gidx)
    assert n.min() == min_alleles + 1


def test_a_locus_wider_than_a_group_refuses_the_list(exe):
    assert run(exe, 2, AMAX, 0, 2, 23, PANEL) is None
    assert run(exe, 2, AMAX, 0, 2, 24, PANEL) is not None
    # every index has to fit an int: L * Amax * K + sub_stride < 2^31 with two subgenomes
    assert run(exe, 1 << 15, 1 << 15, 0, 2, NGMAX, [1], stride=1 << 30) is None
    assert run(exe, 1 << 15, 1 << 15, 0, 1, NGMAX, [1], stride=1 << 30) is not None
