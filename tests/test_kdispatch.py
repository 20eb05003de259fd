"""The run-time K -> compile-time KMAX dispatcher (instruct_amd/csrc/isg_kdispatch.h): every named ladder picks, for every K in 1 .. 64,
the kernel instance the launch sites have always picked -- the first rung >= K, the last rung for everything above it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "kdispatch_emul.cpp")

# the rungs, written out from the launch sites' tables (DESIGN.md "K up to 64": the dispatcher)
LADDERS = {
    "KL_ZQ": [2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 64],
    "KL_ZQ_COOP": [2, 3, 4, 5, 6, 8, 12, 16, 24, 32],
    "KL_ZQ_8": [2, 3, 4, 5, 6, 8],
    "KL_ZQ_EXACT": [2, 3, 4, 5, 6, 7, 8],
    "KL_P4": [2, 4, 6, 8, 12, 16, 24, 32],
    "KL_P4_BLOCK": [2, 4, 6, 8, 12, 16],
    "KL_P4_GENO": [4, 8, 12, 16, 32],
}


def expected(rungs, K):
    for r in rungs:
        if K <= r:
            return r
    return rungs[-1]


@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kdispatch") / "kdispatch_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe, SRC])
    rows = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        f = line.split()
        rows[f[0]] = [int(x) for x in f[1:]]
    return rows


def test_every_ladder_is_printed(chosen):
    assert sorted(chosen) == sorted(LADDERS)
    assert all(len(v) == 64 for v in chosen.values())


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_first_rung_not_below_K_and_last_rung_catches_all(chosen, name):
    assert chosen[name] == [expected(LADDERS[name], K) for K in range(1, 65)]


def test_spot_values(chosen):
    """the cases that tell the ladders apart"""
    at = lambda name, K: chosen[name][K - 1]
    assert at("KL_ZQ", 1) == 2 and at("KL_ZQ", 7) == 8 and at("KL_ZQ", 9) == 12 and at("KL_ZQ", 32) == 32 and at("KL_ZQ", 33) == 64 and at("KL_ZQ", 64) == 64
    assert at("KL_ZQ_COOP", 7) == 8 and at("KL_ZQ_COOP", 25) == 32 and at("KL_ZQ_COOP", 33) == 32
    assert at("KL_ZQ_8", 7) == 8 and at("KL_ZQ_8", 9) == 8 and at("KL_ZQ_8", 64) == 8
    assert at("KL_ZQ_EXACT", 1) == 2 and at("KL_ZQ_EXACT", 7) == 7 and at("KL_ZQ_EXACT", 9) == 8
    assert at("KL_P4", 3) == 4 and at("KL_P4", 5) == 6 and at("KL_P4", 20) == 24 and at("KL_P4", 33) == 32
    assert at("KL_P4_BLOCK", 9) == 12 and at("KL_P4_BLOCK", 20) == 16
    assert at("KL_P4_GENO", 1) == 4 and at("KL_P4_GENO", 5) == 8 and at("KL_P4_GENO", 17) == 32
