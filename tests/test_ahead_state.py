"""The launch-ahead bookkeeping of the replay iteration (instruct_amd/csrc/isg_ahead.h), compiled on the host: every invalidation rule
clears exactly the items that read what was written, nothing sets an item but ahead_set, the likelihood total lives and dies with its
sweep, only the counts cross an iteration boundary, and settling is idempotent."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "ahead_emul.cpp")

FREQF, EXPECT, LKH, TOTAL, COUNTS = 1, 2, 4, 8, 16
ALL = 31
# what each ahead result reads: freqf <- freq; the ZQ prologue <- qq, freqf (freq), alpha; the likelihood sweep <- Z, qq, generations, tables
# (freq); its total <- the sweep; the counts <- Z
CLEARS = {
    "wrote_z": COUNTS | LKH | TOTAL,
    "wrote_freq": FREQF | EXPECT | LKH | TOTAL,
    "wrote_qq": EXPECT | LKH | TOTAL,
    "wrote_gen": LKH | TOTAL,
    "wrote_alpha": EXPECT,
    "chain_init": ALL,
    "end_iteration": ALL & ~COUNTS,
}


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ahead") / "ahead_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    rows = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        f = line.split()
        rows[f[0]] = [int(x) for x in f[1:]] if all(x.isdigit() for x in f[1:]) else f[1:]
    return rows


def test_bits_are_distinct(out):
    assert out["BITS"] == [FREQF, EXPECT, LKH, TOTAL, COUNTS, ALL, 4]


@pytest.mark.parametrize("rule", sorted(CLEARS))
def test_rule_clears_exactly_its_items(out, rule):
    # from everything: exactly the rule's items go, and the pending look (alpha's, bit 3) stays
    assert out["all_" + rule] == [ALL & ~CLEARS[rule], 1 << 3]
    for b in (FREQF, EXPECT, LKH, TOTAL, COUNTS):
        start = LKH | TOTAL if b == TOTAL else b
        assert out["one_%d_%s" % (b, rule)] == [start & ~CLEARS[rule], 0], (b, rule)
    assert out["none_" + rule] == [0, 0]  # a rule sets nothing


def test_a_z_write_spares_freqf_and_the_prologue(out):
    assert out["all_wrote_z"][0] == FREQF | EXPECT


def test_only_the_counts_cross_an_iteration(out):
    assert out["all_end_iteration"][0] == COUNTS


def test_total_goes_with_its_sweep(out):
    assert out["init"] == [0, 0]
    assert out["total_without_sweep"] == [0, 0]
    assert out["sweep_then_total"] == [LKH | TOTAL, 0]
    assert out["take_total"] == [1] and out["after_take_total"] == [LKH, 0]
    assert out["take_sweep"] == [1] and out["after_take_sweep"] == [0, 0]
    assert out["take_again"] == [0]  # an item is used once
    for rule, clears in CLEARS.items():
        if clears & LKH:
            assert clears & TOTAL, rule


def test_has_and_unknown_bits(out):
    assert out["has_counts"] == ["1", "has_both", "1", "has_expect", "0"]
    assert out["unknown_bit"] == [COUNTS | FREQF, 0]


def test_settle_is_idempotent(out):
    assert out["two_looks"][1] == (1 << 0) | (1 << 2)
    assert out["one_waited"][1] == 1 << 2
    assert out["settle"] == [(1 << 2) | (1 << 1)]
    assert out["settled"][1] == 0
    assert out["settle_again"] == [0]
    assert out["settled_again"] == out["settled"]  # the items are not touched by settling
