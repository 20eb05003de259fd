"""The granule layout of the cooperative update_ZQ kernels (instruct_amd/csrc/isg_coop_layout.h): for every K in 1 .. 32, G in
{1, 2, 3, 11, 32, 128}, 2 and 4 allele copies and 1, 3 and 8 passes over the loci, coop_layout gives the values the kernels
computed for themselves before it existed -- the formulas are written out again here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "coop_layout_emul.cpp")
BLOCK = 256
GS = [1, 2, 3, 11, 32, 128]
PASSES = [1, 3, 8]


def expected(copies, G, K, Lp):
    wmode = G * (BLOCK // 64) * ((K + 2) // 3) <= BLOCK
    npass = (Lp + G * BLOCK - 1) // (G * BLOCK)
    pack = 4 if (not wmode and copies * BLOCK * npass < 4096) else 3
    bits = 12 if pack == 4 else 16
    W = (K + pack - 1) // pack
    ngran = G * (BLOCK // 64) * W if wmode else G * W
    return (int(wmode), pack, bits, W, ngran)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coop_layout") / "coop_layout_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe, SRC])
    rows, limits = {}, None
    for line in subprocess.check_output([exe], text=True).splitlines():
        f = line.split()
        if f[0] == "LIMITS":
            limits = tuple(int(x) for x in f[1:])
        else:
            v = [int(x) for x in f]
            rows[tuple(v[:4])] = tuple(v[4:])
    return rows, limits


def cases():
    for copies in (2, 4):
        for G in GS:
            for npass in PASSES:
                for Lp in (npass * G * BLOCK, (npass - 1) * G * BLOCK + 1):
                    for K in range(1, 33):
                        yield copies, G, K, Lp, npass


def test_every_case_is_printed(emul):
    rows, limits = emul
    assert sorted(rows) == sorted(set(c[:4] for c in cases()))
    assert limits == (4, 128, 11)


@pytest.mark.parametrize("copies", [2, 4])
def test_layout_is_the_kernels_own_formula(emul, copies):
    rows, _ = emul
    n = 0
    for cp, G, K, Lp, npass in cases():
        if cp != copies:
            continue
        assert (Lp + G * BLOCK - 1) // (G * BLOCK) == npass
        assert rows[(cp, G, K, Lp)] == expected(cp, G, K, Lp), (cp, G, K, Lp)
        n += 1
    assert n == len(GS) * len(PASSES) * 2 * 32


def test_both_sides_of_the_12_bit_edge(emul):
    """copies * BLOCK * npass < 4096: 2 copies pack 4 x 12 bits up to 7 passes, 4 copies up to 3"""
    rows, _ = emul
    at = lambda cp, G, K, npass: rows[(cp, G, K, npass * G * BLOCK)]
    assert at(2, 128, 9, 1)[1:3] == (4, 12) and at(2, 128, 9, 3)[1:3] == (4, 12) and at(2, 128, 9, 8)[1:3] == (3, 16)
    assert at(4, 128, 9, 1)[1:3] == (4, 12) and at(4, 128, 9, 3)[1:3] == (4, 12) and at(4, 128, 9, 8)[1:3] == (3, 16)
    assert at(4, 32, 32, 8)[1:3] == (3, 16) and at(2, 32, 32, 3)[1:3] == (4, 12)
    # few workgroups: the wave form is always 3 x 16 bits
    assert at(2, 3, 5, 1) == (1, 3, 16, 2, 3 * 4 * 2) and at(4, 11, 9, 1) == (1, 3, 16, 3, 11 * 4 * 3) and at(2, 11, 32, 1)[0] == 0


def test_granules_fit_the_exchange_buffer(emul):
    """every case (the host launches G <= ISG_COOP_GMAX workgroups and K <= 32): W words per publisher and all of an
    individual's granules stay inside CoopBuf.gran[slot]"""
    rows, (ring, gmax, wmax) = emul
    for (cp, G, K, Lp), (wmode, pack, bits, W, ngran) in rows.items():
        assert G <= gmax and W <= wmax and ngran <= gmax * wmax, (cp, G, K, Lp)
        assert pack * bits == 48 and pack * W >= K  # the tag has the upper 16 bits; every cluster has a field
        if not wmode:  # a workgroup's count of one cluster fits its field
            npass = (Lp + G * BLOCK - 1) // (G * BLOCK)
            assert cp * BLOCK * npass < (1 << bits), (cp, G, K, Lp)
