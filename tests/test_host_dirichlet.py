"""The host side of replay update_P (instruct_amd/csrc/isg_host_dirichlet.h) on the CPU: tests/emul/host_dirichlet_emul.cpp runs the
sampler, the pass over all Dirichlets of a sweep, the uniform tape and the layout helpers and prints what is asserted here.  Doubles and
generator states are compared bit for bit, without a tolerance.  The program is also built with the address and undefined-behaviour
sanitizers and run on its own."""
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "host_dirichlet_emul.cpp")
CSRC = os.path.join(ROOT, "instruct_amd", "csrc")
HEADER = "isg_host_dirichlet.h"


def _build_and_run(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-pthread"] + extra + ["-o", exe, SRC])
    return subprocess.check_output([exe], text=True)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("host_dirichlet")


@pytest.fixture(scope="module")
def emul(tmp):
    text = _build_and_run(tmp, "host_dirichlet_emul", [])
    rows = {}
    for line in text.splitlines():
        f = line.split()
        rows.setdefault(f[0], []).append(f[1:])
    return text, rows


def test_sanitizer_build_runs_clean_and_prints_the_same(emul, tmp):
    """the stand-alone program under -fsanitize=address,undefined: no report (either would end it with a non-zero status), same lines"""
    text = _build_and_run(tmp, "host_dirichlet_emul_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert text == emul[0]


def test_rdirich_pre_equals_isg_rdirich(emul):
    """at least 20 000 Dirichlets of 2 .. 32 components, counts from 0..3, 0..59 and 0..19999: the same doubles, the same end state of the
    generator and the same number of uniforms as isg_rdirich(..., add = 1.0) -- every one of them"""
    (total, equal, one, low, high), = [[int(x) for x in r] for r in emul[1]["RDIRICH"]]
    assert total >= 20000 and equal == total
    assert one > 1000 and low > 1000 and high > 100000   # shape 1 (rexp), shapes either side of 2.5


def test_whole_pass_equals_the_reference_loop(emul):
    rows = {r[0]: [int(x) for x in r[1:]] for r in emul[1]["PASS"]}
    assert sorted(rows) == ["skip_off", "skip_on", "two_subgenomes", "two_subgenomes_large"]
    for name, (ngamma, formula, used, same_out, same_state) in rows.items():
        assert ngamma == formula and same_out == 1 and same_state == 1, name
        assert used >= ngamma   # every gamma takes a uniform at least
    # K = 3, L = 9, loci 1 and 5 with one allele: passed over without consuming anything, or one gamma each
    assert rows["skip_off"][0] == rows["skip_on"][0] + 3 * 2
    assert rows["skip_off"][2] != rows["skip_on"][2]


def test_tape_of_every_length_gives_the_same_draws(emul):
    """the run-out path: the loop leaves the tape while 64 uniforms per gamma plus 64 remain and goes on with the generator"""
    (used, lengths, equal, never, midway, to_end), = [[int(x) for x in r] for r in emul[1]["TAPE"]]
    assert lengths == used + 64 * 5 + 64 + 8 + 1 and equal == lengths
    assert never > 0 and midway > 1000 and to_end > 0
    need = {(int(n), int(en)): int(v) for n, en, v in emul[1]["NEED"]}
    assert need == {(0, 0): 0, (0, 1): 0, (4095, 0): 0, (4095, 1): 0, (4096, 0): 0, (4096, 1): 3 * 4096 + 65536, (100000, 0): 0, (100000, 1): 365536}


def _layout(emul, name):
    out = []
    for r in emul[1]["LAYOUT"]:
        if r[0] == name:
            colon = r.index(":")
            out.append(([int(x) for x in r[1:colon]], np.array([int(x) for x in r[colon + 1:]], dtype=np.int64)))
    return out


def test_frequency_layouts(emul):
    seen = []
    for (K, L, A, KP, Lp, inverse), dev in _layout(emul, "freq_to_device"):
        ref = 100 + np.arange(K * L * A)
        want = np.full(Lp * A * KP, -1)
        for k in range(K):
            for j in range(L):
                for a in range(A):
                    want[(j * A + a) * KP + k] = ref[(k * L + j) * A + a]
        assert inverse == 1 and np.array_equal(dev, want), (K, L, A, KP)
        seen.append((K, A, KP > K, Lp > L))
    for (K, L, A, KP, Lp, inverse), ref in _layout(emul, "freq_from_device"):
        dev = 500 + np.arange(Lp * A * KP)
        want = np.array([dev[(j * A + a) * KP + k] for k in range(K) for j in range(L) for a in range(A)])
        assert inverse == 1 and np.array_equal(ref, want), (K, L, A, KP)
    assert any(k % 4 and pad and lp for k, a, pad, lp in seen) and {a for _, a, _, _ in seen} == {2, 5}


def test_count_layouts(emul):
    ones, boths = _layout(emul, "counts_one"), _layout(emul, "counts_both")
    assert len(ones) == len(boths) == 4
    for ((K, L, A), one), (_, both) in zip(ones, boths):
        c1, c2 = 10 + np.arange(L * A * K), 7000 + 3 * np.arange(L * A * K)
        idx = np.array([(j * A + a) * K + k for k in range(K) for j in range(L) for a in range(A)])
        assert np.array_equal(one, c1[idx]) and np.array_equal(both, c1[idx] + c2[idx]), (K, L, A)


def test_byte_rows_to_ints(emul):
    ins, outs = _layout(emul, "bytes_in"), _layout(emul, "bytes_out")
    assert [d[3] for d, _ in ins] == [2, 4]
    for ((N, L, Lp, C), rows), (_, out) in zip(ins, outs):
        assert Lp > L and (rows == 255).any() and (rows != 255).any()
        want = [(-1 if rows[(i * Lp + j) * C + k] == 255 else rows[(i * Lp + j) * C + k]) for i in range(N) for j in range(L) for k in range(C)]
        assert np.array_equal(out, np.array(want)), C


def test_sources_keep_one_copy_of_the_host_loop():
    """the second copy of the accept test and the hand-written transpositions stay gone"""
    for path in glob.glob(os.path.join(CSRC, "*")):
        text = open(path, errors="replace").read()
        for word in ("host_rdirich(", "host_rgamma2_try(", "(HostGammaCoef *)", "qq_dirty_host"):
            assert word not in text, (word, path)
        if os.path.basename(path) != HEADER:
            assert "freq_stage[" not in text, path
    header = open(os.path.join(CSRC, HEADER)).read()
    includes = [l.split()[1] for l in header.splitlines() if l.startswith("#include")]
    assert [i for i in includes if i.startswith('"')] == ['"isg_math.h"', '"isg_wh.h"', '"isg_sampler.h"']
    assert all("hip" not in i for i in includes)
