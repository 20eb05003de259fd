"""The tiling, padding and lane maps of the posterior co-ancestry flush (instruct_amd/csrc/isg_coanc.h), run on the host: the
workgroup decode visits every tile pair of the lower triangle once, the paddings are the stated roundings, and the kernel's walk
through the f64 matrix instruction's documented lane maps reproduces the plain loops (tests/emul/coanc_emul.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "coanc_emul.cpp")
NS = list(range(1, 301)) + [10000]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coanc") / "coanc_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe, SRC])
    rows = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        f = line.split()
        rows.setdefault(f[0], []).append(tuple(int(x) for x in f[1:]))
    return rows


def test_tile_constants(emul):
    (tile, sub, kstep, nsub), = emul["TILE"]
    assert sub == 16 and kstep == 4  # the 16 x 16 x 4 instruction
    assert tile % sub == 0 and nsub == tile // sub and nsub >= 2  # at least two independent accumulators per wave


def test_decode_visits_every_lower_tile_pair_once(emul):
    (tile, _, _, _), = emul["TILE"]
    got = {r[0]: r[1:] for r in emul["DECODE"]}
    assert sorted(got) == NS
    for n in NS:
        T = (n + tile - 1) // tile
        assert got[n] == (T, T * (T + 1) // 2, 0), n


def test_paddings(emul):
    (tile, _, _, _), = emul["TILE"]
    assert emul["PAD"] == [(k, (k + 3) // 4 * 4) for k in range(1, 65)]
    assert emul["NP"] == [(n, (n + tile - 1) // tile * tile, (n + tile - 1) // tile) for n in NS]


def test_lane_maps_reproduce_the_triple_loop(emul):
    assert emul["MFMA"] == [(0,)]


def test_emulated_syrk_over_three_tiles_equals_the_plain_loop(emul):
    (tile, _, _, _), = emul["TILE"]
    assert len(emul["SYRK"]) >= 1
    for n, k, nb, bad in emul["SYRK"]:
        assert (n + tile - 1) // tile == 3 and nb == 2 and bad == 0, (n, k, nb, bad)
