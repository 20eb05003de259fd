"""GPU (pytest -m gpu): the walk engine in three launches (k_wk_block, k_wk_compose2, k_wk_down; instruct_amd/csrc/isg_walk.h,
INSTRUCT_WALK_FUSED, on by default) and in the five it replaces (INSTRUCT_WALK_FUSED=0).  Either way the chain equals the canonical oracle
after every iteration, bit for bit, and takes the same paths to get there: the same sweeps settle on the device, in the same segments and
blocks, with the same probes and rounds -- also where windows are missed and a sweep goes round again."""
import subprocess

import numpy as np
import pytest

import orc
from instruct_amd import capi, synth

pytestmark = pytest.mark.gpu
SEEDS = (13, 4, 1972)
ITER = 4
SWITCHES = ("INSTRUCT_WALK_FUSED", "INSTRUCT_WALK_SEG", "INSTRUCT_ZQ_SPEC_SEG", "INSTRUCT_WALK_TRIM", "INSTRUCT_WALK_TRIM_K")


@pytest.fixture(scope="module", autouse=True)
def _libs():
    orc.build()
    capi.load()


def _data(case):
    N, L, K, miss, nall = case
    if nall is None:
        return synth.make_diploid(N, L, K)
    return synth.code_diploid(synth.raw_alleles(N, L, K, 2, nall, miss, 11))


def _state(c):
    return dict(z=c.z().copy(), qq=c.qq().copy(), qqnum=c.qqnum().copy(), freq=c.freq().copy(), seeds=c.seeds(), alpha=c.alpha(), totallkh=c.totallkh())


_ORACLE = {}


def _oracle(case):
    """the oracle's state after each of ITER iterations: computed once per data set, compared against by every run"""
    if case not in _ORACLE:
        geno, an, mi = _data(case)
        K = case[2]
        o = orc.OrcChain(geno, an, mi, K, math=orc.MATH_ISG, accum=orc.ACC_EXACT, sched=orc.SCHED_REPLAY)
        o.setseeds(*SEEDS)
        initd = np.array([np.float32(o.ran1()) for _ in range(K)], dtype=np.float32)
        o.chain_init(initd)
        states = []
        for _ in range(ITER):
            o.iteration()
            states.append(_state(o))
        _ORACLE[case] = (geno, an, mi, initd, states)
    return _ORACLE[case]


def _run(case, tag):
    """ITER iterations of a fresh chain (the switches are read when it is created), each compared with the oracle's; its statistics"""
    geno, an, mi, initd, states = _oracle(case)
    K = case[2]
    h = capi.HipChain(geno, an, mi, K, rng_sched=capi.SCHED_REPLAY)
    h.setseeds(*SEEDS)
    assert np.array_equal(np.array([np.float32(h.ran1()) for _ in range(K)], dtype=np.float32), initd)
    h.chain_init(initd)
    for it in range(ITER):
        h.iteration()
        got, want = _state(h), states[it]
        for name in ("z", "qq", "qqnum", "freq"):
            assert np.array_equal(got[name], want[name]), (case, tag, it, name)
        for name in ("seeds", "alpha", "totallkh"):
            assert got[name] == want[name], (case, tag, it, name)
    pd, zs, fb = h.p_device_stats(), h.zq_spec_stats(), h.zq_fallbacks()
    h.close()
    return pd, zs, fb


P_DATA = (300, 3000, 5, 0.02, 2)
ZQ_DATA = (600, 4000, 5, None, None)
ZQ_WIDE = (1100, 1500, 5, None, None)
SHAPES = {
    "update_P_two_segments": (P_DATA, {}),                                            # 13 super-blocks
    "update_P_segments_of_512": (P_DATA, {"INSTRUCT_WALK_SEG": "512"}),              # many segments of one super-block
    "update_ZQ_settled": (ZQ_DATA, {}),                                               # probe rounds and re-walks
    "update_ZQ_segments_of_256": (ZQ_DATA, {"INSTRUCT_ZQ_SPEC_SEG": "256"}),         # re-walks over several segments with kept origins
    "update_ZQ_two_super_blocks": (ZQ_WIDE, {}),
    "missed_windows": (P_DATA, {"INSTRUCT_WALK_TRIM_K": "0.02", "INSTRUCT_WALK_SEG": "512"}),   # missed windows and the retry
}
P_KEYS = ("device_sweeps", "host_sweeps", "retried", "failed_runs", "segments", "blocks", "table_bytes")
ZQ_KEYS = ("tried", "settled", "lost", "probes", "rounds", "retried", "table_bytes", "segments", "fail_bits", "lost_fail_bits")


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_three_launches_and_five_give_the_oracles_chain_by_the_same_paths(shape, monkeypatch):
    case, env = SHAPES[shape]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    pd1, zs1, fb1 = _run(case, "three launches")
    monkeypatch.setenv("INSTRUCT_WALK_FUSED", "0")
    pd0, zs0, fb0 = _run(case, "five launches")
    print(shape, pd1, zs1, fb1)
    for key in P_KEYS:
        assert pd1[key] == pd0[key], (key, pd1, pd0)
    for key in ZQ_KEYS:
        assert zs1[key] == zs0[key], (key, zs1, zs0)
    assert fb1 == fb0
    if shape == "missed_windows":
        assert pd1["retried"] >= 1 or pd1["host_sweeps"] >= 1, pd1
        assert pd1["failed_runs"] >= 1, pd1
    else:
        assert pd1["device_sweeps"] == ITER and pd1["host_sweeps"] == 0, pd1
    if shape == "update_P_two_segments":
        assert pd1["segments"] == 2, pd1
    if shape == "update_P_segments_of_512":
        assert pd1["segments"] > 10, pd1
    if case[4] is None:   # the shapes of update_ZQ: settled by the interval resolver, nothing handed on
        assert fb1 == 0 and zs1["settled"] >= 1, zs1
    if shape == "update_ZQ_segments_of_256":
        assert zs1["segments"] >= 3, zs1


def test_tetraploid_chain_takes_the_three_launches_and_equals_the_oracle(tmp_path, monkeypatch):
    """ploidy 4 runs the same engine: the generated case x_spec (tests/test_gpu_poly.py), whose update_ZQ the interval resolver settles, line
    by line against the canonical oracle by both routes, with the same statistics"""
    import test_gpu_poly as tp
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    name = "x_spec"
    N, L, K, A, miss, u, b, t, e, r, j, seeds = tp.EXTRA[name]
    raw = tp.extra_data(name)
    txt, out = str(tmp_path / (name + ".txt")), str(tmp_path / (name + ".can"))
    synth.write_text_polyploid(txt, raw)
    args = [tp.DUMP, txt, out] + [str(x) for x in (K, N, L, u, b, t, e, r, j) + tuple(seeds)] + ["1", "1"]
    assert subprocess.call(args) == 0
    want = [l for l in tp.gu.parse(out) if l.startswith("it ") or l.startswith("chain zqinit")]
    obs, alleleid, allelenum = synth.code_tetraploid(raw)
    stats = []
    for fused in ("1", "0"):
        monkeypatch.setenv("INSTRUCT_WALK_FUSED", fused)
        got = tp.hip_lines(name, tp.EXTRA[name], raw, 0)
        assert len(got) == len(want) and len(got) == 1 + 6 * u
        for g, w in zip(got, want):
            assert tp._norm(g) == tp._norm(w), (fused, g, w)
        ch = capi.HipPolyChain(obs, alleleid, allelenum, K)
        ch.setseeds(*seeds)
        ch.chain_init(np.array([np.float32(ch.ran1()) for _ in range(K)], dtype=np.float32))
        for _ in range(4):
            ch.iteration()
        stats.append((ch.zq_spec_stats(), ch.p_device_stats()))
        ch.close()
    (zs1, pd1), (zs0, pd0) = stats
    for key in ZQ_KEYS:
        assert zs1[key] == zs0[key], (key, zs1, zs0)
    for key in P_KEYS:
        assert pd1[key] == pd0[key], (key, pd1, pd0)
    assert zs1["settled"] >= 3 and zs1["lost"] == 0, zs1
    assert pd1["device_sweeps"] == 4 and pd1["host_sweeps"] == 0, pd1
