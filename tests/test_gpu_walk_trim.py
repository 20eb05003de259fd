"""GPU (pytest -m gpu): the walk engine's tables evaluated over the columns a row can be entered at only (wk_trim_range,
instruct_amd/csrc/isg_walk.h; INSTRUCT_WALK_TRIM, on by default).  With the rows trimmed and with every column evaluated
(INSTRUCT_WALK_TRIM=0) the chain equals the canonical oracle after every iteration and takes the same paths to get there: the same sweeps
settle on the device, with the same probes and rounds -- no trimmed byte lies on a walk's way.  A spread far too small sends sweeps round
again or to the host loop, with the same values."""
import subprocess

import numpy as np
import pytest

import orc
from instruct_amd import capi, synth

pytestmark = pytest.mark.gpu
SEEDS = (13, 4, 1972)
ITER = 4


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
    """the oracle's state after each of ITER iterations: computed once per shape, compared against by every run"""
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


CASES = [
    # N, L, K, missing, alleles (None: synth.make_diploid)
    (300, 3000, 5, 0.02, 2),   # update_P: several blocks and super-blocks
    (40, 700, 4, 0.05, 4),     # update_P: rare alleles, shapes 1 (one uniform), 2, 3 .. mixed with large ones
    (600, 4000, 5, None, None),   # update_ZQ: the interval resolver settles the sweeps itself
    (250, 6000, 10, None, None),  # update_ZQ: K = 10 has no block resolver behind it
]


@pytest.mark.parametrize("case", CASES)
def test_trimmed_tables_give_the_oracles_chain_by_the_same_paths_as_untrimmed_ones(case, monkeypatch):
    monkeypatch.delenv("INSTRUCT_WALK_TRIM", raising=False)
    monkeypatch.delenv("INSTRUCT_WALK_TRIM_K", raising=False)
    pd1, zs1, fb1 = _run(case, "trim")
    monkeypatch.setenv("INSTRUCT_WALK_TRIM", "0")
    pd0, zs0, fb0 = _run(case, "every column")
    print(case, pd1, zs1)
    for key in ("device_sweeps", "host_sweeps", "retried", "failed_runs", "segments", "blocks", "table_bytes"):
        assert pd1[key] == pd0[key], (key, pd1, pd0)
    for key in ("tried", "settled", "lost", "probes", "rounds", "retried", "table_bytes", "segments"):
        assert zs1[key] == zs0[key], (key, zs1, zs0)
    assert pd1["device_sweeps"] == ITER and pd1["host_sweeps"] == 0, pd1
    assert fb1 == fb0
    if case[4] is None:   # the shapes of update_ZQ: settled by the interval resolver, nothing handed on
        assert fb1 == 0 and zs1["settled"] >= 2, zs1


def test_a_spread_far_too_small_sends_sweeps_round_again_with_the_same_values(monkeypatch):
    """Segments of 512 groups: the first block of each is entered at its only entry column, so with a fiftieth of sigma its rows keep
    the margin of 8 columns around the predicted drift and no more -- of 29 such blocks per sweep some are left for certain
    (tests/test_walk_trim.py: one block is enough there).  The sweep is tried again and then drawn by the host loop."""
    monkeypatch.setenv("INSTRUCT_WALK_TRIM_K", "0.02")
    monkeypatch.setenv("INSTRUCT_WALK_SEG", "512")
    pd, zs, fb = _run(CASES[0], "forced miss")
    print(pd, zs)
    assert pd["retried"] >= 1 or pd["host_sweeps"] >= 1, pd
    assert pd["failed_runs"] >= 1, pd


def test_tetraploid_chain_with_trimmed_tables_equals_the_oracle(tmp_path, monkeypatch):
    """ploidy 4 runs the same engine: the smallest generated case whose update_ZQ the interval resolver settles (tests/test_gpu_poly.py,
    x_spec), line by line against the canonical oracle, the sweeps taken by the device paths"""
    import test_gpu_poly as tp
    monkeypatch.delenv("INSTRUCT_WALK_TRIM", raising=False)
    monkeypatch.delenv("INSTRUCT_WALK_TRIM_K", raising=False)
    name = "x_spec"
    N, L, K, A, miss, u, b, t, e, r, j, seeds = tp.EXTRA[name]
    raw = tp.extra_data(name)
    txt, out = str(tmp_path / (name + ".txt")), str(tmp_path / (name + ".can"))
    synth.write_text_polyploid(txt, raw)
    args = [tp.DUMP, txt, out] + [str(x) for x in (K, N, L, u, b, t, e, r, j) + tuple(seeds)] + ["1", "1"]
    assert subprocess.call(args) == 0
    want = [l for l in tp.gu.parse(out) if l.startswith("it ") or l.startswith("chain zqinit")]
    got = tp.hip_lines(name, tp.EXTRA[name], raw, 0)
    assert len(got) == len(want) and len(got) == 1 + 6 * u
    for g, w in zip(got, want):
        assert tp._norm(g) == tp._norm(w)
    obs, alleleid, allelenum = synth.code_tetraploid(raw)
    ch = capi.HipPolyChain(obs, alleleid, allelenum, K)
    ch.setseeds(*seeds)
    ch.chain_init(np.array([np.float32(ch.ran1()) for _ in range(K)], dtype=np.float32))
    for _ in range(4):
        ch.iteration()
    zs, pd = ch.zq_spec_stats(), ch.p_device_stats()
    ch.close()
    assert zs["settled"] >= 3 and zs["lost"] == 0, zs
    assert pd["device_sweeps"] == 4 and pd["host_sweeps"] == 0, pd
