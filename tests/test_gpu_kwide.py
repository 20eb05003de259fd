"""GPU (pytest -m gpu): diploid chains with 33 to 64 clusters -- the K-generic wide kernels (DESIGN.md §4 "K up to 64") against the
canonical oracle, every sweep; the interval resolver at K > 32; the drop-in and the launcher against the reference program at K > 32."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import make_golden_kwide as mk
import orc
from instruct_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ["z", "qq", "qqnum", "generation", "alpha", "self_rates", "freq", "indvlkh", "totallkh"]


@pytest.fixture(scope="module", autouse=True)
def _libs():
    orc.build()
    capi.load()


def _pair(geno, an, mi, K, sched, mode=2, e=1):
    h = capi.HipChain(geno, an, mi, K, mode=mode, back_refl=e, rng_sched=sched)
    o = orc.OrcChain(geno, an, mi, K, mode=mode, back_refl=e, math=orc.MATH_ISG, accum=orc.ACC_EXACT, sched=sched)
    h.setseeds(13, 4, 1972)
    o.setseeds(13, 4, 1972)
    initd = np.array([h.ran1() for _ in range(K)], dtype=np.float32)
    assert np.array_equal(initd, np.array([o.ran1() for _ in range(K)], dtype=np.float32))
    h.chain_init(initd)
    o.chain_init(initd)
    return h, o


def _same(h, o, names, where):
    for n in names:
        a, b = getattr(h, n)(), getattr(o, n)()
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, np.asarray(b)), (where, n)
        else:
            assert a == b, (where, n, a, b)


def _sweeps(h, o, iters, sched):
    """mode 2 sweep by sweep (mcmc.c:208-235), every state array compared after each"""
    pos = ["seeds"] if sched == capi.SCHED_REPLAY else []
    _same(h, o, ["z", "qq", "qqnum", "generation", "alpha"] + pos, "init")
    o.lib.orc_iter_advance.argtypes = [C.c_void_p]
    h.lib.isg_iter_advance.argtypes = [C.c_void_p]
    for it in range(iters):
        h.update_P(); o.update_P()
        _same(h, o, ["count_alleles", "freq"] + pos, (it, "P"))
        h.update_S_POP(); o.update_S_POP()
        _same(h, o, ["self_rates", "state"] + pos, (it, "S"))
        h.update_G(); o.update_G()
        _same(h, o, ["generation"] + pos, (it, "G"))
        h.update_ZQ(0); o.update_ZQ(0)
        _same(h, o, ["z", "qq", "qqnum"] + pos, (it, "ZQ"))
        h.update_alpha(); o.update_alpha()
        _same(h, o, ["alpha"] + pos, (it, "A"))
        h.cal_lkh(); o.cal_lkh()
        _same(h, o, ["indvlkh", "totallkh"], (it, "L"))
        o.lib.orc_iter_advance(o.h)
        h.lib.isg_iter_advance(h.h)
    assert o.error() == 0


@pytest.mark.parametrize("K", [33, 40, 64])
def test_replay_default_path_every_sweep_and_the_interval_resolver_settles(K):
    geno, an, mi = synth.make_diploid(256, 2000, K)
    h, o = _pair(geno, an, mi, K, capi.SCHED_REPLAY)
    _sweeps(h, o, 3, capi.SCHED_REPLAY)
    st = h.zq_spec_stats()
    # the interval resolver runs at every K; at this small shape it settles K = 33's sweeps, at K = 40 and 64 (clusters of a few
    # copies per individual) it loses them to the chain kernels -- the state above is the oracle's either way
    assert st["tried"] >= 1 and h.zq_fallbacks() == 0, st
    if K == 33:
        assert st["settled"] >= 1 and st["lost"] == 0, st
    h.close()


@pytest.mark.parametrize("K", [33, 40, 64])
def test_keyed_schedule_every_sweep(K):
    geno, an, mi = synth.make_diploid(256, 2000, K)
    h, o = _pair(geno, an, mi, K, capi.SCHED_KEYED)
    _sweeps(h, o, 3, capi.SCHED_KEYED)
    h.close()


@pytest.mark.parametrize("mode,e", [(0, 1), (1, 1), (2, 0), (2, 1), (3, 1), (4, 1), (4, 0), (5, 1)])
def test_every_mode_at_K_40(mode, e):
    geno, an, mi = synth.code_diploid(synth.raw_alleles(60, 300, 40, 2, 3, 0.03, 41))
    h, o = _pair(geno, an, mi, 40, capi.SCHED_REPLAY, mode=mode, e=e)
    for it in range(3):
        h.iteration()
        o.iteration()
        _same(h, o, ALL + ["state", "seeds"], (mode, e, it))
    assert o.error() == 0
    h.close()


def test_forced_fallbacks_at_K_64(monkeypatch):
    """no interval resolver, no block resolver, no cooperative kernel: the single-workgroup chain form of the wide k_zq"""
    for k in ("INSTRUCT_ZQ_SPEC_RESOLVE", "INSTRUCT_ZQ_RESOLVE", "INSTRUCT_ZQ_COOP"):
        monkeypatch.setenv(k, "0")
    geno, an, mi = synth.make_diploid(96, 1200, 64)
    h, o = _pair(geno, an, mi, 64, capi.SCHED_REPLAY)
    for it in range(3):
        h.iteration()
        o.iteration()
        _same(h, o, ALL + ["seeds"], it)
    assert h.zq_spec_stats()["tried"] == 0
    h.close()


@pytest.mark.parametrize("sched", [capi.SCHED_REPLAY, capi.SCHED_KEYED])
def test_K_32_and_33_on_the_same_data(sched):
    """the last register-resident instance and the first wide one"""
    geno, an, mi = synth.make_diploid(128, 1500, 33)
    for K in (32, 33):
        h, o = _pair(geno, an, mi, K, sched)
        for it in range(3):
            h.iteration()
            o.iteration()
            _same(h, o, ALL + (["seeds"] if sched == capi.SCHED_REPLAY else []), (K, it))
        h.close()


def test_K_above_64_and_ploidy_4_above_32_are_refused():
    geno, an, mi = synth.make_diploid(20, 50, 3)
    with pytest.raises(RuntimeError, match=r"K must be in 1\.\.64 for ploidy 2"):
        capi.HipChain(geno, an, mi, 65)
    obs, alleleid, allelenum = synth.code_tetraploid(gu.make_golden.poly_data_for("t1"))
    with pytest.raises(RuntimeError, match=r"K must be in 1\.\.32 for ploidy 4"):
        capi.HipPolyChain(obs, alleleid, allelenum, 33)


def _body(path):
    return [l for l in open(path, "rb").read().split(b"\n")
            if not (l.strip().startswith((b"Data File:", b"Output File:")) or b"InStruct" in l and b"-d" in l)]


def test_dropin_cli_at_K_40_equals_reference_cli_output(tmp_path):
    exe = os.path.join(ROOT, "oracle", "_ref", "InStruct_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/InStruct_hip not built (needs the reference objects; built in the dev container)")
    out = tmp_path / "out.txt"
    log = subprocess.run([exe, "-d", os.path.join(gu.GOLDEN, "kwide_cli.txt"), "-o", str(out)] + mk.K40_CLI,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert log.returncode == 0 and b"THE JOB IS SUCCESSFULLY FINISHED" in log.stdout, log.stdout[-2000:]
    assert _body(str(out)) == _body(os.path.join(gu.GOLDEN, "k40_cli_output.txt"))


def test_launcher_k_scan_across_32_equals_reference(tmp_path):
    """-ik 1 -kv 32 33: one worker per K on the one GPU, K = 33 on the wide kernels"""
    exe = os.path.join(ROOT, "oracle", "_ref", "InStruct_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/InStruct_hip not built (needs the reference objects; built in the dev container)")
    from instruct_amd import build
    build.build_host()
    out = tmp_path / "k.txt"
    log = subprocess.run([mk.MGPU, "--exe", exe, "--gpus", "1", "--", "-d", os.path.join(gu.GOLDEN, "kwide_cli.txt"), "-o", str(out)] + mk.KSCAN_32_33_CLI,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert log.returncode == 0, log.stdout[-3000:]
    assert _body(str(out)) == _body(os.path.join(gu.GOLDEN, "kscan_32_33_output.txt"))
