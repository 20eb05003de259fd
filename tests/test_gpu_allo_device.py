"""GPU: the allotetraploid chain (-p 4 -ap 0) in the replay schedule with update_P_allo on the walk engine (two Dirichlets per (cluster, locus),
the second subgenome's counts and frequencies behind the first's) and the genotype draw's single precision pre-decision (geno_one_allo).  Every case: every dump line -- hz, hgeno,
hcnt, hfreq, hfreq2, the tables, the seeds after every sweep -- equal to the canonical oracle's (oracle/orc_dump_poly ... 1 1 0 1), and
isg_p_device_stats says which path drew the sweeps."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import orc
import test_gpu_poly as tp
import test_gpu_poly_alleles as tpa

pytestmark = pytest.mark.gpu
DUMP = tp.DUMP
ALLO, ALLO_EXTRA = tp.ALLO, tp.ALLO_EXTRA

# the pre-decision over many draws: N=200, L=600, K=4, 6 alleles, 10 % missing -- 200 x 540 loci x 12 iterations, nearly all of them with 2, 3 or 4
# observed alleles (7, 12, 6 candidates): about 1.2 million genotype draws; the oracle takes 12 s for it on one CPU core.  "conv": the same chain on
# data of two clusters, 40 iterations (the oracle: 35 s); "conv2": that data with K=2.  The three oracle runs are started with the module's
# first test and waited for by its last ones.  name: (cfg, clusters the data is drawn from)
BIG = {
    "big": ((200, 600, 4, 6, 0.10, 12, 1, 1, 1, 1, 1, (41, 9, 2011)), 4),
    "conv": ((200, 600, 4, 6, 0.10, 40, 1, 1, 1, 1, 1, (41, 9, 2011)), 2),
    "conv2": ((200, 600, 2, 6, 0.10, 40, 1, 1, 1, 1, 1, (41, 9, 2011)), 2),
}
SHAPES = (40, 400, 3, tuple((1, 2, 5, 9)[j % 4] for j in range(400)), 0.20, 3, 1, 1, 1, 1, 1, (43, 11, 2013))


def big_data(tag):
    from instruct_amd import synth
    cfg, clusters = BIG[tag]
    return synth.raw_alleles(cfg[0], cfg[1], clusters, 4, cfg[3], cfg[4], 20261101)


@pytest.fixture(scope="module", autouse=True)
def _build():
    orc.build()


@pytest.fixture(scope="module", autouse=True)
def big_oracle(tmp_path_factory, _build):
    """the two long oracle runs, started with the module's first test and collected by its last ones"""
    from instruct_amd import synth
    d = tmp_path_factory.mktemp("allo_big")
    procs = {}
    for tag, (cfg, _) in BIG.items():
        txt, out = str(d / (tag + ".txt")), str(d / (tag + ".can"))
        synth.write_text_polyploid(txt, big_data(tag))
        N, L, K, A, miss, u, b, t, e, r, j, seeds = cfg
        args = [DUMP, txt, out] + [str(x) for x in (K, N, L, u, b, t, e, r, j) + tuple(seeds)] + ["1", "1", "0", "1"]
        procs[tag] = (subprocess.Popen(args, stdout=subprocess.DEVNULL), out)
    yield procs
    for p, _ in procs.values():
        if p.poll() is None:
            p.kill()
            p.wait()


@pytest.fixture(scope="module")
def oracle(tmp_path_factory, _build):
    """name -> (cfg, raw, the canonical oracle's lines), computed once per data set"""
    from instruct_amd import synth
    d = tmp_path_factory.mktemp("allo_dev")
    cache = {}

    def get(name):
        if name not in cache:
            if name in ALLO:
                cfg, raw = ALLO[name], gu.make_golden.allo_data_for(name)
            elif name in ALLO_EXTRA:
                cfg = ALLO_EXTRA[name]
                raw = synth.raw_alleles(cfg[0], cfg[1], cfg[2], 4, cfg[3], cfg[4], 20260401 + sorted(ALLO_EXTRA).index(name))
            elif name == "shapes":   # loci of 1, 2, 5 and 9 alleles in one panel: groups of one gamma, many zero counts (shape exactly 1)
                cfg, raw = SHAPES, tpa.mga.panel(SHAPES[0], SHAPES[3], SHAPES[2], SHAPES[4], 20261102)
            elif name == "k9_on_three":   # the xa_a3k9 shape with data of three clusters: two thirds of the counts are zero
                cfg = ALLO_EXTRA["xa_a3k9"]
                raw = synth.raw_alleles(cfg[0], cfg[1], 3, 4, cfg[3], cfg[4], 20261103)
            else:
                cfg, raw = tpa.WIDE[name][:12], tpa.wide_data(name)
            txt = str(d / (name + ".txt"))
            synth.write_text_polyploid(txt, raw)
            cache[name] = (cfg, raw, tp._allo_oracle(txt, str(d / (name + ".can")), cfg, True))
        return cache[name]
    return get


@pytest.fixture
def stats(monkeypatch):
    """what isg_p_device_stats says when tests/test_gpu_poly.py's hip_lines closes its chain"""
    from instruct_amd import capi
    seen = []
    close = capi.HipPolyChain.close

    def closing(self):
        if getattr(self, "h", None):
            z = self.z()
            used = z[:, :, 0] >= 0
            seen.append(dict(self.p_device_stats(), same_cluster=float((z == z[:, :, :1]).all(axis=2)[used].mean())))
        close(self)
    monkeypatch.setattr(capi.HipPolyChain, "close", closing)
    return seen


def same_lines(got, want, u):
    assert len(got) == len(want) == 1 + 6 * u
    for g, w in zip(got, want):
        assert tp._norm(g) == tp._norm(w), (g, w)


@pytest.mark.parametrize("name", sorted(ALLO) + sorted(ALLO_EXTRA))
def test_golden_and_generated_cases_draw_update_P_on_the_device(name, oracle, stats):
    cfg, raw, want = oracle(name)
    same_lines(tp.hip_lines(name, cfg, raw, allo=True), want, cfg[5])
    st = stats[-1]
    print("STATS", name, st)
    assert st["device_sweeps"] == cfg[5] and st["host_sweeps"] == 0, st


@pytest.mark.parametrize("env", [{}, {"INSTRUCT_WALK_SEG": "193"}, {"INSTRUCT_WALK_SEG": "65"}, {"INSTRUCT_WALK_K": "1"}], ids=["default", "seg193", "seg65", "k1"])
def test_walk_engine_shapes(env, oracle, stats, monkeypatch):
    """2400 groups of 1, 2, 5 and 9 gammas, 20 % missing.  INSTRUCT_WALK_SEG=193: 13 segments (the plan cuts them at multiples of 64 where it can:
    192 groups); =65: 37 segments of 65 groups, an odd length, so that the two Dirichlets of one (cluster, locus) fall into different blocks
    and segments; INSTRUCT_WALK_K=1: windows of one sigma are missed, the tables are built again with wider ones, and what is missed again goes to
    the host loop -- which redraws both subgenomes from the same stream position."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, raw, want = oracle("shapes")
    from instruct_amd import synth
    assert sorted(set(synth.code_tetraploid(raw)[2])) == [1, 2, 5, 9]
    same_lines(tp.hip_lines("shapes", cfg, raw, allo=True), want, cfg[5])
    st = stats[-1]
    print("STATS", env, st)
    assert st["device_sweeps"] + st["host_sweeps"] == cfg[5], st
    if "INSTRUCT_WALK_K" in env:
        assert st["retried"] >= 1, st
    else:
        assert st["host_sweeps"] == 0, st
        assert st["segments"] == {"193": 13, "65": 37}.get(env.get("INSTRUCT_WALK_SEG"), 1), st


def test_nine_clusters_on_data_of_three(oracle, stats):
    cfg, raw, want = oracle("k9_on_three")
    same_lines(tp.hip_lines("k9_on_three", cfg, raw, allo=True), want, cfg[5])
    assert stats[-1]["device_sweeps"] == cfg[5] and stats[-1]["host_sweeps"] == 0, stats[-1]


def test_a_lost_device_sweep_is_redrawn_by_the_host_loop(oracle, stats, monkeypatch):
    """INSTRUCT_P_TEST_ABORT=2: the second sweep is treated as lost after k_pdirich_at has written freq and freq2"""
    monkeypatch.setenv("INSTRUCT_P_TEST_ABORT", "2")
    cfg, raw, want = oracle("xa_a4k5")
    same_lines(tp.hip_lines("xa_a4k5", cfg, raw, allo=True), want, cfg[5])
    assert stats[-1]["host_sweeps"] == 1 and stats[-1]["device_sweeps"] == cfg[5] - 1, stats[-1]


@pytest.mark.parametrize("env", [{"INSTRUCT_P_DEVICE": "0"}, {"INSTRUCT_P_DEVICE": "0", "INSTRUCT_HOST_TAPE": "0"}], ids=["tape", "no_tape"])
def test_host_loop_forced(env, oracle, stats, monkeypatch):
    """xa_a3k9: at most 9 x 700 x 3 x 2 = 37800 gammas per sweep, above the 4096 from which the host loop takes its uniforms from the device"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, raw, want = oracle("xa_a3k9")
    same_lines(tp.hip_lines("xa_a3k9", cfg, raw, allo=True), want, cfg[5])
    assert stats[-1]["device_sweeps"] == 0, stats[-1]


def test_wide_allele_context_draws_on_the_device(oracle, stats):
    """loci of 32, 18, 23, 1, 2 and 4 alleles: closed-form rows, groups of up to 32 gammas"""
    cfg, raw, want = oracle("wa_allo")
    got = tpa.hip_lines(cfg, raw, 0, allo=True)
    same_lines(got, want, cfg[5])
    assert stats[-1]["device_sweeps"] == cfg[5] and stats[-1]["host_sweeps"] == 0, stats[-1]


def _big_lines(big_oracle, tag):
    p, out = big_oracle[tag]
    assert p.wait(timeout=600) == 0
    return [l for l in gu.parse(out) if l.startswith("it ") or l.startswith("chain zqinit")]


@pytest.mark.parametrize("pre", ["1", "0"])
@pytest.mark.parametrize("tag", ["big", "conv", "conv2"])
def test_pre_decision_equals_the_oracle_over_many_draws(tag, pre, big_oracle, stats, monkeypatch):
    """big: 12 iterations on data of four clusters (2 % of the loci end with their four copies in one cluster: the dot-product path).  conv: 40
    iterations of the same chain on data of two clusters (31 %); conv2: K=2 on that data, where the chain ends with 75 % of the loci in one cluster,
    so that the same-cluster path, which reads the genotype table, decides most draws.  With the pre-decision on and off (INSTRUCT_ALLO_PREFILTER=0)."""
    monkeypatch.setenv("INSTRUCT_ALLO_PREFILTER", pre)
    cfg = BIG[tag][0]
    got = tp.hip_lines(tag, cfg, big_data(tag), allo=True)
    same_lines(got, _big_lines(big_oracle, tag), cfg[5])
    print("STATS", tag, pre, stats[-1])
    assert stats[-1]["device_sweeps"] == cfg[5], stats[-1]
    if tag == "conv2":
        assert stats[-1]["same_cluster"] > 0.5, stats[-1]
