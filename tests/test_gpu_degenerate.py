"""GPU (pytest -m gpu): parity on the degenerate data shapes of tests/degenerate.py -- loci typed in nobody, one-allele loci (first, last, on
both sides of the 64-locus boundary of the rank words), individuals typed nowhere or at one locus, a whole 64-locus word of one individual
missing, data without a single ambiguous genotype, N = 1, L = 1.  tests/test_degenerate_oracle.py shows on the CPU that the oracle equals the
reference on them; here the device equals the canonical oracle, bit for bit:

  ploidy 4   every dump line (as tests/test_gpu_poly.py) on both schedules and both tetraploid variants; `deg` and `hom` once per forced route
             of the replay schedule, each asserted from the path statistics (printed: `STATS ...`, pytest -s shows them); the reference's own
             trajectories (tests/golden/tg_*.golden: discrete state and seeds equal, doubles within 1e-9); what the dump cannot see (its hfreq
             skips loci with fewer than two alleles): freq == 1.0 exactly at the one-allele loci after every update_P, counts 0 at the untyped
             loci, z and geno -1 wherever nothing is typed, indvlkh 0.0 for the untyped individual, the keyed layout; run() with launch-ahead;
             the drop-in program's result files
  diploid    every input x every mode x both schedules, sweep by sweep for 3 iterations, then run(3): every array and the seeds equal to the
             canonical oracle's; `single` (one-allele loci handed in through the ABI) on the default device route of update_P, without the
             walk tables' trim, and in mode 2 on the other update_ZQ routes.

What binds (scratch builds of the library with one thing changed, this module run once against each on the MI355X):
  update_P's group list built with min_alleles = 1 for ploidy 4 (both variants): 21 cases fail.  With the direct checks, first at
      `freq[k][j][0] == 1.0` of _direct_checks (0.0 is read); without them (test_matches_reference_trajectory) at `it 0 P`, where hfreq is the
      reference's and the seeds are not: the stream position after update_P differs.  The keyed cases pass: the list is the replay schedule's.
  amb_run++ counting na == 1 as well: 53 cases fail, from `chain zqinit` on in _compare (every ploidy-4 input, both schedules, `hom` included).
  `allelenum[j] <= 1` -> `< 1` in the diploid context: the 21 cases of `single` fail at ('init', 'z') in _same; the other inputs pass.
  `if (p.nvalid[i] == 0) lo = hi = 0.f;` of k4_zexpect_fin removed: nothing fails, and nothing can: with no typed locus the sums are l = v = 0,
      so h = 1, lo = floor(-1) is raised to 0 by `lo < 0` and hi = ceil(1) is cut to tot = 0 by `hi > tot`: the line restates the two clamps.
"""
import collections
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import degenerate as dg
import golden_util as gu
import orc
import test_gpu_poly as tp
import test_gpu_poly_converged as tc

import make_golden_degenerate as mgd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_ITERS = 6
ROUTED = ("deg", "hom")   # the inputs of the route tests and of run()'s.  Every route is taken at their own size on the MI355X (the statistics assert it): nothing is tiled


def _poly_cases():
    out = []
    for name, p in dg.POLY.items():
        for e in p.es:
            for allo in ((False, True) if p.allo_too else (False,)):
                for sched in (0, 1):
                    out.append((name, e, allo, sched))
    return out


POLY_CASES = _poly_cases()


def _pid(v):
    name, e, allo, sched = v
    return "%s-e%d-%s-%s" % (name, e, "allo" if allo else "auto", "keyed" if sched else "replay")


@pytest.fixture(scope="module")
def oracle_runs(tmp_path_factory):
    """every canonical oracle run of the module, started together (each is one CPU process well under a second); a trajectory is computed
    once and shared.  `deg` (-e 1) and `hom` run 6 iterations (run()'s test); the sweep-by-sweep tests compare the first 3 of them."""
    orc.build()
    d = tmp_path_factory.mktemp("degenerate")
    procs = {}
    for name, e, allo, sched in POLY_CASES:
        iters = RUN_ITERS if (name in ROUTED and e == 1) else dg.ITERS
        procs[(name, e, allo, sched)] = dg.start_oracle(d, "%s.%d.%d.%d" % (name, e, allo, sched), dg.raw(name), dg.POLY[name].K, iters, e=e, sched=sched, allo=allo)
    memo = {}

    def lines(name, e=1, allo=False, sched=0):
        key = (name, e, allo, sched)
        if key not in memo:
            p, out = procs[key]
            assert p.wait(timeout=600) == 0
            memo[key] = [l for l in gu.parse(out) if l.startswith(("it ", "chain zqinit"))]
        return memo[key]
    yield lines
    for p, _ in procs.values():
        if p.poll() is None:
            p.kill()
            p.wait()


def _layout(N, L, K, Amax, amb, allo):
    """include/instruct_hip.h, keyed layout for ploidy 4"""
    SP = (2 if allo else 1) * (16 * Amax + 16)
    SZ = 4 * L + 16 * K + 16
    ZI0 = 1 + amb
    B0 = ZI0 + N * SZ
    offS = K * L * SP
    offZ = offS + 4 * K
    offGE = offZ + N * SZ
    BLK = offGE + amb + 4
    return (SP, SZ, ZI0, B0, offS, offGE, offZ, offGE, BLK)


def _direct_checks(ch, alleleid, allelenum, allo):
    """what the dump's hashes do not cover, asserted after every sweep that writes it; -> a counter of the sweeps checked"""
    one, none = np.flatnonzero(allelenum == 1), np.flatnonzero(allelenum == 0)
    untyped = np.flatnonzero((alleleid > 0).sum(1) == 0)
    seen = collections.Counter()

    def after(name, check):
        sweep = getattr(ch, name)

        def wrapped(*a):
            sweep(*a)
            check()
            seen[name] += 1
        setattr(ch, name, wrapped)

    def nothing_typed(a, what):
        assert np.array_equal(a == -1, np.broadcast_to((alleleid == 0)[:, :, None], a.shape)), what   # -1 exactly where nothing is typed
        assert (a[:, none] == -1).all() and (a[untyped] == -1).all(), what

    def p():
        f = ch.freq()
        assert (f[:, one, 0] == 1.0).all(), f[:, one, 0]   # rdirich over one gamma: g / g
        if allo:
            assert (ch.freq2()[:, one, 0] == 1.0).all()
        c = ch.count_alleles()
        assert (c[:, none, :] == 0).all() and (c[:, one, 1:] == 0).all()
    after("update_P", p)
    after("update_ZQ", lambda: nothing_typed(ch.z(), "z"))
    after("update_geno", lambda: nothing_typed(ch.geno(), "geno"))

    def lk():
        assert (ch.indvlkh()[untyped] == 0.0).all(), ch.indvlkh()[untyped]   # no locus, no term
    after("cal_lkh", lk)
    nothing_typed(ch.z(), "z after chain_init")
    nothing_typed(ch.geno(), "geno after chain_init")
    return seen


def _hip(name, e=1, sched=0, allo=False, iters=dg.ITERS, stats=None, checks=None):
    """tests/test_gpu_poly.py's hip_lines on a named input; stats: a dict that receives the path statistics and the keyed layout when the chain
    is closed; checks: a list that receives the counter of _direct_checks"""
    raw = dg.raw(name)
    p = dg.POLY[name]
    cfg = (raw.shape[0], raw.shape[1], p.K, 0, 0.0, iters, 1, 1, e, 1, iters + 1, dg.SEEDS)

    def hook(ch):
        if checks is not None:
            _, alleleid, allelenum = dg.coded(name)
            checks.append(_direct_checks(ch, alleleid, allelenum, allo))
        if stats is not None:
            close = ch.close

            def close_with_stats():
                if getattr(ch, "h", None):
                    stats.update(tc._stats_of(ch))
                    stats["layout"] = ch.keyed_layout()
                    stats["Amax"] = ch.Amax
                close()
            ch.close = close_with_stats
    return tp.hip_lines(name, cfg, np.array(raw), sched, allo=allo, after_init=hook)


def _compare(got, want, sched, iters=dg.ITERS):
    """line for line; want: the first iterations of a possibly longer oracle run"""
    want = want[:1 + 6 * iters]
    assert len(got) == len(want) == 1 + 6 * iters
    for g, w in zip(got, want):
        if sched:
            g, w = tp._noseeds(g), tp._noseeds(w)
        assert tp._norm(g) == tp._norm(w), (g, w)


# ---- a. every sweep: all inputs, both tetraploid variants, both schedules
@pytest.mark.parametrize("case", POLY_CASES, ids=_pid)
def test_every_sweep_line_for_line(case, oracle_runs):
    """sched 1 = keyed schedule (the sequential seed triple is not defined there and is left out)"""
    name, e, allo, sched = case
    p = dg.POLY[name]
    obs, alleleid, allelenum = dg.coded(name)
    st, checks = {}, []
    got = _hip(name, e, sched, allo, stats=st, checks=checks)
    tc._print_stats("a %s" % _pid(case), st)
    _compare(got, oracle_runs(name, e, allo, sched), sched)
    assert checks[0] == {"update_P": dg.ITERS, "update_ZQ": dg.ITERS, "update_geno": dg.ITERS, "cal_lkh": dg.ITERS}
    amb = dg.amb_of(alleleid, allo)
    assert p.amb is None or amb == p.amb[allo]
    assert st["layout"] == _layout(p.N, p.L, p.K, st["Amax"], amb, allo) and st["Amax"] == max(1, int(allelenum.max()))
    if name == "hom":
        assert st["layout"][2] == 1 and st["layout"][8] == st["layout"][5] + 4   # ZI0 == 1, BLK == offGE + 4: no uniform for any genotype
    if sched == 0:
        pd = st["pdev"]
        assert pd["device_sweeps"] == dg.ITERS and pd["host_sweeps"] == 0, pd   # update_P's Dirichlets resolved on the device in every sweep
        sp = st["spec"]
        assert sp["tried"] == dg.ITERS and sp["settled"] == dg.ITERS and sp["lost"] == 0 and st["fallbacks"] == 0, (sp, st["fallbacks"])   # ... and update_ZQ by the interval resolver


# ---- b. deg and hom once per route of the replay schedule
_S0 = {"INSTRUCT_ZQ_SPEC_RESOLVE": "0"}
ROUTES = [{"INSTRUCT_P_DEVICE": "0"}, _S0, dict(_S0, INSTRUCT_ZQ_RESOLVE_P4="1"), dict(_S0, INSTRUCT_ZQ_TEST_ABORT="2"), {"INSTRUCT_WALK_TRIM": "0"}]
_ROUTE_CASES = [(env, name, allo) for name in ROUTED for allo in (False, True) for env in ROUTES + ([{"INSTRUCT_ALLO_PREFILTER": "0"}] if allo else [])]


@pytest.mark.parametrize("env,name,allo", _ROUTE_CASES, ids=lambda v: tc._envid(v) if isinstance(v, dict) else (v if isinstance(v, str) else ("allo" if v else "auto")))
def test_replay_routes_line_for_line(env, name, allo, oracle_runs, monkeypatch):
    """INSTRUCT_P_DEVICE=0: update_P's host loop; INSTRUCT_ZQ_SPEC_RESOLVE=0: the cooperative chain kernel; with INSTRUCT_ZQ_RESOLVE_P4=1: the
    block resolver; INSTRUCT_ZQ_TEST_ABORT=2: the cooperative sweep of the second update_ZQ counted as aborted and redone by the single-workgroup
    kernel (without the interval resolver, which would take the sweep before the cooperative kernel sees it); INSTRUCT_WALK_TRIM=0: the walk
    tables over every column; INSTRUCT_ALLO_PREFILTER=0: the allotetraploid genotype draw without its single-precision pre-decision."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st, checks = {}, []
    got = _hip(name, 1, 0, allo, stats=st, checks=checks)
    tc._print_stats("b %s %s %s" % (name, "allo" if allo else "auto", tc._envid(env)), st)
    _compare(got, oracle_runs(name, 1, allo, 0), 0)
    assert checks[0]["update_P"] == dg.ITERS
    sp, rs, pd, fb = st["spec"], st["resolve"], st["pdev"], st["fallbacks"]
    if "INSTRUCT_ZQ_SPEC_RESOLVE" in env:
        assert sp["tried"] == 0, sp
    else:
        assert sp["tried"] == dg.ITERS and sp["settled"] == dg.ITERS and sp["lost"] == 0 and fb == 0, (sp, fb)   # the interval resolver settles every sweep
    if "INSTRUCT_ZQ_RESOLVE_P4" in env:
        assert rs["blocks"] >= 1 and rs["launches"] >= 1 and fb == 0, (rs, fb)   # the block resolver (k4_zq_block) took part in the last sweep
    else:
        assert rs["blocks"] == 0 and rs["launches"] == 0, rs
    if "INSTRUCT_ZQ_TEST_ABORT" in env:
        assert fb == 1, fb
    elif "INSTRUCT_ZQ_SPEC_RESOLVE" in env:
        assert fb == 0, fb                                  # nothing was redone behind the path under test
    if "INSTRUCT_P_DEVICE" in env:
        assert pd["device_sweeps"] == 0 and pd["host_sweeps"] == 0 and pd["blocks"] == 0, pd   # no device context at all: the host loop drew
    else:
        assert pd["device_sweeps"] == dg.ITERS and pd["host_sweeps"] == 0, pd


# ---- c. the reference's own trajectories
@pytest.mark.parametrize("name", sorted(mgd.CASES))
def test_matches_reference_trajectory(name):
    """tests/golden/tg_*.golden come from the reference's own sweeps (oracle/ref_dump_poly.c): discrete state and seeds identical after every
    sweep, doubles within 1e-9"""
    inp, allo = mgd.CASES[name]
    want = [l for l in gu.parse(os.path.join(gu.GOLDEN, name + ".golden")) if l.startswith(("it ", "chain zqinit"))]
    got = _hip(inp, 1, 0, allo, iters=mgd.U)
    assert len(got) == len(want) == 1 + 6 * mgd.U
    for g, w in zip(got, want):
        fg, fw = gu.fields(g), gu.fields(w)
        for key in ("hz", "hgeno", "hcnt", "hqqnum", "seeds"):
            assert fg.get(key) == fw.get(key), (key, g, w)
        assert [t for t in g.split() if t.startswith("st")] == [t for t in w.split() if t.startswith("st")]
        a, bb = gu.floats(g), gu.floats(w)
        assert len(a) == len(bb)
        for x, y in zip(a, bb):
            assert x == y or (x != x and y != y) or abs(x - y) <= 1e-9 * max(abs(x), abs(y)), (g, w)


# ---- d. run(): the launch-ahead order
@pytest.mark.parametrize("sched", [0, 1], ids=["replay", "keyed"])
@pytest.mark.parametrize("allo", [False, True], ids=["auto", "allo"])
@pytest.mark.parametrize("name", ROUTED)
def test_run_with_launch_ahead_equals_six_oracle_iterations(name, allo, sched, oracle_runs):
    """run(4) and two isg_iteration calls: what the chain holds afterwards is what the oracle's lines of iteration 5 report (the counts of its P
    line belong to the Z of before its update_ZQ and are not to be had any more); closing the context returns every buffer"""
    from instruct_amd import capi
    gc.collect()   # (a chain an earlier, failed test left open is closed when it is collected: not during this test)
    live = capi.live_buffers()
    obs, alleleid, allelenum = dg.coded(name)
    K = dg.POLY[name].K
    ch = capi.HipPolyChain(obs, alleleid, allelenum, K, back_refl=1, rng_sched=sched, allo=allo)
    assert capi.live_buffers() > live
    ch.setseeds(*dg.SEEDS)
    ch.chain_init(np.array([np.float32(ch.ran1()) for _ in range(K)], dtype=np.float32))
    ch.run(RUN_ITERS - 2)
    ch.iteration()
    ch.iteration()
    last = RUN_ITERS - 1
    got = {"hfreq": tp._hfreq(ch, allelenum),
           "X": "it %d X hexfreq=%s" % (last, orc.fnv_i32(ch.packed(ch.exfreq()).view(np.int32))),
           "S": "it %d S" % last + "".join(" " + float(x).hex() for x in ch.self_rates()) + " hgenofreq=%s" % orc.fnv_i32(ch.packed(ch.genofreq()).view(np.int32)),
           "ZQ": "it %d ZQ hz=%s hqq=%s hqqnum=%s" % (last, orc.fnv_i32(ch.z()), orc.fnv_f64(ch.qq()), orc.fnv_f64(ch.qqnum())),
           "GE": "it %d GE hgeno=%s" % (last, orc.fnv_i32(ch.geno())) + " seeds=%d %d %d" % ch.seeds(),
           "L": "it %d L totallkh=%s hindv=%s" % (last, float(ch.totallkh()).hex(), orc.fnv_f64(ch.indvlkh()))}
    if allo:
        got["hfreq2"] = tp._hfreq(ch, allelenum, ch.freq2())
    one = np.flatnonzero(allelenum == 1)
    f1 = [ch.freq()[:, one, 0]] + ([ch.freq2()[:, one, 0]] if allo else [])
    pd = ch.p_device_stats()
    ch.close()
    assert capi.live_buffers() == live
    assert all((f == 1.0).all() for f in f1), f1
    if sched == 0:
        assert pd["device_sweeps"] == RUN_ITERS and pd["host_sweeps"] == 0, pd
    want = {l.split()[2]: l for l in oracle_runs(name, 1, allo, sched) if l.startswith("it %d " % last)}
    assert sorted(want) == ["GE", "L", "P", "S", "X", "ZQ"]
    fp = gu.fields(want["P"])
    assert got["hfreq"] == fp["hfreq"] and (not allo or got["hfreq2"] == fp["hfreq2"])
    for k in ("X", "L"):
        assert tp._norm(got[k]) == tp._norm(want[k]), k
    for k in ("S", "ZQ"):
        assert tp._norm(got[k]) == tp._norm(tp._noseeds(want[k])), k
    g, w = (tp._noseeds(got["GE"]), tp._noseeds(want["GE"])) if sched else (got["GE"], want["GE"])   # (the stream's position after the last drawing sweep)
    assert tp._norm(g) == tp._norm(w)


# ---- e. the drop-in program
@pytest.mark.parametrize("fname", sorted(mgd.CLI))
def test_dropin_cli_output_on_degenerate_data_equals_reference(fname, tmp_path):
    """`-p 4` through the drop-in on tests/golden/tg_deg.txt, -ap 1 and -ap 0: the result files the reference program wrote"""
    exe = os.path.join(ROOT, "oracle", "_ref", "InStruct_hip")
    assert os.path.exists(exe), "oracle/_ref/InStruct_hip is built by build()"
    out = tmp_path / "out.txt"
    cmd = [exe, "-d", os.path.join(gu.GOLDEN, "tg_deg.txt"), "-o", str(out)] + mgd.CLI[fname]
    log = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert log.returncode == 0 and b"THE JOB IS SUCCESSFULLY FINISHED" in log.stdout, log.stdout[-2000:]

    def body(path):
        return [l for l in open(path, "rb").read().split(b"\n")
                if not (l.strip().startswith((b"Data File:", b"Output File:")) or b"InStruct" in l and b"-d" in l)]
    assert body(str(out)) == body(os.path.join(gu.GOLDEN, fname))


# ---------------------------------------------------------------------------------------------- diploid
SWEEPS = {   # the reference's order (mcmc.c:208-235): sweep -> what it writes
    0: (("update_P", ("count_alleles", "freq")), ("update_Z", ("z", "generation")), ("cal_lkh", ("indvlkh", "totallkh"))),
    1: (("update_P", ("count_alleles", "freq")), ("update_ZQ", ("z", "qq", "qqnum")), ("update_alpha", ("alpha",)), ("cal_lkh", ("indvlkh", "totallkh"))),
    2: (("update_P", ("count_alleles", "freq")), ("update_S_POP", ("self_rates", "state")), ("update_G", ("generation",)), ("update_ZQ", ("z", "qq", "qqnum")),
        ("update_alpha", ("alpha",)), ("cal_lkh", ("indvlkh", "totallkh"))),
    3: (("update_P", ("count_alleles", "freq")), ("update_S_IND", ("self_rates",)), ("update_G", ("generation",)), ("update_ZQ", ("z", "qq", "qqnum")),
        ("update_alpha", ("alpha",)), ("cal_lkh", ("indvlkh", "totallkh"))),
    4: (("update_P", ("count_alleles", "freq")), ("update_S_POP", ("self_rates", "state")), ("update_ZQ", ("z", "qq", "qqnum")), ("update_alpha", ("alpha",)),
        ("cal_lkh", ("indvlkh", "totallkh"))),
    5: (("update_P", ("count_alleles", "freq")), ("update_S_IND", ("self_rates",)), ("update_ZQ", ("z", "qq", "qqnum")), ("update_alpha", ("alpha",)),
        ("cal_lkh", ("indvlkh", "totallkh"))),
}


def _everything(mode):
    if mode == 0:
        return ["z", "generation", "freq", "count_alleles", "indvlkh", "totallkh"]
    return ["z", "qq", "qqnum", "generation", "alpha", "self_rates", "freq", "count_alleles", "indvlkh", "totallkh"] + (["state"] if mode in (2, 4) else [])


@pytest.fixture(scope="module", autouse=True)
def _libs():
    from instruct_amd import capi
    orc.build()
    capi.load().isg_iter_advance.argtypes = [C.c_void_p]
    orc.load().orc_iter_advance.argtypes = [C.c_void_p]


def _dip_pair(name, mode, sched):
    from instruct_amd import capi
    geno, an, mi = dg.diploid(name)
    K = dg.DIPLOID[name].K
    h = capi.HipChain(geno, an, mi, K, mode=mode, rng_sched=sched)
    o = orc.OrcChain(geno, an, mi, K, mode=mode, math=orc.MATH_ISG, accum=orc.ACC_EXACT, sched=sched)
    for ch in (h, o):
        ch.setseeds(*dg.SEEDS)
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


def _dip_sweeps_then_run(h, o, mode, sched, iters=3):
    pos = ["seeds"] if sched == 0 else []
    same = _same
    same(h, o, (["z", "generation"] if mode == 0 else ["z", "qq", "qqnum", "generation", "alpha"]) + pos, "init")
    for it in range(iters):
        for sweep, wrote in SWEEPS[mode]:
            getattr(h, sweep)()
            getattr(o, sweep)()
            same(h, o, list(wrote) + (pos if sweep != "cal_lkh" else []), (it, sweep))
        o.lib.orc_iter_advance(o.h)
        h.lib.isg_iter_advance(h.h)
    same(h, o, _everything(mode) + pos, "sweeps")
    h.run(iters)
    for _ in range(iters):
        o.iteration()
    same(h, o, _everything(mode) + pos, "run")
    assert o.error() == 0


@pytest.mark.parametrize("sched", [0, 1], ids=["replay", "keyed"])
@pytest.mark.parametrize("mode", dg.MODES)
@pytest.mark.parametrize("name", sorted(dg.DIPLOID))
def test_diploid_every_sweep_then_run_bit_exact(name, mode, sched):
    h, o = _dip_pair(name, mode, sched)
    _dip_sweeps_then_run(h, o, mode, sched)
    pd = h.p_device_stats()
    print("STATS %s mode %d sched %d | P device=%d host=%d retried=%d failed_runs=%d" % (name, mode, sched, pd["device_sweeps"], pd["host_sweeps"], pd["retried"], pd["failed_runs"]))
    if name == "single":
        an = dg.diploid(name)[1]
        one = np.flatnonzero(an == 1)
        assert {0, 63, 64, an.size - 1} <= set(one)
        assert (h.count_alleles()[:, one, :] == 0).all() and (h.z()[:, one, :] == -1).all()   # used by nobody
        if sched == 0:   # the default route of update_P at the input's own 130 loci x 3 clusters: the walk engine's group list (min_alleles = 1), in all 6 sweeps
            assert pd["device_sweeps"] == 6 and pd["host_sweeps"] == 0, pd
    h.close()


@pytest.mark.parametrize("mode", dg.MODES)
def test_diploid_single_allele_loci_without_walk_trim(mode, monkeypatch):
    monkeypatch.setenv("INSTRUCT_WALK_TRIM", "0")
    h, o = _dip_pair("single", mode, 0)
    _dip_sweeps_then_run(h, o, mode, 0)
    pd = h.p_device_stats()
    assert pd["device_sweeps"] == 6 and pd["host_sweeps"] == 0, pd
    h.close()


_R0 = dict(_S0, INSTRUCT_ZQ_RESOLVE="0")
_P0 = dict(_S0, INSTRUCT_ZQ_RESOLVE_PERSIST="0")


@pytest.mark.parametrize("env", [_S0, _R0, _P0], ids=tc._envid)
def test_diploid_single_allele_loci_on_the_update_ZQ_routes(env, monkeypatch):
    """mode 2 without the interval resolver: the block resolver with all blocks in one launch (_S0) and with one launch per block (_P0), and
    the chain kernels (_R0)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, o = _dip_pair("single", 2, 0)
    _dip_sweeps_then_run(h, o, 2, 0)
    sp, rs, pd, fb = h.zq_spec_stats(), h.zq_resolve_stats(), h.p_device_stats(), h.zq_fallbacks()
    print("STATS single %s | spec tried=%d | resolve blocks=%d misses=%d launches=%d | P device=%d host=%d | fallbacks=%d" %
          (tc._envid(env), sp["tried"], rs["blocks"], rs["misses"], rs["launches"], pd["device_sweeps"], pd["host_sweeps"], fb))
    assert sp["tried"] == 0 and fb == 0, (sp, fb)
    if "INSTRUCT_ZQ_RESOLVE" in env:
        assert rs["blocks"] == 0 and rs["launches"] == 0, rs
    else:
        assert rs["blocks"] >= 1 and rs["launches"] >= 1, rs
    assert pd["device_sweeps"] == 6 and pd["host_sweeps"] == 0, pd
    h.close()
