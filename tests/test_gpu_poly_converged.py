"""GPU (pytest -m gpu): ploidy-4 parity from converged-chain states (tests/converged_poly.py): the four Z copies of nearly every locus in one
cluster (the genotype-table branch of update_geno and of the likelihood), empty clusters, alpha = 0.003 (update_ZQ's Dirichlets on the gamma
branch below 1), qq entries below the float range, below the double range's normal part and at exactly 0, selfing rates of exactly 0 and 1
(NaN and infinite genotype tables).  The same state is written into the HIP chain (the C ABI's setters) and into the canonical oracle (its
state file) after the same chain_init; every comparison is line for line against the oracle's dump as in tests/test_gpu_poly.py: genotypes,
Z, counts, both float tables, rates and MH states, qq, qqnum, likelihoods, and the seeds on the replay schedule.
tests/test_converged_oracle_poly.py guards, on the CPU, that the oracle is in that regime.  Where a path is forced or known to be taken the
test asserts it from the path statistics, which it also prints (`STATS ...`, pytest -s shows them).

What binds (scratch builds with one guard of a float pre-filter changed, this module run once against each on the MI355X):
  k4_zq_block, `run > 1e-30f` dropped: the six scaled-row cases on the block resolver fail -- the state stays the oracle's, because the sweep
      at the resolved positions checks them and the single-workgroup kernel redoes it; zq_fallbacks() == 0 is what fails;
  bucket_f32 / bucket_from_cum (shared with the diploid kernels; the ploidy-4 sweep and probe kernels call them), `run > 1e-30f` dropped: the six 2^-135 cases fail at `it 0 ZQ`, on every path;
  guard band 6e-6 -> 0, in k4_zq_block or in bucket_f32 / bucket_from_cum: nothing here fails.  A float threshold is off by about 1e-7, so a
      draw flips with a probability of that order: the 5e6 draws of the largest input (pspec) are too few to expect one."""
import numpy as np
import pytest

import converged_poly as cp
import golden_util as gu
import orc
import test_gpu_poly as tp
import test_gpu_poly_alleles as tw

pytestmark = pytest.mark.gpu
VARIANTS = [(allo, sched) for allo in (False, True) for sched in (0, 1)]
EXPS = (120, 135, 142)


@pytest.fixture(scope="module")
def oracle_runs(tmp_path_factory):
    """every canonical oracle run of the module, started together (each is one CPU process); a trajectory is computed once and shared"""
    orc.build()
    d = tmp_path_factory.mktemp("convpoly")
    procs = {}
    for name, c in cp.INPUTS.items():
        for allo, sched in VARIANTS:
            procs[(name, allo, sched)] = cp.start_oracle(d, "%s.%d.%d" % (name, allo, sched), name, c.iters, state=cp.state_of(name), sched=sched, allo=allo)
    for allo in (False, True):
        procs[("e0", allo)] = cp.start_oracle(d, "e0.%d" % allo, "p60", 6, state=cp.state_of("p60", self_rates=cp.RATES_E0), e=0, allo=allo)
        procs[("e1", allo)] = cp.start_oracle(d, "e1.%d" % allo, "p60", 6, state=cp.state_of("p60", self_rates=cp.RATES_E1), e=1, allo=allo)
        for exp in EXPS:
            procs[("scaled", exp, allo)] = cp.start_oracle(d, "sc%d.%d" % (exp, allo), "p60", 2, state=_scaled(exp), allo=allo)
    memo = {}

    def lines(key):
        if key not in memo:
            p, out = procs[key]
            assert p.wait(timeout=600) == 0
            memo[key] = [l for l in gu.parse(out) if l.startswith(("it ", "chain zqinit", "chain injected"))]
        return memo[key]
    yield lines
    for p, _ in procs.values():
        if p.poll() is None:
            p.kill()
            p.wait()


def _scaled(exp):
    return cp.state_of("p60", off=1e-3, scale=2.0 ** -exp)


def _cfg(name, iters, e=1):
    c = cp.INPUTS[name]
    return (c.N, c.L, c.K, c.A, c.miss, iters, 1, 1, e, 1, iters + 1, cp.SEEDS)


def _stats_of(ch):
    return dict(spec=ch.zq_spec_stats(), resolve=ch.zq_resolve_stats(), pdev=ch.p_device_stats(), fallbacks=ch.zq_fallbacks())


def _print_stats(tag, st):
    sp, rs, pd = st["spec"], st["resolve"], st["pdev"]
    print("STATS %s | spec tried=%d settled=%d lost=%d retried=%d probes=%d rounds=%d fail_bits=%d lost_fail_bits=%d | resolve blocks=%d misses=%d launches=%d | "
          "P device=%d host=%d retried=%d failed_runs=%d | fallbacks=%d" % (tag, sp["tried"], sp["settled"], sp["lost"], sp["retried"], sp["probes"], sp["rounds"],
                                                                           sp["fail_bits"], sp["lost_fail_bits"], rs["blocks"], rs["misses"], rs["launches"],
                                                                           pd["device_sweeps"], pd["host_sweeps"], pd["retried"], pd["failed_runs"], st["fallbacks"]))


def _after_init(state, e, stats=None):
    """hip_lines' hook: writes the state, reports it as the oracle's `chain injected` line does; stats: a dict that receives the chain's path
    statistics when hip_lines closes the chain"""
    def hook(ch):
        cp.inject(ch, state)
        line = "chain injected alpha=%s hqq=%s" % (float(ch.alpha()).hex(), orc.fnv_f64(ch.qq())) + "".join(" " + float(x).hex() for x in ch.self_rates())
        if e == 0:
            line += "".join(" st%d" % x for x in ch.state())
        if stats is not None:
            close = ch.close

            def close_with_stats():
                if getattr(ch, "h", None):
                    stats.update(_stats_of(ch))
                close()
            ch.close = close_with_stats
        return [line]
    return hook


def _hip(name, iters, state, e=1, sched=0, allo=False, stats=None):
    hook = _after_init(state, e, stats)
    if name == "pwide":
        return tw.hip_lines(_cfg(name, iters, e), cp.raw(name), sched, allo=allo, after_init=hook)
    return tp.hip_lines(name, _cfg(name, iters, e), cp.raw(name), sched, fast_coder=(name == "pspec"), allo=allo, after_init=hook)


def _compare(got, want, sched=0, iters=None):
    """line for line; iters: the first iterations of a longer oracle run"""
    if iters is not None:
        want = want[:2 + 6 * iters]
    assert len(got) == len(want) and len(got) >= 2 + 6
    for g, w in zip(got, want):
        if sched:
            g, w = tp._noseeds(g), tp._noseeds(w)
        assert tp._norm(g) == tp._norm(w), (g, w)


# ---- a. every sweep: all inputs, both tetraploid variants, both schedules
@pytest.mark.parametrize("allo,sched", VARIANTS, ids=lambda v: None)
@pytest.mark.parametrize("name", sorted(cp.INPUTS))
def test_every_sweep_line_for_line(name, allo, sched, oracle_runs):
    c = cp.INPUTS[name]
    if name == "pwide":
        assert max(cp.coded(name)[2]) == 32
    got = _hip(name, c.iters, cp.state_of(name), sched=sched, allo=allo)
    assert len(got) == 2 + 6 * c.iters
    _compare(got, oracle_runs((name, allo, sched)), sched)


# ---- the setters: the -e 0 MH state goes with the written rates
def test_set_self_rates_sets_the_mh_state_poly():
    """isg_set_self_rates on a -e 0 chain: isg_get_state reports dt_stat of the written rates (the next update_S_POP proposes from it: case b)"""
    from instruct_amd import capi
    obs, alleleid, allelenum = cp.coded("p60")
    for allo in (False, True):
        ch = capi.HipPolyChain(obs, alleleid, allelenum, 6, back_refl=0, allo=allo)
        ch.setseeds(*cp.SEEDS)
        ch.chain_init(np.array([0.5] * 6, dtype=np.float32))
        assert list(ch.state()) == [1] * 6
        ch.set_self_rates(np.array(cp.RATES_E0))
        assert list(ch.state()) == [2, 0, 0, 2, 1, 2] and np.array_equal(ch.self_rates(), np.array(cp.RATES_E0))
        with pytest.raises(capi.IsgError, match="beyond"):
            ch.set_self_rates(np.array([0.5, 0.5, 1.5, 0.5, 0.5, 0.5]))
        assert list(ch.state()) == [2, 0, 0, 2, 1, 2] and np.array_equal(ch.self_rates(), np.array(cp.RATES_E0))   # (a refused vector changes nothing)
        ch.close()


@pytest.mark.parametrize("mode", [2, 4])
def test_set_self_rates_sets_the_mh_state_diploid(mode):
    """the same for the diploid per-cluster rates (mode 2) and inbreeding coefficients (mode 4), whose MH state lives on the device: the
    state read back, and the next update_S_POP, are the oracle's with the rates and dt_stat of them written into it"""
    import converged as cv
    from instruct_amd import capi
    geno, an, mi = cv.data("n60")
    K = 6
    rates = np.array(cp.RATES_E0)
    h = capi.HipChain(geno, an, mi, K, mode=mode, back_refl=0)
    o = orc.OrcChain(geno, an, mi, K, mode=mode, back_refl=0, math=orc.MATH_ISG, accum=orc.ACC_EXACT)
    for ch in (h, o):
        ch.setseeds(13, 4, 1972)
        ch.chain_init(np.array([ch.ran1() for _ in range(K)], dtype=np.float32))
    h.set_self_rates(rates)
    o.set_self_rates(rates)
    o.state()[...] = np.array([2, 0, 0, 2, 1, 2], dtype=np.int32)
    assert list(h.state()) == [2, 0, 0, 2, 1, 2] and np.array_equal(h.self_rates(), rates)
    for it in range(2):
        h.update_P(); o.update_P()
        h.update_S_POP(); o.update_S_POP()
        assert np.array_equal(h.state(), np.asarray(o.state())) and np.array_equal(h.self_rates(), np.asarray(o.self_rates())), it
        assert h.seeds() == o.seeds(), it
    assert o.error() == 0
    h.close()


# ---- b. rate edges
@pytest.mark.parametrize("allo", [False, True], ids=["auto", "allo"])
@pytest.mark.parametrize("e", [0, 1])
def test_rate_edges_line_for_line(e, allo, oracle_runs):
    """-e 0: rates of exactly 0 and 1 (states 2, 0, 0, 2, 1, 2): NaN and infinite genotype tables, totallkh NaN after iteration 0, then the
    Metropolis step from a NaN likelihood, update_ZQ and update_geno beside NaN tables, and a NaN table of an empty cluster that no sum may
    pick up.  -e 1: proposals reflected at 0 and at 1."""
    st = cp.state_of("p60", self_rates=cp.RATES_E0 if e == 0 else cp.RATES_E1)
    got = _hip("p60", 6, st, e=e, allo=allo)
    want = oracle_runs(("e%d" % e, allo))
    if e == 0:
        assert "totallkh=nan" in want[7] and want[7].startswith("it 0 L"), want[7]
        assert want[1].endswith(" st2 st0 st0 st2 st1 st2")
    _compare(got, want)


# ---- c. the path ladder of the replay schedule
_S0 = {"INSTRUCT_ZQ_SPEC_RESOLVE": "0"}
LADDER = [{}, _S0, dict(_S0, INSTRUCT_ZQ_RESOLVE_P4="1"), dict(_S0, INSTRUCT_ZQ_COOP="0"), dict(_S0, INSTRUCT_ZQ_TEST_ABORT="2"),
          {"INSTRUCT_P_DEVICE": "0"}, {"INSTRUCT_P_DEVICE": "0", "INSTRUCT_HOST_TAPE": "0"}, {"INSTRUCT_WALK_TRIM": "0"}]
_LADDER_CASES = [(env, allo) for allo in (False, True) for env in LADDER] + [({"INSTRUCT_ALLO_PREFILTER": "0"}, True)]


def _envid(env):
    return ",".join("%s=%s" % (k.replace("INSTRUCT_", ""), v) for k, v in sorted(env.items())) or "default"


@pytest.mark.parametrize("env,allo", _LADDER_CASES, ids=lambda v: _envid(v) if isinstance(v, dict) else ("allo" if v else "auto"))
def test_replay_paths_line_for_line(env, allo, oracle_runs, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = {}
    got = _hip("p60", 3, cp.state_of("p60"), allo=allo, stats=st)
    _print_stats("c p60 %s %s" % ("allo" if allo else "auto", _envid(env)), st)
    _compare(got, oracle_runs(("p60", allo, 0)), iters=3)
    sp, rs, pd, fb = st["spec"], st["resolve"], st["pdev"], st["fallbacks"]
    if "INSTRUCT_ZQ_SPEC_RESOLVE" in env:
        assert sp["tried"] == 0, sp
    else:
        assert sp["tried"] == 3 and sp["settled"] == 3 and sp["lost"] == 0 and fb == 0, (sp, fb)   # the interval resolver settles every sweep
    if "INSTRUCT_ZQ_RESOLVE_P4" in env:
        assert rs["blocks"] >= 1, rs                     # the block resolver (k4_zq_block) took part in the last sweep
    else:
        assert rs["blocks"] == 0 and rs["launches"] == 0, rs
    if "INSTRUCT_ZQ_TEST_ABORT" in env:
        assert fb == 1, fb                               # the aborted cooperative sweep, redone by the single-workgroup kernel
    elif "INSTRUCT_ZQ_SPEC_RESOLVE" in env:
        assert fb == 0, fb                               # (nothing was redone behind the path under test)
    if "INSTRUCT_P_DEVICE" in env:
        assert pd["device_sweeps"] == 0, pd
    else:
        assert pd["device_sweeps"] == 3 and pd["host_sweeps"] == 0, pd   # update_P's Dirichlets (both subgenomes') resolved on the device


# ---- d. the interval resolver's shape, on its own path and on the block resolver
@pytest.mark.parametrize("env", [{}, dict(_S0, INSTRUCT_ZQ_RESOLVE_P4="1")], ids=_envid)
def test_resolver_routes_pspec(env, oracle_runs, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = {}
    got = _hip("pspec", 4, cp.state_of("pspec"), stats=st)
    _print_stats("d pspec auto %s" % _envid(env), st)
    _compare(got, oracle_runs(("pspec", False, 0)))
    sp, rs, pd = st["spec"], st["resolve"], st["pdev"]
    assert pd["device_sweeps"] == 4 and pd["host_sweeps"] == 0 and st["fallbacks"] == 0, (pd, st["fallbacks"])
    if env:   # every sweep by the block resolver (2 blocks, none missed in the last sweep)
        assert sp["tried"] == 0 and rs["blocks"] >= 1 and rs["launches"] >= 1, (sp, rs)
    else:     # every sweep settled by the interval resolver, one of them on the second try with wider windows (MI355X: retried = 1)
        assert sp["tried"] == 4 and sp["settled"] == 4 and sp["lost"] == 0 and rs["blocks"] == 0, (sp, rs)


# ---- e. the float pre-filters' own guards: sums q f at the lower end of the float range
@pytest.mark.parametrize("env", [{}, _S0, dict(_S0, INSTRUCT_ZQ_RESOLVE_P4="1")], ids=_envid)
@pytest.mark.parametrize("allo", [False, True], ids=["auto", "allo"])
@pytest.mark.parametrize("exp", EXPS)
def test_row_sums_at_the_end_of_the_float_range_go_to_the_exact_path(exp, allo, env, oracle_runs, monkeypatch):
    """The construction of tests/test_gpu_converged.py's test of the same name for ploidy 4.  In a chain's own states a row of qq sums to 1
    and the pre-filters' `run` (the sum of q f over the clusters) is an ordinary float, so their `run > 1e-30f` terms never bind.  A Z draw
    depends on the ratios within a row only and the setter takes any row, so p60's rows (1e-3 off the true cluster) are scaled by a power
    of two, which is exact in double:
      2^-120: the largest entry (7.5e-37) is a normal float, the others (7.5e-40) are subnormal;
      2^-135: the largest entry is 16000 units of the smallest float subnormal, the others 16: thresholds compared in float are off by far
              more than the guard band of 6e-6, and only the `run > 1e-30f` term sends these draws to the double path;
      2^-142: the largest entry is a float subnormal with 7 bits, the others are 0 in float.
    Every draw of the first update_ZQ has to come out as the oracle's (the cooperative kernel's bucket_f32 / bucket_from_cum, the block
    resolver's k4_zq_block, the interval resolver's probes); after it qq is a Dirichlet draw again."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    state = _scaled(exp)
    big, small = np.float32(state.qq.max()), np.float32(state.qq.min())
    assert (1.2e-38 < big < 1e-30 and 0 < small < 1.2e-38) if exp == 120 else (0 < big < 1.2e-38 and (small == 0 or exp == 135))
    st = {}
    got = _hip("p60", 2, state, allo=allo, stats=st)
    _print_stats("e p60 %s 2^-%d %s" % ("allo" if allo else "auto", exp, _envid(env)), st)
    _compare(got, oracle_runs(("scaled", exp, allo)))
    sp, rs, fb = st["spec"], st["resolve"], st["fallbacks"]
    # MI355X: the interval resolver loses both sweeps with uncertain bytes left after every round (fail bit 64: the rows' Dirichlet shapes at
    # alpha = 0.003) and the cooperative kernel takes them; the block resolver takes both (3 blocks, 1 missed); nothing goes to the
    # single-workgroup kernel
    assert fb == 0, fb
    if "INSTRUCT_ZQ_RESOLVE_P4" in env:
        assert sp["tried"] == 0 and rs["blocks"] >= 1, (sp, rs)
    elif env:
        assert sp["tried"] == 0 and rs["blocks"] == 0, (sp, rs)
    else:
        assert sp["tried"] >= 1 and rs["blocks"] == 0, (sp, rs)


# ---- f. isg_run (the launch-ahead order) from the state
@pytest.mark.parametrize("allo,sched", VARIANTS, ids=lambda v: None)
def test_sweeps_then_run_line_set(allo, sched, oracle_runs):
    """3 iterations sweep by sweep, then run(3): what the chain holds afterwards is what the oracle's lines of iteration 5 report (the
    counts of its P line belong to the Z of before its update_ZQ and are not to be had any more)"""
    from instruct_amd import capi
    obs, alleleid, allelenum = cp.coded("p60")
    c = cp.INPUTS["p60"]
    ch = capi.HipPolyChain(obs, alleleid, allelenum, c.K, back_refl=1, rng_sched=sched, allo=allo)
    ch.setseeds(*cp.SEEDS)
    ch.chain_init(np.array([np.float32(ch.ran1()) for _ in range(c.K)], dtype=np.float32))
    cp.inject(ch, cp.state_of("p60"))
    for _ in range(3):
        ch.update_P()
        ch.update_S_POP()
        ch.update_ZQ(0)
        ch.update_geno()
        ch.cal_lkh()
        ch.lib.isg_iter_advance(ch.h)
    ch.run(3)
    got = {"hfreq": tp._hfreq(ch, allelenum),
           "X": "it 5 X hexfreq=%s" % orc.fnv_i32(ch.packed(ch.exfreq()).view(np.int32)),
           "S": "it 5 S" + "".join(" " + float(x).hex() for x in ch.self_rates()) + " hgenofreq=%s" % orc.fnv_i32(ch.packed(ch.genofreq()).view(np.int32)),
           "ZQ": "it 5 ZQ hz=%s hqq=%s hqqnum=%s" % (orc.fnv_i32(ch.z()), orc.fnv_f64(ch.qq()), orc.fnv_f64(ch.qqnum())),
           "GE": "it 5 GE hgeno=%s" % orc.fnv_i32(ch.geno()) + " seeds=%d %d %d" % ch.seeds(),
           "L": "it 5 L totallkh=%s hindv=%s" % (float(ch.totallkh()).hex(), orc.fnv_f64(ch.indvlkh()))}
    if allo:
        got["hfreq2"] = tp._hfreq(ch, allelenum, ch.freq2())
    ch.close()
    want = {l.split()[2]: l for l in oracle_runs(("p60", allo, sched)) if l.startswith("it 5 ")}
    assert sorted(want) == ["GE", "L", "P", "S", "X", "ZQ"]
    fp = gu.fields(want["P"])
    assert got["hfreq"] == fp["hfreq"] and (not allo or got["hfreq2"] == fp["hfreq2"])
    for k in ("X", "L"):
        assert tp._norm(got[k]) == tp._norm(want[k]), k
    for k in ("S", "ZQ"):
        assert tp._norm(got[k]) == tp._norm(tp._noseeds(want[k])), k
    g, w = (tp._noseeds(got["GE"]), tp._noseeds(want["GE"])) if sched else (got["GE"], want["GE"])   # (the stream's position after the last drawing sweep)
    assert tp._norm(g) == tp._norm(w)
