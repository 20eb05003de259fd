"""GPU (pytest -m gpu): parity from converged-chain states (tests/converged.py): empty clusters, qqnum 0 for most (individual, cluster)
pairs, alpha far below 1, qq entries below the float range and at exactly 0.  The same state is written into the HIP chain (the C ABI's
setters) and into the canonical oracle after the same chain_init; every comparison is bit-exact (np.array_equal / ==), seeds on the
replay schedule.  Where a path is forced or a route of the interval resolver is known to be taken, the test asserts it from the path
statistics; the interval resolver's cases also print them (`STATS ...`, pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest

import converged as cv
import orc
from instruct_amd import capi

pytestmark = pytest.mark.gpu
ALL = ["z", "qq", "qqnum", "generation", "alpha", "self_rates", "freq", "indvlkh", "totallkh", "state"]


@pytest.fixture(scope="module", autouse=True)
def _libs():
    orc.build()
    lib = capi.load()
    lib.isg_iter_advance.argtypes = [C.c_void_p]
    orc.load().orc_iter_advance.argtypes = [C.c_void_p]


def _hip(name, sched=capi.SCHED_REPLAY, e=1):
    """the HIP chain of a named input after chain_init, with the converged state written into it"""
    c = cv.INPUTS[name]
    geno, an, mi = cv.data(name)
    h = capi.HipChain(geno, an, mi, c.K, mode=c.mode, back_refl=e, rng_sched=sched)
    h.setseeds(13, 4, 1972)
    h.chain_init(np.array([h.ran1() for _ in range(c.K)], dtype=np.float32))
    cv.inject(h, cv.state_of(name))
    return h


def _orc(name, sched=capi.SCHED_REPLAY, e=1):
    c = cv.INPUTS[name]
    geno, an, mi = cv.data(name)
    o = orc.OrcChain(geno, an, mi, c.K, mode=c.mode, back_refl=e, math=orc.MATH_ISG, accum=orc.ACC_EXACT, sched=sched)
    o.setseeds(13, 4, 1972)
    o.chain_init(np.array([o.ran1() for _ in range(c.K)], dtype=np.float32))
    cv.inject(o, cv.state_of(name))
    return o


def _same(h, o, names, where):
    for n in names:
        a, b = getattr(h, n)(), getattr(o, n)()
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, np.asarray(b)), (where, n)
        else:
            assert a == b, (where, n, a, b)


def _stats(h, tag=None):
    """the path statistics; printed (pytest -s) for the interval resolver's cases, which pass a tag"""
    sp, rs, pd, fb = h.zq_spec_stats(), h.zq_resolve_stats(), h.p_device_stats(), h.zq_fallbacks()
    if tag is None:
        return sp, rs, pd, fb
    print("STATS %s | spec tried=%d settled=%d lost=%d retried=%d probes=%d rounds=%d fail_bits=%d lost_fail_bits=%d | resolve blocks=%d misses=%d "
          "launches=%d D=%d | P device=%d host=%d | fallbacks=%d" % (tag, sp["tried"], sp["settled"], sp["lost"], sp["retried"], sp["probes"], sp["rounds"],
                                                                   sp["fail_bits"], sp["lost_fail_bits"], rs["blocks"], rs["misses"], rs["launches"], rs["D"],
                                                                   pd["device_sweeps"], pd["host_sweeps"], fb))
    return sp, rs, pd, fb


def _sweeps(h, o, mode, iters, sched):
    """the public sweeps one by one in the reference's order (mcmc.c:208-235), the state they wrote compared after each"""
    pos = ["seeds"] if sched == capi.SCHED_REPLAY else []
    _same(h, o, ["z", "qq", "generation", "alpha", "self_rates"] + pos, "injected")   # (qqnum is stale until the first update_ZQ)
    for it in range(iters):
        h.update_P(); o.update_P()
        _same(h, o, ["count_alleles", "freq"] + pos, (it, "P"))
        if mode in (2, 4):
            h.update_S_POP(); o.update_S_POP()
            _same(h, o, ["self_rates", "state"] + pos, (it, "S"))
        if mode in (3, 5):
            h.update_S_IND(); o.update_S_IND()
            _same(h, o, ["self_rates"] + pos, (it, "SI"))
        if mode in (2, 3):
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


# ---- a. every sweep, both schedules; then the launch-ahead order
@pytest.mark.parametrize("sched", [capi.SCHED_REPLAY, capi.SCHED_KEYED])
@pytest.mark.parametrize("name,e", [("n60", 1), ("n60", 0), ("m1", 1), ("m3", 1), ("m4", 1), ("m5", 1), ("n150", 1)])
def test_every_sweep_then_run_bit_exact(name, e, sched):
    h, o = _hip(name, sched, e), _orc(name, sched, e)
    _sweeps(h, o, cv.INPUTS[name].mode, 6, sched)
    h.run(6)
    for _ in range(6):
        o.iteration()
    _same(h, o, ALL + (["seeds"] if sched == capi.SCHED_REPLAY else []), "run(6)")
    assert o.error() == 0 and o.alpha() < 1
    h.close()


@pytest.mark.parametrize("sched", [capi.SCHED_REPLAY, capi.SCHED_KEYED])
def test_state_written_after_run_replaces_what_was_requested_ahead(sched):
    """the setters in the middle of a chain: run() ends with next iteration's counts and tape requested ahead from the state that is then
    overwritten -- Z, qq, alpha, and here the generations and selfing rates too"""
    c = cv.INPUTS["n60"]
    h, o = _hip("n60", sched), _orc("n60", sched)
    st = cv.converged_state(c.N, c.K, c.Ktrue, c.a0, c.mode, generation=np.full(c.N, 3, dtype=np.int32), self_rates=np.linspace(0.1, 0.9, c.K))
    pos = ["seeds"] if sched == capi.SCHED_REPLAY else []
    for rep in range(2):
        h.run(2)
        o.iteration(); o.iteration()
        _same(h, o, ALL + pos, ("before", rep))
        cv.inject(h, st)
        cv.inject(o, st)
        _same(h, o, ["z", "qq", "generation", "alpha", "self_rates"] + pos, ("written", rep))
    h.run(2)
    o.iteration(); o.iteration()
    _same(h, o, ALL + pos, "after")
    assert o.error() == 0
    h.close()


# ---- b. every update_ZQ path of the replay schedule (the ladder of test_gpu_parity's kernel-variant test)
_S0 = {"INSTRUCT_ZQ_SPEC_RESOLVE": "0"}
_R0 = dict(_S0, INSTRUCT_ZQ_RESOLVE="0")
_P0 = dict(_S0, INSTRUCT_ZQ_RESOLVE_PERSIST="0")
LADDER = [{}, _S0, dict(_S0, INSTRUCT_ZQ_RESOLVE_UNITS="16"), dict(_S0, INSTRUCT_ZQ_RESOLVE_A="0.6"), dict(_S0, INSTRUCT_ZQ_RESOLVE_A="12"),
          _P0, dict(_P0, INSTRUCT_ZQ_RESOLVE_UNITS="16"), dict(_P0, INSTRUCT_ZQ_RESOLVE_A="0.6"), dict(_P0, INSTRUCT_ZQ_RESOLVE_A="12"),
          _R0, dict(_R0, INSTRUCT_ZQ_PIPE="0"),
          dict(_R0, INSTRUCT_ZQ_PIPE_XCD="0"), dict(_R0, INSTRUCT_ZQ_SPEC="0"), dict(_R0, INSTRUCT_ZQ_XCD="1"),
          dict(_R0, INSTRUCT_ZQ_SPEC="0", INSTRUCT_ZQ_XCD="1"), dict(_R0, INSTRUCT_ZQ_COOP="0"),
          {"INSTRUCT_P_DEVICE": "0"}, {"INSTRUCT_LL_INT": "0"}, {"INSTRUCT_LL_TABLES": "0"},
          {"INSTRUCT_P_DEVICE": "0", "INSTRUCT_HOST_TAPE": "0"}]


def _envid(env):
    return ",".join("%s=%s" % (k.replace("INSTRUCT_", ""), v) for k, v in sorted(env.items())) or "default"


@pytest.fixture(scope="module")
def three_iterations():
    """the canonical oracle's state after each of 3 iterations from a named input's converged state, replay schedule: computed once per
    input and shared by the cases of the ladder (nobody writes into it)"""
    memo = {}

    def get(name):
        if name not in memo:
            o = _orc(name)
            memo[name] = _trajectory(o, 3)
        return memo[name]
    return get


class _Snap:
    """a frozen copy of a chain's state with the getters' names"""
    def __init__(self, ch):
        for n in ALL + ["seeds"]:
            v = getattr(ch, n)()
            v = np.array(v) if isinstance(v, np.ndarray) else v
            setattr(self, n, lambda v=v: v)


def _trajectory(o, iters):
    out = []
    for _ in range(iters):
        o.iteration()
        out.append(_Snap(o))
    assert o.error() == 0
    return out


@pytest.mark.parametrize("env", LADDER, ids=_envid)
@pytest.mark.parametrize("name", ["n60", "n150", "m1", "passes"])
def test_replay_zq_paths_bit_exact(name, env, monkeypatch, three_iterations):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = three_iterations(name)
    h = _hip(name)
    for it in range(3):
        h.iteration()
        _same(h, want[it], ALL + ["seeds"], (_envid(env), it))
    sp, rs, pd, fb = _stats(h)
    K = cv.INPUTS[name].K
    assert fb == 0, fb   # (nothing was redone by the single-workgroup kernel behind the path under test)
    if "INSTRUCT_ZQ_SPEC_RESOLVE" in env:
        assert sp["tried"] == 0, sp
        if "INSTRUCT_ZQ_RESOLVE" in env:
            assert rs["blocks"] == 0 and rs["launches"] == 0, rs     # no block resolver either: the chain kernels
        elif K <= 8:
            assert rs["blocks"] >= 1, rs                             # (the block resolver exists up to K = 8)
    if "INSTRUCT_P_DEVICE" in env:
        assert pd["device_sweeps"] == 0, pd
    h.close()


# ---- the float pre-filters' own guard: sums q f at the lower end of the float range
@pytest.mark.parametrize("name,env,sched", [("n60", {}, capi.SCHED_REPLAY), ("n60", {}, capi.SCHED_KEYED), ("n60", _S0, capi.SCHED_REPLAY),
                                            ("n60", _R0, capi.SCHED_REPLAY), ("m1", {}, capi.SCHED_REPLAY), ("big5", {}, capi.SCHED_REPLAY)],
                         ids=lambda v: _envid(v) if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("exp", [120, 135, 142])
def test_row_sums_at_the_end_of_the_float_range_go_to_the_exact_path(exp, name, env, sched, monkeypatch):
    """In a chain's own states a row of qq sums to 1, and the sum of q f over the clusters -- the pre-filters' `run` -- stays an ordinary
    float however small the other entries are: the `run > 1e-30f` guards never bind there (with those terms taken out of a scratch build
    every other test of this module still passes).  A Z draw depends on the ratios within the row only, and the setter takes any row,
    so the rows are scaled by a power of two (exact in double):
      2^-120: the largest entry (7.5e-37) is a normal float, the others (7.5e-40) are subnormal;
      2^-135: the largest entry is 16000 units of the smallest subnormal, the others 16: the products q f are a handful of units each,
              thresholds compared in float are off by more than the guard band of 6e-6 `run` (a hundredth of a unit), and only the
              `run > 1e-30f` term sends these draws to the double path -- without it the n60 and big5 cases here fail;
      2^-142: the largest entry is a float subnormal with 7 bits, the others are 0 in float.
    Every draw of the first update_ZQ has to come out as the oracle's (K <= 8: bucket_f32; above: bucket_from_cum; the block
    resolver's minrun; the interval resolver's probes); after it qq is a Dirichlet draw again.  (Where a resolver is in front, that first
    sweep ends with the single-workgroup kernel -- zq_fallbacks() is 1 -- which is as good an answer as any: only the state is asserted.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = cv.state_of(name)
    st = st._replace(qq=st.qq * 2.0 ** -exp)
    big, small = np.float32(st.qq.max()), np.float32(st.qq.min())
    assert (1.2e-38 < big < 1e-30 and 0 < small < 1.2e-38) if exp == 120 else (0 < big < 1.2e-38 and (small == 0 or exp == 135))
    c = cv.INPUTS[name]
    geno, an, mi = cv.data(name)
    h = capi.HipChain(geno, an, mi, c.K, mode=c.mode, rng_sched=sched)
    o = orc.OrcChain(geno, an, mi, c.K, mode=c.mode, math=orc.MATH_ISG, accum=orc.ACC_EXACT, sched=sched)
    for ch in (h, o):
        ch.setseeds(13, 4, 1972)
        ch.chain_init(np.array([ch.ran1() for _ in range(c.K)], dtype=np.float32))
        cv.inject(ch, st)
    _sweeps(h, o, c.mode, 2, sched)
    h.close()


# ---- c. the block resolver's instance of every K
@pytest.mark.parametrize("persist", ["1", "0"])
@pytest.mark.parametrize("K", cv.BLOCK_K)
def test_replay_block_resolver_every_K_bit_exact(K, persist, monkeypatch):
    monkeypatch.setenv("INSTRUCT_ZQ_RESOLVE_PERSIST", persist)
    monkeypatch.setenv("INSTRUCT_ZQ_SPEC_RESOLVE", "0")
    name = "blk%d" % K
    h, o = _hip(name), _orc(name)
    for it in range(3):
        h.iteration()
        o.iteration()
        _same(h, o, ALL + ["seeds"], it)
    sp, rs, pd, fb = _stats(h)
    assert fb == 0 and sp["tried"] == 0 and rs["blocks"] >= 1 and (rs["launches"] == 1) == (persist == "1"), (fb, sp, rs)
    h.close()


# ---- d. wide K
@pytest.mark.parametrize("sched", [capi.SCHED_REPLAY, capi.SCHED_KEYED])
@pytest.mark.parametrize("name", ["k40", "k64"])
def test_wide_K_every_sweep_bit_exact(name, sched):
    h, o = _hip(name, sched), _orc(name, sched)
    _sweeps(h, o, 2, 3, sched)
    assert h.zq_fallbacks() == 0
    h.close()


def test_wide_K_forced_fallbacks_bit_exact(monkeypatch):
    """no interval resolver, no block resolver, no cooperative kernel: the single-workgroup chain form of the wide k_zq"""
    for k in ("INSTRUCT_ZQ_SPEC_RESOLVE", "INSTRUCT_ZQ_RESOLVE", "INSTRUCT_ZQ_COOP"):
        monkeypatch.setenv(k, "0")
    h, o = _hip("k64"), _orc("k64")
    for it in range(3):
        h.iteration()
        o.iteration()
        _same(h, o, ALL + ["seeds"], it)
    sp, rs, pd, fb = _stats(h)
    assert sp["tried"] == 0 and rs["blocks"] == 0, (sp, rs)
    h.close()


# ---- e. where the interval resolver engages; f. a lost sweep under launch-ahead (on `passes`, whose sweeps settle)
# What the routes of isg_spec_hip.inc do from these states (MI355X, the statistics after each run(1)); every route is asserted once below.
#   big5, default and under WALK_K=1.0 / ROUNDS=0 / BAND=0 / SEG=256: every sweep the resolver tries misses a window (fail bit 1), is
#   tried `again` with wider windows, misses again and is lost; it sits out 1, then 2 sweeps: tried = lost = retried = 1, 2, 2, 3.  The block
#   resolver behind it takes the sweep with 14, 6, 7, 1 of its 15, 12, 13, 11 blocks missed.  WALK_K=1.0 also sends 2 of update_P's 4 sweeps
#   to the host loop.
#   big5, KSIG=1.0: the first sweep still has uncertain bytes on its path after the 2 blind and 12 extra rounds (4982 probes, fail bit 64).
#   big10, KSIG=1.0 (with or without ROUNDS=0): the first sweep settles in the extra rounds (9 rounds, 774 probes > 2 N: two sweeps sat out).
@pytest.fixture(scope="module")
def big5_ref():
    return _trajectory(_orc("big5"), 4)


@pytest.fixture(scope="module")
def big10_ref():
    return _trajectory(_orc("big10"), 4)


def _run_by_one(h, want, tag):
    """run(1) (launch-ahead is live inside run) against the oracle's trajectory; the statistics after every iteration"""
    per = []
    for it in range(len(want)):
        h.run(1)
        _same(h, want[it], ALL + ["seeds"], (tag, it))
        per.append(_stats(h, "%s it=%d" % (tag, it)))
    return per


def test_interval_resolver_default_path_big5(big5_ref, monkeypatch):
    monkeypatch.delenv("INSTRUCT_ZQ_SPEC_TEST_ABORT", raising=False)
    h = _hip("big5")
    per = _run_by_one(h, big5_ref, "e big5 default")
    sp, rs, pd, fb = per[-1]
    assert sp["tried"] >= 1 and pd["device_sweeps"] >= 1, (sp, pd)
    assert sp["lost"] >= 1 and sp["lost_fail_bits"] != 0, sp       # a natural loss (nothing forces it)
    assert sp["retried"] >= 1, sp                                  # ... after the `again` route with wider windows
    assert sp["tried"] < len(per), sp                              # the cooldown: sweeps sat out after losses in a row
    sp0, rs0 = per[0][0], per[0][1]
    assert sp0["lost"] == 1 and rs0["misses"] >= 1, (sp0, rs0)     # the block resolver took the lost sweep, with blocks of its own missed
    assert fb == 0
    h.close()


def test_interval_resolver_default_path_big10(big10_ref):
    h = _hip("big10")
    sp, rs, pd, fb = _run_by_one(h, big10_ref, "e big10 default")[-1]
    assert sp["tried"] >= 1 and rs["blocks"] == 0, (sp, rs)   # (no block resolver behind K = 10: a lost sweep goes to the chain kernels)
    h.close()


@pytest.mark.parametrize("knob", ["INSTRUCT_WALK_K=1.0", "INSTRUCT_ZQ_SPEC_ROUNDS=0", "INSTRUCT_ZQ_SPEC_KSIG=1.0", "INSTRUCT_ZQ_SPEC_BAND=0",
                                  "INSTRUCT_ZQ_SPEC_SEG=256"])
def test_interval_resolver_knobs_big5(knob, big5_ref, monkeypatch):
    monkeypatch.setenv(*knob.split("="))
    h = _hip("big5")
    per = _run_by_one(h, big5_ref, "e big5 " + knob)
    sp, rs, pd, fb = per[-1]
    assert sp["tried"] >= 1, sp
    if knob == "INSTRUCT_ZQ_SPEC_KSIG=1.0":
        assert sp["lost_fail_bits"] & (32 | 64), sp                # uncertain bytes left after every round
        assert per[0][0]["rounds"] > 2, per[0][0]                  # (the rounds with a look each ran)
    if knob == "INSTRUCT_WALK_K=1.0":
        assert pd["host_sweeps"] >= 1 and pd["device_sweeps"] >= 1, pd   # update_P's windows are missed too: its host loop redoes the sweep
    h.close()


def test_interval_resolver_settles_in_the_extra_rounds_big10(big10_ref, monkeypatch):
    """no blind rounds, narrow shape intervals: the sweep is settled by the rounds that look each time"""
    monkeypatch.setenv("INSTRUCT_ZQ_SPEC_ROUNDS", "0")
    monkeypatch.setenv("INSTRUCT_ZQ_SPEC_KSIG", "1.0")
    h = _hip("big10")
    per = _run_by_one(h, big10_ref, "e big10 ROUNDS=0,KSIG=1.0")
    sp0 = per[0][0]
    assert sp0["settled"] == 1 and sp0["rounds"] > 0 and sp0["probes"] > 0, sp0
    h.close()


@pytest.mark.parametrize("n", [1, 2])
def test_lost_sweep_under_launch_ahead_discards_the_early_likelihood(n, three_iterations, monkeypatch):
    """A sweep the interval resolver settles in its blind rounds has written Z (k_zq_at ran) when the host looks, and cal_lkh's sweep is
    enqueued early behind it.  INSTRUCT_ZQ_SPEC_TEST_ABORT=n declares the n-th call of the resolver lost after the fact (n counts calls,
    a retry with wider windows included): qq is restored, the block resolver redoes the sweep from the same stream position, and the
    likelihood taken early -- from the Z that is overwritten -- must not be what totallkh reports.
    big5's sweeps cannot show this: every one of them is lost on its own before k_zq_at writes anything (see above).  The sweeps of
    `passes` (N = 6, L = 40000 -> K = 3) settle with at most one round of probes and no retry (tried = settled = 3 over 3 iterations
    when nothing is aborted), so call n is iteration n's sweep, and the statistics below say that it would have settled.
    What this does and does not check: the state, the stream position and totallkh after the rollback and the redo are the oracle's.
    A sweep that is forced to lose had resolved the right positions, so the Z and qq the block resolver writes again are the ones
    k_zq_at wrote: a likelihood kept from the early sweep would have the same bits (a scratch build that keeps it passes this test).
    Telling the two apart needs a sweep that writes a WRONG Z and is then lost on its own (fail bit 32), which no documented switch
    produces within a test's length."""
    monkeypatch.setenv("INSTRUCT_ZQ_SPEC_TEST_ABORT", str(n))
    h = _hip("passes")
    per = _run_by_one(h, three_iterations("passes"), "f passes TEST_ABORT=%d" % n)
    for it, (sp, rs, pd, fb) in enumerate(per):
        lost = 1 if it + 1 >= n else 0
        assert sp["tried"] == it + 1 and sp["lost"] == lost and sp["settled"] == it + 1 - lost and sp["retried"] == 0, (it, sp)
        assert sp["lost_fail_bits"] == 0 and fb == 0, (it, sp, fb)   # the one loss is the forced one: the sweep itself had no fail bit
    sp, rs = per[n - 1][0], per[n - 1][1]
    assert sp["fail_bits"] == 0 and sp["rounds"] <= 2 and rs["blocks"] >= 1, (sp, rs)   # settled blind; the block resolver took it over
    h.close()
