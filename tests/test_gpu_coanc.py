"""GPU (pytest -m gpu): the posterior co-ancestry matrix accumulated on the device (isg_coanc_*, DESIGN.md "Posterior co-ancestry").

Exact data first: rows of Q made of multiples of 1/64, so every product is a multiple of 2^-12 and every sum of at most 7 * 64 of
them is exact in double whatever the order -- a misplaced row or column of the f64 matrix instruction's result cannot hide behind a
tolerance.  The library returns sum / steps; `(x / 7) * 7 == x` does NOT hold for every such x (1166 of the multiples of 2^-12 up to 7
fail it), so the exact tests compare the returned mean with `exact sum / steps`, the same one division in double: distinct sums
give distinct quotients, so this is the bit-for-bit statement about the sum.  Then running chains against the canonical oracle with
the derived bound 2 n 2^-53 max(1, sum), n = steps (Kp + 1); mode 0; both tetraploid kinds; the life cycle; the drop-in."""
import glob
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import orc
from instruct_amd import capi, coanc, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
# every N and every K of the two lists at least once; 130 = three tiles, 63 / 64 / 65 the tile edge, K = 33 and 64 the wide contexts
EXACT_SHAPES = [(1, 1), (16, 2), (17, 3), (63, 4), (64, 5), (65, 8), (130, 33), (130, 64), (17, 64), (65, 1)]
SNAPS = 7


@pytest.fixture(scope="module", autouse=True)
def _libs():
    orc.build()
    capi.load()


def _exact_q(N, K, s):
    """[N][K] multiples of 1/64, rows summing to 1; weights fall with k (no symmetry under reversing k) and move with the row"""
    rng = np.random.default_rng(1000 * N + 10 * K + s)
    w = 1.0 / (1.0 + np.arange(K))
    q = np.empty((N, K))
    for i in range(N):
        p = np.roll(w, i % K) * rng.random(K)
        q[i] = rng.multinomial(64, p / p.sum()) / 64.0
    assert np.array_equal(q.sum(axis=1), np.ones(N))
    return q


def _chain(N, K, sched=capi.SCHED_REPLAY):
    geno, an, mi = synth.make_diploid(N, 40, K)
    h = capi.HipChain(geno, an, mi, K, rng_sched=sched)
    h.setseeds(13, 4, 1972)
    h.chain_init(np.array([h.ran1() for _ in range(K)], dtype=np.float32))
    return h


def _kp(K):
    return (K + 3) // 4 * 4


def _tol_sum(steps, K, expected_sum):
    """a sum of n non-negative doubles in any order is within (n - 1) u of the exact sum, relative; doubled because the
    reference sum is rounded too; n = steps (Kp + 1) covers the products' own roundings and the division / multiplication by steps"""
    return 2 * steps * (_kp(K) + 1) * U * np.maximum(1.0, expected_sum)


@pytest.mark.parametrize("batch", [1, 3, 0])
@pytest.mark.parametrize("N,K", EXACT_SHAPES)
def test_exact_data_bit_for_bit(N, K, batch):
    h = _chain(N, K)
    qs = [_exact_q(N, K, s) for s in range(SNAPS)]
    if K >= 3 and N >= 16:
        assert not np.array_equal(qs[0], qs[0][::-1]) and not np.array_equal(qs[0], qs[0][:, ::-1])
        assert not np.array_equal(qs[0] @ qs[0].T, (qs[0] @ qs[0].T)[::-1, ::-1])
    sums = np.cumsum([q @ q.T for q in qs], axis=0)  # exact: multiples of 2^-12 below 2^3
    assert np.array_equal(sums[-1] * 4096, np.rint(sums[-1] * 4096))
    h.coanc_begin(batch)
    for s, q in enumerate(qs):
        h.set_qq(q)
        h.coanc_step()
        if s == 3:  # mid-run: with batch 3 one snapshot is held, unflushed
            mean4, steps4 = h.coanc_fetch()
            assert steps4 == 4
            assert np.array_equal(mean4, sums[3] / 4.0), np.argwhere(mean4 != sums[3] / 4.0)[:8]
            assert np.array_equal(mean4 * 4, sums[3])
    mean, steps = h.coanc_fetch()
    assert steps == SNAPS
    want = sums[-1] / float(SNAPS)
    assert np.array_equal(mean, want), np.argwhere(mean != want)[:8]
    assert np.array_equal(np.rint(mean * steps * 4096) / 4096, sums[-1])
    assert np.array_equal(mean, mean.T)
    again, steps2 = h.coanc_fetch()
    assert steps2 == SNAPS and again.tobytes() == mean.tobytes()
    assert np.array_equal(h.qq(), qs[-1])  # the uploaded state is untouched
    h.coanc_end()
    h.close()


def test_same_calls_same_bits_on_inexact_data():
    """two runs of the same calls: the same bits (nothing else is promised about the order of the additions)"""
    out = []
    for _ in range(2):
        h = _chain(130, 5)
        h.coanc_begin(3)
        for _ in range(4):
            h.iteration()
            h.coanc_step()
        out.append(h.coanc_fetch()[0].tobytes())
        h.close()
    assert out[0] == out[1]


def _pair(geno, an, mi, K, sched, mode=2):
    h = capi.HipChain(geno, an, mi, K, mode=mode, rng_sched=sched)
    o = orc.OrcChain(geno, an, mi, K, mode=mode, math=orc.MATH_ISG, accum=orc.ACC_EXACT, sched=sched)
    h.setseeds(13, 4, 1972)
    o.setseeds(13, 4, 1972)
    initd = np.array([h.ran1() for _ in range(K)], dtype=np.float32)
    assert np.array_equal(initd, np.array([o.ran1() for _ in range(K)], dtype=np.float32))
    h.chain_init(initd)
    o.chain_init(initd)
    return h, o


@pytest.fixture(scope="module", params=[(3, capi.SCHED_REPLAY), (3, capi.SCHED_KEYED), (40, capi.SCHED_REPLAY), (40, capi.SCHED_KEYED)],
                ids=["K3-replay", "K3-keyed", "K40-replay", "K40-keyed"])
def running(request):
    """N = 70, L = 200: 6 iterations of twin chains, a step after each, batch 4 (one full flush, one partial at the fetch)"""
    K, sched = request.param
    geno, an, mi = synth.make_diploid(70, 200, K)
    h, o = _pair(geno, an, mi, K, sched)
    h.coanc_begin(4)
    want = np.zeros((70, 70))
    for _ in range(6):
        h.iteration()
        o.iteration()
        h.coanc_step()
        q = o.qq()
        want += q @ q.T
    mean, steps = h.coanc_fetch()
    state = {"qq": (h.qq(), np.array(o.qq())), "seeds": (h.seeds(), o.seeds())}  # a copy: the oracle's arrays go with the oracle
    assert o.error() == 0
    h.close()
    return K, sched, mean, steps, want, state


def test_running_chain_against_the_oracle(running):
    K, sched, mean, steps, want, state = running
    assert steps == 6
    err = np.abs(mean * steps - want)
    tol = _tol_sum(6, K, want)
    print("K %d sched %d: max error of the sum %.3e, smallest bound %.3e" % (K, sched, err.max(), tol.min()))
    assert np.all(err <= tol), (err.max(), tol.min())
    assert np.array_equal(mean, mean.T)
    # accumulating has not disturbed the chain
    assert np.array_equal(*state["qq"])
    if sched == capi.SCHED_REPLAY:
        assert state["seeds"][0] == state["seeds"][1]


def _invariants(mean, K, tol):
    assert mean.min() >= 0.0 and mean.max() <= 1.0, (mean.min(), mean.max())
    d = np.diag(mean)
    assert np.all(d >= 1.0 / K - tol), d.min()
    assert np.all(mean ** 2 <= np.outer(d, d) + tol)


def test_invariants_of_the_running_chain(running):
    K, _, mean, steps, _, _ = running
    _invariants(mean, K, 2 * steps * (_kp(K) + 1) * U)


def test_mode_0_counts_the_steps_two_individuals_share_a_cluster():
    N, L, K, iters = 60, 100, 4, 5
    geno, an, mi = synth.make_diploid(N, L, K)
    h = capi.HipChain(geno, an, mi, K, mode=0)
    h.setseeds(13, 4, 1972)
    h.chain_init(np.array([h.ran1() for _ in range(K)], dtype=np.float32))
    h.coanc_begin(2)
    count = np.zeros((N, N))
    for _ in range(iters):
        h.iteration()
        h.coanc_step()
        g = h.generation()
        count += g[:, None] == g[None, :]
    mean, steps = h.coanc_fetch()
    assert steps == iters
    assert np.array_equal(mean, count / float(iters))
    assert np.array_equal(mean * steps, count)  # x / 5 * 5 == x for these integers
    assert np.array_equal(np.diag(mean), np.ones(N))
    # an uploaded assignment is what the next step sees
    g = (np.arange(N, dtype=np.int32) * 7) % K
    h.coanc_begin(0)
    h.set_generation(g)
    h.coanc_step()
    mean, steps = h.coanc_fetch()
    assert steps == 1 and np.array_equal(mean, (g[:, None] == g[None, :]).astype(np.float64))
    h.close()


@pytest.mark.parametrize("name,allo", [("t1", False), ("ta1", True)])
def test_ploidy_4_against_the_chains_own_qq(name, allo):
    cases = gu.make_golden.ALLO_CASES if allo else gu.make_golden.POLY_CASES
    N, L, K = cases[name][:3]
    raw = gu.make_golden.allo_data_for(name) if allo else gu.make_golden.poly_data_for(name)
    obs, alleleid, allelenum = synth.code_tetraploid(raw)
    ch = capi.HipPolyChain(obs, alleleid, allelenum, K, allo=allo)
    ch.setseeds(13, 4, 1972)
    ch.chain_init(np.array([np.float32(ch.ran1()) for _ in range(K)], dtype=np.float32))
    ch.coanc_begin(2)
    want = np.zeros((N, N))
    for _ in range(3):
        ch.iteration()
        ch.coanc_step()
        q = ch.qq()
        want += q @ q.T
    mean, steps = ch.coanc_fetch()
    assert steps == 3 and mean.shape == (N, N)
    assert np.all(np.abs(mean * steps - want) <= _tol_sum(3, K, want))
    _invariants(mean, K, 2 * 3 * (_kp(K) + 1) * U)
    ch.close()


def test_lifecycle_messages_reset_and_buffers():
    live0 = capi.live_buffers()
    h = _chain(17, 3)
    live_ctx = capi.live_buffers()
    with pytest.raises(capi.IsgError, match="isg_coanc_step: isg_coanc_begin first"):
        h.coanc_step()
    with pytest.raises(capi.IsgError, match="isg_coanc_fetch: isg_coanc_begin first"):
        h.coanc_fetch()
    h.coanc_begin(2)
    assert capi.live_buffers() == live_ctx + 2
    with pytest.raises(capi.IsgError, match="isg_coanc_fetch: no step"):
        h.coanc_fetch()
    q1, q2 = _exact_q(17, 3, 1), _exact_q(17, 3, 2)
    for q in (q1, q1, q2):
        h.set_qq(q)
        h.coanc_step()
    assert h.coanc_fetch()[1] == 3
    h.coanc_begin(5)  # a second begin starts from zero
    assert capi.live_buffers() == live_ctx + 2
    with pytest.raises(capi.IsgError, match="no step"):
        h.coanc_fetch()
    h.set_qq(q2)
    h.coanc_step()
    mean, steps = h.coanc_fetch()
    assert steps == 1 and np.array_equal(mean, q2 @ q2.T)
    with pytest.raises(capi.IsgError, match="batch"):
        h.coanc_begin(-1)
    h.coanc_end()
    assert capi.live_buffers() == live_ctx
    with pytest.raises(capi.IsgError, match="isg_coanc_begin first"):
        h.coanc_step()
    h.coanc_begin()
    h.coanc_step()
    assert capi.live_buffers() == live_ctx + 2
    h.close()  # without coanc_end
    assert capi.live_buffers() == live0


def test_flush_and_snapshot_are_profiled_under_their_names():
    h = _chain(65, 5)
    h.profile(True)
    h.coanc_begin(2)
    for _ in range(5):
        h.coanc_step()
    h.coanc_fetch()
    res = h.profile_results()
    assert res["k_coanc_snap"][1] == 5 and res["k_coanc_syrk"][1] == 3, res
    h.close()


def _body(path):
    return [l for l in open(path, "rb").read().split(b"\n")
            if not (l.strip().startswith((b"Data File:", b"Output File:")) or b"InStruct" in l and b"-d" in l)]


C1_CLI = ["-K", "3", "-L", "100", "-N", "50", "-p", "2", "-u", "200", "-b", "100", "-t", "10", "-c", "2", "-v", "2", "-g", "1", "-r", "5", "-j", "5",
          "-lb", "0", "-a", "0", "-s", "13", "4", "1972", "-pi", "0", "-pf", "1"]


SWITCH = b"INSTRUCT_COANC_OUT"


@pytest.fixture(scope="module")
def dropin_exe(tmp_path_factory):
    """oracle/_ref/InStruct_hip when it was built from this tree's instruct_amd/host/mcmc_hip.c (it names the switch).  A
    binary left from another revision of the shim -- oracle/_ref is built where the reference sources are and travels from there,
    and it runs to the end and writes the same result file, it just never looks at the variable -- is not the drop-in under test: the
    shim is then compiled from this tree and linked against the same oracle/_ref/libref_driver.a, which holds the reference driver
    with its main, by the recipe of oracle/Makefile's InStruct_hip rule."""
    exe = os.path.join(ROOT, "oracle", "_ref", "InStruct_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/InStruct_hip not built (needs the reference objects; built in the dev container)")
    with open(exe, "rb") as f:
        if SWITCH in f.read():
            return exe
    drv = os.path.join(ROOT, "oracle", "_ref", "libref_driver.a")
    assert os.path.exists(drv), "oracle/_ref/InStruct_hip predates this tree's mcmc_hip.c and oracle/_ref/libref_driver.a is not there to link a current one"
    d = tmp_path_factory.mktemp("dropin")
    obj, exe, pkg = str(d / "mcmc_hip.o"), str(d / "InStruct_hip"), os.path.join(ROOT, "instruct_amd")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(pkg, "host", "mcmc_hip.c"), "-o", obj])
    subprocess.check_call(["gcc", "-o", exe, obj, drv, "-L" + pkg, "-linstruct_hip", "-Wl,-rpath," + pkg, "-lm"])
    return exe


@pytest.mark.parametrize("which", ["mode2", "mode0"])
def test_dropin_writes_one_file_per_finished_chain_and_the_same_result_file(which, tmp_path, dropin_exe):
    exe = dropin_exe
    cli, golden = {"mode2": (C1_CLI, "c1_cli_output.txt"), "mode0": (gu.make_golden.MODE0_CLI, "c1_mode0_cli_output.txt")}[which]
    out = tmp_path / "out.txt"
    prefix = str(tmp_path / "co")
    log = subprocess.run([exe, "-d", os.path.join(gu.GOLDEN, "c1.txt"), "-o", str(out)] + cli, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         timeout=600, env=dict(os.environ, INSTRUCT_COANC_OUT=prefix))
    assert log.returncode == 0 and b"THE JOB IS SUCCESSFULLY FINISHED" in log.stdout, log.stdout[-2000:]
    assert _body(str(out)) == _body(os.path.join(gu.GOLDEN, golden))
    assert b"coanc" not in log.stdout.replace(prefix.encode(), b"")
    finished = [c for c in (1, 2) if b"Chain %d has an empty cluster" % c not in log.stdout]
    files = sorted(glob.glob(prefix + ".chain*.coanc"))
    assert files == [prefix + ".chain%d.coanc" % c for c in finished] and finished, (exe, sorted(os.listdir(str(tmp_path))), log.stdout[-1500:])
    tol = 2 * 10 * (4 + 1) * U
    mats = []
    for f in files:
        mean, steps = coanc.read(f)
        assert mean.shape == (50, 50) and steps == 10  # -u 200 -b 100 -t 10
        _invariants(mean, 3, tol)
        if which == "mode0":
            assert np.array_equal(mean * steps, np.rint(mean * steps)) and np.array_equal(np.diag(mean), np.ones(50))
        mats.append((mean, steps))
    both, total = coanc.combine(mats)
    assert total == 10 * len(mats)
    _invariants(both, 3, tol)
