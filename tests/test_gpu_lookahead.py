"""GPU (pytest -m gpu): isg_iteration's launch-ahead mode (DESIGN.md "Replay iteration: looks and launch-ahead") changes the order in which
independent kernels are enqueued around the host looks, and nothing else: a chain driven through run() leaves every state array and the
stream position bit for bit where the same chain driven sweep by sweep (which never launches ahead) leaves them -- with the switch on
and off, when a sweep is lost and its ahead results are discarded and redone, on the other update_P / update_ZQ paths, in the other
modes, on the keyed schedule, with getters and setters between the iterations, and from two threads at once."""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

from instruct_amd import capi, synth

pytestmark = pytest.mark.gpu

SWEEPS = {
    0: ("update_P", "update_Z", "cal_lkh"),
    1: ("update_P", "update_ZQ", "update_alpha", "cal_lkh"),
    2: ("update_P", "update_S_POP", "update_G", "update_ZQ", "update_alpha", "cal_lkh"),
    3: ("update_P", "update_S_IND", "update_G", "update_ZQ", "update_alpha", "cal_lkh"),
    4: ("update_P", "update_S_POP", "update_ZQ", "update_alpha", "cal_lkh"),
    5: ("update_P", "update_S_IND", "update_ZQ", "update_alpha", "cal_lkh"),
}
ARRAYS = ("z", "qq", "qqnum", "freq", "generation", "self_rates", "indvlkh")
MAIN = (400, 900, 5)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = capi.load()
    lib.isg_iter_advance.argtypes = [C.c_void_p]


def _chain(data, K, mode=2, sched=capi.SCHED_REPLAY, seeds=(13, 4, 1972)):
    geno, an, mi = data
    ch = capi.HipChain(geno, an, mi, K, mode=mode, type_freq=1, back_refl=1, rng_sched=sched)
    ch.setseeds(*seeds)
    ch.initd = np.array([ch.ran1() for _ in range(K)], dtype=np.float32)
    ch.chain_init(ch.initd)
    ch.mode = mode
    return ch


def _by_sweeps(ch, n=1):
    """the reference order: the public sweeps one by one, as the parity tests drive them"""
    for _ in range(n):
        for f in SWEEPS[ch.mode]:
            getattr(ch, f)()
        ch.lib.isg_iter_advance(ch.h)


def _state(ch):
    s = {name: getattr(ch, name)() for name in ARRAYS}
    s["alpha"], s["totallkh"], s["seeds"] = ch.alpha(), ch.totallkh(), tuple(ch.seeds())
    return s


def _same(a, b, tag):
    for name in ARRAYS:
        assert np.array_equal(a[name], b[name]), (tag, name)
    for name in ("alpha", "totallkh", "seeds"):
        assert a[name] == b[name] or (a[name] != a[name] and b[name] != b[name]), (tag, name, a[name], b[name])


@pytest.fixture(scope="module")
def main_data():
    N, L, K = MAIN
    return synth.make_diploid(N, L, K)


@pytest.fixture(scope="module")
def main_ref(main_data):
    """chain B of the main case: 30 iterations sweep by sweep; (totallkh, seeds) after every one, the whole state after some"""
    ch = _chain(main_data, MAIN[2])
    trace, snaps = [], {}
    for it in range(1, 31):
        _by_sweeps(ch)
        trace.append((ch.totallkh(), tuple(ch.seeds())))
        if it in (1, 2, 10, 30):
            snaps[it] = _state(ch)
    ch.close()
    return trace, snaps


def test_run_equals_sweep_by_sweep(main_data, main_ref):
    trace, snaps = main_ref
    a = _chain(main_data, MAIN[2])
    a.run(30)
    _same(_state(a), snaps[30], "run(30)")
    assert a.zq_spec_stats()["tried"] > 0 and a.p_device_stats()["device_sweeps"] > 0, (a.zq_spec_stats(), a.p_device_stats())
    a.close()
    b = _chain(main_data, MAIN[2])
    for it in range(30):
        b.run(1)
        assert (b.totallkh(), tuple(b.seeds())) == trace[it], it
    _same(_state(b), snaps[30], "30 x run(1)")
    b.close()


def test_switch_off_gives_the_same_chain(main_data, main_ref, monkeypatch):
    states = {}
    for v in ("0", "1"):
        monkeypatch.setenv("INSTRUCT_LOOKAHEAD", v)
        ch = _chain(main_data, MAIN[2])
        ch.run(30)
        states[v] = _state(ch)
        ch.close()
    _same(states["0"], states["1"], "INSTRUCT_LOOKAHEAD 0 / 1")
    _same(states["0"], main_ref[1][30], "INSTRUCT_LOOKAHEAD=0")


def test_lost_ZQ_sweep_discards_the_early_likelihood(main_data, main_ref, monkeypatch):
    monkeypatch.setenv("INSTRUCT_ZQ_SPEC_TEST_ABORT", "3")
    ch = _chain(main_data, MAIN[2])
    for it in range(30):
        ch.run(1)
        assert (ch.totallkh(), tuple(ch.seeds())) == main_ref[0][it], it
    assert ch.zq_spec_stats()["lost"] >= 1 and ch.zq_spec_stats()["tried"] > 0, ch.zq_spec_stats()
    _same(_state(ch), main_ref[1][30], "lost update_ZQ")
    ch.close()


def test_lost_P_sweep_redoes_the_frequency_copies(main_data, main_ref, monkeypatch):
    monkeypatch.setenv("INSTRUCT_P_TEST_ABORT", "2")
    ch = _chain(main_data, MAIN[2])
    for it in range(30):
        ch.run(1)
        assert (ch.totallkh(), tuple(ch.seeds())) == main_ref[0][it], it
    st = ch.p_device_stats()
    assert st["host_sweeps"] >= 1 and st["device_sweeps"] > 0, st
    _same(_state(ch), main_ref[1][30], "lost update_P")
    ch.close()


@pytest.mark.parametrize("env", ["INSTRUCT_P_DEVICE", "INSTRUCT_ZQ_SPEC_RESOLVE"])
def test_other_paths(main_data, main_ref, monkeypatch, env):
    """update_P's host loop with its own ahead request; update_ZQ by the block resolver"""
    monkeypatch.setenv(env, "0")
    ch = _chain(main_data, MAIN[2])
    ch.run(10)
    if env == "INSTRUCT_P_DEVICE":
        assert ch.p_device_stats()["device_sweeps"] == 0
    else:
        assert ch.zq_spec_stats()["tried"] == 0
    _same(_state(ch), main_ref[1][10], env)
    ch.close()


def test_ragged_shape_with_missing_data():
    """L = 301 (padded to 304), K = 3, 10 % missing: the ranks of the used loci come from the table"""
    data = synth.code_diploid(synth.raw_alleles(200, 301, 3, 2, 2, 0.10, 7))
    a, b = _chain(data, 3), _chain(data, 3)
    a.run(20)
    _by_sweeps(b, 20)
    _same(_state(a), _state(b), "ragged")
    assert a.p_device_stats()["device_sweeps"] > 0
    a.close()
    b.close()


@pytest.mark.parametrize("mode", [0, 1, 3, 4, 5])
def test_small_chain_in_the_other_modes(mode):
    data = synth.code_diploid(synth.raw_alleles(64, 100, 5, 2, 2, 0.0, 7))
    a, b = _chain(data, 5, mode=mode), _chain(data, 5, mode=mode)
    a.run(5)
    _by_sweeps(b, 5)
    _same(_state(a), _state(b), ("mode", mode))
    a.close()
    b.close()


def test_keyed_schedule(main_data):
    a, b = _chain(main_data, MAIN[2], sched=capi.SCHED_KEYED), _chain(main_data, MAIN[2], sched=capi.SCHED_KEYED)
    a.run(20)
    _by_sweeps(b, 20)
    _same(_state(a), _state(b), "keyed")
    a.close()
    b.close()


@pytest.mark.parametrize("getter", ["seeds", "alpha", "totallkh", "qq"])
def test_getter_first_after_run(main_data, main_ref, getter):
    ch = _chain(main_data, MAIN[2])
    ch.run(1)
    got = getattr(ch, getter)()
    want = main_ref[1][1][getter]
    assert np.array_equal(np.asarray(got), np.asarray(want)), getter
    _same(_state(ch), main_ref[1][1], getter)
    ch.run(1)
    _same(_state(ch), main_ref[1][2], getter + ", next iteration")
    ch.close()


@pytest.mark.parametrize("writer", ["set_z", "chain_init"])
def test_writer_of_Z_after_run_drops_the_counts_taken_ahead(main_data, writer):
    a, b = _chain(main_data, MAIN[2]), _chain(main_data, MAIN[2])
    a.run(1)
    _by_sweeps(b)
    for ch in (a, b):
        if writer == "set_z":
            z = ch.z()
            ch.set_z(np.ascontiguousarray(np.where(z >= 0, (z + 1) % MAIN[2], z)))
        else:
            ch.chain_init(ch.initd)
    a.run(1)
    _by_sweeps(b)
    _same(_state(a), _state(b), writer)
    a.close()
    b.close()


def test_two_chains_from_two_threads():
    data = synth.make_diploid(200, 300, 5)
    seeds = [(13, 4, 1972), (101, 202, 303)]
    want = []
    for s in seeds:
        ch = _chain(data, 5, seeds=s)
        ch.run(10)
        want.append(_state(ch))
        ch.close()
    chains = [_chain(data, 5, seeds=s) for s in seeds]
    errors = []

    def work(ch):
        try:
            ch.run(10)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(ch,)) for ch in chains]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, ch in enumerate(chains):
        _same(_state(ch), want[k], ("thread", k))
        ch.close()


def test_mailbox_goes_with_the_context(main_data):
    gc.collect()
    live = capi.live_buffers()
    ch = _chain(main_data, MAIN[2])
    assert capi.live_buffers() > live
    ch.run(3)
    ch.close()
    assert capi.live_buffers() == live
