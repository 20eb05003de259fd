"""GPU: every device and pinned host allocation of a context is gone when the context is.  isg_diag_live_buffers() counts the live
allocations of the library (instruct_amd/csrc/isg_devbuf.h owns all of them): for each kind of context -- each with the buffers only it
has -- the count after create / run / destroy is exactly the count before.  A condition, not a measurement."""
import gc

import numpy as np
import pytest

import golden_util  # noqa: F401  (puts tests/golden on the path)
import make_golden_alleles as mga
from instruct_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_chain_pending():
    gc.collect()  # a chain some earlier test left to the collector is destroyed now, not between two readings of the counter


def _diploid(N=50, L=100, K=3, nall=2):
    return synth.code_diploid(synth.raw_alleles(N, L, K, 2, nall, 0.03, 7))


def _start(ch, K):
    ch.setseeds(13, 4, 1972)
    ch.chain_init(np.array([ch.ran1() for _ in range(K)], dtype=np.float32))


# name: (environment, mode, schedule, what the variant allocates that the others do not)
DIPLOID = {
    "replay": ({}, 2, capi.SCHED_REPLAY),
    "chain_kernels": ({"INSTRUCT_ZQ_SPEC_RESOLVE": "0", "INSTRUCT_ZQ_RESOLVE": "0"}, 2, capi.SCHED_REPLAY),  # uniform tape, pipe granules, d_spop
    "host_update_P": ({"INSTRUCT_P_DEVICE": "0"}, 2, capi.SCHED_REPLAY),                                    # the pinned host tape
    "mode4": ({}, 4, capi.SCHED_REPLAY),
    "mode5": ({}, 5, capi.SCHED_REPLAY),
    "keyed": ({}, 2, capi.SCHED_KEYED),
}


@pytest.mark.parametrize("name", sorted(DIPLOID))
def test_diploid_context_returns_every_buffer(name, monkeypatch):
    env, mode, sched = DIPLOID[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # host_update_P: the host loop takes its uniforms from the device only from 4096 gammas on (K L A = 3 x 800 x 2)
    geno, an, mi = _diploid(60, 800, 3) if name == "host_update_P" else _diploid()
    live = capi.live_buffers()
    ch = capi.HipChain(geno, an, mi, 3, mode=mode, rng_sched=sched)
    assert capi.live_buffers() > live
    _start(ch, 3)
    ch.run(4)
    ch.close()
    assert capi.live_buffers() == live


def test_running_means_are_returned_with_the_context():
    geno, an, mi = _diploid()
    live = capi.live_buffers()
    ch = capi.HipChain(geno, an, mi, 3)
    _start(ch, 3)
    before = capi.live_buffers()
    ch.store_begin(with_freq=True)
    assert capi.live_buffers() == before + 7  # qq, qq2, indvlkh, gen, gen2, freq, freq2
    for _ in range(3):
        ch.run(1)
        ch.store_step()
    with_means = capi.live_buffers()  # (the sweeps allocate what they need when they first need it)
    ch.store_begin(with_freq=True)    # a second begin replaces the means, it does not add to them
    assert capi.live_buffers() == with_means
    ch.close()
    assert capi.live_buffers() == live


def _tetraploid(sizes=(4, 3, 2, 4, 1, 4) * 7, N=60, K=3):
    return synth.code_tetraploid(mga.panel(N, sizes, K, 0.03, 20261101))


# name: (allo, environment, allele counts per locus or None for the default panel)
POLY = {
    "auto": (False, {}, None),
    "allo": (True, {}, None),
    "allo_wide": (True, {}, (20, 3, 5, 2)),   # a locus above 16 alleles: the wide path (closed-form rows, no code -> row map)
    "auto_block_resolver": (False, {"INSTRUCT_ZQ_RESOLVE_P4": "1", "INSTRUCT_ZQ_SPEC_RESOLVE": "0"}, None),
}


@pytest.mark.parametrize("name", sorted(POLY))
def test_tetraploid_context_returns_every_buffer(name, monkeypatch):
    allo, env, sizes = POLY[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    obs, alleleid, allelenum = _tetraploid(sizes, 30, 2) if sizes else _tetraploid()
    K = 2 if sizes else 3
    live = capi.live_buffers()
    ch = capi.HipPolyChain(obs, alleleid, allelenum, K, allo=allo)
    assert capi.live_buffers() > live
    _start(ch, K)
    ch.run(3)
    ch.close()
    assert capi.live_buffers() == live


def test_tetraploid_contexts_in_a_row_do_not_accumulate():
    """one device list per allele class hangs off every ploidy 4 context (4 classes here): the K scan and the multi-chain driver create
    many contexts per process"""
    obs, alleleid, allelenum = _tetraploid()
    assert len(set(allelenum.tolist())) == 4
    live = capi.live_buffers()
    for _ in range(4):
        ch = capi.HipPolyChain(obs, alleleid, allelenum, 3)
        _start(ch, 3)
        ch.run(1)
        ch.close()
        assert capi.live_buffers() == live


def test_failed_create_returns_what_it_had_allocated(monkeypatch):
    """mode 4 without its table is refused at the END of isg_ctx_create, after every allocation"""
    monkeypatch.setenv("INSTRUCT_LL_TABLES", "0")
    geno, an, mi = _diploid()
    live = capi.live_buffers()
    with pytest.raises(capi.IsgError, match="mode 4 needs its log-likelihood table"):
        capi.HipChain(geno, an, mi, 3, mode=4)
    assert capi.live_buffers() == live
