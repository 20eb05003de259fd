"""The walk engine's tables evaluated over the columns a row can be entered at only (wk_trim_range, instruct_amd/csrc/isg_walk.h), under host
emulation: the trimmed run gives every Dirichlet the start position of the sequential sampler; inside a row's range the table is the
untrimmed table byte for byte, outside it is WK_IRR; a walk that leaves the range is reported as a missed window, never answered wrongly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
LIB = os.path.join(EMUL, "libwalk_trim_emul.so")
SRCS = [os.path.join(EMUL, "walk_trim_emul.cpp")] + [os.path.join(ROOT, "instruct_amd", "csrc", f) for f in
                                                     ("isg_walk.h", "isg_walk_plan.h", "isg_sampler.h", "isg_wh.h", "isg_math.h")]
SEEDS = (13, 4, 1972)
WK_IRR = 0xFF


def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRCS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-o", LIB, SRCS[0]])
    return C.CDLL(LIB)


def _seeds(s):
    return C.c_long(s[0]), C.c_long(s[1]), C.c_long(s[2])


def groups_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def run_exact(gam0, cnt, seeds=SEEDS, rho_hi=0.8, sigma=1.0, kwin=5.0, seg_groups=24576, scale=1.0, nthreads=256, trim_k=None, tape=0):
    l = lib()
    G = len(gam0) - 1
    gam0 = np.ascontiguousarray(gam0, dtype=np.int32)
    cnt = np.ascontiguousarray(cnt, dtype=np.int32)
    T = np.zeros(G + 1, dtype=np.uint64)
    out = np.zeros(8, dtype=np.uint64)
    rc = l.wt_exact(gam0.ctypes, G, cnt.ctypes, *_seeds(seeds), C.c_double(rho_hi), C.c_double(sigma), C.c_double(kwin), seg_groups, C.c_float(scale), nthreads,
                    C.c_double(kwin if trim_k is None else trim_k), tape, T.ctypes, out.ctypes)
    Tr = np.zeros(G + 1, dtype=np.uint64)
    tot = C.c_ulonglong(0)
    l.wt_ref_exact(gam0.ctypes, G, cnt.ctypes, *_seeds(seeds), Tr.ctypes, C.byref(tot))
    return rc, T, out, Tr, tot.value


def _check_exact(name, gam0, cnt, **kw):
    rc, T, out, Tr, tot = run_exact(gam0, cnt, **kw)
    print("%s: %d blocks, %d segments, %d rows trimmed, %.1f %% of the decisions evaluated" % (name, out[3], out[4], out[7], 100.0 * out[5] / out[6]))
    assert rc == 0 and out[1] == 0, out
    assert np.array_equal(T, Tr) and out[0] == tot
    assert out[7] > 0 and out[5] < out[6]   # something was trimmed
    return out


def test_trimmed_exact_run_equals_sequential_sampler_large_counts():
    rng = np.random.default_rng(41)
    sizes = rng.integers(2, 5, size=3000)
    _check_exact("large counts", groups_of(sizes), rng.integers(50, 9000, size=int(sizes.sum())))


def test_trimmed_exact_run_with_counts_0_1_2_mixed_in():
    """shape 1 consumes ONE uniform and is never rejected: the positions turn odd and the predicted drift per row is uneven"""
    rng = np.random.default_rng(42)
    sizes = rng.integers(2, 5, size=3000)
    cnt = rng.choice([0, 0, 1, 1, 2, 2, 3, 5, 9, 40, 700, 3000, 8000], size=int(sizes.sum()))
    _check_exact("counts 0 1 2 mixed", groups_of(sizes), cnt, sigma=1.2, tape=1)


@pytest.mark.parametrize("seg", [1024, 2048, 24576])
def test_trimmed_exact_run_several_segments_and_small_blocks(seg):
    rng = np.random.default_rng(43)
    G = 6000 + 37                              # the last block of the run (and of most segments) is short
    gam0 = groups_of(np.full(G, 2))
    cnt = rng.integers(50, 9000, size=2 * G)
    out = _check_exact("seg %d" % seg, gam0, cnt, seg_groups=seg)
    assert out[4] == -(-G // seg)


def test_trimmed_blocks_of_fewer_than_64_groups():
    """groups of 64 gammas: the plan shrinks its blocks until a block's table fits the LDS"""
    rng = np.random.default_rng(44)
    G = 900
    gam0 = groups_of(np.full(G, 64))
    cnt = rng.integers(0, 60, size=64 * G)
    _check_exact("64 gammas per group", gam0, cnt, sigma=1.2)


def _spec_problem(N, K, nv, seed, lo=150, hi=5000):
    rng = np.random.default_rng(seed)
    gam0 = (np.arange(N + 1) * K).astype(np.int32)
    B = np.arange(N + 1, dtype=np.uint64) * np.uint64(2 * nv + 2 * K)
    gpos = np.zeros(N * K + 1, dtype=np.uint64)
    for m in range(K):
        gpos[m:N * K:K] = B[:N] + np.uint64(2 * nv + 2 * m)
    gpos[N * K] = B[N]
    alpha = 3.7
    lam = rng.integers(lo, hi, size=(N, K)).astype(np.float64)
    half = np.ceil(4.5 * np.sqrt(lam * 0.8)) + 1
    alo = (lam - half + alpha).astype(np.float32).reshape(-1)
    ahi = (lam + half + alpha).astype(np.float32).reshape(-1)
    atrue = np.ascontiguousarray((lam + np.round((rng.random((N, K)) * 2 - 1) * (half - 1)) + alpha).reshape(-1), dtype=np.float64)
    return gam0, gpos, alo, ahi, atrue


@pytest.mark.parametrize("seg,band", [(4096, 24), (256, 24), (320, 40)])
def test_trimmed_interval_resolver_end_to_end_lenient_walk_probes_strict_walk(seg, band):
    """as the untrimmed resolver test: the strict walk enters the later segments a little off the lenient walk's entry, inside the entry
    columns the rows' ranges are built around"""
    l = lib()
    N, K = 1200, 5
    gam0, gpos, alo, ahi, atrue = _spec_problem(N, K, 600, 31)
    T = np.zeros(N + 1, dtype=np.uint64)
    Tref = np.zeros(N + 1, dtype=np.uint64)
    out = np.zeros(8, dtype=np.uint64)
    rc = l.wt_spec(gam0.ctypes, N, gpos.ctypes, alo.ctypes, ahi.ctypes, atrue.ctypes, *_seeds(SEEDS), C.c_double(1.0), C.c_double(5.0), seg, band, 2 * band + 32, 256, C.c_double(5.0),
                   T.ctypes, Tref.ctypes, out.ctypes)
    print("interval seg %d: %d probes, %d rows trimmed, %.1f %% of the decisions evaluated" % (seg, out[2], out[6], 100.0 * out[4] / out[5]))
    assert rc == 0 and out[0] == 0 and out[1] == 0, out
    assert np.array_equal(T, Tref)
    assert out[2] > 0 and out[3] == -(-N // seg)
    assert out[6] > 0 and out[4] < out[5]


def _tables(mode, tape, seg_groups=2048):
    l = lib()
    out = np.zeros(11, dtype=np.uint64)
    if mode == "exact":
        rng = np.random.default_rng(51)
        G = 2500
        gam0 = groups_of(np.full(G, 2))
        cnt = np.ascontiguousarray(rng.choice([0, 1, 2, 7, 300, 4000, 9000], size=2 * G), dtype=np.int32)
        rc = l.wt_tables(gam0.ctypes, G, cnt.ctypes, None, None, None, *_seeds(SEEDS), C.c_double(0.8), C.c_double(1.2), C.c_double(5.0), seg_groups, C.c_float(1.0), 256,
                         C.c_double(5.0), tape, 0, out.ctypes)
    else:
        N, K = 1200, 5
        gam0, gpos, alo, ahi, _ = _spec_problem(N, K, 600, 31)
        rc = l.wt_tables(gam0.ctypes, N, None, gpos.ctypes, alo.ctypes, ahi.ctypes, *_seeds(SEEDS), C.c_double(0.8), C.c_double(1.0), C.c_double(5.0), 512, C.c_float(1.0), 256,
                         C.c_double(5.0), tape, 80, out.ctypes)
    return rc, out


@pytest.mark.parametrize("mode", ["exact", "interval"])
@pytest.mark.parametrize("tape", [0, 1])
def test_trimmed_table_is_the_untrimmed_table_inside_the_ranges_and_irregular_outside(mode, tape):
    """(a byte whose group rejects more than WK_PADC = 64 attempts could differ near a range's end: the untrimmed table has the same limit at
    the end of its rows, and at a third of a rejection per attempt no group of these sizes comes near it)"""
    rc, out = _tables(mode, tape)
    print("%s, %s: %d of %d blocks keep every column (%d clamped), %d rows trimmed, %d bytes inside, %d outside, %.1f %% of the decisions evaluated"
          % (mode, "tape" if tape else "generated", out[7], out[9], out[10], out[6], out[2], out[3], 100.0 * out[4] / out[5]))
    assert rc == 0, rc
    assert out[0] == 0, "bytes inside a row's range differ from the untrimmed table: %d" % out[0]
    assert out[1] == 0, "bytes outside a row's range are not WK_IRR: %d" % out[1]
    assert out[3] > 0 and out[6] > 0 and out[4] < out[5]


def test_last_block_of_a_segment_and_a_clamped_window_keep_every_column():
    rc, out = _tables("exact", 0)
    assert rc == 0
    assert out[7] >= 2 and out[10] >= 1, out   # last blocks of the two segments; windows clamped at offset 0 at the run's start
    assert out[8] == 0, "blocks that must keep every column were trimmed: %d" % out[8]
    assert out[7] < out[9]


def test_leaving_a_rows_range_is_a_missed_window_not_an_irregular_byte_and_never_a_wrong_answer():
    """Blocks of 64 x 16 gammas drift by sigma sqrt(1024) = 30 rejections; the run's first block is entered at its only entry column, so a
    spread of a fiftieth of sigma leaves its rows the margin of 8 columns (and what the rounding to 32 adds) and no more."""
    rng = np.random.default_rng(5)
    G = 1000
    gam0 = groups_of(np.full(G, 16))
    cnt = rng.integers(50, 9000, size=16 * G)
    rc, T, out, Tr, tot = run_exact(gam0, cnt, trim_k=0.02)
    assert rc == 0
    assert out[1] & 1, out                                        # a window was missed ...
    assert not out[1] & 2, out                                    # ... and no irregular byte is blamed
    assert out[0] == 0                                            # nothing is handed out
    for k in (0.0, None):                                         # the same run with every column, and with the walk's own spread
        rc, T, out, Tr, tot = run_exact(gam0, cnt, trim_k=k)
        assert rc == 0 and out[1] == 0 and np.array_equal(T, Tr) and out[0] == tot, (k, out)


def test_in_block_drift_stays_inside_the_spread_the_rows_are_trimmed_with():
    """what wk_trim_range assumes, measured with the sequential sampler: the rejections of a block's earlier rows, against the block's
    prediction in proportion to the gammas, in units of kwin sigma sqrt(gammas before the row) + 8 at kwin = 4, sigma = 0.95"""
    l = lib()
    rng = np.random.default_rng(61)
    sets = []
    G = 25000
    c1 = rng.integers(3000, 5000, size=2 * G)
    sets.append(("2 gammas, counts about 4000", groups_of(np.full(G, 2)), c1, 0.49))
    c2 = c1.copy()
    c2[rng.choice(2 * G, size=2000, replace=False)] = rng.integers(0, 3, size=2000)
    sets.append(("... 2000 counts of 0..2 mixed in", groups_of(np.full(G, 2)), c2, 0.49))
    G3 = 10000
    c3 = np.concatenate([rng.multinomial(6000, rng.dirichlet(np.ones(5))) for _ in range(G3)])
    sets.append(("5 gammas, multinomial counts", groups_of(np.full(G3, 5)), c3, None))
    for name, gam0, cnt, _ in sets:
        G = len(gam0) - 1
        gam0 = np.ascontiguousarray(gam0, dtype=np.int32)
        cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        Tr = np.zeros(G + 1, dtype=np.uint64)
        tot = C.c_ulonglong(0)
        l.wt_ref_exact(gam0.ctypes, G, cnt.ctypes, *_seeds(SEEDS), Tr.ctypes, C.byref(tot))
        out = np.zeros(3, dtype=np.uint64)
        rc = l.wt_drift(gam0.ctypes, G, cnt.ctypes, Tr.ctypes, C.c_double(0.8), C.c_double(0.95), C.c_double(4.0), 12800, C.c_float(1.0), out.ctypes)
        print("%s: worst in-block deviation %.2f of the spread over %d blocks (against the per-row sum of the predictions: %.2f)" % (name, out[0] * 1e-6, out[1], out[2] * 1e-6))
        assert rc == 0 and out[0] < 1000000, (name, out)
