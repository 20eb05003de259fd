"""CPU: the converged-chain states of tests/converged.py on the oracle alone.

(1) Regime guard: from every named input's injected state, over the iterations the GPU tests run from it, the chain stays where real
    converged chains are -- alpha below 1, no cluster beyond the true ones above 1 % of the copies, qq entries below the smallest
    float subnormal (and, where the table says so, exactly 0).  These are conditions on the INPUTS: an input that misses one is to be
    changed, the condition stays.
(2) The oracle's reference configuration (libm, sequential sums) and its canonical one (the device's math and exact accumulation) walk
    the same chain from the first six states for 40 iterations: the GPU tests' yardstick is the reference's arithmetic there too.
"""
import math

import numpy as np
import pytest

import converged as cv
import orc

F32_DENORM_MIN = 1.4e-45


@pytest.fixture(scope="module", autouse=True)
def _lib():
    orc.build()


def _oracle(name, math_=orc.MATH_ISG, accum=orc.ACC_EXACT, sched=orc.SCHED_REPLAY, e=1):
    c = cv.INPUTS[name]
    geno, an, mi = cv.data(name)
    o = orc.OrcChain(geno, an, mi, c.K, mode=c.mode, back_refl=e, math=math_, accum=accum, sched=sched)
    o.setseeds(13, 4, 1972)
    o.chain_init(np.array([o.ran1() for _ in range(c.K)], dtype=np.float32))
    cv.inject(o, cv.state_of(name))
    return o


def test_inject_writes_the_state_and_leaves_the_rest():
    c = cv.INPUTS["n60"]
    o = _oracle("n60")
    st = cv.state_of("n60")
    z = o.z()
    assert (o.valid() == 0).any()   # (the input has missing loci: they stay masked)
    assert np.array_equal(z, np.broadcast_to(np.where(o.valid()[:, :, None] != 0, st.z[:, None, None], -1), z.shape))
    assert np.array_equal(o.qq(), st.qq) and np.allclose(st.qq.sum(1), 1.0, atol=1e-15) and o.alpha() == c.a0
    g, s = o.generation().copy(), o.self_rates().copy()
    o.set_generation(g[::-1].copy())
    o.set_self_rates(s[::-1].copy())
    assert np.array_equal(o.generation(), g[::-1]) and np.array_equal(o.self_rates(), s[::-1])
    assert cv.converged_state(4, 1, 2, 0.05, 2).z.max() == 0   # K = 1 on two-cluster data


# (the schedules each input is run on by tests/test_gpu_converged.py)
GUARD = [(n, s, 1) for n in cv.GUARDED for s in ((orc.SCHED_REPLAY, orc.SCHED_KEYED) if not n.startswith("big") else (orc.SCHED_REPLAY,))]
GUARD += [("n60", s, 0) for s in (orc.SCHED_REPLAY, orc.SCHED_KEYED)]   # (n60 is also run with -e 0)


@pytest.mark.parametrize("name,sched,e", GUARD)
def test_regime_guard(name, sched, e):
    c = cv.INPUTS[name]
    o = _oracle(name, sched=sched, e=e)
    qmin, zeros = 1.0, 0
    for it in range(c.iters):
        o.iteration()
        assert o.alpha() < 1, (it, o.alpha())
        assert cv.extras(o.z(), c.K, c.Ktrue) < 0.01, it
        qq = o.qq()
        qmin = min(qmin, float(qq.min()))
        zeros += int((qq == 0).sum())
        assert math.isfinite(o.totallkh()), it
    assert o.error() == 0
    assert qmin < F32_DENORM_MIN, qmin
    if c.zeros:
        assert zeros >= 1


@pytest.mark.parametrize("name", cv.FIRST_SIX)
def test_reference_and_canonical_configuration_agree(name):
    a, b = _oracle(name, orc.MATH_LIBM, orc.ACC_SEQ), _oracle(name)

    def close(x, y, tol=1e-9):
        x, y = np.atleast_1d(np.asarray(x, dtype=float)), np.atleast_1d(np.asarray(y, dtype=float))
        return x.shape == y.shape and bool(np.all((x == y) | (np.abs(x - y) <= tol * np.abs(y))))
    for it in range(40):
        a.iteration()
        b.iteration()
        for n in ("z", "generation", "qqnum", "seeds"):
            assert np.array_equal(np.asarray(getattr(a, n)()), np.asarray(getattr(b, n)())), (it, n)
        for n in ("qq", "alpha", "self_rates", "totallkh"):
            assert close(getattr(a, n)(), getattr(b, n)()), (it, n)
    assert a.error() == 0 and b.error() == 0
