"""CPU: the converged-chain states of tests/converged_poly.py on the ploidy-4 oracle alone (oracle/orc_dump_poly with a state file).

Regime guard: from every named input's injected state, over the iterations tests/test_gpu_poly_converged.py runs from it, both tetraploid
variants and both schedules stay where that module claims to be testing -- the four Z copies of nearly every used locus in one cluster
(update_geno's and the likelihood's genotype-table branch), exact zeros in qq, empty clusters wherever K > Ktrue -- and the -e 0 rate
vector reaches the NaN tables.  These are conditions on the INPUTS, read from the oracle's `reg` lines: an input that misses one is to be
changed, the condition stays.

Measured with the committed inputs (canonical configuration `1 1`, seeds 51 9 2021; smallest same-cluster share over the run's iterations,
exact zeros per iteration, clusters with sum qq < 0.01):
  input   variant  schedule  same-cluster  zeros   empty
  p60     auto     replay    0.999707      31..42  4          (keyed 0.999824, 29..47, 4)
  p60     allo     replay    0.991607      27..43  2..4       (keyed 0.995657, 20..40, 2..4)
  p60k2   auto     replay    0.998943      5..13   0          (keyed 1.0, 4..8, 0)
  p60k2   allo     replay    0.999472      6..10   0          (keyed 0.999061, 2..13, 0)
  pa10    auto     replay    0.991342      8..19   1..3       (keyed 0.997835, 15..20, 3)
  pa10    allo     replay    0.952381      10..18  0..3       (keyed 0.987013, 10..23, 1..3)
  pk20    auto     replay    0.99995       55..66  18         (keyed 0.999699, 53..64, 18)
  pk20    allo     replay    0.998195      55..65  18         (keyed 0.999047, 56..74, 18)
  pspec   auto     replay    0.999993      28..46  2          (keyed 0.999979, 38..49, 2)
  pspec   allo     replay    0.999989      34..48  2          (keyed 0.999968, 24..47, 2)
  pwide   auto     replay    1.0           11..17  2          (keyed 1.0, 10..16, 2)
  pwide   allo     replay    0.992754      13..24  1..2       (keyed 0.996377, 7..14, 2)
  (pa10 allo has no empty cluster left in iterations 5..7 of the replay schedule: it has 3 in iteration 0 and 1 or 2 until then)
-e 0 rates (1, 0, 0.0005, 0.9995, 0.5, 1) on p60, 6 iterations, (NaN, infinite) table entries and whether totallkh is finite:
  auto  (20400, 600, no) (10200, 300, yes) (10200, 300, yes) (10200, 300, yes) (20400, 600, yes) (10200, 300, yes)
  allo  (9600, 50400, no) (4800, 25200, yes) then no NaN entry
  same-cluster share at least 0.999941 (auto) and 0.998004 (allo).  -e 1 rates: no NaN entry, share at least 0.999941 / 0.992311.
p60 from chain_init, nothing injected, 8 iterations: same-cluster share 0.0055..0.0079 (auto), 0.0050..0.0072 (allo), no zero in qq, no empty cluster.
"""
import pytest

import converged_poly as cp
import golden_util as gu
import orc

VARIANTS = [(allo, sched) for allo in (False, True) for sched in (0, 1)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every oracle run of the module, started together (each is one CPU process of 0.1 .. 3 s)"""
    orc.build()
    d = tmp_path_factory.mktemp("convpoly")
    procs = {}
    for name, c in cp.INPUTS.items():
        for allo, sched in VARIANTS:
            procs[(name, allo, sched)] = cp.start_oracle(d, "%s.%d.%d" % (name, allo, sched), name, c.iters, state=cp.state_of(name), sched=sched, allo=allo)
    for allo in (False, True):
        procs[("e0", allo)] = cp.start_oracle(d, "e0.%d" % allo, "p60", 6, state=cp.state_of("p60", self_rates=cp.RATES_E0), e=0, allo=allo)
        procs[("e1", allo)] = cp.start_oracle(d, "e1.%d" % allo, "p60", 6, state=cp.state_of("p60", self_rates=cp.RATES_E1), e=1, allo=allo)
        # nothing injected (every entry of the state file is nan = keep): the same run as without a state file, with `reg` lines
        keep = cp.state_of("p60", a0=float("nan"), off=float("nan"))
        procs[("plain", allo)] = cp.start_oracle(d, "plain.%d" % allo, "p60", 8, state=keep, allo=allo)
        procs[("nostate", allo)] = cp.start_oracle(d, "nostate.%d" % allo, "p60", 8, allo=allo)
    yield procs
    for p, _ in procs.values():
        if p.poll() is None:
            p.kill()
            p.wait()


def _lines(runs, key):
    p, out = runs[key]
    assert p.wait(timeout=600) == 0
    return gu.parse(out)


@pytest.mark.parametrize("allo,sched", VARIANTS)
@pytest.mark.parametrize("name", sorted(cp.INPUTS))
def test_regime_guard(name, allo, sched, runs):
    c = cp.INPUTS[name]
    reg = cp.regime(_lines(runs, (name, allo, sched)))
    print("REG %s allo=%d sched=%d same>=%.6f zeros=%d..%d empty=%d..%d" % (name, allo, sched, min(r.same for r in reg), min(r.zeros for r in reg),
                                                                          max(r.zeros for r in reg), min(r.empty for r in reg), max(r.empty for r in reg)))
    assert [r.step for r in reg] == list(range(c.iters))
    for r in reg:
        assert r.same >= 0.95, r
        assert r.nan == 0 and r.inf == 0 and r.lkhfinite == 1, r
    assert sum(r.zeros for r in reg) >= 1
    assert min(r.qmin for r in reg) < 1.4e-45    # (below the smallest float subnormal)
    if c.K > c.Ktrue:
        assert max(r.empty for r in reg) >= 1
    else:
        assert all(r.empty == 0 for r in reg)


@pytest.mark.parametrize("allo", [False, True])
def test_selfing_rate_one_reaches_the_nan_tables(allo, runs):
    lines = _lines(runs, ("e0", allo))
    inj = [l for l in lines if l.startswith("chain injected")]
    assert len(inj) == 1 and inj[0].endswith(" st2 st0 st0 st2 st1 st2")   # (the MH states follow the written rates)
    reg = cp.regime(lines)
    print("REG e0 allo=%d %s" % (allo, [(r.nan, r.inf, r.lkhfinite) for r in reg]))
    assert len(reg) == 6 and all(r.same >= 0.95 for r in reg)
    assert reg[0].nan > 0 and reg[0].inf > 0 and reg[0].lkhfinite == 0                  # a NaN table that is read
    assert any(r.nan > 0 and r.lkhfinite == 1 for r in reg[1:]), reg                   # ... and later one that nobody reads
    assert any(l.startswith("it 0 L totallkh=nan") or l.startswith("it 0 L totallkh=-nan") for l in lines)


@pytest.mark.parametrize("allo", [False, True])
def test_rates_at_the_reflecting_ends_stay_in_the_regime(allo, runs):
    reg = cp.regime(_lines(runs, ("e1", allo)))
    assert len(reg) == 6
    for r in reg:
        assert r.same >= 0.95 and r.nan == 0 and r.lkhfinite == 1 and r.empty >= 1, r


@pytest.mark.parametrize("allo", [False, True])
def test_contrast_and_untouched_output(allo, runs):
    """the same data from chain_init: (almost) no locus has its four copies in one cluster.  A state file of nan entries injects nothing:
    apart from its `chain injected` and `reg` lines the dump is the one without a state file, line for line."""
    plain, nostate = _lines(runs, ("plain", allo)), _lines(runs, ("nostate", allo))
    reg = cp.regime(plain)
    print("REG plain allo=%d same=%.6f..%.6f" % (allo, min(r.same for r in reg), max(r.same for r in reg)))
    assert len(reg) == 8
    for r in reg:
        assert r.same < 0.05 and r.zeros == 0 and r.empty == 0, r
    assert not any(l.startswith(("reg ", "chain injected")) for l in nostate)
    assert [l for l in plain if not l.startswith(("reg ", "chain injected"))] == nostate
