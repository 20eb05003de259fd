"""GPU: ploidy 4 with 17..32 alleles per locus (the wide-allele path: closed-form genotype rows, k4_exfreq_w / k4_genfreq_w) against
 (1) the canonical oracle (oracle/orc_dump_poly ... 1 1) in the replay and keyed schedules: every dump line identical, on mixed panels
     with one locus where all 32 alleles occur, loci of 17..24 alleles and loci of 1..4 alleles, both tetraploid variants;
 (2) the REAL reference's trajectories above 16 alleles (tests/golden/tw_*.golden): discrete state identical, doubles within 1e-9;
 (3) the reference program's result file for `-p 4` on a file with more than 16 alleles (drop-in);
and the refusals: 33 alleles, and genotype tables larger than half of the free device memory."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import orc

import make_golden_alleles as mga

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(orc.ORC_DIR, "orc_dump_poly")

# name: (N, L, K, allele counts per locus, missing, u, b, t, e, r, j, seeds, allo).  The oracle finds rows in closed form as the kernels do
# (one run is well under a second); all oracle runs are started at once.  wa_auto_e0: K = 3 and -e 0 (selfing rates reach exactly 0 and 1),
# a locus at the 32-allele cap, one at the 17-allele floor of the wide path (classes below and above 256 rows: single- and multi-trip
# strided loops), and 3 and 1 alleles for the n >= 3 / n >= 4 guards.
WIDE = {
    "wa_auto": (40, 7, 2, (32, 17, 24, 1, 2, 3, 4), 0.03, 2, 1, 1, 1, 1, 1, (51, 7, 1999), False),
    "wa_allo": (40, 6, 2, (32, 18, 23, 1, 2, 4), 0.03, 2, 1, 1, 0, 1, 1, (52, 8, 2000), True),
    "wa_auto_e0": (40, 5, 3, (32, 20, 17, 3, 1), 0.03, 2, 1, 1, 0, 1, 1, (53, 9, 2001), False),
}


def wide_data(name):
    N, L, K, sizes, miss = WIDE[name][:5]
    return mga.panel(N, sizes, K, miss, 20261030 + sorted(WIDE).index(name))


def hip_lines(cfg, raw, sched=0, allo=False, after_init=None):
    """Drives the C ABI sweep by sweep and formats the state as oracle/isg_oracle_poly.c's dump does (as tests/test_gpu_poly.py)."""
    from instruct_amd import capi, synth
    N, L, K, A, miss, u, b, t, e, r, j, seeds = cfg[:12]
    obs, alleleid, allelenum = synth.code_tetraploid(raw)
    ch = capi.HipPolyChain(obs, alleleid, allelenum, K, back_refl=e, rng_sched=sched, allo=allo)
    ch.setseeds(*seeds)
    initd = np.array([np.float32(ch.ran1()) for _ in range(K)], dtype=np.float32)
    lines = []
    sd = lambda: " seeds=%d %d %d" % ch.seeds()
    ch.chain_init(initd)
    lines.append("chain zqinit hz=%s hqq=%s" % (orc.fnv_i32(ch.z()), orc.fnv_f64(ch.qq())) + sd())
    if after_init is not None:   # (tests/converged_poly.py: a state written into the chain; the lines it reports, if any)
        lines.extend(after_init(ch) or [])
    for step in range(u):
        ch.update_P()
        lines.append("it %d P hcnt=%s hfreq=%s" % (step, _hcnt(ch, allelenum), _hfreq(ch, allelenum)) +
                     (" hfreq2=%s" % _hfreq(ch, allelenum, ch.freq2()) if allo else "") + sd())
        lines.append("it %d X hexfreq=%s" % (step, orc.fnv_i32(ch.packed(ch.exfreq()).view(np.int32))))
        ch.update_S_POP()
        s = "it %d S" % step + "".join(" " + float(x).hex() for x in ch.self_rates())
        if e == 0:
            s += "".join(" st%d" % x for x in ch.state())
        lines.append(s + " hgenofreq=%s" % orc.fnv_i32(ch.packed(ch.genofreq()).view(np.int32)) + sd())
        ch.update_ZQ(0)
        lines.append("it %d ZQ hz=%s hqq=%s hqqnum=%s" % (step, orc.fnv_i32(ch.z()), orc.fnv_f64(ch.qq()), orc.fnv_f64(ch.qqnum())) + sd())
        ch.update_geno()
        lines.append("it %d GE hgeno=%s" % (step, orc.fnv_i32(ch.geno())) + sd())
        ch.cal_lkh()
        lines.append("it %d L totallkh=%s hindv=%s" % (step, float(ch.totallkh()).hex(), orc.fnv_f64(ch.indvlkh())))
        ch.lib.isg_iter_advance(ch.h)
    ch.close()
    return lines


def _hcnt(ch, allelenum):
    c = ch.count_alleles()
    mask = np.arange(ch.Amax)[None, :] < allelenum[:, None]
    return orc.fnv_i32(np.ascontiguousarray(c[:, mask]))


def _hfreq(ch, allelenum, f=None):
    f = ch.freq() if f is None else f
    mask = (np.arange(ch.Amax)[None, :] < allelenum[:, None]) & (allelenum[:, None] > 1)
    return orc.fnv_f64(np.ascontiguousarray(f[:, mask]))


def _norm(line):
    toks = []
    for t in line.split():
        k, eq, v = t.partition("=")
        cand = v if eq else t
        if cand.startswith(("0x", "-0x")) or cand in ("inf", "-inf", "nan"):
            toks.append((k if eq else "") + repr(float.fromhex(cand) if "x" in cand else float(cand)))
        else:
            toks.append(t)
    return " ".join(toks)


def _noseeds(line):
    return line.split(" seeds=")[0]


@pytest.fixture(scope="module")
def oracle_runs(tmp_path_factory):
    """every canonical oracle run of the module, started together (each is one CPU process)"""
    orc.build()
    from instruct_amd import synth
    d = tmp_path_factory.mktemp("wide")
    procs = {}
    for name in sorted(WIDE):
        N, L, K, sizes, miss, u, b, t, e, r, j, seeds, allo = WIDE[name]
        txt = str(d / (name + ".txt"))
        synth.write_text_polyploid(txt, wide_data(name))
        for sched in (0, 1):
            out = str(d / ("%s.%d.can" % (name, sched)))
            args = [DUMP, txt, out] + [str(x) for x in (K, N, L, u, b, t, e, r, j) + tuple(seeds)] + ["1", "1", str(sched)] + (["1"] if allo else [])
            procs[(name, sched)] = (subprocess.Popen(args, stdout=subprocess.DEVNULL), out)
    yield procs
    for p, _ in procs.values():
        if p.poll() is None:
            p.kill()
            p.wait()


def _oracle_lines(oracle_runs, name, sched):
    p, out = oracle_runs[(name, sched)]
    assert p.wait(timeout=600) == 0
    return [l for l in gu.parse(out) if l.startswith("it ") or l.startswith("chain zqinit")]


@pytest.mark.parametrize("sched", [0, 1])
@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_alleles_bit_identical_to_canonical_oracle(name, sched, oracle_runs):
    """sched 1 = keyed schedule (the sequential seed triple is not defined there and is left out)"""
    cfg = WIDE[name]
    from instruct_amd import synth
    _, _, allelenum = synth.code_tetraploid(wide_data(name))
    assert tuple(allelenum) == cfg[3] and max(allelenum) == 32
    got = hip_lines(cfg, wide_data(name), sched, allo=cfg[-1])
    want = _oracle_lines(oracle_runs, name, sched)
    assert len(got) == len(want) == 1 + 6 * cfg[5]
    for g, w in zip(got, want):
        if sched:
            g, w = _noseeds(g), _noseeds(w)
        assert _norm(g) == _norm(w), (g, w)


@pytest.mark.parametrize("name", sorted(mga.CASES))
def test_wide_alleles_match_reference_trajectory(name):
    """tests/golden/tw_*.golden come from the reference's own sweeps (oracle/ref_dump_poly.c): discrete state and seeds identical after
    every sweep, doubles within 1e-9"""
    cfg = mga.CASES[name]
    want = [l for l in gu.parse(os.path.join(gu.GOLDEN, name + ".golden")) if l.startswith("it ") or l.startswith("chain zqinit")]
    got = hip_lines(cfg, mga.data_for(name), allo=cfg[-1])
    assert len(got) == len(want)
    for g, w in zip(got, want):
        fg, fw = gu.fields(g), gu.fields(w)
        for key in ("hz", "hgeno", "hcnt", "hqqnum", "seeds"):
            assert fg.get(key) == fw.get(key), (key, g, w)
        assert [t for t in g.split() if t.startswith("st")] == [t for t in w.split() if t.startswith("st")]
        a, bb = gu.floats(g), gu.floats(w)
        assert len(a) == len(bb)
        for x, y in zip(a, bb):
            assert x == y or (x != x and y != y) or abs(x - y) <= 1e-9 * max(abs(x), abs(y)), (g, w)


@pytest.mark.parametrize("allo", [False, True])
def test_33_alleles_are_refused(allo):
    from instruct_amd import capi, synth
    obs, alleleid, allelenum = synth.code_tetraploid(mga.panel(12, (33, 3), 2, 0.0, 7))
    assert tuple(allelenum) == (33, 3)
    with pytest.raises(capi.IsgError, match="up to 32 alleles"):
        capi.HipPolyChain(obs, alleleid, allelenum, 2, allo=allo)


def test_tables_beyond_half_the_free_device_memory_are_refused():
    """32 alleles (allotetraploid: 278 784 genotypes), K = 32, 3000 loci: the five padded tables would take 535 GB"""
    from instruct_amd import capi, synth
    raw = np.tile(np.arange(1, 33, dtype=np.int32).reshape(8, 1, 4), (1, 3000, 1))
    obs, alleleid, allelenum = synth.code_tetraploid(raw)
    assert allelenum.min() == allelenum.max() == 32
    with pytest.raises(capi.IsgError, match="genotype tables need [0-9]+ bytes"):
        capi.HipPolyChain(obs, alleleid, allelenum, 32, allo=True)
    # the refusal leaves no error behind for the next context of the process
    obs, alleleid, allelenum = synth.code_tetraploid(mga.panel(12, (17, 3), 2, 0.0, 8))
    ch = capi.HipPolyChain(obs, alleleid, allelenum, 2)
    ch.chain_init(np.array([0.25, 0.5], dtype=np.float32))
    ch.iteration()
    assert np.isfinite(ch.totallkh())
    ch.close()


def test_dropin_cli_output_above_16_alleles_equals_reference(tmp_path):
    """`-p 4 -ap 1` through the drop-in on tests/golden/tw_auto.txt (loci of 17..24 alleles): the result file the reference
    program wrote (tests/golden/tw_cli_output.txt)"""
    exe = os.path.join(ROOT, "oracle", "_ref", "InStruct_hip")
    assert os.path.exists(exe), "oracle/_ref/InStruct_hip is built by build()"
    out = tmp_path / "out.txt"
    cmd = [exe, "-d", os.path.join(gu.GOLDEN, "tw_auto.txt"), "-o", str(out)] + mga.TW_CLI
    log = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert log.returncode == 0 and b"THE JOB IS SUCCESSFULLY FINISHED" in log.stdout, log.stdout[-2000:]

    def body(path):
        return [l for l in open(path, "rb").read().split(b"\n")
                if not (l.strip().startswith((b"Data File:", b"Output File:")) or b"InStruct" in l and b"-d" in l)]
    assert body(str(out)) == body(os.path.join(gu.GOLDEN, "tw_cli_output.txt"))
