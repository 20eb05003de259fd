"""Converged-chain states for the ploidy-4 parity tests.  TEST INFRASTRUCTURE ONLY (a plain module, not a conftest), the tetraploid
counterpart of tests/converged.py.

A tetraploid chain started at chain_init has the four Z copies of a locus in one cluster at well under 1 % of the loci within the few
iterations the parity tests run, never redraws alpha (so update_ZQ's Dirichlets never take the gamma branch below 1) and never feeds a
zero or a subnormal qq entry to the update_ZQ kernels.  A converged chain -- and every chain of a K scan above the true K -- is elsewhere.
The regime is reached at iteration 0 by writing the same state into the HIP chain (the C ABI's setters) and into the oracle
(oracle/orc_dump_poly's trailing state-file argument) after the same chain_init:

  qq[i][k] = `off` for every cluster but (i % Ktrue) % K, which holds 1 - (K - 1) off;  alpha = a0;  optionally the K selfing rates.

Z cannot be written for ploidy 4 and need not be: the first update_ZQ draws it from the injected qq.  The state file holds alpha, the K
rates (nan = keep the chain's own) and the N x K qq entries as hexadecimal doubles, one per line.
"""
from __future__ import annotations

import collections
import functools
import os
import subprocess

import numpy as np

import orc
from instruct_amd import synth

DUMP = os.path.join(orc.ORC_DIR, "orc_dump_poly")
SEEDS = (51, 9, 2021)
A0, OFF = 0.003, 1e-30

# name: individuals, loci, true clusters -> clusters of the chain, alleles, missing share, iterations the GPU tests run from the state
Input = collections.namedtuple("Input", "N L Ktrue K A miss iters seed")
INPUTS = {
    "p60":   Input(60, 300, 2, 6, 4, 0.05, 8, 20261114),      # the main case
    "p60k2": Input(60, 300, 2, 2, 4, 0.05, 8, 20261114),      # no empty cluster, every locus same-cluster
    "pa10":  Input(40, 12, 2, 5, 10, 0.05, 8, 20261103),      # 715 genotypes per locus
    "pk20":  Input(30, 700, 2, 20, 3, 0.05, 4, 20261104),     # several workgroups per individual, K > 16, 18 empty clusters
    "pspec": Input(120, 2500, 2, 4, 4, 0.05, 4, 20261105),    # the interval resolver's shape (x_spec of tests/test_gpu_poly.py)
    "pwide": Input(40, 7, 2, 4, 32, 0.03, 3, None),       # the wa_auto panel of tests/test_gpu_poly_alleles.py: wide-allele table kernels
}
# seed: of synth.raw_alleles.  p60's is one at which, from the -e 0 rate vector below, both tetraploid variants keep cluster 0 at rate 1 through
# iteration 0 (NaN tables that are read: totallkh is NaN) and later hold a NaN table for an empty cluster only (totallkh finite); of the
# seeds 20261101..20261140, 7 do (20261114, ..17, ..28, ..29, ..37, ..38, ..40).  tests/test_converged_oracle_poly.py guards it.
# p60's selfing-rate vectors.  -e 0: states 2, 0, 0, 2, 1, 2 with exactly 0 and exactly 1 among the rates (at rate 1 the oracle's genotype
# tables hold NaN and +-inf and totallkh is NaN); -e 1: the reflection of the proposal at both ends
RATES_E0 = (1.0, 0.0, 0.0005, 0.9995, 0.5, 1.0)
RATES_E1 = (1e-12, 1.0 - 1e-12, 0.01, 0.99, 0.5, 0.03)

State = collections.namedtuple("State", "qq alpha self_rates")


@functools.lru_cache(maxsize=None)
def raw(name):
    """the raw alleles [N][L][4] of a named input; computed once and shared: do not write into it"""
    c = INPUTS[name]
    if name == "pwide":
        import test_gpu_poly_alleles as wide
        out = wide.wide_data("wa_auto")
        assert out.shape == (c.N, c.L, 4)
    else:
        out = synth.raw_alleles(c.N, c.L, c.Ktrue, 4, c.A, c.miss, c.seed)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def coded(name):
    """(obs, alleleid, allelenum) of a named input, shared: do not write into them"""
    out = synth.code_tetraploid(np.array(raw(name)))
    for a in out:
        a.setflags(write=False)
    return out


def converged_state(N, K, Ktrue, a0=A0, off=OFF, self_rates=None, scale=1.0):
    """qq [N][K] (every row times `scale`: a draw of Z depends on the ratios within a row only), alpha, the K rates or None"""
    qq = np.full((N, K), float(off))
    qq[np.arange(N), (np.arange(N) % Ktrue) % K] = 1.0 - (K - 1) * float(off)
    return State(qq * scale, float(a0), None if self_rates is None else np.asarray(self_rates, dtype=np.float64))


def state_of(name, **kw):
    c = INPUTS[name]
    return converged_state(c.N, c.K, c.Ktrue, **kw)


def write_state(path, state):
    K = state.qq.shape[1]
    rates = [float("nan")] * K if state.self_rates is None else [float(x) for x in state.self_rates]
    with open(path, "w") as f:
        f.write("\n".join(float(x).hex() for x in [state.alpha] + rates + list(state.qq.ravel())) + "\n")


def inject(chain, state):
    """Writes the state into a capi.HipPolyChain after chain_init"""
    chain.set_qq(np.ascontiguousarray(state.qq))
    chain.set_alpha(state.alpha)
    if state.self_rates is not None:
        chain.set_self_rates(np.ascontiguousarray(state.self_rates))


def oracle_args(name, txt, out, iters, e=1, sched=0, allo=False, state_path=None):
    """the canonical oracle on a named input: b = t = r = 1, and j beyond the run's length (the restart check `cnt_step == j` would end
    the run at the first empty cluster)"""
    c = INPUTS[name]
    args = [DUMP, txt, out] + [str(x) for x in (c.K, c.N, c.L, iters, 1, 1, e, 1, iters + 1) + SEEDS] + ["1", "1", str(sched), "1" if allo else "0"]
    return args + ([state_path] if state_path else [])


def start_oracle(d, tag, name, iters, state=None, **kw):
    """starts one oracle process in directory d (files tag.*); -> (process, output path)"""
    txt = os.path.join(str(d), name + ".txt")
    if not os.path.exists(txt):
        synth.write_text_polyploid(txt, np.array(raw(name)))
    sp = None
    if state is not None:
        sp = os.path.join(str(d), tag + ".state")
        write_state(sp, state)
    out = os.path.join(str(d), tag + ".can")
    return subprocess.Popen(oracle_args(name, txt, out, iters, state_path=sp, **kw), stdout=subprocess.DEVNULL), out


Reg = collections.namedtuple("Reg", "step same zeros qmin empty nan inf lkhfinite")


def regime(lines):
    """the `reg` lines of an oracle dump"""
    out = []
    for l in lines:
        if l.startswith("reg "):
            t = l.split()
            f = dict(x.split("=") for x in t[2:])
            out.append(Reg(int(t[1]), float(f["same"]), int(f["zeros"]), float.fromhex(f["qmin"]), int(f["empty"]), int(f["nan"]), int(f["inf"]),
                           int(f["lkhfinite"])))
    return out
