"""Wall time and per-kernel time of the ploidy-4 iteration with 32 alleles observed at every locus (the wide-allele path), GPU box.

    python tools/gpu_poly_alleles_time.py [N L K [iterations]]          # default 2000 100 10 2
    rocprofv3 --kernel-trace --stats -d DIR -o wide -- python tools/gpu_poly_alleles_time.py

For autotetraploid and allotetraploid chains in the replay and keyed schedules: context creation, chain init and every
iteration's wall time, then the chain's own per-kernel profile (k4_exfreq_w and k4_genfreq_w separately; one k4_genfreq_w launch
covers the K L tables of one set of selfing rates).  The JSON goes to $TOOL_OUT/poly_alleles_time.json (default tool_out/).
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instruct_amd import capi  # noqa: E402

A = 32


def panel(N, L, K, seed):
    """coded tetraploid data: allele codes 0..31 from per-(cluster, locus) Dirichlet(1..1) frequencies, every code present at
    every locus (the first 8 individuals carry all 32); obs = sorted distinct codes, -1 padded"""
    rng = np.random.default_rng(seed)
    raw = np.empty((N, L, 4), dtype=np.int32)
    f = rng.dirichlet(np.ones(A), size=(K, L))
    cum = np.cumsum(f, axis=-1)
    u = rng.random((N, L, 4))
    for i in range(N):
        raw[i] = np.minimum((u[i][:, :, None] > cum[i % K][:, None, :]).sum(-1), A - 1)
    raw[:8] = np.arange(A, dtype=np.int32).reshape(8, 1, 4)
    s = np.sort(raw, axis=-1)
    keep = np.concatenate([np.ones((N, L, 1), bool), s[..., 1:] != s[..., :-1]], axis=-1)
    obs = np.full((N, L, 4), -1, dtype=np.int32)
    alleleid = keep.sum(-1).astype(np.int32)
    pos = np.cumsum(keep, axis=-1) - 1
    ii, jj, cc = np.nonzero(keep)
    obs[ii, jj, pos[ii, jj, cc]] = s[ii, jj, cc]
    return obs, alleleid, np.full(L, A, dtype=np.int32)


def run(obs, alleleid, allelenum, K, allo, sched, iters):
    rec = {}
    t = time.time()
    ch = capi.HipPolyChain(obs, alleleid, allelenum, K, rng_sched=sched, allo=allo)
    rec["ctx_s"] = time.time() - t
    ch.setseeds(13, 4, 1972)
    initd = np.array([np.float32(ch.ran1()) for _ in range(K)], dtype=np.float32)
    t = time.time()
    ch.chain_init(initd)
    ch.totallkh()
    rec["init_s"] = time.time() - t
    ch.profile(True)
    rec["iter_s"] = []
    for _ in range(iters):
        t = time.time()
        ch.iteration()
        rec["totallkh"] = ch.totallkh()
        rec["iter_s"].append(time.time() - t)
    rec["kernels_ms"] = {k: {"total": ms, "launches": n, "each": ms / n} for k, (ms, n) in ch.profile_results().items()}
    ch.close()
    return rec


def main():
    N, L, K = (int(x) for x in sys.argv[1:4]) if len(sys.argv) > 3 else (2000, 100, 10)
    iters = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    t = time.time()
    obs, alleleid, allelenum = panel(N, L, K, 20261016)
    print("data N=%d L=%d K=%d, %d alleles at every locus: %.1fs" % (N, L, K, A, time.time() - t), flush=True)
    out = {"N": N, "L": L, "K": K, "alleles": A, "runs": {}}
    for allo in (False, True):
        for sched in (capi.SCHED_REPLAY, capi.SCHED_KEYED):
            name = "%s_%s" % ("allo" if allo else "auto", "keyed" if sched == capi.SCHED_KEYED else "replay")
            rec = run(obs, alleleid, allelenum, K, allo, sched, iters)
            out["runs"][name] = rec
            print("%-12s ctx %.2fs init %.3fs iterations %s" % (name, rec["ctx_s"], rec["init_s"], " ".join("%.4fs" % x for x in rec["iter_s"])), flush=True)
            for k, v in sorted(rec["kernels_ms"].items(), key=lambda kv: -kv[1]["total"]):
                print("    %-18s %10.3f ms total %5d launches %10.3f ms each" % (k, v["total"], v["launches"], v["each"]))
    d = os.environ.get("TOOL_OUT", "tool_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "poly_alleles_time.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
