"""Times the allotetraploid replay chain (-p 4 -ap 0) at BASELINE config 5's shape on the GPU:

    python tools/gpu_allo_time.py [iterations per block = 10] [N = 10000] [L = 20000] [K = 10]

N x L tetraploid loci with 4 alleles and 5 % missing from the C generator (host/synth_fast.c).  5 warm-up iterations; three blocks of timed
iterations with the per-kernel events off (host clock around isg_run + a read of the likelihood, which waits for the stream); then one
profiled block driven sweep by sweep: the host clock around update_P (its host loop, or the walk engine up to the look that brings back the
stream position; the stream is drained before it) and the per-kernel event times, k4_geno among them.  The last line is JSON."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instruct_amd import capi, synth

P_KERNELS = ("k4_sweep_counts", "k_pd_prep", "k_tapef_P", "k_wk_centers_P", "k_wk_table_P", "k_wk_walk_P", "k_pdirich_at", "k_freqf", "k4_exfreq", "k4_exfreq_w")

per = int(sys.argv[1]) if len(sys.argv) > 1 else 10
N, L, K = (int(sys.argv[k]) if len(sys.argv) > k else d for k, d in ((2, 10000), (3, 20000), (4, 10)))
obs, alleleid, allelenum = synth.make_tetraploid_fast(N, L, K, 4, 0.05, 20260105)
ch = capi.HipPolyChain(obs, alleleid, allelenum, K, allo=True)
ch.setseeds(13, 4, 1972)
ch.chain_init(np.array([np.float32(ch.ran1()) for _ in range(K)], dtype=np.float32))
ch.run(5)
ch.totallkh()
blocks = []
for b in range(3):
    t = time.perf_counter()
    ch.run(per)
    lk = ch.totallkh()
    blocks.append((time.perf_counter() - t) / per * 1e3)
    print("block %d: %.3f ms per iteration, totallkh %.6e" % (b, blocks[-1], lk), flush=True)
ch.profile(True)
tp = 0.0
for it in range(per):
    t = time.perf_counter()
    ch.update_P()
    tp += time.perf_counter() - t
    ch.update_S_POP()
    ch.update_ZQ(0)
    ch.update_geno()
    ch.cal_lkh()
    ch.totallkh()   # the stream is empty when the next update_P starts
    ch.lib.isg_iter_advance(ch.h)
ch.profile(False)
prof = {k: ms / per for k, (ms, n) in ch.profile_results().items()}
for k, ms in sorted(prof.items(), key=lambda kv: -kv[1]):
    print("%-18s %10.3f ms per iteration" % (k, ms))
pd = ch.p_device_stats()
out = {"shape": [N, L, K], "iterations_per_block": per, "ms_per_iteration": [round(x, 3) for x in blocks], "median_ms": round(sorted(blocks)[1], 3),
       "update_P_call_ms": round(tp / per * 1e3, 3), "update_P_kernels_ms": round(sum(prof.get(k, 0.0) for k in P_KERNELS), 3),
       "k4_geno_ms": round(prof.get("k4_geno", 0.0), 3), "update_P_device_sweeps": pd["device_sweeps"], "update_P_host_sweeps": pd["host_sweeps"],
       "segments": pd["segments"], "seeds": list(ch.seeds()), "totallkh": ch.totallkh()}
if hasattr(ch.lib, "isg_diag_allo_prefilter"):   # a library built with -DISG_DIAG_ALLO_PREFILTER counts the genotype draws it redoes in double
    import ctypes
    v = (ctypes.c_long * 2)()
    ch.lib.isg_diag_allo_prefilter(v)
    out["geno_draws"], out["geno_draws_redone"] = v[0], v[1]
    out["redone_share"] = v[1] / max(v[0], 1)
ch.close()
print(json.dumps(out))
