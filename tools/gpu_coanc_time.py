"""Times the posterior co-ancestry accumulation (isg_coanc_*) at BASELINE config 3, N = 10000, L = 5000, K = 5, replay:

    python tools/gpu_coanc_time.py [batches = 1,0] [iterations = 60] [N = 10000] [L = 5000] [K = 5]

For each batch (0 = the library's default): the isg_profile time of k_coanc_syrk per flush and of k_coanc_snap per step, taken over
16 steps on a chain that stands still (the flush's time does not depend on Q's values), then the iteration time with a co-ancestry
step every 10th iteration (the reference's default thinning) against the same run without, host clock around the loop and a read
of the likelihood that waits for the stream.  The yardstick of the flush: 16 N^2 / 2 bytes, the lower triangle read and written once,
over the bandwidth isg_copy_bandwidth measures on this card.  The JSON goes to $TOOL_OUT/coanc_time.json (default tool_out/)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instruct_amd import capi, synth

batches = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1, 0]
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 60
N, L, K = (int(sys.argv[k]) if len(sys.argv) > k else d for k, d in ((3, 10000), (4, 5000), (5, 5)))
THIN, STEPS = 10, 16

geno, an, mi = synth.make_diploid(N, L, K)
ch = capi.HipChain(geno, an, mi, K)
ch.setseeds(13, 4, 1972)
ch.chain_init(np.array([ch.ran1() for _ in range(K)], dtype=np.float32))
ch.run(5)
ch.totallkh()
copy_gbs = capi.copy_bandwidth(0)
floor_ms = 16.0 * N * N / 2 / (copy_gbs * 1e9) * 1e3
out = {"shape": [N, L, K], "copy_gbs": round(copy_gbs, 1), "flush_bytes": 16 * N * N // 2, "flush_floor_ms": round(floor_ms, 4), "batches": {}}
print("copy bandwidth %.1f GB/s: the flush moves %.1f MB, floor %.4f ms" % (copy_gbs, 16.0 * N * N / 2 / 1e6, floor_ms), flush=True)


def run_block(with_coanc):
    t = time.perf_counter()
    for it in range(iters):
        ch.iteration()
        if with_coanc and (it + 1) % THIN == 0:
            ch.coanc_step()
    ch.totallkh()
    return (time.perf_counter() - t) / iters * 1e3


plain = sorted(run_block(False) for _ in range(3))[1]
out["iteration_ms_without"] = round(plain, 4)
print("iteration without co-ancestry: %.4f ms" % plain, flush=True)
for b in batches:
    ch.coanc_begin(b)
    ch.coanc_step()
    ch.coanc_fetch()  # warm: first launches of both kernels
    ch.coanc_begin(b)
    ch.profile_reset()
    ch.profile(True)
    for _ in range(STEPS):
        ch.coanc_step()
    mean, steps = ch.coanc_fetch()
    ch.profile(False)
    prof = ch.profile_results()
    syrk_ms, flushes = prof["k_coanc_syrk"]
    snap_ms, snaps = prof["k_coanc_snap"]
    ch.profile_reset()
    ch.coanc_begin(b)
    with_ms = sorted(run_block(True) for _ in range(3))[1]
    rec = {"flushes": flushes, "syrk_ms_per_flush": round(syrk_ms / flushes, 4), "syrk_over_floor": round(syrk_ms / flushes / floor_ms, 3),
           "syrk_ms_per_step": round(syrk_ms / STEPS, 4), "snap_ms_per_step": round(snap_ms / snaps, 5), "iteration_ms_with": round(with_ms, 4),
           "added_ms_per_stored_step": round((with_ms - plain) * THIN, 4), "diag_mean": float(np.diag(mean).mean()), "steps": steps}
    out["batches"]["default" if b == 0 else str(b)] = rec
    print("batch %s: %s" % (b or "default", json.dumps(rec)), flush=True)
    ch.coanc_end()
ch.close()
d = os.environ.get("TOOL_OUT", "tool_out")
os.makedirs(d, exist_ok=True)
with open(os.path.join(d, "coanc_time.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
