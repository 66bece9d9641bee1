"""What the sharded k-means++ seeding's per-iteration host round trips cost on
one MI355X: sharding.kmeans_pp_sharded over in-process shards of one context
(sharding.LocalExchange: no network, so this is the host/device part of the
exchange alone) against lshkm_kmeans_pp, which runs its K - 1 iterations on the
stream with no round trip. The calls alternate inside each repetition; wall
time around calls that end in a device synchronise. Prints one JSON line.

    python tools/time_kpp_shard.py [--N 10000000] [--d 128] [--K 256] [--shards 1,2] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from amd import PKG, lshkm  # noqa: E402

sys.path.insert(0, PKG)
import sharding as sh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--shards", default="1,2")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric", default="euclidean")
    a = ap.parse_args()
    worlds = [int(w) for w in a.shards.split(",")]
    ctx = lshkm.Context(0)
    X = ctx.synth(0x5EED + 1, a.N, a.d)
    seed = 7

    def single(K):
        return lshkm.kmeans_pp_rows(ctx, X, K, a.metric, seed).astype(np.int64)

    ops = {}
    for w in worlds:
        spans = [sh.shard_range(a.N, w, r) for r in range(w)]
        ops[w] = (spans, [lshkm.KppShard(ctx, X[r0:r0 + n], a.metric) for r0, n in spans])

    def sharded(w, K):
        spans, o = ops[w]
        return sh.kmeans_pp_sharded(o, [s[0] for s in spans], [s[1] for s in spans], a.N, K, seed,
                                    exchange=sh.LocalExchange())[0]

    calls = {"single_device": single}
    for w in worlds:
        calls[f"shards_{w}"] = (lambda K, w=w: sharded(w, K))
    for fn in calls.values():          # warm up every call at this N (code objects, workspaces)
        fn(min(a.K, 4))
    ctx.sync()
    times = {k: [] for k in calls}
    want = None
    for _ in range(a.reps):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = fn(a.K)
            ctx.sync()
            times[name].append(time.perf_counter() - t0)
            want = rows if want is None else want
            assert np.array_equal(rows, want), name        # the same rows from every path
    line = {"N": a.N, "d": a.d, "K": a.K, "metric": a.metric, "reps": a.reps,
            "s": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()},
            "ms_per_iteration": {k: float(np.median(v)) * 1e3 / max(a.K - 1, 1) for k, v in times.items()}}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
