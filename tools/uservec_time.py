#!/usr/bin/env python3
"""Time of clusters_to_user_vectors on the device at the C5 shard shape
(DESIGN.md §5d): V visits (default 10M), K = 1024 clusters, 100 coins, one or
two coins per tweet (1.5 on average) drawn as floor(100 u^3) -- skewed to the
low coins --, about four fifths of the scores positive: the shape
`gen_uservec_golden --time` builds for the reference's own function. The
tweet table and the visit list are made on the device; every clustered vector
is a tweet.

HIP events around each call, one warm-up call, the median of --reps calls; the
sums (lshkm_user_sums) and the finish (lshkm_user_finish) are timed apart and
together. --check also forms every chain on the host (a stable sort, then
sequential adds) and compares the device's sums and flags bit for bit. Prints
one JSON line.

    python tools/uservec_time.py [--visits 10000000] [--reps 7] [--check]
"""
import argparse
import importlib.util
import json
import os
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load():
    spec = importlib.util.spec_from_file_location("lshkm_amd", os.path.join(ROOT, "crypto-recommendation_amd", "lshkm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check(sums, known, assign, score, ci_ptr, ci_idx, K, C):
    """The sums against the host's: incidences in visit order, a stable sort by
    key, then every chain by np.add.accumulate (sequential fp64 adds)."""
    import numpy as np
    n = np.diff(ci_ptr)
    visit = np.repeat(np.arange(len(n)), n)                       # tweet v is visit v here
    key = assign[visit].astype(np.int64) * C + ci_idx
    want_known = np.zeros(K * C, np.uint8)
    want_known[key] = 1
    pos = score[visit] > 0
    key, x = key[pos], score[visit][pos]
    order = np.argsort(key, kind="stable")
    key, x = key[order], x[order]
    bounds = np.searchsorted(key, np.arange(K * C + 1))
    want = np.zeros(K * C)
    for c in range(K * C):
        if bounds[c + 1] > bounds[c]:
            want[c] = np.add.accumulate(np.concatenate([[0.0], x[bounds[c]:bounds[c + 1]]]))[-1]
    return (np.array_equal(want.view(np.uint64), sums.reshape(-1).view(np.uint64)) and
            np.array_equal(want_known, known.reshape(-1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--visits", type=int, default=10_000_000)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--coins", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--check", action="store_true", help="compare the sums with sequential chains formed on the host")
    a = ap.parse_args()
    lk = load()
    ctx = lk.Context(0)
    torch = ctx.torch
    V, K, C = a.visits, a.clusters, a.coins
    g = torch.Generator(device=ctx.dev)
    g.manual_seed(0xC5)
    # one tweet per visit: 1 or 2 distinct coins, ascending
    u = torch.rand((V, 2), generator=g, device=ctx.dev, dtype=torch.float64)
    coin = (C * u * u * u).to(torch.int32).clamp_(max=C - 1)
    two = torch.rand((V,), generator=g, device=ctx.dev) < 0.5
    two &= coin[:, 0] != coin[:, 1]
    lo, hi = torch.minimum(coin[:, 0], coin[:, 1]), torch.maximum(coin[:, 0], coin[:, 1])
    n = 1 + two.to(torch.int64)
    ci_ptr = torch.zeros((V + 1,), dtype=torch.int64, device=ctx.dev)
    torch.cumsum(n, 0, out=ci_ptr[1:])
    ci_idx = torch.empty((int(ci_ptr[-1].item()),), dtype=torch.int32, device=ctx.dev)
    ci_idx[ci_ptr[:-1]] = torch.where(two, lo, coin[:, 0])
    ci_idx[ci_ptr[:-1][two] + 1] = hi[two]
    t = torch.rand((V,), generator=g, device=ctx.dev, dtype=torch.float64) * 10.0 - 2.0      # four fifths positive
    score = t / torch.sqrt(t * t + 15.0)
    tw = torch.arange(V, dtype=torch.int32, device=ctx.dev)
    assign = torch.randint(0, K, (V,), generator=g, device=ctx.dev, dtype=torch.int32)
    table = (score, ci_ptr, ci_idx)
    del u, coin, two, lo, hi, n, t

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize(ctx.dev)
        return e0.elapsed_time(e1), out

    sums_ms, fin_ms = [], []
    for r in range(a.reps + 1):
        ms, (s, k) = timed(lambda: lk.user_sums(ctx, tw, assign, table, K, C))
        ms2, fin = timed(lambda: lk.user_finish(ctx, s, k))
        if r:                                     # the first call allocates the workspace
            sums_ms.append(ms)
            fin_ms.append(ms2)
    checked = None
    if a.check:
        checked = bool(check(s.cpu().numpy(), k.cpu().numpy(), assign.cpu().numpy(), score.cpu().numpy(),
                             ci_ptr.cpu().numpy(), ci_idx.cpu().numpy(), K, C))
    print(json.dumps({"row": "uservec_device", "checked_bit_for_bit": checked, "visits": V, "K": K, "coins": C, "mentions": int(ci_idx.numel()),
                      "reps": a.reps, "sums_ms_median": round(statistics.median(sums_ms), 3),
                      "sums_ms_min": round(min(sums_ms), 3), "sums_ms_max": round(max(sums_ms), 3),
                      "finish_ms_median": round(statistics.median(fin_ms), 3),
                      "total_ms_median": round(statistics.median([x + y for x, y in zip(sums_ms, fin_ms)]), 3),
                      "kept": int(fin[0].shape[0])}))


if __name__ == "__main__":
    main()
