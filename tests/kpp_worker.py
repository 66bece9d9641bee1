"""One rank of the multi-rank k-means++ test (tests/test_gpu_kmeanspp_multirank.py).

Not a test module: launched as `python tests/kpp_worker.py RANK WORLD PORT OUTDIR`
(several ranks sharing the one MI355X over gloo, or one rank with WORLD = 1 for
the single-process reference). Per leg, on this rank's contiguous row shard:
sharding.kmeans_pp_sharded over lshkm.KppShard (the exchange over
torch.distributed), then one ShardedLloyd.step() from that seeding; saves the
chosen rows, C0, the cluster IDs and the new centers to OUTDIR/rank<R>.npz."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from amd import PKG, lshkm  # noqa: E402

sys.path.insert(0, PKG)
import sharding as sh  # noqa: E402

# name: (data seed, N, d, K, metric, k-means++ seed)
LEGS = {"e32": (0x5EED, 50_000, 32, 8, "euclidean", 71), "c128": (0x5EED ^ 9, 20_000, 128, 8, "cosine", 72)}


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = lshkm.Context(0)
    res = {}
    for leg, (dseed, N, d, K, metric, seed) in LEGS.items():
        row0, n = sh.shard_range(N, world, rank)
        X = ctx.synth(dseed, n, d, row0=row0)
        rows, C0 = sh.kmeans_pp_sharded(lshkm.KppShard(ctx, X, metric), row0, n, N, K, seed)
        it = sh.ShardedLloyd(lshkm, ctx, None, X, torch.from_numpy(C0).to(ctx.dev), sh.local_src_rows(rows, row0, n),
                             metric=metric)
        it.step()
        res.update({f"{leg}_rows": rows, f"{leg}_C0": C0, f"{leg}_assign": it.assign.cpu().numpy(),
                    f"{leg}_centers": it.C.cpu().numpy()})
    np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
    ctx.sync()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
