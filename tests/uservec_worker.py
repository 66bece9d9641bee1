"""One rank of the multi-rank user-vector test (tests/test_gpu_uservec_multirank.py).

Not a test module: launched as `python tests/uservec_worker.py RANK WORLD PORT OUTDIR`
(several ranks sharing the one MI355X over gloo). On this rank's contiguous
shard of the `mid` fixture's clustered rows: sharding.clusters_to_user_vectors_sharded
(the (sum, known) carry rank to rank over torch.distributed, the totals
finished on every rank); saves the bundle to OUTDIR/rank<R>.npz."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import uservec_np as unp  # noqa: E402
from amd import PKG, lshkm  # noqa: E402

sys.path.insert(0, PKG)
import sharding as sh  # noqa: E402


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = lshkm.Context(0)
    g = unp.load("mid")
    tweets = lshkm.Tweets(*unp.paths("mid"))
    tw = tweets.match(unp.strs(g, "row_id"))
    row0, n = sh.shard_range(len(tw), world, rank)
    assign = torch.from_numpy(np.ascontiguousarray(g["row_cluster"][row0:row0 + n])).to(ctx.dev)
    U, mean, unk_ptr, unk_idx, src, ids = sh.clusters_to_user_vectors_sharded(lshkm, ctx, tweets, tw[row0:row0 + n], assign,
                                                                              int(g["params"][2]))
    np.savez(os.path.join(out, f"rank{rank}.npz"), x=U.cpu().numpy(), mean=mean.cpu().numpy(), unk_ptr=unk_ptr.cpu().numpy(),
             unk_idx=unk_idx.cpu().numpy(), src=src.cpu().numpy(), ids=np.array([int(i) for i in ids], np.int32))
    ctx.sync()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
