"""Time the fused hash+assign pass (library event timing) for the library in
LSHKM_LIB (default: the product build); profiling aid for kernel variants."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from amd import lshkm  # noqa: E402

N, D, K, L, KF = int(os.environ.get("TF_N", 10_000_000)), 128, int(os.environ.get("TF_K", 256)), 5, 4
ctx = lshkm.Context(0)
lib = lshkm.lib()
X = ctx.synth(0x5EED, N, D)
V, t, r, _ = lshkm.params_lsh_euclidean(12345, L, KF, D, 0.4)
lsh = lshkm.LSH(ctx, "euclidean", D, KF, L, N // 100, 0.4, V=V, t=t, r=r)
rows = (np.arange(K) * (N // K)).astype(np.int64)
Cc = X[torch.from_numpy(rows).to(X.device)].double()
dev = X.device
tuples = torch.empty((N, L, KF), dtype=torch.int32, device=dev)
bucket = torch.empty((N, L), dtype=torch.int32, device=dev)
assign = torch.empty((N,), dtype=torch.int32, device=dev)
dist = torch.empty((N,), dtype=torch.float64, device=dev)
p = lambda x: C.c_void_p(x.data_ptr())
# TF_SRC=1: the centroid override of a Lloyd step (the rows the centroids were taken from), as bench.py passes it
src32 = rows.astype(np.int32)
src = src32.ctypes.data_as(C.c_void_p) if os.environ.get("TF_SRC") == "1" else None
lshkm._ck(lib.lshkm_ctx_enable_timing(ctx.h, 1))
ms = C.c_float()
ts = []
for it in range(8):
    lshkm._ck(lib.lshkm_hash_assign(lsh.h, p(X), N, p(Cc), K, src, p(tuples), None, p(bucket), p(assign), p(dist)))
    lshkm._ck(lib.lshkm_last_kernel_ms(ctx.h, C.byref(ms)))
    if it >= 2:
        ts.append(ms.value)
torch.cuda.synchronize()
ctx.reset_stats()
t0 = torch.cuda.Event(enable_timing=True)
t1 = torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
t0.record()
for _ in range(5):
    lshkm._ck(lib.lshkm_hash_assign(lsh.h, p(X), N, p(Cc), K, src, p(tuples), None, p(bucket), p(assign), p(dist)))
t1.record()
torch.cuda.synchronize()
print(f"{os.path.basename(os.environ.get('LSHKM_LIB', 'liblshkm.so'))}: fused pass {np.median(ts):.3f} ms, "
      f"whole call {t0.elapsed_time(t1) / 5:.3f} ms, ambiguous {ctx.stat(lshkm.STAT_ASSIGN_AMBIG) // 5}, hash fix-up rows {ctx.stat(lshkm.STAT_HASH_FIX) // 5}, soft-x87 hash values {ctx.stat(lshkm.STAT_HASH_EXACT) // 5}, "
      f"checksum {int(assign.sum().item())} {float(dist.sum().item()):.6f}", flush=True)
