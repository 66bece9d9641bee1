"""Timings of the SURVEY §8 rows beside the headline (one MI355X): each row's
device call at a production-like size, inputs resident in HBM: "gpu_s" is the
time per call with calls back to back (HIP events on the library's stream, as
bench.py times its steps), "call_s" the median of single calls between host
syncs (host launch and sync latency included) -- next to the CPU restatement (oracle/, one
thread, OMP_NUM_THREADS=1, kind "port") on a bounded sample of the same
workload, scaled to the row's unit. Prints one JSON line per row.

    python tools/bench_rows.py [--rows cosine,kpp,range,sil,pam,update,lsh,cube,recom,csv,f64,cv,lshpc,cubepc,nearest,knn] [--no-cpu]
    python tools/bench_rows.py --rows main_program --main-dir DIR [--main-ref-seconds S]
"""
import argparse
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402
from amd import lshkm  # noqa: E402


class GpuTime(float):
    """Seconds per call, back to back (HIP events on the library's stream around
    reps calls, as bench.py times its steps); .call: the median of single calls
    each bracketed by host syncs (host launch and sync latency included)."""
    call = None


def gpu_time(ctx, fn, reps=5):
    fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    ctx.sync()
    torch.cuda.synchronize()
    t = GpuTime(e0.elapsed_time(e1) / 1e3 / reps)
    t.call = float(np.median(ts))
    t.calls = 2 * reps + 1          # fn's calls here (stat counters divide by it)
    return t


def cpu_time(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0



def cv_users(N, d, seed=0xBE7C4, known_256=128):
    """The users tools/gen_cv_golden.cpp --time forms (its make_users, kind 0):
    counter-based splitmix64 scores in [-1, 3), each known with probability
    known_256 / 256 (two at least), the mean = the known scores' sum in index
    order / their number, unknown indexes holding it. (x, mean, unk_ptr, unk_idx)."""
    def mix(z):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over="ignore"):
        idx = np.arange(N * d, dtype=np.uint64)
        score = (mix(np.uint64(seed) + np.uint64(2) * idx) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 * 4.0 - 1.0
        known = (mix(np.uint64(seed) + np.uint64(2) * idx + np.uint64(1)) >> np.uint64(56)).astype(np.int64) < known_256
    score, known = score.reshape(N, d), known.reshape(N, d)
    for i in np.nonzero(known.sum(axis=1) < 2)[0]:
        for j in range(d):
            if known[i].sum() >= 2:
                break
            known[i, j] = True
    mean = np.add.accumulate(np.where(known, score, 0.0), axis=1)[:, -1] / known.sum(axis=1)
    x = np.where(known, score, mean[:, None])
    ui = np.nonzero(~known)[1].astype(np.int32)
    up = np.concatenate([[0], np.cumsum((~known).sum(axis=1))]).astype(np.int64)
    return x, mean, up, ui


HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md


def emit(row, unit, units, t_gpu, cpu=None, note="", bytes_per_unit=None):
    line = {"row": row, "unit": unit, "units": units, "gpu_s": float(t_gpu), "gpu_rate": units / t_gpu}
    if getattr(t_gpu, "call", None) is not None:
        line["call_s"] = t_gpu.call          # one call between host syncs
    if bytes_per_unit:
        # algorithmic HBM bytes of the whole call (stated per unit) over its time per call
        gbs = units * bytes_per_unit / t_gpu / 1e9
        line["roofline"] = {"bound": "hbm", "bytes_per_unit": bytes_per_unit, "achieved": gbs,
                            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}
    if cpu:
        cu, ct, sample = cpu
        line["cpu_baseline"] = {"rate": cu / ct, "kind": "port", "cores": 1, "sample": sample}
        line["gpu_over_cpu"] = line["gpu_rate"] / line["cpu_baseline"]["rate"]
    if note:
        line["note"] = note
    print(json.dumps(line), flush=True)


def cube_probes_for(cube, Q, k, target):
    """The probe count (> 1) at which the users of Q see, on average, closest to
    `target` neighbours in the built cube, and that average: for probes > 1 a
    user's buckets are a prefix of its full probe sequence."""
    rp, _ = cube.buckets()
    sizes = np.diff(rp)
    uv = cube.vertices(Q).cpu().numpy()
    vs, n = np.unique(uv, return_counts=True)
    mean = np.zeros(1 << k)
    for v, c in zip(vs, n):
        mean += c * np.cumsum(sizes[oracle.cube_probe_seq(int(v), 1 << k, k)])
    mean /= len(uv)                                   # mean[p]: the average over p + 1 buckets, i.e. probes = p
    p = 2 + int(np.argmin(np.abs(mean[2:] - target)))
    return p, float(mean[p])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="cosine,kpp,range,sil,pam,update,lsh,cube,recom,csv,f64")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cv-sizes", default="20000,1000000", help="user counts of the cv row")
    ap.add_argument("--lshpc-sizes", default="20000,200000", help="user counts of the lshpc row")
    ap.add_argument("--pam-shapes", default="100000x16,1000000x256", help="NxK list of the pam row (d = 128)")
    ap.add_argument("--nearest-part", default="all", choices=["all", "new", "lloyd"], help="what the nearest row measures")
    ap.add_argument("--nearest-lloyd-n", type=int, default=0, help="nearest row: rows of the Lloyd route (0: all)")
    ap.add_argument("--main-dir", default="", help="main_program row: the directory gen_main_golden --time wrote")
    ap.add_argument("--main-ref-seconds", type=float, default=0.0, help="main_program row: the reference's seconds")
    a = ap.parse_args()
    rows = set(a.rows.split(","))
    ctx = lshkm.Context(0)
    cpu = not a.no_cpu

    if "update" in rows:     # k_means (update.hpp:37-86), exact-order sums, C3 shape
        N, d, K = 10_000_000, 128, 256
        X = ctx.synth(0x5EED, N, d)
        src = (np.arange(K) * (N // K)).astype(np.int64)
        C = X[torch.from_numpy(src).to(ctx.dev)].double()
        asg, _ = lshkm.lloyd_assign(ctx, X, C, "euclidean", src.astype(np.int32))
        t = gpu_time(ctx, lambda: lshkm.kmeans_update(ctx, X, asg, C, "euclidean", 0.05))
        c = None
        if cpu:
            n = 1_000_000
            Xh, ah = X[:n].cpu().numpy(), asg[:n].cpu().numpy()
            c = (n, cpu_time(lambda: oracle.kmeans_update(Xh, ah, C.cpu().numpy(), "euclidean", 0.05)),
                 f"{n} rows, K={K}, d={d}")
        emit("k_means update", "rows/s", N, t, c, "N=10M, d=128, K=256; bytes: the row + its cluster id",
             bytes_per_unit=4 * d + 4)
        del X

    if "cosine" in rows:     # lloyds_assignment, cosine metric (assignment.hpp:52-75)
        N, d, K = 10_000_000, 128, 256
        X = ctx.synth(0x5EED + 4, N, d)
        src = (np.arange(K) * (N // K)).astype(np.int64)
        C = X[torch.from_numpy(src).to(ctx.dev)].double()
        ctx.reset_stats()
        t = gpu_time(ctx, lambda: lshkm.lloyd_assign(ctx, X, C, "cosine"))
        amb = ctx.stat(lshkm.STAT_ASSIGN_AMBIG) / t.calls
        cfix = ctx.stat(lshkm.STAT_COS_FIX) / t.calls
        os.environ["LSHKM_ASSIGN_PATH"] = "exact"
        te = gpu_time(ctx, lambda: lshkm.lloyd_assign(ctx, X, C, "cosine"), reps=1)
        del os.environ["LSHKM_ASSIGN_PATH"]
        c = None
        if cpu:
            n = 20_000
            Xh = X[:n].cpu().numpy()
            c = (n, cpu_time(lambda: oracle.lloyd_assign(Xh, C.cpu().numpy(), "cosine", None)), f"{n} rows, K={K}")
        emit("lloyds_assignment (cosine)", "rows/s", N, t, c,
             f"N=10M, d=128, K=256; hi-only f16 kernel (normalised centroids), {amb:.0f} rows/call to the pruned exact "
             f"pass, {cfix:.0f} winner distances/call to the soft-x87 chain; "
             f"exact all-K pass alone {te * 1e3:.1f} ms; bytes: the row + cluster id and distance",
             bytes_per_unit=4 * d + 12)
        # main.cpp's cosine flow in one pass: CosineGGen buckets (L=5, k=4) + cosine Lloyd
        R, _ = lshkm.params_lsh_cosine(12345, 5, 4, d)
        lsh = lshkm.LSH(ctx, "cosine", d, 4, 5, R=R)
        th = gpu_time(ctx, lambda: lshkm.hash_assign(lsh, X, C, tuples=False, bucket=True, metric="cosine"))
        tsep = gpu_time(ctx, lambda: (lsh.hash(X, tuples=False, phi=False), lshkm.lloyd_assign(ctx, X, C, "cosine")))
        emit("hash_assign (cosine LSH + cosine Lloyd)", "rows/s", N, th, None,
             f"N=10M, d=128, L=5, k=4, K=256, one pass (lshkm_hash_assign_metric); the two separate calls "
             f"{tsep * 1e3:.2f} ms; bytes: the row + cluster id, distance and 5 bucket ids",
             bytes_per_unit=4 * d + 12 + 4 * 5)
        del X

    if "kpp" in rows:        # k_means_pp (initialization.hpp:71-156)
        N, d, K = 1_000_000, 128, 64
        X = ctx.synth(0x5EED + 1, N, d)
        t = gpu_time(ctx, lambda: lshkm.kmeans_pp_rows(ctx, X, K, "euclidean", 7), reps=3)
        c = None
        if cpu:
            n = 100_000
            Xh = X[:n].cpu().numpy()
            c = (n * K, cpu_time(lambda: oracle.kmeans_pp(Xh, K, "euclidean", 7)), f"{n} rows, K={K}")
        emit("k_means_pp", "row-centroid steps/s", N * K, t, c,
             "N=1M, d=128, K=64, euclidean; bytes: one pass over the rows and D^2 per centroid",
             bytes_per_unit=4 * d + 8)
        del X

    if "range" in rows:      # lsh_range_assignment (assignment.hpp:108-217)
        N, d, K, L, k = 1_000_000, 128, 256, 5, 4
        X = ctx.synth(0x5EED + 2, N, d)
        V, tt, r, _ = lshkm.params_lsh_euclidean(77, L, k, d, 4.0)
        lsh = lshkm.LSH(ctx, "euclidean", d, k, L, N // 100, 4.0, V=V, t=tt, r=r)
        lsh.build(X)
        src = (np.arange(K) * (N // K)).astype(np.int32)
        Q = X[torch.from_numpy(src.astype(np.int64)).to(ctx.dev)]
        C = Q.double()

        def run():
            ptr, ci = lsh.query(Q, filtered=False, device=True)
            return lshkm.range_assign(ctx, X, C, ptr, ci, "euclidean", src_rows=src)
        t = gpu_time(ctx, run, reps=3)
        c = None
        if cpu:
            n = 100_000
            Xs = X[:n].contiguous()
            lsh2 = lshkm.LSH(ctx, "euclidean", d, k, L, n // 100, 4.0, V=V, t=tt, r=r)
            lsh2.build(Xs)
            s2 = (np.arange(K) * (n // K)).astype(np.int32)
            Q2 = Xs[torch.from_numpy(s2.astype(np.int64)).to(ctx.dev)]
            p2, c2 = lsh2.query(Q2, filtered=False)
            Xh, C2 = Xs.cpu().numpy(), Q2.double().cpu().numpy()
            c = (n, cpu_time(lambda: oracle.range_assign(Xh, C2, p2, c2, "euclidean", src_rows=s2)), f"{n} rows, K={K}")
        emit("lsh_range_assignment", "rows/s", N, t, c, "N=1M, d=128, K=256, L=5, k=4, w=4 (query + range + Lloyd rest)")
        del X

    if "sil" in rows:        # silhouette_cluster (silhouette.hpp:31-144)
        N, d, K = 100_000, 128, 16
        X = ctx.synth(0x5EED + 3, N, d)
        src = (np.arange(K) * (N // K)).astype(np.int64)
        C = X[torch.from_numpy(src).to(ctx.dev)].double()
        asg, _ = lshkm.lloyd_assign(ctx, X, C, "euclidean", src.astype(np.int32))
        pairs = float(np.sum(np.bincount(asg.cpu().numpy(), minlength=K).astype(np.float64) ** 2) * 2)
        t = gpu_time(ctx, lambda: lshkm.silhouette(ctx, X, asg, C, "euclidean"), reps=3)
        c = None
        if cpu:
            n = 10_000
            Xh = X[:n].cpu().numpy()
            ah, _ = oracle.lloyd_assign(Xh, C.cpu().numpy(), "euclidean", None)
            p2 = float(np.sum(np.bincount(ah, minlength=K).astype(np.float64) ** 2) * 2)
            c = (p2, cpu_time(lambda: oracle.silhouette(Xh, ah, C.cpu().numpy(), "euclidean")), f"{n} rows, K={K}")
        emit("silhouette_cluster", "distance pairs/s", pairs, t, c, "N=100k, d=128, K=16")
        del X

    if "pam" in rows:        # pam_lloyds (update.hpp:89-142): the product library, then the test build
        # with the exact chain forced and with the MFMA screen forced for every cluster
        import amd
        sw = amd.switched()
        sctx = sw.Context(0)
        shapes = [(int(s[0]), 128, int(s[1])) for s in (p.split("x") for p in a.pam_shapes.split(","))]
        for N, d, K in shapes:
            for kind in ("grid", "normal"):
                X = ctx.synth(0x5EED + 3, N, d, kind=kind)
                src = (np.arange(K) * (N // K)).astype(np.int64)
                C = X[torch.from_numpy(src).to(ctx.dev)].double()
                asg, _ = lshkm.lloyd_assign(ctx, X, C, "euclidean", src.astype(np.int32))
                sizes = np.bincount(asg.cpu().numpy(), minlength=K).astype(np.float64)
                pairs = float(np.sum(sizes ** 2))
                reps = 2 if pairs > 2e9 else 3
                t = gpu_time(ctx, lambda: lshkm.pam_update(ctx, X, asg, K, "euclidean"), reps=reps)
                res, times, left = {}, {}, 0
                for path in ("exact", "screen"):
                    os.environ["LSHKM_PAM_PATH"] = path
                    sctx.reset_stats()
                    res[path] = sw.pam_update(sctx, X, asg, K, "euclidean")
                    if path == "screen":
                        left = sctx.stat(sw.STAT_PAM_EXACT)
                    times[path] = gpu_time(sctx, lambda: sw.pam_update(sctx, X, asg, K, "euclidean"), reps=reps)
                    del os.environ["LSHKM_PAM_PATH"]
                same = all(np.array_equal(res["exact"][i], res["screen"][i]) for i in (0, 2))
                emit("pam_lloyds", "distance pairs/s", pairs, t, None,
                     f"N={N}, d={d}, K={K}, {kind} rows, clusters of {int(sizes.min())}..{int(sizes.max())}; exact-only "
                     f"{times['exact'] * 1e3:.2f} ms, screen forced {times['screen'] * 1e3:.2f} ms with {left} of {N} "
                     f"members ({left / N:.4%}) left to the exact chain; results equal: {same}")
                del X

    if "lsh" in rows:        # create_LSH_hashtables + get_LSH_filtered_combined_buckets (C2)
        N, d, L, k = 1_000_000, 128, 5, 4
        X = ctx.synth(0x5EED, N, d)
        V, tt, r, _ = lshkm.params_lsh_euclidean(12345, L, k, d, 0.4)
        lsh = lshkm.LSH(ctx, "euclidean", d, k, L, N // 100, 0.4, V=V, t=tt, r=r)
        tb = gpu_time(ctx, lambda: lsh.build(X))
        c = None
        if cpu:
            n = 200_000
            Xh = X[:n].cpu().numpy()
            c = (n, cpu_time(lambda: oracle.bucket_csr(oracle.lsh_hash_euclid(Xh, V, tt, np.float32(0.4), r, N // 100)[2],
                                                       N // 100)), f"{n} rows")
        emit("create_LSH_hashtables", "rows/s", N, tb, c,
             "C2: N=1M, d=128, L=5, k=4, w=0.4, nb=10k; bytes: the row + per table its bucket key and CSR slot",
             bytes_per_unit=4 * d + 5 * 8)
        nq = 65_536
        qrows = torch.arange(nq, device=ctx.dev) * (N // nq)
        Q = X[qrows]
        alias = qrows.to(torch.int32)
        tq = gpu_time(ctx, lambda: lsh.query(Q, True, alias, device=True))
        tot = int(lsh.query(Q, True, alias, device=True)[0][-1])
        emit("get_LSH_filtered_combined_buckets", "queries/s", nq, tq, None,
             f"65,536 dataset-row queries, C2 index; {tot} rows returned",)
        del X

    if "cube" in rows:       # create_hypercube + get_hypercube_combined_buckets (C4)
        N, d, k = 10_000_000, 128, 14
        X = ctx.synth(0x5EED, N, d)
        V, tt, st = lshkm.params_cube_euclidean(4242, k, d, 2.0)
        cubes = []

        def fresh_build():        # create_hypercube: new generators, an empty coin memo
            c = lshkm.Cube(ctx, "euclidean", d, k, 2.0, V=V, t=tt, rng_state=st)
            c.build(X)
            cubes.append(c)
        tb = gpu_time(ctx, fresh_build, reps=3)
        cube = cubes[-1]
        tr = gpu_time(ctx, lambda: cube.build(X), reps=3)
        emit("create_hypercube", "rows/s", N, tb, None,
             f"C4: N=10M, d=128, d'=14, w=2 (euclidean F coins), fresh cube each build; "
             f"rebuild with the coins already drawn {tr * 1e3:.2f} ms; bytes: the row + its vertex and CSR slot",
             bytes_per_unit=4 * d + 8)
        nq = 65_536
        Q = X[torch.arange(nq, device=ctx.dev) * (N // nq)]
        tq = gpu_time(ctx, lambda: cube.query(Q, 14, device=True), reps=3)
        tot = int(cube.query(Q, 14, device=True)[0][-1])
        emit("get_hypercube_combined_buckets", "queries/s", nq, tq, None,
             f"65,536 queries, probes=14 (Hamming<=1); {tot} candidate rows returned (bytes: 4 B read + 4 B "
             f"written per candidate)", bytes_per_unit=8.0 * tot / nq)
        del X

    if "recom" in rows:      # get_P_closest + get_top_N_recom (crypto_rec.hpp:213-325)
        N, d, Q, P, NT = 200_000, 100, 20_000, 20, 5
        rng = np.random.default_rng(5)
        Xh = rng.integers(-40, 41, size=(N, d)).astype(np.float64) / 8.0
        X = torch.from_numpy(Xh).to(ctx.dev)
        Uh = Xh[rng.integers(0, N, Q)]
        U = torch.from_numpy(Uh).to(ctx.dev)
        cand = [np.sort(rng.choice(N, 200, replace=False)).astype(np.int32) for _ in range(Q)]
        cp = torch.from_numpy(np.cumsum([0] + [len(c) for c in cand]).astype(np.int64)).to(ctx.dev)
        ci = torch.from_numpy(np.concatenate(cand)).to(ctx.dev)
        t = gpu_time(ctx, lambda: lshkm.p_closest(ctx, X, U, cp, ci, P))
        c = None
        if cpu:
            q2 = 2000
            cph, cih = cp[:q2 + 1].cpu().numpy(), ci[:int(cp[q2])].cpu().numpy()
            c = (q2, cpu_time(lambda: oracle.p_closest(Xh, Uh[:q2], cph, cih, P)), f"{q2} users x 200 candidates")
        emit("get_P_closest", "users/s", Q, t, c, f"N={N}, d={d}, {Q} users x 200 candidates, P={P}")

    if "f64" in rows:        # the reference's own shapes: fp64 user vectors, d = number of coins
        # (main.cpp:149-222 cosine LSH recommend, :240-281 clustering recommend; crypto_rec.hpp:78-140)
        # main.cpp:155-168: every user queries the cosine index over all users
        # (k = 4: a bucket holds ~N/16 users per table, so the work grows as N^2)
        N, d, P, NT = 20_000, 100, 20, 5
        rng = np.random.default_rng(11)
        Xh = rng.standard_normal((N, d))                  # general doubles: the _f64 entry points
        X = torch.from_numpy(Xh).to(ctx.dev)
        R, _ = lshkm.params_lsh_cosine(12345, 5, 4, d)
        lsh = lshkm.LSH(ctx, "cosine", d, 4, 5, R=R)
        tb = gpu_time(ctx, lambda: lsh.build(X))
        emit("create_LSH_hashtables (cosine, fp64 rows)", "rows/s", N, tb, None,
             f"N={N}, d={d} fp64 user vectors, L=5, k=4 (main.cpp:155); bytes: the fp64 row + per table its "
             f"bucket key and CSR slot", bytes_per_unit=8 * d + 5 * 8)
        nq = N
        qrows = torch.arange(nq, device=ctx.dev)
        Q = X[qrows]
        alias = qrows.to(torch.int32)
        tq = gpu_time(ctx, lambda: lsh.query(Q, True, alias, device=True), reps=3)
        cptr, cidx = lsh.query(Q, True, alias, device=True)
        tot = int(cptr[-1])
        emit("get_LSH_filtered_combined_buckets (cosine, fp64 rows)", "queries/s", nq, tq, None,
             f"every user of N={N} as a query; {tot} candidate rows ({tot / nq:.0f} per query); bytes: 4 B "
             f"read + 4 B written per candidate", bytes_per_unit=8.0 * tot / nq)
        tp = gpu_time(ctx, lambda: lshkm.p_closest(ctx, X, Q, cptr, cidx, P), reps=3)
        emit("get_P_closest (fp64 rows)", "candidates/s", tot, tp, None,
             f"{nq} users x {tot / nq:.0f} candidates, d={d}, P={P}; bytes: the candidate's fp64 row (the {N} rows "
             f"fit the Infinity Cache: L2/MALL bandwidth, not HBM)", bytes_per_unit=8 * d + 4)
        idx, sim, cnt = lshkm.p_closest(ctx, X, Q, cptr, cidx, P)
        xm = X.mean(dim=1).contiguous()
        um = xm[qrows].contiguous()
        unk = [np.sort(rng.choice(d, 20, replace=False)).astype(np.int32) for _ in range(nq)]
        up = torch.from_numpy(np.arange(nq + 1, dtype=np.int64) * 20).to(ctx.dev)
        ui = torch.from_numpy(np.concatenate(unk)).to(ctx.dev)
        tn = gpu_time(ctx, lambda: lshkm.top_n_recom(ctx, X, xm, um, up, ui, idx, sim, cnt, NT), reps=3)
        emit("get_top_N_recom (fp64 rows)", "users/s", nq, tn, None, f"{nq} users, P={P}, 20 unknown coins each, N={NT}")
        del lsh, cptr, cidx, X
        # clustering recommendation's Lloyd + k_means on fp64 user vectors (main.cpp:248-258), at 1M users
        N, K = 1_000_000, 256
        X = torch.from_numpy(rng.standard_normal((N, d))).to(ctx.dev)
        src = (np.arange(K) * (N // K)).astype(np.int64)
        C = X[torch.from_numpy(src).to(ctx.dev)].clone()
        for metric in ("euclidean", "cosine"):
            ctx.reset_stats()
            t = gpu_time(ctx, lambda: lshkm.lloyd_assign(ctx, X, C, metric))
            amb = ctx.stat(lshkm.STAT_ASSIGN_AMBIG) / t.calls
            emit(f"lloyds_assignment ({metric}, fp64 rows)", "rows/s", N, t, None,
                 f"N={N}, d={d} fp64, K={K}; {amb:.0f} rows/call to the exact pass; bytes: the fp64 row + id and "
                 f"distance", bytes_per_unit=8 * d + 12)
        asg, _ = lshkm.lloyd_assign(ctx, X, C, "euclidean")
        t = gpu_time(ctx, lambda: lshkm.kmeans_update(ctx, X, asg, C, "euclidean", 0.05))
        emit("k_means update (fp64 rows)", "rows/s", N, t, None, f"N={N}, d={d} fp64, K={K}; bytes: the fp64 row + id",
             bytes_per_unit=8 * d + 4)
        del X

    if "cv" in rows:         # lsh_rec_10_fold_validation_A (main.cpp:393-437)
        d, k, L, P, div = 100, 4, 5, 20, 4
        tsec, seeds = 1546300800, np.arange(1, 11, dtype=np.uint64)       # gen_cv_golden --time: time(), the clock
        for N in (int(v) for v in a.cv_sizes.split(",")):
            xh, xmh, uph, uih = cv_users(N, d)
            X, xm, up, ui = (torch.from_numpy(v).to(ctx.dev) for v in (xh, xmh, uph, uih))
            res = {}

            def whole():
                res["v"] = lshkm.lsh_validate10(ctx, X, xm, up, ui, "cosine", k, L, div, 0.01, P, tsec, tsec, seeds)
            t = gpu_time(ctx, whole, reps=2)
            mae, fs, fc = res["v"]
            # fold 0's parts through the public pieces (what the driver chains on its stream)
            F = N // 10
            split = torch.from_numpy(lshkm.cv_split10(tsec, N).ravel().astype(np.int64)).to(ctx.dev)
            draw = torch.full((N,), int(lshkm.cv_draws([tsec])[0, 0]), dtype=torch.int32, device=ctx.dev)
            H, hm, hi, old = lshkm.cv_hide(ctx, X, xm, up, ui, draw)
            W, Wm = X[split].contiguous(), xm[split].contiguous()
            W[:F], Wm[:F] = H[split[:F]], hm[split[:F]]
            hi0, old0 = hi[split[:F]].contiguous(), old[split[:F]].contiguous()
            R, _ = lshkm.params_lsh_cosine(int(seeds[0]), L, k, d)
            lsh = lshkm.LSH(ctx, "cosine", d, k, L, R=R)
            Q = W[:F].contiguous()
            parts = {"hash_build": gpu_time(ctx, lambda: lsh.build(W), reps=2)}
            ptr, idx = lsh.query(Q, True, device=True)
            parts["query_exclude"] = gpu_time(ctx, lambda: lshkm.cv_exclude(ctx, *lsh.query(Q, True, device=True), 0, F), reps=2)
            eptr, eidx = lshkm.cv_exclude(ctx, ptr, idx, 0, F)
            parts["p_closest"] = gpu_time(ctx, lambda: lshkm.p_closest(ctx, W, Q, eptr, eidx, P), reps=2)
            ni, ns, nc = lshkm.p_closest(ctx, W, Q, eptr, eidx, P)
            hp = torch.arange(F + 1, dtype=torch.int64, device=ctx.dev)
            parts["predict"] = gpu_time(ctx, lambda: lshkm.predicted_scores(ctx, W, Wm, Wm[:F], hp, hi0, ni, ns, nc), reps=2)
            pred = lshkm.predicted_scores(ctx, W, Wm, Wm[:F], hp, hi0, ni, ns, nc)
            parts["sum"] = gpu_time(ctx, lambda: lshkm.cv_fold_sum(ctx, hi0, old0, pred, eptr), reps=2)
            ks, cnt, _ = lshkm.cv_fold_sum(ctx, hi0, old0, pred, eptr)
            ctx.sync()
            same = float(ks[0]) == fs[0] and int(cnt[0]) == fc[0]
            cand = int(eptr[-1])
            emit("lsh_rec_10_fold_validation_A", "users/s", 10 * F, t, None,
                 f"N={N}, d={d} fp64 users, cosine, k={k}, L={L}, P={P}; mae {mae!r} ({float(mae).hex()}), "
                 f"{int(fc.sum())} users calculated; fold 0 through the public pieces (ms): "
                 + ", ".join(f"{n} {v * 1e3:.2f}" for n, v in parts.items())
                 + f"; {cand} candidates after exclusion ({cand / F:.0f} per user); fold 0 sum equals the driver's: {same}")
            del X, W, H, lsh, ptr, idx, eptr, eidx

    def event_ms(fn, warm=3, reps=10):
        """HIP events around single calls: (median, min, max) ms of reps after warm warm-ups."""
        ms = []
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            ctx.sync()
            torch.cuda.synchronize()
            if i >= warm:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    if "lshpc" in rows:      # main.cpp:160-162 from the index: the lists sequence against lshkm_lsh_p_closest
        d, k, L, P = 100, 4, 5, 20
        tsec, seeds = 1546300800, np.arange(1, 11, dtype=np.uint64)

        for N in (int(v) for v in a.lshpc_sizes.split(",")):
            # the cv row's fold-0 inputs: the pool W in split order, fold 0's users hidden, excluded as rows [0, F)
            xh, xmh, uph, uih = cv_users(N, d)
            X, xm, up, ui = (torch.from_numpy(v).to(ctx.dev) for v in (xh, xmh, uph, uih))
            F = N // 10
            split = torch.from_numpy(lshkm.cv_split10(tsec, N).ravel().astype(np.int64)).to(ctx.dev)
            draw = torch.full((N,), int(lshkm.cv_draws([tsec])[0, 0]), dtype=torch.int32, device=ctx.dev)
            H, hm, hi, old = lshkm.cv_hide(ctx, X, xm, up, ui, draw)
            W = X[split].contiguous()
            W[:F] = H[split[:F]]
            R, _ = lshkm.params_lsh_cosine(int(seeds[0]), L, k, d)
            lsh = lshkm.LSH(ctx, "cosine", d, k, L, R=R)
            lsh.build(W)
            Q = W[:F].contiguous()
            del X, H
            out = {}

            def sequence():
                eptr, eidx = lshkm.cv_exclude(ctx, *lsh.query(Q, True, device=True), 0, F)
                out["seq"] = lshkm.p_closest(ctx, W, Q, eptr, eidx, P)
                out["cand"] = int(eptr[-1])

            def direct():
                out["new"] = lshkm.lsh_p_closest(ctx, lsh, W, Q, P, exclude=(0, F))
            t_seq = event_ms(sequence)
            ctx.reset_stats()
            t_new = event_ms(direct)
            st = [ctx.stat(i) // 13 for i in (12, 13, 14, 15)]
            same = all(torch.equal(g, w) for g, w in zip((out["new"][0], out["new"][1].view(torch.int64), out["new"][2]),
                                                         (out["seq"][0], out["seq"][1].view(torch.int64), out["seq"][2])))
            print(json.dumps({
                "row": "lshpc", "users": F, "pool": 10 * F, "d": d, "k": k, "L": L, "P": P,
                "candidates": out["cand"], "sequence_ms": {"median": t_seq[0], "min": t_seq[1], "max": t_seq[2]},
                "lsh_p_closest_ms": {"median": t_new[0], "min": t_new[1], "max": t_new[2]},
                "speedup_median": t_seq[0] / t_new[0], "bar_new_max_below_sequence_min": t_new[2] < t_seq[1],
                "stat_settled": st[0], "stat_lists": st[1], "stat_kept": st[2], "stat_seen": st[3],
                "outputs_identical": same,
                "note": "query + exclusion + p_closest against lshkm_lsh_p_closest on the same handle; HIP events, "
                        "median of 10 after 3 warm-ups; stats per call"}), flush=True)
            del W, Q, lsh, out

    if "cubepc" in rows:     # the same from a built hypercube: cube.query + p_closest against lshkm_cube_p_closest
        # k = 6; probes: the count at which a user sees on average closest to 0.41 of the pool, the lshpc row's
        # share (8,130 / 20,000, 82,579 / 200,000): these rows fill the 64 vertices unevenly, so it is found, not set
        d, k, P = 100, 6, 20
        tsec, seeds = 1546300800, np.arange(1, 11, dtype=np.uint64)
        for N in (int(v) for v in a.lshpc_sizes.split(",")):
            # the cv row's fold-0 inputs, as the lshpc row's: the pool W in split order, fold 0's users hidden
            xh, xmh, uph, uih = cv_users(N, d)
            X, xm, up, ui = (torch.from_numpy(v).to(ctx.dev) for v in (xh, xmh, uph, uih))
            F = N // 10
            split = torch.from_numpy(lshkm.cv_split10(tsec, N).ravel().astype(np.int64)).to(ctx.dev)
            draw = torch.full((N,), int(lshkm.cv_draws([tsec])[0, 0]), dtype=torch.int32, device=ctx.dev)
            H, hm, hi, old = lshkm.cv_hide(ctx, X, xm, up, ui, draw)
            W = X[split].contiguous()
            W[:F] = H[split[:F]]
            R, st = lshkm.params_cube_cosine(int(seeds[0]), k, d)
            cube = lshkm.Cube(ctx, "cosine", d, k, R=R, rng_state=st)
            cube.build(W)
            Q = W[:F].contiguous()
            del X, H
            probes, _ = cube_probes_for(cube, Q, k, 0.41 * 10 * F)
            out = {}

            def sequence():
                ptr, idx = cube.query(Q, probes, device=True)
                out["seq"] = lshkm.p_closest(ctx, W, Q, ptr, idx, P)
                out["cand"] = int(ptr[-1])

            def direct():
                out["new"] = lshkm.cube_p_closest(ctx, cube, W, Q, probes, P)
            t_seq = event_ms(sequence)
            ctx.reset_stats()
            t_new = event_ms(direct)
            st = [ctx.stat(i) // 13 for i in (12, 13, 14, 15)]
            same = all(torch.equal(g, w) for g, w in zip((out["new"][0], out["new"][1].view(torch.int64), out["new"][2]),
                                                         (out["seq"][0], out["seq"][1].view(torch.int64), out["seq"][2])))
            print(json.dumps({
                "row": "cubepc", "users": F, "pool": 10 * F, "d": d, "k": k, "probes": probes, "P": P,
                "candidates": out["cand"], "candidates_per_user": out["cand"] / F,
                "sequence_ms": {"median": t_seq[0], "min": t_seq[1], "max": t_seq[2]},
                "cube_p_closest_ms": {"median": t_new[0], "min": t_new[1], "max": t_new[2]},
                "speedup_median": t_seq[0] / t_new[0], "bar_new_max_below_sequence_min": t_new[2] < t_seq[1],
                "stat_settled": st[0], "stat_lists": st[1], "stat_kept": st[2], "stat_seen": st[3],
                "outputs_identical": same,
                "note": "cube.query + p_closest against lshkm_cube_p_closest on the same handle; HIP events, "
                        "median of 10 after 3 warm-ups; stats per call"}), flush=True)
            del W, Q, cube, out

    if "nearest" in rows:    # min_vector_*_dist (utils.hpp:107-140) for all queries: lshkm_min_vector_dist
        # --nearest-part new: the call, its counters and the CPU port; lloyd: the only route without it,
        # lshkm_lloyd_assign (exact mode) with the rows as fp64 centroids, over the first --nearest-lloyd-n rows
        shapes = [("grid fp32", 1_000_000, 128, 4096, "euclidean"), ("grid fp32", 1_000_000, 128, 4096, "cosine"),
                  ("cv_users fp64", 200_000, 20, 20_000, "cosine")]
        S = (lshkm.STAT_NEAREST_SETTLED, lshkm.STAT_NEAREST_SCAN, lshkm.STAT_NEAREST_EXACT)
        for kind, N, d, nq, metric in shapes:
            if kind == "grid fp32":
                X, Q = ctx.synth(0x5EED + 21, N, d), ctx.synth(0x5EED + 22, nq, d)
            else:
                X = torch.from_numpy(cv_users(N, d)[0]).to(ctx.dev)
                Q = torch.from_numpy(cv_users(nq, d, seed=0xBE7C5)[0]).to(ctx.dev)
            line = {"row": "nearest", "rows": kind, "N": N, "d": d, "nq": nq, "metric": metric}
            if a.nearest_part in ("new", "all"):
                out = {}

                def call():
                    out["new"] = lshkm.min_vector_dist(ctx, X, Q, metric)
                ctx.reset_stats()
                t_new = event_ms(call, warm=2, reps=5)
                st = [ctx.stat(i) // 7 for i in S]
                line.update({"min_vector_dist_ms": {"median": t_new[0], "min": t_new[1], "max": t_new[2]},
                             "pairs_per_s": N * nq / (t_new[0] / 1e3), "stat_settled": st[0], "stat_scan": st[1],
                             "stat_exact": st[2], "exact_per_query": st[2] / nq})
                if cpu:
                    m = 256
                    Xh, Qh = X.cpu().numpy(), Q[:m].cpu().numpy()
                    t0 = time.perf_counter()
                    wa, wd = oracle.lloyd_assign(Qh, Xh, metric)
                    tc = time.perf_counter() - t0
                    line.update({"cpu_port": {"queries": m, "seconds": tc, "cores": int(os.environ["OMP_NUM_THREADS"]),
                                              "pairs_per_s": N * m / tc},
                                 "gpu_over_cpu": (N * nq / (t_new[0] / 1e3)) / (N * m / tc),
                                 "identical_to_port": bool(np.array_equal(out["new"][0][:m].cpu().numpy().view(np.uint64),
                                                                          wd.view(np.uint64)) and
                                                           np.array_equal(out["new"][1][:m].cpu().numpy(), wa))})
            if a.nearest_part in ("lloyd", "all"):
                Nl = min(N, a.nearest_lloyd_n or N)
                Xl = X[:Nl]
                Cc = Xl.double()
                ctx.set_dist_mode("exact")
                try:
                    ctx.reset_stats()
                    got = {}

                    def lloyd():
                        got["a"], got["d"] = lshkm.lloyd_assign(ctx, Q, Cc, metric)
                    t_l = event_ms(lloyd, warm=1, reps=3)
                    amb = ctx.stat(lshkm.STAT_ASSIGN_AMBIG) // 4
                finally:
                    ctx.set_dist_mode("certified")
                t_s = event_ms(lambda: got.update(n=lshkm.min_vector_dist(ctx, Xl, Q, metric)), warm=1, reps=3)
                line.update({"lloyd_route": {"N": Nl, "ms": {"median": t_l[0], "min": t_l[1], "max": t_l[2]},
                                             "queries_to_its_exact_pass": amb,
                                             "min_vector_dist_ms_same_N": {"median": t_s[0], "min": t_s[1], "max": t_s[2]},
                                             "speedup_median": t_l[0] / t_s[0],
                                             "identical": bool(torch.equal(got["d"].view(torch.int64),
                                                                           got["n"][0].view(torch.int64)) and
                                                               torch.equal(got["a"], got["n"][1]))}})
                del Cc
            line["note"] = ("HIP events around single calls, median / min / max after warm-ups (5 reps the call, 3 the "
                            "Lloyd route); stats per call; cpu_port: oracle.lloyd_assign over 256 of the queries")
            print(json.dumps(line), flush=True)
            del X, Q

    if "knn" in rows:        # lshkm_knn for k = 1, 10, 64 on the nearest row's shapes, next to lshkm_min_vector_dist
        shapes = [("grid fp32", 1_000_000, 128, 4096, "euclidean"), ("grid fp32", 1_000_000, 128, 4096, "cosine"),
                  ("cv_users fp64", 200_000, 20, 20_000, "cosine")]
        S = (lshkm.STAT_KNN_SETTLED, lshkm.STAT_KNN_SCAN, lshkm.STAT_KNN_EXACT)
        for kind, N, d, nq, metric in shapes:
            if kind == "grid fp32":
                X, Q = ctx.synth(0x5EED + 21, N, d), ctx.synth(0x5EED + 22, nq, d)
            else:
                X = torch.from_numpy(cv_users(N, d)[0]).to(ctx.dev)
                Q = torch.from_numpy(cv_users(nq, d, seed=0xBE7C5)[0]).to(ctx.dev)
            out = {}
            t_min = event_ms(lambda: out.update(min=lshkm.min_vector_dist(ctx, X, Q, metric)), warm=2, reps=5)
            m, D = 16, None
            if cpu and N <= 200_000:     # the oracle's exact distance of every (query, row) pair, one row at a time
                Xh, Qh = X.cpu().numpy(), np.ascontiguousarray(Q[:m].cpu().numpy(), np.float64)
                D = np.stack([oracle.lloyd_assign(Qh, Xh[j:j + 1], metric)[1] for j in range(N)], axis=1)
            for k in (1, 10, 64):
                ctx.reset_stats()
                t = event_ms(lambda: out.update(knn=lshkm.knn(ctx, X, Q, k, metric)), warm=2, reps=5)
                st = [ctx.stat(i) // 7 for i in S]
                line = {"row": "knn", "rows": kind, "N": N, "d": d, "nq": nq, "metric": metric, "k": k,
                        "knn_ms": {"median": t[0], "min": t[1], "max": t[2]},
                        "min_vector_dist_ms": {"median": t_min[0], "min": t_min[1], "max": t_min[2]},
                        "over_min_vector_dist": t[0] / t_min[0], "stat_settled": st[0], "stat_scan": st[1],
                        "stat_exact": st[2], "exact_per_query": st[2] / nq}
                if k == 1:
                    nan0 = torch.isnan(out["min"][0])
                    line["identical_to_min_vector_dist"] = bool(
                        torch.equal(out["knn"][0][:, 0][~nan0], out["min"][1][~nan0]) and
                        torch.equal(out["knn"][1][:, 0][~nan0].view(torch.int64), out["min"][0][~nan0].view(torch.int64)))
                if D is not None:
                    order = np.stack([np.lexsort((np.arange(N), np.where(np.isnan(r), 0.0, r), np.isnan(r)))[:k] for r in D])
                    line["identical_to_port"] = bool(
                        np.array_equal(out["knn"][0][:m].cpu().numpy(), order.astype(np.int32)) and
                        np.array_equal(out["knn"][1][:m].cpu().numpy().view(np.uint64),
                                       np.take_along_axis(D, order, 1).view(np.uint64)))
                line["note"] = ("HIP events around single calls, median / min / max of 5 after 2 warm-ups, "
                                "lshkm_min_vector_dist timed the same way in the same process; stats per call; "
                                "identical_to_port: the oracle's per-row distance matrix over 16 of the queries "
                                "(N <= 200,000)")
                print(json.dumps(line), flush=True)
            del X, Q, out

    if "main_program" in rows:   # the whole program (main.cpp:36-390) on the files of gen_main_golden --time FACTOR DIR
        sys.path.insert(0, os.path.join(ROOT, "crypto-recommendation_amd"))
        import recommend
        if not a.main_dir:
            raise SystemExit("main_program: --main-dir DIR (written by tools/gen_main_golden --time FACTOR DIR)")
        conf, tweets_csv = os.path.join(a.main_dir, "cluster.conf"), os.path.join(a.main_dir, "tweets.csv")
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "out.txt")
            ts = []
            for _ in range(3):                                         # the first call warms the context
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = recommend.run_recommendation(ctx, conf, tweets_csv, out, clock0=1, time0=1546300800)
                ctx.sync()
                ts.append(time.perf_counter() - t0)
            with open(out, "rb") as f:
                got = f.read()
        mask = lambda data: [b"" if ln.startswith(b"Execution Time: ") else ln for ln in data.split(b"\n")]
        times = [int(ln.split(b" ")[2]) for ln in got.split(b"\n") if ln.startswith(b"Execution Time: ")]
        line = {"row": "main_program", "dir": os.path.basename(os.path.normpath(a.main_dir)),
                "users": int(len(res["user_ids"])), "fake_users": int(res["fake_users"]["x"].shape[0]),
                "first_call_s": ts[0], "call_s": float(min(ts[1:])), "block_ms": times,
                "note": "run_recommendation, files in and file out, host reading and writing included; "
                        "call_s: the faster of two calls after the first"}
        ref_out = os.path.join(a.main_dir, "expected.out")
        if os.path.exists(ref_out):                                    # the reference's own file for these inputs
            with open(ref_out, "rb") as f:
                line["output_identical"] = mask(f.read()) == mask(got)
        if a.main_ref_seconds:
            line["reference_s"] = a.main_ref_seconds
            line["reference_kind"] = "the reference's main, g++ -O0, 1 core (gen_main_golden --time)"
            line["reference_over_call"] = a.main_ref_seconds / line["call_s"]
        print(json.dumps(line), flush=True)

    if "csv" in rows:        # VectorReader (vector_reader.hpp:54-85)
        n, d = 200_000, 64
        Xh = np.random.default_rng(9).standard_normal((n, d)).astype(np.float32)
        with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as f:
            for i in range(n):
                f.write(f"{i}," + ",".join(repr(float(v)) for v in Xh[i]) + "\n")
            path = f.name
        mb = os.path.getsize(path) / 1e6
        t0 = time.perf_counter(); lshkm.read_vectors(path, ",", 1, 0); t = time.perf_counter() - t0
        t1 = time.perf_counter(); lshkm.read_vectors(path, ",", 1, 1); t1 = time.perf_counter() - t1
        os.unlink(path)
        emit("VectorReader::read", "MB/s", mb, t, (mb, t1, f"{mb:.0f} MB, 1 thread of the same parser"),
             f"{n} x {d} CSV, all host threads (host-side row)")


if __name__ == "__main__":
    main()
