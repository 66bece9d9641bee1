"""The reference's whole program (main.cpp:36-390) on the MI355X path: tweets in,
the recommendations file out.

    cluster.conf -> get_config; the project-2 clustering (cluster.run_proj2)
    tweets, lexicon, coins -> Tweets; tweets_to_user_vectors (the users) and
    clusters_to_user_vectors over the project-2 assignment (the fake users)
    A  "Cosine LSH"                 an index over the users, the users asking, N = 5
    B  "Cosine LSH"                 an index over the fake users, the users asking, N = 2
    C  "Clustering Recommendation"  rand_selection + Lloyd / k_means on the users,
                                    each user with its own cluster, N = 5
    D  "Clustering Recommendation"  k_means_pp + the same loop on the fake users,
                                    each user with its nearest centroid's cluster, N = 2

Host orchestration in Python over the C ABI (the reference's main is host code
too); every step runs in liblshkm, the file is written by lshkm_recom_write.
The user vectors are general doubles: every device step is the `_f64` entry
point. Every seed of the reference is a reading of system_clock (which the
block timers read too); program_seeds names the readings. Where the reference
would prompt on stdin (a missing -d, -o or number_of_clusters) this raises
LshkmError. The printed execution times are this driver's own.

    python recommend.py -d IN -o OUT [-validate] [--config ./cluster.conf] [--clock0 N]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

import lshkm
from cluster import run_proj2
from lshkm import LshkmError

TITLES = {"A": "Cosine LSH", "B": "Cosine LSH", "C": "Clustering Recommendation", "D": "Clustering Recommendation"}
N_TOP = {"A": 5, "B": 2, "C": 5, "D": 2}          # main.cpp:167, :213, :266, :370
NAME_INDEX = 4                                    # main.cpp:168, :214, :267, :371


def program_seeds(clock0, validate=False):
    """The program's readings of system_clock::now(), in order, for a clock that
    starts at clock0 and advances by one per reading: the project-2 k_means_pp
    seed (initialization.hpp:75), then per block t1, its one seed, t2; with
    -validate the ten folds' create_LSH_hashtables seeds follow A's t2
    (main.cpp:180-183), so every later reading moves by ten. Returns a dict of
    the named readings, `folds` (a list, empty without validate) and `readings`
    (13 or 23)."""
    c = int(clock0)
    s = {"proj2": c, "A_t1": c + 1, "A_lsh": c + 2, "A_t2": c + 3}
    c += 4
    s["folds"] = [c + i for i in range(10)] if validate else []
    c += len(s["folds"])
    for blk, what in (("B", "lsh"), ("C", "rand"), ("D", "kpp")):
        s[f"{blk}_t1"], s[f"{blk}_{what}"], s[f"{blk}_t2"] = c, c + 1, c + 2
        c += 3
    s["readings"] = c - int(clock0)
    return s


def format_double(v):
    """std::cout << double: 6 significant digits, %g rules."""
    if math.isnan(v):
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    return "%g" % v


def kmeans_loop(ctx, X, rows, max_iters, min_dist):
    """main.cpp:248-254 / :342-347: euclidean Lloyd + k_means from the dataset
    rows `rows` (the override of lloyds_assignment applies while the centroids
    are dataset rows) until no center moved by min_dist or max_iters. Returns
    (assign int32 tensor, centers fp64 tensor)."""
    torch = ctx.torch
    C = X[torch.from_numpy(rows.astype(np.int64)).to(ctx.dev)].double()
    src = rows
    it, cont, assign = 0, True, None
    while cont and it < max_iters:
        assign, _ = lshkm.lloyd_assign(ctx, X, C, "euclidean", src)
        Cn, _, cont = lshkm.kmeans_update(ctx, X, assign, C, "euclidean", min_dist)
        if cont:          # k_means replaces every center (update.hpp:70-79)
            C, src = Cn, None
        it += 1
    if assign is None:
        raise LshkmError("max_algo_iterations < 1: no assignment is made")
    return assign, C


def _resolve(base, path):
    return path if os.path.isabs(path) else os.path.join(base, path)


def _bundle(b):
    U, mean, unk_ptr, unk_idx, src, ids = b
    return dict(x=U.cpu().numpy(), mean=mean.cpu().numpy(), unk_ptr=unk_ptr.cpu().numpy(),
                unk_idx=unk_idx.cpu().numpy(), src=src.cpu().numpy(), ids=np.array(ids, dtype=object))


def run_recommendation(ctx, config_path, input_path, output_path, validate=False, clock0=None, time0=None):
    """main.cpp:36-390. clock0: the first reading of the clock (program_seeds;
    None: this moment in nanoseconds); time0: the time(0) constant of
    split_to_10 / hide_one_score (None: this moment in seconds). Returns a dict:
    blocks {A, B, C, D: {top [nq][N] int32, skip [nq] bool, ids}}, user_ids,
    users / fake_users (x, mean, unk_ptr, unk_idx, src, ids), validation (the
    10-fold value, or None), seeds, P -- numpy arrays."""
    if not input_path:
        raise LshkmError("no input file: pass -d (the reference asks on stdin)")
    if not output_path:
        raise LshkmError("no output file: pass -o (the reference asks on stdin)")
    conf = lshkm.load_config(config_path)
    if not conf.has_cluster_num:
        raise LshkmError(f"{config_path}: number_of_clusters is missing (the reference asks on stdin)")
    torch = ctx.torch
    seeds = program_seeds(time.time_ns() if clock0 is None else clock0, validate)
    time0 = int(time.time()) if time0 is None else int(time0)
    base = os.path.dirname(os.path.abspath(config_path))
    delim = chr(conf.csv_delimiter[0])
    K, k, L = conf.cluster_num, conf.k, conf.L
    iters, min_dist = conf.max_algo_iterations, conf.min_dist_kmeans

    # main.cpp:81-137: the project-2 clustering, the tweets, both user-vector lists
    p2 = run_proj2(ctx, config_path, seeds["proj2"])
    if len(set(p2["ids"])) != len(p2["ids"]):
        # the reference's k_means_pp caches distances under "<row ID>to<centroid ID>"
        # (initialization.hpp:97-109): rows that share an ID share distances there
        raise LshkmError(f"{conf.proj_2_input.decode()}: duplicated row IDs (the reference's k_means_pp would mix "
                         "their distances; lshkm_kmeans_pp takes no IDs)")
    tweets =lshkm.Tweets(input_path, _resolve(base, conf.lexicon_file.decode()), _resolve(base, conf.query_file.decode()),
                          delim)
    users = lshkm.tweets_to_user_vectors(ctx, tweets)
    fake = lshkm.clusters_to_user_vectors(ctx, tweets, tweets.match(p2["ids"]),
                                          torch.from_numpy(np.ascontiguousarray(p2["assign"], np.int32)).to(ctx.dev),
                                          conf.proj_2_cluster_num)
    U, um, up, ui, _, ids = users
    F, fm = fake[0], fake[1]
    if U.shape[0] == 0 or F.shape[0] == 0:
        raise LshkmError("no user vectors" if U.shape[0] == 0 else "no cluster-derived user vectors")
    id_pack = lshkm._pack_ids(ids)
    nq = U.shape[0]
    blocks = {}
    validation = None

    def emit(blk, top, skip, t1, first=False):
        ctx.sync()
        ms = int((time.perf_counter() - t1) * 1000.0)
        top_h = top.cpu().numpy()
        skip_h = np.zeros(nq, bool) if skip is None else skip.cpu().numpy().astype(bool)
        lshkm.recom_write(tweets, output_path, TITLES[blk], id_pack, top_h, skip_h, ms, append=not first,
                          name_index=NAME_INDEX)
        blocks[blk] = dict(top=top_h, skip=skip_h, ids=np.array(ids, dtype=object))

    def start():
        ctx.sync()
        return time.perf_counter()

    # A (main.cpp:149-185) and B (:195-230): the index over `pool`, the users asking
    for blk, (X, xm) in (("A", (U, um)), ("B", (F, fm))):
        t1 = start()
        lsh = lshkm.create_LSH_hashtables(ctx, X, "cosine", k, L, conf.lsh_bucket_div, conf.euclidean_h_w,
                                          seeds[f"{blk}_lsh"])
        try:
            top, cnt = lshkm.lsh_recommend(ctx, lsh, X, xm, U, um, up, ui, tweets.P, N_TOP[blk])
            emit(blk, top, cnt == 0, t1, first=blk == "A")
        finally:
            lsh.close()
        if blk == "A" and validate:
            validation = lshkm.lsh_rec_10_fold_validation_A(ctx, U, um, up, ui, "cosine", k, L, conf.lsh_bucket_div,
                                                            conf.euclidean_h_w, tweets.P, time0, time0, seeds["folds"])
            print(" aa" + format_double(validation), flush=True)

    # C (main.cpp:240-276): the users clustered, each with its own cluster
    t1 = start()
    assign, _ = kmeans_loop(ctx, U, lshkm.rand_selection_rows(nq, K, seeds["C_rand"]), iters, min_dist)
    crow, crows = lshkm.clusters(ctx, assign, K)
    emit("C", lshkm.cluster_top_n(ctx, U, um, crow, crows, U, um, assign, up, ui, N_TOP["C"]), None, t1)

    # D (main.cpp:334-381): the fake users clustered, each user with its nearest centroid's cluster
    t1 = start()
    assign, C = kmeans_loop(ctx, F, lshkm.kmeans_pp_rows(ctx, F, K, "euclidean", seeds["D_kpp"]), iters, min_dist)
    crow, crows = lshkm.clusters(ctx, assign, K)
    ucl, _ = lshkm.lloyd_assign(ctx, U, C, "euclidean", None)          # the inline argmin of main.cpp:356-364
    size = crow[1:] - crow[:-1]
    emit("D", lshkm.cluster_top_n(ctx, F, fm, crow, crows, U, um, ucl, up, ui, N_TOP["D"]), size[ucl.long()] == 0, t1)

    res = dict(blocks=blocks, user_ids=np.array(ids, dtype=object), users=_bundle(users), fake_users=_bundle(fake),
               validation=validation, seeds=seeds, P=tweets.P)
    tweets.close()
    return res


def parse_args(argv):
    """get_recommendation_args (main.cpp:489-509) plus --config and --clock0."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], allow_abbrev=False)
    ap.add_argument("-d", dest="input", help="the tweet file")
    ap.add_argument("-o", dest="output", help="the output file")
    ap.add_argument("-validate", dest="validate", action="store_true", help="10-fold validation after block A")
    ap.add_argument("--config", default="./cluster.conf")
    ap.add_argument("--clock0", type=int, default=None, help="the first clock reading (default: now)")
    ap.add_argument("--time0", type=int, default=None, help="the time(0) constant (default: now)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.input is None:
        raise LshkmError("no input file: pass -d (the reference asks on stdin)")
    if a.output is None:
        raise LshkmError("no output file: pass -o (the reference asks on stdin)")
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    ctx = lshkm.Context(a.device)
    run_recommendation(ctx, a.config, a.input, a.output, a.validate, a.clock0, a.time0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
