"""numpy statement of the user vectors from scored tweets: the update loop and
the finishing loop of tweets_to_user_vectors / clusters_to_user_vectors
(lib/crypto_rec.hpp:78-210) over a list of visits. Every sum is the sequential
chain in the reference's order (a Python loop of fp64 adds, never np.sum).
Pinned to the reference's own output by tests/test_uservec_cpu.py; the
expectation of tests/test_gpu_uservec.py."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "uservec")
CASES = ["mid", "tiny"]


def load(name):
    return np.load(os.path.join(DIR, name + ".npz"))


def paths(name):
    """(tweets, lexicon, coins) files of a case."""
    return tuple(os.path.join(DIR, f"{name}_{k}.csv") for k in ("tweets", "lexicon", "coins"))


def strs(g, key):
    b = g[key].tobytes()
    off = g[key + "_off"]
    return [b[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def user_sums(tw, grp, score, ci_ptr, ci_idx, G, C, carry=None):
    """crypto_rec.hpp:97-102 / :166-171 over the visits in order: (sum [G][C], known [G][C] uint8)."""
    sums = np.zeros((G, C), np.float64) if carry is None else np.array(carry[0], np.float64)
    known = np.zeros((G, C), np.uint8) if carry is None else (np.asarray(carry[1]) != 0).astype(np.uint8)
    for t, g in zip(np.asarray(tw).tolist(), np.asarray(grp).tolist()):
        if t < 0 or g < 0:
            continue
        s = score[t]
        for j in ci_idx[ci_ptr[t]:ci_ptr[t + 1]].tolist():
            if s > 0:
                sums[g, j] = sums[g, j] + s
            known[g, j] = 1
    return sums, known


def user_finish(sums, known):
    """crypto_rec.hpp:107-137 / :177-207 for every group, the kept ones in group
    order: (U, mean, unk_ptr, unk_idx, src)."""
    G, C = sums.shape
    U, mean, ptr, idx, src = [], [], [0], [], []
    with np.errstate(all="ignore"):
        for g in range(G):
            s = np.float64(0.0)
            n = 0
            unk = []
            useless = True
            for i in range(C):
                if known[g, i] == 0:
                    unk.append(i)
                else:
                    s = s + sums[g, i]
                    n += 1
                if sums[g, i] != 0:
                    useless = False
            if useless:
                continue
            m = s / np.float64(n)
            row = sums[g].copy()
            row[unk] = m
            U.append(row)
            mean.append(m)
            idx += unk
            ptr.append(len(idx))
            src.append(g)
    return (np.array(U, np.float64).reshape(len(U), C), np.array(mean, np.float64), np.array(ptr, np.int64),
            np.array(idx, np.int32), np.array(src, np.int32))


def user_slots(user_ids):
    """Per-tweet user IDs -> (a group number per tweet, the IDs in group order),
    groups numbered in first-seen order. A user's vector does not depend on its
    slot, so this serves where the reference's slot order (the user map's hash
    order, which only the library restates) is not what is being checked."""
    seen = {}
    return np.array([seen.setdefault(u, len(seen)) for u in user_ids], np.int32), list(seen)
