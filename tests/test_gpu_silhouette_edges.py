"""GPU parity: lshkm_silhouette at its structural edges (tests/sil_cases.py):
out[K+1] and the per-row s[N] against oracle.silhouette, bit for bit, NaN bits
included. The cases reach what the workload shapes of test_gpu_silhouette.py
do not: d % 4 != 0 (the scalar tail of sil_euclid, the unpaired branch of
sil_point_kernel), fp32 rows with d % 8 == 4, d = 512 / 513 (the LDS row's
limit and sil_point_thread_kernel), clusters around the 64-member batch, an odd
N, pairs across a cluster boundary, a singleton, an empty nearest cluster,
K = 1 / 2 / 65 / 257 / 300, tied and NaN centroid distances, inf, overflowing
and subnormal squares, one off-grid value at either end of a grid matrix, and
the API's edges. tests/test_sil_cases_cpu.py shows on the host that each case
has its property; tests/test_oracle_golden.py::test_sil_edges pins the oracle
to the reference's own code at the edges it otherwise only restates."""
import numpy as np
import pytest

import oracle
import sil_cases as sc
from amd import lshkm

pytestmark = pytest.mark.gpu

ERR_ARG = -1                    # LSHKM_ERR_ARG
NAN = sc.DEFAULT_NAN


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def to_dev(ctx, a):
    return ctx.torch.from_numpy(np.array(a)).to(ctx.dev)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(ctx, X, assign, C, metric):
    out, s = lshkm.silhouette(ctx, to_dev(ctx, X), to_dev(ctx, assign), to_dev(ctx, C), metric)
    return out, s.cpu().numpy()


_EXPECT = {}


def expect(key, X, assign, C, metric):
    """oracle.silhouette, once per case."""
    if key not in _EXPECT:
        _EXPECT[key] = oracle.silhouette(X, assign, C, metric)
    return _EXPECT[key]


def check(ctx, X, assign, C, metric, want, what):
    out, s = run(ctx, X, assign, C, metric)
    wout, ws = want
    bad = np.nonzero(bits(s) != bits(ws))[0]
    assert bad.size == 0, (what, str(X.dtype), bad[:8], s[bad[:4]], ws[bad[:4]])
    assert np.array_equal(bits(out), bits(wout)), (what, str(X.dtype), out, wout)


def row_types(X):
    """The rows as given, and in the other row type when that loses nothing:
    fp32 rows widened to fp64, fp64 rows with an fp32 image narrowed."""
    if X.dtype == np.float32:
        return [X, X.astype(np.float64)]
    with np.errstate(over="ignore"):
        x32 = X.astype(np.float32)
    return [X, x32] if np.array_equal(x32.astype(np.float64), X, equal_nan=True) else [X]


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("label", list(sc.CASES))
def test_case_vs_oracle(ctx, label):
    X, assign, C, metric, _ = sc.case(label)
    want = expect(label, X, assign, C, metric)
    for Xt in row_types(X):
        check(ctx, Xt, assign, C, metric, want, label)


@pytest.mark.parametrize("label", list(sc.AGRID))
def test_almost_grid_flag_is_fresh(ctx, label):
    """The all-grid matrix (the x*x kernel), the matrix with one off-grid value
    (pow's restatement), and the all-grid matrix again, on one context."""
    X, assign, C, metric, _ = sc.case(label)
    Xg, ag, Cg, mg, base = sc.almost_grid_base(label)
    wg = expect(base, Xg, ag, Cg, mg)
    w = expect(label, X, assign, C, metric)
    for Xt, Xgt in zip(row_types(X), row_types(Xg)):
        check(ctx, Xgt, ag, Cg, mg, wg, base + " before")
        check(ctx, Xt, assign, C, metric, w, label)
        check(ctx, Xgt, ag, Cg, mg, wg, base + " after")


@pytest.mark.parametrize("name", sc.fixtures())
def test_fixture_vs_reference(ctx, name):
    x, assign, C, metric, sil, s = sc.fixture(name)
    for Xt in row_types(x):
        check(ctx, Xt, assign, C, metric, (sil, s), name)


def test_fixtures_present():
    assert sc.fixtures() == sorted(sc.FIXTURE_NAMES)


# ------------------------------------------------------------------ the API
def call(ctx, X, N, d, assign, C, K, metric, out, s, f64=False):
    """lshkm_silhouette / _f64 as the C ABI takes it; X, assign, C, s device
    tensors or None, out a host array or None."""
    fn = lshkm.lib().lshkm_silhouette_f64 if f64 else lshkm.lib().lshkm_silhouette
    rc = fn(ctx.h, lshkm._t_ptr(X), N, d, lshkm._t_ptr(assign), lshkm._t_ptr(C), K, metric, lshkm._np_ptr(out),
            lshkm._t_ptr(s))
    ctx.sync()
    return rc


SENT = 12345.0


def test_no_rows(ctx):
    K, d = 5, 7
    C = to_dev(ctx, oracle.synth(3, K, d).astype(np.float64))
    for metric in (0, 1):
        for X, a in ((None, None), (to_dev(ctx, np.zeros((1, d), np.float32)), to_dev(ctx, np.zeros(1, np.int32)))):
            out = np.full(K + 1, SENT)
            s = to_dev(ctx, np.full(4, SENT))
            assert call(ctx, X, 0, d, a, C, K, metric, out, s) == 0
            assert np.all(bits(out) == NAN), out            # 0/0 in every slot
            assert np.all(s.cpu().numpy() == SENT)          # s is untouched
    wout, _ = oracle.silhouette(np.zeros((0, d), np.float32), np.zeros(0, np.int32), C.cpu().numpy(), "euclidean")
    assert np.all(bits(wout) == NAN)


@pytest.mark.parametrize("K,c", [(1, 0), (3, 1), (3, 2)])
def test_one_row(ctx, K, c):
    d = 5
    X = oracle.synth(4, 1, d, kind="normal")
    C = oracle.synth(5, K, d).astype(np.float64)
    assign = np.full(1, c, np.int32)
    for metric in ("euclidean", "cosine"):
        want = oracle.silhouette(X, assign, C, metric)
        if metric == "euclidean" or K > 1:
            assert np.all(bits(want[0]) == NAN) and np.all(bits(want[1]) == NAN)
        else:
            # K = 1 under cosine: d(x, x) is a rounding residue e, a = b = e, s = (e - e) / e
            assert want[1][0] == 0.0 and np.all(want[0] == 0.0)
        for Xt in row_types(X):
            check(ctx, Xt, assign, C, metric, want, ("N=1", K, c, metric))


def test_null_s(ctx):
    for label in ("planted-d3-f32-eu-normal-odd", "kedge-k300-d7-cos", "planted-d513-f32-eu-grid"):
        X, assign, C, metric, _ = sc.case(label)
        wout, _ = expect(label, X, assign, C, metric)
        N, d = X.shape
        out = np.full(len(C) + 1, SENT)
        rc = call(ctx, to_dev(ctx, X), N, d, to_dev(ctx, assign), to_dev(ctx, C), len(C), lshkm._METRIC[metric], out, None)
        assert rc == 0
        assert np.array_equal(bits(out), bits(wout)), label


def test_refused_arguments(ctx):
    label = "kedge-k2-d7-eu"
    Xh, ah, Ch, metric, _ = sc.case(label)
    N, d = Xh.shape
    K = len(Ch)
    X, a, C = to_dev(ctx, Xh), to_dev(ctx, ah), to_dev(ctx, Ch)
    X64 = to_dev(ctx, Xh.astype(np.float64))
    bad = {
        "K = 0": dict(K=0),
        "d = 0": dict(d=0),
        "metric = 2": dict(metric=2),
        "null C": dict(C=None),
        "null out_host": dict(out=None),
        "null X, N > 0": dict(X=None),
        "N = -1": dict(N=-1),
        "N = 2^31": dict(N=1 << 31),
    }
    for f64 in (False, True):
        for what, ch in bad.items():
            host = np.full(K + 1, SENT)
            s = to_dev(ctx, np.full(N, SENT))
            args = dict(X=X64 if f64 else X, N=N, d=d, assign=a, C=C, K=K, metric=0, out=host, s=s)
            args.update(ch)
            rc = call(ctx, args["X"], args["N"], args["d"], args["assign"], args["C"], args["K"], args["metric"],
                      args["out"], args["s"], f64=f64)
            assert rc == ERR_ARG, (what, f64, rc)
            assert np.all(host == SENT), what               # the host's out is untouched
            assert np.all(s.cpu().numpy() == SENT), what    # and the device's s
    # the context still works
    check(ctx, Xh, ah, Ch, metric, expect(label, Xh, ah, Ch, metric), label)


def test_workspace_reuse(ctx):
    """A small, a large and the small call again on one context give what a fresh
    context gives (and what the oracle says)."""
    order = ["kedge-k65-d7-eu", "planted-d512-f64-eu-general", "kedge-k65-d7-eu", "kedge-k1-d8-eu"]
    one = lshkm.Context(0)
    try:
        for label in order:
            X, assign, C, metric, _ = sc.case(label)
            fresh = lshkm.Context(0)
            try:
                fout, fs = run(fresh, X, assign, C, metric)
            finally:
                fresh.close()
            out, s = run(one, X, assign, C, metric)
            assert np.array_equal(bits(out), bits(fout)) and np.array_equal(bits(s), bits(fs)), label
            wout, ws = expect(label, X, assign, C, metric)
            assert np.array_equal(bits(out), bits(wout)) and np.array_equal(bits(s), bits(ws)), label
    finally:
        one.close()
