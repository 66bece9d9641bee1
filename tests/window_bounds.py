"""csrc/tile.h's split-f16 bounds and csrc/hash_tile.h's certificate window,
restated for the tests that plant values against them (test_window_model_cpu
holds the restated constants to the header's, bit for bit)."""
import numpy as np

U_ANY, U_RN = 2.0 ** -23, 2.0 ** -24
SPLIT_DROPPED, SPLIT_RESID, LO_SHARE = 2.0 ** -22, 2 * 2.0 ** -22, 2.0 ** -10
MARGIN = 1.0 + 2.0 ** -8
# hash tile: 16 additions of the step's hi MFMA, 48 on the lo products, 7 VALU step additions
FU_A1H = (16 * U_ANY + 48 * U_ANY * LO_SHARE + 7 * U_RN + SPLIT_DROPPED + SPLIT_RESID) * MARGIN
# 3-product tile: 128 chained hi additions, 256 on the lo products, c rounded to f32
FU_A1 = (128 * U_ANY + 256 * U_ANY * LO_SHARE + U_RN + SPLIT_DROPPED + SPLIT_RESID) * MARGIN
FU_A2 = 2.0 ** -24
# the constants these replaced, as literals
FU_A1H_PARENT = 1.25 * 2.0 ** -18
FU_A1_PARENT = 1.25 * 2.0 ** -16
G = (2.0 ** -22 + 2.0 ** -20) * (1.0 + 2.0 ** -18)


def window(Xh, Vf, tf, w, a1h):
    """certify_floor_f32's B = |y| G + |x| P + Q for every (row, function) in
    fp64 (hash_window's P and Q without their 1 + 2^-18 inflations and f32
    roundings: below 2^-15 relative), euclidean (w > 0, y = (x.v + t) / w) or
    cosine (w = None, y = x.v, no G term: certify_sign_f32). Returns (y, B)."""
    x = Xh.astype(np.float64)
    nx = np.linalg.norm(x, axis=1)
    pn, v1 = np.linalg.norm(Vf, axis=1), np.abs(Vf).sum(axis=1)
    if w is None:
        y = x @ Vf.T
        P = a1h * pn + FU_A2 * np.sqrt(Vf.shape[1])
        Q = FU_A2 * v1 + 2.0 ** -126
        return y, nx[:, None] * P[None, :] + Q[None, :]
    y = (x @ Vf.T + tf) / w
    P = (a1h * pn + FU_A2 * np.sqrt(Vf.shape[1])) / w
    Q = (FU_A2 * v1 + (2.0 ** -40 + 2.0 ** -23) * np.abs(tf)) / w + 2.0 ** -126
    return y, np.abs(y) * G + nx[:, None] * P[None, :] + Q[None, :]
