"""What the point-weight tests share (test_weighted_loss.py, test_gpu_weighted_loss.py): the float64 numpy reference
of the weighted Lp terms, loss and gradient (gnot_lp_loss_weighted / train.LpLoss(point_weights=)), built on lp_util,
the float64 weighted channel statistics (gnot_channel_stats_weighted), and the seeded weights of the GPU tests."""
import numpy as np

import lp_util as L

KINDS, DIFFERENTIABLE, CASES = L.KINDS, L.DIFFERENTIABLE, L.CASES


def weights(sizes, seed=0, empty_head=False):
    """[sum sizes] fp32: about a quarter exact zeros, the rest U(0.1, 3) (no powers of two); every sample keeps a
    positive weight.  empty_head: rows 0..2047 of every sample of 2049 rows are zero too -- a whole empty 2048-row
    split, and a sample whose only weighted row is its last."""
    rng = np.random.default_rng(100 * seed + sum(sizes))
    w = rng.uniform(0.1, 3.0, sum(sizes)) * (rng.random(sum(sizes)) >= 0.25)
    off = L.offsets(sizes)
    for b, n in enumerate(sizes):
        w[off[b + 1] - 1] = max(w[off[b + 1] - 1], 0.7)      # the last row of every sample is weighted
        if empty_head and n == 2049:
            w[off[b]:off[b] + 2048] = 0.0
    return w.astype(np.float32)


def terms(kind, pred, tgt, off, w):
    """e[b, c] in float64 over the rows with w > 0 (the others are never read: they may hold NaN)"""
    p, t, w = (np.asarray(v, dtype=np.float64) for v in (pred, tgt, w))
    out = np.empty((len(off) - 1, p.shape[1]))
    for b in range(len(off) - 1):
        s = slice(off[b], off[b + 1])
        on = w[s] > 0
        wb, d, tb = w[s][on][:, None], (p[s] - t[s])[on], t[s][on]
        out[b] = {"rel2": lambda: np.sqrt((wb * d ** 2).sum(0) / (wb * tb ** 2).sum(0)),
                  "rel1": lambda: (wb * np.abs(d)).sum(0) / (wb * np.abs(tb)).sum(0),
                  "relinf": lambda: np.abs(d).max(0) / np.abs(tb).max(0),
                  "mse": lambda: (wb * d ** 2).sum(0) / wb.sum(),
                  "l1": lambda: (wb * np.abs(d)).sum(0) / wb.sum(),
                  "linf": lambda: np.abs(d).max(0)}[kind]()
    return out


def loss(kind, pred, tgt, off, w, comp_weights=None):
    """(1/B) sum_b sum_c w^_c e[b, c] in float64"""
    e = terms(kind, pred, tgt, off, w)
    return float((e * L.norm_weights(comp_weights, e.shape[1])).sum() / e.shape[0])


def grad(kind, pred, tgt, off, w, comp_weights=None):
    """d loss / d p' in float64 (the four differentiable kinds); exact zeros on the rows with w == 0"""
    p, t, w = (np.asarray(v, dtype=np.float64) for v in (pred, tgt, w))
    B, C = len(off) - 1, p.shape[1]
    cw = L.norm_weights(comp_weights, C) / B
    g = np.zeros_like(p)
    for b in range(B):
        s = slice(off[b], off[b + 1])
        on = w[s] > 0
        wb, d, tb = w[s][on][:, None], (p[s] - t[s])[on], t[s][on]
        if kind == "rel2":
            num, den = (wb * d ** 2).sum(0), (wb * tb ** 2).sum(0)
            gb = cw * wb * d / (den * np.sqrt(num / den))
        elif kind == "rel1":
            gb = cw * wb * np.sign(d) / (wb * np.abs(tb)).sum(0)
        elif kind == "mse":
            gb = cw * 2 * wb * d / wb.sum()
        elif kind == "l1":
            gb = cw * wb * np.sign(d) / wb.sum()
        else:
            raise ValueError(kind)
        rows = np.arange(off[b], off[b + 1])[on]
        g[rows] = gb
    return g


def compact(pred, tgt, off, w):
    """(pred, tgt, off, w) with the rows of weight zero taken out"""
    w = np.asarray(w)
    on = w > 0
    sizes = [int(on[off[b]:off[b + 1]].sum()) for b in range(len(off) - 1)]
    return np.asarray(pred)[on], np.asarray(tgt)[on], L.offsets(sizes), w[on]


def stats_reference(src, w):
    """(mean64 [C], std64 [C]) of the fp32 values under the fp32 weights, in float64: mean = sum w v / V1 and the
    reliability-weights variance sum w (v - mean)^2 / (V1 - V2 / V1); std 0 where that divisor is not positive.
    Rows with w == 0 are not read."""
    w = np.asarray(w, dtype=np.float64)
    on = w > 0
    v, wv = np.asarray(src, dtype=np.float64)[on], w[on][:, None]
    v1, v2 = wv.sum(), (wv ** 2).sum()
    mean = (wv * v).sum(0) / v1
    dof = v1 - v2 / v1
    std = np.sqrt((wv * (v - mean) ** 2).sum(0) / dof) if dof > 0 else np.zeros(v.shape[1])
    return mean, std
