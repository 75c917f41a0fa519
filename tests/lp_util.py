"""What the Lp-loss tests share (test_lp_loss.py, test_gpu_lp_loss.py): the float64 numpy reference of the six
kinds of gnot_lp_loss / train.LpLoss -- terms, loss and gradient -- and the seeded packed inputs of the GPU tests."""
import numpy as np

KINDS = ("rel2", "rel1", "relinf", "mse", "l1", "linf")
DIFFERENTIABLE = ("rel2", "rel1", "mse", "l1")

# (sample sizes, channels): a one-row sample, a sample one row past the 2048-row split, an odd size, three
# channels; and 4097 = 2 * 2048 + 1 beside the exact multiple 4096, one channel
CASES = [([1, 2049, 300], 3), ([4097, 4096], 1)]


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64).tolist()


def inputs(sizes, C, seed=0):
    """(pred, tgt) as float32 numpy arrays [sum sizes, C]: randn predictions, randn + 0.5 targets, so every
    denominator of a relative kind is positive"""
    import torch
    gen = torch.Generator().manual_seed(1000 * seed + sum(sizes) + C)
    rows = sum(sizes)
    return (torch.randn(rows, C, generator=gen).numpy(), (torch.randn(rows, C, generator=gen) + 0.5).numpy())


def norm_weights(weights, C):
    """w_c / sum w in float64; 1 / C each without weights"""
    w = np.full(C, 1.0) if weights is None else np.asarray(weights, dtype=np.float64)
    return w / w.sum()


def terms(kind, pred, tgt, off):
    """e[b, c] in float64; pred is the (de-normalised) prediction"""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    out = np.empty((len(off) - 1, p.shape[1]))
    for b in range(len(off) - 1):
        d, tb = p[off[b]:off[b + 1]] - t[off[b]:off[b + 1]], t[off[b]:off[b + 1]]
        n = off[b + 1] - off[b]
        out[b] = {"rel2": lambda: np.sqrt((d ** 2).sum(0) / (tb ** 2).sum(0)),
                  "rel1": lambda: np.abs(d).sum(0) / np.abs(tb).sum(0),
                  "relinf": lambda: np.abs(d).max(0) / np.abs(tb).max(0),
                  "mse": lambda: (d ** 2).sum(0) / n,
                  "l1": lambda: np.abs(d).sum(0) / n,
                  "linf": lambda: np.abs(d).max(0)}[kind]()
    return out


def loss(kind, pred, tgt, off, weights=None):
    """(1/B) sum_b sum_c w^_c e[b, c] in float64"""
    e = terms(kind, pred, tgt, off)
    return float((e * norm_weights(weights, e.shape[1])).sum() / e.shape[0])


def grad(kind, pred, tgt, off, weights=None):
    """d loss / d p' in float64 (the four differentiable kinds), from the closed forms"""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    B, C = len(off) - 1, p.shape[1]
    w = norm_weights(weights, C) / B
    g = np.empty_like(p)
    for b in range(B):
        s = slice(off[b], off[b + 1])
        d, tb, n = p[s] - t[s], t[s], off[b + 1] - off[b]
        if kind == "rel2":
            num, den = (d ** 2).sum(0), (tb ** 2).sum(0)
            g[s] = w * d / (den * np.sqrt(num / den))
        elif kind == "rel1":
            g[s] = w * np.sign(d) / np.abs(tb).sum(0)
        elif kind == "mse":
            g[s] = w * 2 * d / n
        elif kind == "l1":
            g[s] = w * np.sign(d) / n
        else:
            raise ValueError(kind)
    return g
