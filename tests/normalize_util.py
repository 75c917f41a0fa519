"""Shared by test_normalize.py and test_gpu_normalize.py: the inputs, the float64 reference and the bars of the
gnot_channel_stats tests, and a float32 numpy restatement of the kernel's scheme (csrc/stats.hip), operation by
operation, so the bars can be checked against the scheme without a GPU."""
import numpy as np

STAT_ROWS = 4096            # csrc/stats.hip kStatRows
F = np.float32
STATS_ROWS_CASES = (1, 2, 255, 256, 257, 70001)
CONST = 3.7


def stats_inputs(rows, seed=0):
    """[rows, 5] fp32: N(0,1), 1e4 + N(0,1), the constant 3.7, U(0,8), 1e-3 N(0,1)"""
    rng = np.random.default_rng(seed + rows)
    cols = [rng.standard_normal(rows), 1e4 + rng.standard_normal(rows), np.full(rows, CONST),
            rng.uniform(0, 8, rows), 1e-3 * rng.standard_normal(rows)]
    return np.stack(cols, 1).astype(np.float32)


def stats_reference(src):
    """(mean64 [C], std64 [C]) of the fp32 values in float64; std unbiased, 0 for one row"""
    s = src.astype(np.float64)
    return s.mean(0), (s.std(0, ddof=1) if len(s) > 1 else np.zeros(s.shape[1]))


def stats_bars(mean64, std64):
    """the issue's bars: |mean - mean64| <= 16 2^-24 |mean64| + 1e-5 std64, |std - std64| <= 1e-5 std64"""
    return 16 * 2.0 ** -24 * np.abs(mean64) + 1e-5 * std64, 1e-5 * std64


def _tree(lanes):
    """block_sum: 256 lanes through a binary tree, fp32"""
    red = lanes.astype(F).copy()
    s = 128
    while s:
        red[:s] = red[:s] + red[s:2 * s]
        s >>= 1
    return red[0]


def _strided(n, term):
    """sum over i < n of term(i), lane t taking i = t, t + 256, ... in order, then the tree.  term maps an index
    array to fp32 values"""
    acc = np.zeros(256, F)
    for j in range(-(-n // 256)):
        idx = j * 256 + np.arange(256)
        ok = idx < n
        acc = np.where(ok, acc + term(np.minimum(idx, n - 1)).astype(F), acc).astype(F)
    return _tree(acc)


def stats_restatement(src, eps=1e-8):
    """{mean, std, rstd} as csrc/stats.hip computes them, in numpy float32 (every operation rounded, no
    contraction; the two fmaf of the kernel evaluated in float64 and rounded once)"""
    src = np.asarray(src, F)
    rows, C = src.shape
    nslice = -(-rows // STAT_ROWS)
    out = np.zeros((3, C), F)
    for c in range(C):
        m, s, q, ns = [], [], [], []
        for k in range(nslice):
            x = src[k * STAT_ROWS:(k + 1) * STAT_ROWS, c]
            n = len(x)
            pivot = x[0]
            mk = F(pivot + _strided(n, lambda i: x[i] - pivot) / F(n))
            sk = _strided(n, lambda i: x[i] - mk)
            # q = fmaf(d, d, q): the product is exact in float64, the sum rounded once to fp32
            acc = np.zeros(256, F)
            for j in range(-(-n // 256)):
                idx = j * 256 + np.arange(256)
                ok = idx < n
                d = (x[np.minimum(idx, n - 1)] - mk).astype(np.float64)
                acc = np.where(ok, (d * d + acc.astype(np.float64)).astype(F), acc).astype(F)
            m.append(mk), s.append(sk), q.append(_tree(acc)), ns.append(F(n))
        m, s, q, ns = (np.array(v, F) for v in (m, s, q, ns))
        pivot = m[0]
        mean = F(pivot + _strided(nslice, lambda k: ns[k] * (m[k] - pivot) + s[k]) / F(rows))
        d = (m - mean).astype(F)
        Q = _strided(nslice, lambda k: q[k] + d[k] * (F(2) * s[k] + ns[k] * d[k]))
        sd = F(np.sqrt(max(Q, F(0)) / F(rows - 1))) if rows > 1 else F(0)
        const = rows == 1 or sd <= F(1e-6) * abs(mean)
        out[:, c] = (mean, F(0) if const else sd, F(1) if const else F(1) / (sd + F(eps)))
    return out
