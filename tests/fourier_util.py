"""Shared pieces of tests/test_fourier.py (CPU) and tests/test_gpu_fourier.py: the model cases, their inputs,
the float64 formula of the embedding, and the float64 reference of a model with an embedding -- the stock-torch
port (oracle/torch_port.py) of the WIDE configuration applied to gnot_amd.fourier_features of the inputs,
differentiated through fourier_features down to the raw inputs."""
import numpy as np
import torch

import golden_util as GU

# input_dim 2, theta_dim 1, input_func_dim 3, one block, 3 experts; n_mlp_num_layers = 2
CASES = {
    "d64": dict(d=64, n_head=4, I=2, nx=3, nf=2),
    "d256": dict(d=256, n_head=8, I=1, nx=3, nf=0),
    "d64b": dict(d=64, n_head=4, I=1, nx=4, nf=1),
}
NS, MS = [129, 64, 1], [17, 5, 1]          # query points / input-function points per sample (packed)
IN, TH, F, OUT = 2, 1, 3, 1
NL = 1                                     # n_mlp_num_layers: two Linears per MLP


def width(n):
    return 4 * n + 3 if n > 0 else 1


def raw_args(case, out_dim=OUT):
    """the constructor arguments of gnot_amd.GNOT(..., x_fourier=, fn_fourier=) for a case"""
    c = CASES[case]
    return (IN, TH, F, out_dim, 1, c["d"], NL, c["d"], c["d"], 3, c["n_head"], c["I"])


def wide_cfg(case, out_dim=OUT):
    """the reference configuration (golden_util / torch_port form) the case's model equals on embedded inputs"""
    c = CASES[case]
    return dict(input_dim=IN * width(c["nx"]), theta_dim=TH, input_func_dim=F * width(c["nf"]), out_dim=out_dim,
                n_attn_layers=1, d=c["d"], n_mlp_num_layers=NL, n_expert=3, n_head=c["n_head"],
                n_input_functions=c["I"])


def models(case, seed=5, out_dim=OUT):
    """(A, B): the model with the embedding and the plain wide model holding A's state_dict (CPU, fp32)"""
    from gnot_amd import GNOT
    c = CASES[case]
    torch.manual_seed(seed)
    A = GNOT(*raw_args(case, out_dim), x_fourier=c["nx"], fn_fourier=c["nf"])
    B = GNOT(*GU.model_args(wide_cfg(case, out_dim)))
    B.load_state_dict(A.state_dict())
    return A, B


def inputs(case, Ns=NS, Ms=MS, seed=3, out_dim=OUT):
    """per-sample float64 inputs, rounded to fp32 values so that every arithmetic sees the same numbers:
    xs[b] [N_b, 2] in [-1, 1], thetas[b] [1], fns_ps[b][i] [M_b, 3] in [-1, 1], Gs[b] [N_b, out]"""
    I = CASES[case]["I"]
    rng = np.random.default_rng(seed)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    xs = [r32(rng.uniform(-1, 1, (n, IN))) for n in Ns]
    thetas = [r32(rng.random(TH)) for _ in Ns]
    fns_ps = [[r32(rng.uniform(-1, 1, (m, F))) for _ in range(I)] for m in Ms]
    Gs = [r32(rng.standard_normal((n, out_dim))) for n in Ns]
    return xs, thetas, fns_ps, Gs


def formula64(v, n):
    """the definition written out in numpy float64: [..., C] -> [..., C (4 n + 3)], channel-major blocks
    [v, cos(f_0 v) .. cos(f_2n v), sin(f_0 v) .. sin(f_2n v)], f_k = 2^(k - n)"""
    v = np.asarray(v, np.float64)
    if n == 0:
        return v
    W = 4 * n + 3
    out = np.empty(v.shape[:-1] + (v.shape[-1] * W,))
    for c in range(v.shape[-1]):
        out[..., c * W] = v[..., c]
        for k in range(2 * n + 1):
            f = 2.0 ** (k - n)
            out[..., c * W + 1 + k] = np.cos(f * v[..., c])
            out[..., c * W + 2 * n + 2 + k] = np.sin(f * v[..., c])
    return out


def formula64_bwd(v, g, n):
    """dv = g_0 + sum_k f_k (cos(f_k v) g_sin,k - sin(f_k v) g_cos,k) in float64, and the bound's scale
    S = |g_0| + sum_k f_k (|g_cos,k| + |g_sin,k|); v [R, C], g [R, >= C W]"""
    v, g = np.asarray(v, np.float64), np.asarray(g, np.float64)
    W = 4 * n + 3
    dv, S = np.zeros(v.shape), np.zeros(v.shape)
    for c in range(v.shape[1]):
        dv[:, c] = g[:, c * W]
        S[:, c] = np.abs(g[:, c * W])
        for k in range(2 * n + 1):
            f = 2.0 ** (k - n)
            gc, gs = g[:, c * W + 1 + k], g[:, c * W + 2 * n + 2 + k]
            dv[:, c] += f * (np.cos(f * v[:, c]) * gs - np.sin(f * v[:, c]) * gc)
            S[:, c] += f * (np.abs(gc) + np.abs(gs))
    return dv, S


def _pull(v, g, n, dt):
    """the gradient g of fourier_features(v, n) pulled back to v by torch autograd in dtype dt (float64 result)"""
    from gnot_amd import fourier_features
    t = torch.tensor(np.asarray(v), dtype=dt).requires_grad_(True)
    if t.numel() == 0 or n == 0:
        return np.asarray(g, np.float64).copy()
    fourier_features(t, n).backward(torch.tensor(np.asarray(g), dtype=dt))
    return t.grad.double().numpy().copy()


def _pass(case, cfg, params, xs, thetas, fns_ps, Gs, groups, dtype):
    """golden_util._port_pass of the wide configuration on fourier_features (in `dtype`) of the inputs, dx and
    dfns pulled back through fourier_features to the raw widths"""
    from gnot_amd import fourier_features
    c = CASES[case]
    dt = getattr(torch, dtype)
    emb = lambda a, n: fourier_features(torch.tensor(np.asarray(a), dtype=dt), n).numpy()
    ex = [emb(x, c["nx"]) for x in xs]
    ef = [[emb(f, c["nf"]) for f in fs] for fs in fns_ps]
    res, grads = GU._port_pass(cfg, params, ex, thetas, ef, Gs, groups, dtype)
    for b, r in enumerate(res):
        if r is None:
            continue
        r["dx"] = _pull(xs[b], r["dx"], c["nx"], dt)
        r["dfns"] = [_pull(fns_ps[b][i], r["dfns"][i], c["nf"], dt) for i in range(len(r["dfns"]))]
    return res, grads


def reference(case, params, xs, thetas, fns_ps, Gs, groups=None, out_dim=OUT):
    """golden_util.port_reference for a model with an embedding: (samples, grads, e32), dx / dfns at the raw
    widths, e32 the float32 port's own distance from the float64 one (both through fourier_features)"""
    cfg = wide_cfg(case, out_dim)
    if groups is None:
        groups = [[b] for b in range(len(xs)) if len(xs[b]) > 0]
    p64 = _pass(case, cfg, params, xs, thetas, fns_ps, Gs, groups, "float64")
    p32 = _pass(case, cfg, params, xs, thetas, fns_ps, Gs, groups, "float32")
    return GU._port_compare(cfg, xs, thetas, fns_ps, Gs, p64, p32)


def params64(model):
    return {k: v.detach().double().cpu().numpy() for k, v in model.state_dict().items()}
