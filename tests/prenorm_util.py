"""Shared pieces of the pre-norm tests (tests/test_prenorm.py on the CPU, tests/test_gpu_prenorm*.py): the model
cases and their inputs, the float64 reference of GNOT(..., pre_norm=True) -- the stock-torch port
(oracle/torch_port.py) with its `_attention` receiving layer-normalised `query` and `srcs`, wrapped at run time
and restored on exit -- and the float64 numpy formula of the parameter-free LayerNorm and of its backward."""
import contextlib

import numpy as np
import torch

import golden_util as GU

EPS = 1e-5
# input_dim 2, theta_dim 1, input_func_dim 3, out_dim 2, 3 experts, n_mlp_num_layers 2
IN, TH, F, OUT, E, NL = 2, 1, 3, 2, 3, 2
NS, MS = [129, 64, 1], [17, 5, 1]          # query points / input-function points per sample (packed)
# the smallest cases that reach each kernel family the option touches
CASES = {
    "d64": dict(d=64, n_head=4, I=2, L=2),       # chain.hip; batched key/value jobs of 2 functions x 2 blocks, one fnn{i}
    "d40": dict(d=40, n_head=2, I=0, L=1),       # internal width 48: statistics over 40 of 48 columns; cross in self mode
    "d30": dict(d=30, n_head=5, I=1, L=1),       # padded heads
    "d200": dict(d=200, n_head=5, I=1, L=1),     # layer-wise chains at internal width 256
    "d256": dict(d=256, n_head=8, I=1, L=1),     # chain2 / linear2
    "d320": dict(d=320, n_head=5, I=1, L=1),     # chainw
    "d64s": dict(d=64, n_head=4, I=1, L=1),      # the point-sharded run
}


def cfg_of(case):
    c = CASES[case]
    return dict(input_dim=IN, theta_dim=TH, input_func_dim=F, out_dim=OUT, n_attn_layers=c["L"], d=c["d"],
                n_mlp_num_layers=NL, n_expert=E, n_head=c["n_head"], n_input_functions=c["I"])


def model(case, seed=5, **kw):
    """GNOT(..., pre_norm=True) of a case on the CPU (kw overrides, e.g. pre_norm=False)"""
    from gnot_amd import GNOT
    torch.manual_seed(seed)
    return GNOT(*GU.model_args(cfg_of(case)), **dict(dict(pre_norm=True), **kw))


def params64(m):
    """the Linear parameters as float64 arrays (the port's state dict: without the pre_norm_eps buffer)"""
    return {k: v.detach().double().cpu().numpy() for k, v in m.named_parameters()}


def inputs(case, Ns=NS, Ms=MS, seed=3):
    """per-sample float64 inputs holding fp32 values (as tests/fourier_util.py): xs[b] [N_b, 2] in [-1, 1],
    thetas[b] [1], fns_ps[b][i] [M_b, 3], Gs[b] [N_b, out]"""
    I = CASES[case]["I"]
    rng = np.random.default_rng(seed)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    xs = [r32(rng.uniform(-1, 1, (n, IN))) for n in Ns]
    thetas = [r32(rng.random(TH)) for _ in Ns]
    fns_ps = [[r32(rng.uniform(-1, 1, (m, F))) for _ in range(I)] for m in Ms]
    Gs = [r32(rng.standard_normal((n, OUT))) for n in Ns]
    return xs, thetas, fns_ps, Gs


@contextlib.contextmanager
def pre_norm_port(eps=EPS, seen=None):
    """Inside the context oracle.torch_port._attention normalises its `query` and `srcs` arguments with
    F.layer_norm(h, (d,), eps=eps) (no affine) first: the port then IS the pre-norm model.  Only the port
    module's own name is replaced, and it is restored on exit.  seen: a list that receives (raw, normalised)
    of every normalised tensor, in call order (query, then the sources)."""
    import torch.nn.functional as Fn
    from oracle import torch_port
    plain = torch_port._attention

    def ln(h):
        y = Fn.layer_norm(h, (h.shape[-1],), eps=eps)
        if seen is not None:
            seen.append((h.detach().clone(), y.detach().clone()))
        return y

    def attention(p, prefix, query, srcs, H, key_names, value_names):
        nq = ln(query)
        # without input functions the source IS the query (model.py:88-104): one normalisation, as in the engine
        ns = [nq if s is query else ln(s) for s in srcs]
        return plain(p, prefix, nq, ns, H, key_names, value_names)

    torch_port._attention = attention
    try:
        yield
    finally:
        torch_port._attention = plain


def reference(cfg, params, xs, thetas, fns_ps, Gs, groups=None):
    """golden_util.port_reference of the pre-norm model: (samples, grads, e32) as check_parity /
    check_parity_per_sample take them, e32 the float32 pre-norm port's own distance from the float64 one"""
    if groups is None:
        groups = [[b] for b in range(len(xs)) if len(xs[b]) > 0]
    with pre_norm_port():
        p64 = GU._port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float64")
        p32 = GU._port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float32")
    return GU._port_compare(cfg, xs, thetas, fns_ps, Gs, p64, p32)


def fixture(case, Ns=NS, Ms=MS):
    """(model on the CPU, inputs, fx): fx the dict check_parity_per_sample takes (samples, grads, e32, out)"""
    m = model(case)
    xs, thetas, fns_ps, Gs = inputs(case, Ns, Ms)
    samples, grads, e32 = reference(cfg_of(case), params64(m), xs, thetas, fns_ps, Gs)
    fx = dict(samples=samples, grads=grads, e32=e32, out=np.concatenate([s["out"] for s in samples]))
    return m, (xs, thetas, fns_ps, Gs), fx


def ln64(x, C=None, eps=EPS):
    """(y, rstd) of the parameter-free LayerNorm over the first C columns, float64: biased variance"""
    x = np.asarray(x, np.float64)
    C = x.shape[-1] if C is None else C
    v = x[..., :C]
    mean = v.mean(-1, keepdims=True)
    d = v - mean
    rstd = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    return d * rstd, rstd[..., 0]


def ln64_bwd(y, rstd, dy):
    """dx = rstd (dy - mean(dy) - y mean(dy y)) in float64 from a forward's y [R, C] and rstd [R]"""
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    r = np.asarray(rstd, np.float64)[:, None]
    return r * (dy - dy.mean(-1, keepdims=True) - y * (dy * y).mean(-1, keepdims=True))


# ------------------------------------------------------------------ running a case on the device
def run_gpu(m, data, dev):
    """forward_packed + backward of model m (already on dev) on the packed inputs of `data`; returns
    dict(out, grads, dx, dtheta, dfns) of float64 arrays"""
    xs, thetas, fns_ps, Gs = data
    I = len(fns_ps[0])
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    x = t(np.concatenate(xs)).requires_grad_(True)
    theta = t(np.stack(thetas)).requires_grad_(True)
    fns = [t(np.concatenate([fns_ps[b][i] for b in range(len(xs))])).requires_grad_(True) for i in range(I)]
    x_off = np.concatenate([[0], np.cumsum([len(a) for a in xs])]).tolist()
    fn_offs = [np.concatenate([[0], np.cumsum([len(fns_ps[b][i]) for b in range(len(xs))])]).tolist() for i in range(I)]
    for p in m.parameters():
        p.grad = None
    out = m.forward_packed(x, x_off, theta, fns, fn_offs)
    (out * t(np.concatenate(Gs))).sum().backward()
    torch.cuda.synchronize()
    g = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).double().cpu().numpy()
    return dict(out=out.detach().double().cpu().numpy(), grads={k: g(p) for k, p in m.named_parameters()},
                dx=g(x), dtheta=g(theta), dfns=[g(f) for f in fns])


# ------------------------------------------------------------------ the row kernels' test inputs and bounds
WIDTHS = [1, 2, 3, 4, 5, 63, 64, 65, 200, 255, 256, 257, 1000, 1024]
ROWS = [1, 3, 4, 5, 257]
FAMILIES = ["normal", "offset", "constant", "tiny"]
U = 2.0 ** -24


def kernel_rows(C, rows, family, seed=0):
    """(x, dy) float32 [rows, C]: N(0, 1); 1e4 + N(0, 1); constant rows (one value per row); 1e-20 N(0, 1), whose
    variance is far below eps.  dy is N(0, 1)."""
    rng = np.random.default_rng([seed, C, rows, FAMILIES.index(family)])
    n = rng.standard_normal((rows, C))
    x = {"normal": n, "offset": 1e4 + n, "constant": np.repeat(rng.uniform(-3, 3, (rows, 1)), C, 1),
         "tiny": 1e-20 * n}[family]
    return x.astype(np.float32), rng.standard_normal((rows, C)).astype(np.float32)


def fwd_ratios(x, y, rstd, eps=EPS):
    """a float32 forward (y, rstd) of the rows x against float64: the largest |y - y64| / (2^-24 (rstd64 max_j |x_rj|
    + |y64|)) over the elements and the largest |rstd - rstd64| / (2^-24 rstd64) over the rows"""
    y64, r64 = ln64(x, eps=eps)
    scale = U * (r64[:, None] * np.abs(np.asarray(x, np.float64)).max(1, keepdims=True) + np.abs(y64))
    err = np.abs(np.asarray(y, np.float64) - y64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0, 0.0, err / scale)
    return float(q.max()), float((np.abs(np.asarray(rstd, np.float64) - r64) / (U * r64)).max())


def bwd_ratio(y, rstd, dy, dx):
    """a float32 backward dx against the float64 formula fed the SAME float32 y and rstd: the largest
    |dx - dx64| / (2^-24 rstd (|dy_r|_1 / C (1 + |y|) + |dy|)) over the elements"""
    y, dy, r = np.asarray(y, np.float64), np.asarray(dy, np.float64), np.asarray(rstd, np.float64)[:, None]
    scale = U * r * (np.abs(dy).sum(1, keepdims=True) / y.shape[1] * (1 + np.abs(y)) + np.abs(dy))
    err = np.abs(np.asarray(dx, np.float64) - ln64_bwd(y, r[:, 0], dy))
    return float(np.where(err == 0, 0.0, err / scale).max())


def torch_ratios(C, rows, family):
    """(forward ratio, rstd ratio, backward ratio) of torch's own float32 layer_norm on the CPU for one input set"""
    x, dy = kernel_rows(C, rows, family)
    t = torch.tensor(x, requires_grad=True)
    y, _, rstd = torch.native_layer_norm(t, (C,), None, None, EPS)
    y.backward(torch.tensor(dy))
    y, rstd = y.detach().numpy(), rstd.detach().numpy().reshape(rows)
    return fwd_ratios(x, y, rstd) + (bwd_ratio(y, rstd, dy, t.grad.numpy()),)
