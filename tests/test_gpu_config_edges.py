"""Model-configuration edges a plan accepts, checked per sample and per output row against float64.

gnot_plan_create takes a much wider range of constructor arguments than the other parity files run: MLP depth
is a run-time loop count of the chain kernels, the expert count decides how many 16-wide tiles the gate
softmax spans, the number of input functions decides whether the MFMA attention passes fit LDS and how the
batched K/V jobs split, the block count how many accumulating launches the d(fn encoding) backward-data
takes, and an input / output width above 16 makes the first / last Linear of a chain run at the full tile
count with a ragged column count.  Every case here is one such edge on one kernel family:

  A  d = 64,  4 heads    chain.hip / linear.hip
  M  d = 128, 8 heads    the same kernels at 8 tiles (input / output widths only)
  B  d = 256, 8 heads    chain2.hip / linear2.hip
  D  d = 320, 10 heads   chainw.hip
  W  d = 640, 10 heads   the K-split tables (internal width above 512)

Base configuration: input_dim 2, theta_dim 1, input_func_dim 3, out_dim 2, L = 1, two-layer MLPs, 2 experts,
1 input function.  Batch of every case: Ns = [65, 1, 130] (a partial 64-point chunk, a single-point sample, a
sample boundary inside a 128-row chain block), input-function points [33, 1, 17] per sample, rotated by one
for each further input function.

  nl0, nl6     n_mlp_num_layers 0 (the two Linears of 1) and 6
  L0, L0-I0    no block: encoder and decoder only; with an input function its encoder's gradients and dfns
               are exact zeros
  L5           n_attn_layers 5 with two-Linear MLPs: 10 d(fn) segments per input function, launches of 8 + 2
               (kMaxSeg 8); on W (kMaxSeg 4, I = 2) launches of 4 + 4 + 2
  th0          theta_dim 0: theta is [B, 0], dtheta comes back [B, 0]
  E16, E17     the last one-tile gate and the first multi-tile one; E64 (A, I = 0) the cap E = d; E1 the
               one-expert chains (chain2.hip grid mode 0, chainw.hip)
  I3 .. I8     input functions.  Under the forced-MFMA path (attn_path "mfma") the apply passes need
               apply_lds_bytes<dh>(nsrc, H, bwd) = ((bwd ? 2 : 1) nsrc H (dh/16)^2 64 4 + nsrc H dh) 4 bytes of
               LDS against kApplyLdsMax = 163,840 (attn_mfma.hip), else attn.hip runs.  B (H = 8, dh = 32):
               33,792 per source forward, 66,560 backward, so
                 I = 1, 2   forward MFMA, backward MFMA
                 I = 3      forward MFMA (101,376), backward attn.hip (199,680): the first backward fallback
                 I = 4      forward MFMA (135,168, the largest), backward attn.hip
                 I = 5      forward attn.hip (168,960), backward attn.hip
                 I = 8      both attn.hip; fills AttnApplyArgs::state[8]
               D (H = 10, dh = 32): 42,240 / 83,200 per source; I = 3 forward MFMA (126,720), backward attn.hip
               (249,600).  A (H = 4, dh = 16): 4,352 / 8,448 per source, I = 8 on MFMA both ways (34,816 /
               67,584).  W (H = 10, dh = 64): one source already needs 166,400 forward, so every apply pass of
               W runs attn.hip on either path; the self-attention calls (nsrc = 1) of the other families stay
               on MFMA throughout.
  io16, io17   (input_dim, theta_dim, input_func_dim, out_dim) = (9, 7, 16, 16), the last one-tile width, and
               (9, 8, 17, 17), the first full-width one, ragged; ioD every width equal to d

The reference is golden_util.port_reference: one B = 1 float64 call of the stock-torch port per sample plus
its float32 pass for e32.  Every fp32 case is checked with check_parity_per_sample at the project's rule
(1e-4 ||ref|| + 20 e32: whole batch, per sample, per output row), must give the same bits twice, the same
output and parameter gradients with and without input gradients, and finite results.  The reference alone
never lets a case pass: _assemble asserts that 20 e32 stays within a quarter of the 1e-4 term for the output
per sample and per row, and tests/test_config_edge_references.py asserts that for every case on a machine
with no GPU.  Every case prints one "CFGE" line; profiles/config_edges_parity.txt is that output on the MI355X.
"""
import functools

import numpy as np
import pytest
import torch

from golden_util import check_parity_per_sample, rel
from test_gpu_geometry import _assemble, _log, _params, _run, _same_bits
from test_gpu_parity import attn_path, build_model  # noqa: F401

pytestmark = pytest.mark.gpu

NS = [65, 1, 130]
M0 = [33, 1, 17]
FAMILIES = {"A": (64, 4), "M": (128, 8), "B": (256, 8), "D": (320, 10), "W": (640, 10)}
BASE = dict(input_dim=2, theta_dim=1, input_func_dim=3, out_dim=2, n_attn_layers=1, n_mlp_num_layers=2, n_expert=2,
            n_input_functions=1)
_SHORT = dict(nl="n_mlp_num_layers", L="n_attn_layers", th="theta_dim", E="n_expert", I="n_input_functions")


def _io(i, t, f, o):
    return dict(input_dim=i, theta_dim=t, input_func_dim=f, out_dim=o)


IO16, IO17 = _io(9, 7, 16, 16), _io(9, 8, 17, 17)

# edge name -> (families, what it changes in BASE)
EDGES = {
    "nl0": ("ABD", dict(nl=0)),
    "nl6": ("ABD", dict(nl=6)),
    "L0-I0": ("AB", dict(L=0, I=0)),
    "L0": ("AB", dict(L=0)),
    "L5": ("AD", dict(L=5, nl=1)),
    "L5-I2": ("W", dict(L=5, nl=1, I=2)),
    "th0": ("ABD", dict(th=0)),
    "E16": ("ABD", dict(E=16)),
    "E17": ("ABD", dict(E=17)),
    "E64-I0": ("A", dict(E=64, I=0)),
    "E1": ("BD", dict(E=1)),
    "I3": ("BD", dict(I=3)),
    "I4": ("B", dict(I=4)),
    "I5": ("B", dict(I=5)),
    "I8": ("ABW", dict(I=8)),
    "io16": ("MB", IO16),
    "io17": ("MB", IO17),
    "io16-I2": ("A", dict(IO16, I=2)),
    "io17-I2": ("A", dict(IO17, I=2)),
    "ioD": ("AB", None),        # every width equal to d: filled in by _cfg
}
CASES = [(f, e) for e, (fams, _) in EDGES.items() for f in fams]

# a case whose reference misses the vacuity bar of _assemble gets another seed here (never a wider rule).  Worst
# 20 e32 over the 1e-4 term per output row at seed 17 -> at the seed chosen (per sample it is about half that):
# B/nl0 0.32 -> 0.10, D/nl0 0.36 -> 0.15, D/L5 0.29 -> 0.13, W/L5-I2 0.39 -> 0.12, B/I8 0.52 -> 0.03; W/I8 passes at
# seed 17 with 0.22, too close to the bar to hold on another host's fp32 BLAS: 0.04.  Every other case: at most 0.12.
SEEDS = {("B", "nl0"): 22, ("D", "nl0"): 21, ("D", "L5"): 20, ("W", "L5-I2"): 22, ("B", "I8"): 23, ("W", "I8"): 18}


def _cfg(family, edge):
    d, H = FAMILIES[family]
    over = EDGES[edge][1]
    if over is None:
        over = {"A": _io(40, 24, 64, 64), "B": _io(200, 56, 256, 256)}[family]
    return dict(BASE, d=d, n_head=H, **{_SHORT.get(k, k): v for k, v in over.items()})


def _fn_points(I):
    """points of input function i per sample: M0 rotated by i"""
    return [M0[i % 3:] + M0[:i % 3] for i in range(I)]


@functools.lru_cache(maxsize=None)
def _case(family, edge):
    """one reference per case, shared by both attention paths and the bf16 / recompute runs"""
    cfg = _cfg(family, edge)
    I = cfg["n_input_functions"]
    Ms = _fn_points(I)
    seed = SEEDS.get((family, edge), 17)
    rng = np.random.default_rng(seed)
    xs = [rng.random((n, cfg["input_dim"])) for n in NS]
    thetas = [rng.random(cfg["theta_dim"]) for _ in NS]
    fns_ps = [[rng.random((Ms[i][b], cfg["input_func_dim"])) for i in range(I)] for b in range(len(NS))]
    Gs = [rng.standard_normal((n, cfg["out_dim"])) for n in NS]
    return _assemble(cfg, _params(cfg, seed), xs, thetas, fns_ps, Gs)


def unused_encoder_nonzeros(grads, dfns):
    """L = 0 with an input function: the names of the input_func_mlps gradients and dfns that are not exact zeros"""
    enc = [k for k in grads if k.startswith("input_func_mlps.")]
    assert enc, "no input-function encoder in this case"
    bad = [k for k in enc if np.any(np.asarray(grads[k]) != 0.0)]
    return bad + [f"dfn{i}" for i, f in enumerate(dfns) if np.any(np.asarray(f) != 0.0)]


def _assert_finite(got):
    arrays = [got["out"], got["dx"], got["dtheta"], *got["dfns"], *got["grads"].values()]
    assert all(np.isfinite(a).all() for a in arrays), "non-finite result"


@pytest.mark.parametrize("family,edge", CASES)
def test_config_edge_per_sample_parity(family, edge, attn_path):
    fx = _case(family, edge)
    cfg = fx["cfg"]
    m = build_model(fx["params"], cfg)
    plain = _run(m, fx, want=False)
    got = _run(m, fx)
    again = _run(m, fx)
    _log("fp32", family, edge, attn_path, got, fx, tag="CFGE")
    _assert_finite(got)
    assert got["dtheta"].shape == (len(NS), cfg["theta_dim"])
    assert not _same_bits(plain, got), "asking for input gradients changed the output or a parameter gradient"
    assert not _same_bits(got, again), "a second run gave other bits"
    if cfg["n_attn_layers"] == 0 and cfg["n_input_functions"] > 0:
        assert not unused_encoder_nonzeros(got["grads"], got["dfns"])
    errs = check_parity_per_sample(got, fx)
    assert not errs, errs


@pytest.mark.parametrize("family,edge", [("B", "E17"), ("B", "nl0"), ("B", "I3"), ("B", "io17"), ("A", "nl6")])
def test_config_edge_bf16_mode(family, edge, attn_path):
    """bf16 mode: the project's whole-batch bar (1e-2 on the output and on the concatenated gradients against
    float64, tests/test_gpu_bf16.py), finiteness, and a result that really differs from the fp32 one."""
    fx = _case(family, edge)
    m = build_model(fx["params"], fx["cfg"])
    fp32 = _run(m, fx)
    m.set_precision("bf16")
    got = _run(m, fx)
    _log("bf16", family, edge, attn_path, got, fx, tag="CFGE")
    _assert_finite(got)
    keys = sorted(fx["grads"])
    cat = lambda g: np.concatenate([np.ravel(g[k]) for k in keys])
    e_out, e_grad = rel(got["out"], fx["out"]), rel(cat(got["grads"]), cat(fx["grads"]))
    assert e_out < 1e-2 and e_grad < 1e-2, (e_out, e_grad)
    d_out, d_grad = rel(got["out"], fp32["out"]), rel(cat(got["grads"]), cat(fp32["grads"]))
    assert d_out > 1e-6 and d_grad > 1e-6, ("the bf16 mode changed nothing", d_out, d_grad)


@pytest.mark.parametrize("family,edge", [("B", "E17"), ("D", "nl6"), ("A", "L5")])
def test_config_edge_moe_recompute_bitwise(family, edge, attn_path):
    """MoE recompute re-runs the expert forward in the backward: bitwise the saved-activation result, input
    gradients included."""
    fx = _case(family, edge)
    m = build_model(fx["params"], fx["cfg"])
    saved = _run(m, fx)
    m.set_moe_recompute(True)
    rec = _run(m, fx)
    assert not _same_bits(saved, rec)


@functools.lru_cache(maxsize=None)
def _padded_theta0_case():
    """B = 3, N = 65, M = 33 on family A with theta_dim = 0, in the reference calling convention (one padded
    port call, cut per sample)"""
    cfg = _cfg("A", "th0")
    B, N, M = 3, 65, 33
    rng = np.random.default_rng(29)
    x = rng.random((B, N, cfg["input_dim"]))
    fn = rng.random((B, M, cfg["input_func_dim"]))
    thetas = [np.zeros(0) for _ in range(B)]
    Gs = [rng.standard_normal((N, cfg["out_dim"])) for _ in range(B)]
    return _assemble(cfg, _params(cfg, 29), list(x), thetas, [[f] for f in fn], Gs, groups=[[0, 1, 2]])


def test_theta0_padded_call(attn_path):
    """the reference calling convention m(x[B, N, 2], theta[B, 0], fns) with theta_dim = 0"""
    fx = _padded_theta0_case()
    cfg = fx["cfg"]
    B, N, M = 3, 65, 33
    m = build_model(fx["params"], cfg)
    dev = torch.device("cuda")
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).requires_grad_(True)
    x, th = t(fx["x"].reshape(B, N, -1)), t(fx["theta"])
    assert th.shape == (B, 0)
    fns = t(fx["fns"][0].reshape(1, B, M, -1))
    out = m(x, th, fns)
    assert out.shape == (B, N, cfg["out_dim"])
    (out * torch.tensor(fx["G"].reshape(B, N, -1), dtype=torch.float32, device=dev)).sum().backward()
    torch.cuda.synchronize()
    assert th.grad is not None and th.grad.shape == (B, 0)
    np64 = lambda a: a.detach().double().cpu().numpy()
    got = dict(out=np64(out).reshape(B * N, -1), grads={k: np64(p.grad) for k, p in m.named_parameters()},
               dx=np64(x.grad).reshape(B * N, -1), dtheta=np64(th.grad), dfns=[np64(fns.grad)[0].reshape(B * M, -1)])
    _log("fp32", "A", "th0-padded_3x65", attn_path, got, fx, tag="CFGE")
    errs = check_parity_per_sample(got, fx)
    assert not errs, errs
