"""Shared pieces of the option-combination tests (tests/test_option_combos.py on the CPU,
tests/test_gpu_option_combos.py): models with any subset of pre-norm, attention dropout and the Fourier embedding,
and their float64 reference -- the three single-option references composed, nothing new: the stock-torch port
(oracle/torch_port.py) inside prenorm_util.pre_norm_port() and, inside that, dropout_util.masked_port(masks) (the
mask multiplies the output of the attention that read the normalised rows), run on gnot_amd.fourier_features of
the inputs and differentiated through the embedding down to the raw widths as tests/fourier_util.py does.

One condition on the inputs: a non-empty sample needs at least one point of every input function.  With
N_b > 0 and M_b = 0 the port's normaliser is 0 / 0 and the reference itself is NaN."""
import contextlib

import numpy as np
import torch

import dropout_util as DU
import fourier_util as FU
import golden_util as GU
import prenorm_util as PU

OPTS = frozenset({"prenorm", "drop", "fourier"})
TRIPLE = ("prenorm", "drop", "fourier")
# input_dim 2, theta_dim 1, input_func_dim 3, out_dim 2, 3 experts, n_mlp_num_layers 2: prenorm_util's
IN, TH, F, OUT, E, NL = PU.IN, PU.TH, PU.F, PU.OUT, PU.E, PU.NL
# query points / input-function points per sample (packed): an empty sample that still counts in the dropout key's
# sample index, a one-point sample, a sample ending on a 64-point chunk edge, 129 crossing one by a point; no
# non-empty sample with an empty input function
NS, MS = [129, 0, 64, 1], [17, 5, 3, 1]
# The smallest cases that reach each kernel family the options touch.  nx / nf: the Fourier orders of x and of the
# input functions.  A plan takes an embedded input up to the hidden width: 2 (4 nx + 3) + 1 <= d and
# 3 (4 nf + 3) <= d.  c30 and c40 carry the largest orders that fit: nx = 2 (23 columns of 30; nx = 3 needs 31),
# nf = 1 (21 of 30; nf = 2 needs 33); nx = 4 (39 of 40; nx = 5 needs 47), and no input function to embed at c40.
# seed: the weights' seed where it is not 5 (seed_of).  With two blocks at nn.Linear's default init the attention calls are a
# small part of c64's output, and at seed 5 losing an option moves the reference's output by 0.6 to 1.0e-2 only;
# seed 12 is the first of 0 .. 23 at which every one of the three moves exceeds 1.2e-2
# (tests/test_option_combos.py asserts more than 1e-2).
CASES = {
    "c64": dict(d=64, n_head=4, I=2, L=2, nx=3, nf=2, seed=12),   # chain.hip; batched key/value jobs of 2 functions x 2 blocks
    "c40": dict(d=40, n_head=2, I=0, L=1, nx=4, nf=0),     # internal width 48; cross call in self mode (one shared norm)
    "c30": dict(d=30, n_head=5, I=1, L=1, nx=2, nf=1),     # padded heads
    "c256": dict(d=256, n_head=8, I=1, L=1, nx=3, nf=2),   # chain2.hip / linear2.hip, 256 x 256 weight gradient
    "c320": dict(d=320, n_head=5, I=1, L=1, nx=3, nf=2),   # chainw.hip
    "c64s": dict(d=64, n_head=4, I=1, L=1, nx=3, nf=2),    # the point-sharded run
}


def cfg_of(case):
    """the raw configuration (golden_util / torch_port form): the widths of the caller's tensors"""
    c = CASES[case]
    return dict(input_dim=IN, theta_dim=TH, input_func_dim=F, out_dim=OUT, n_attn_layers=c["L"], d=c["d"],
                n_mlp_num_layers=NL, n_expert=E, n_head=c["n_head"], n_input_functions=c["I"])


def _orders(opts, nx, nf, I):
    return (nx, nf if I > 0 else 0) if "fourier" in opts else (0, 0)


def wide_cfg(cfg, nx, nf):
    """the configuration of the Linears: the embedded widths"""
    return dict(cfg, input_dim=cfg["input_dim"] * FU.width(nx), input_func_dim=cfg["input_func_dim"] * FU.width(nf))


def _check(opts):
    opts = frozenset(opts)
    assert opts <= OPTS, sorted(opts - OPTS)
    return opts


def seed_of(case, seed=None):
    """the weights' seed of a case: the caller's, else the table's own, else 5 (prenorm_util's)"""
    return CASES[case].get("seed", 5) if seed is None else seed


def model(case, opts, seed=None, **kw):
    """gnot_amd.GNOT of a case on the CPU with the options of `opts` (a subset of OPTS) on, its weights drawn
    under seed_of(case, seed); kw overrides"""
    from gnot_amd import GNOT
    opts, c = _check(opts), CASES[case]
    args = {}
    if "prenorm" in opts:
        args.update(pre_norm=True)
    if "drop" in opts:
        args.update(attn_dropout=DU.P_DROP, dropout_seed=DU.SEED)
    if "fourier" in opts:
        args.update(x_fourier=c["nx"], fn_fourier=c["nf"])
    torch.manual_seed(seed_of(case, seed))
    return GNOT(*GU.model_args(cfg_of(case)), **dict(args, **kw))


def params64(case, opts, seed=None):
    """the parameters of model(case, opts, seed) as float64 arrays, built without the HIP library: the plain model
    of the embedded widths draws the same Linears in the same order (pre-norm and dropout add no parameter), and
    only a constructor with a Fourier order probes a plan"""
    from gnot_amd import GNOT
    c = CASES[case]
    nx, nf = _orders(_check(opts), c["nx"], c["nf"], c["I"])
    torch.manual_seed(seed_of(case, seed))
    m = GNOT(*GU.model_args(wide_cfg(cfg_of(case), nx, nf)))
    return {k: v.detach().double().numpy() for k, v in m.named_parameters()}


def inputs(case, Ns=NS, Ms=MS, seed=3):
    """per-sample float64 inputs holding fp32 values (prenorm_util.inputs for this file's cases): xs[b] [N_b, 2]
    in [-1, 1], thetas[b] [1], fns_ps[b][i] [M_b, 3], Gs[b] [N_b, out]"""
    I = CASES[case]["I"]
    rng = np.random.default_rng(seed)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    xs = [r32(rng.uniform(-1, 1, (n, IN))) for n in Ns]
    thetas = [r32(rng.random(TH)) for _ in Ns]
    fns_ps = [[r32(rng.uniform(-1, 1, (m, F))) for _ in range(I)] for m in Ms]
    Gs = [r32(rng.standard_normal((n, OUT))) for n in Ns]
    return xs, thetas, fns_ps, Gs


@contextlib.contextmanager
def port(opts, masks=None, seen=None):
    """Inside the context oracle.torch_port IS the model with the options of `opts`: pre_norm_port() outside,
    masked_port(masks) inside, so that the mask multiplies what the attention made of the normalised rows.  Yields
    masked_port's call counter (None without dropout); every wrapper restores the port on exit.  seen: pre_norm_port's
    list of the (raw, normalised) tensors."""
    opts = _check(opts)
    with contextlib.ExitStack() as stack:
        if "prenorm" in opts:
            stack.enter_context(PU.pre_norm_port(seen=seen))
        yield stack.enter_context(DU.masked_port(masks)) if "drop" in opts else None


def embedded_pass(wide, nx, nf, params, xs, thetas, fns_ps, Gs, groups, dtype):
    """fourier_util._pass with the orders instead of a case name: golden_util._port_pass of the wide
    configuration on fourier_features (in `dtype`) of the inputs, dx and dfns pulled back through
    fourier_features to the raw widths"""
    from gnot_amd import fourier_features
    dt = getattr(torch, dtype)
    emb = lambda a, n: fourier_features(torch.tensor(np.asarray(a), dtype=dt), n).numpy()
    ex = [emb(x, nx) for x in xs]
    ef = [[emb(f, nf) for f in fs] for fs in fns_ps]
    res, grads = GU._port_pass(wide, params, ex, thetas, ef, Gs, groups, dtype)
    for b, r in enumerate(res):
        if r is None:
            continue
        r["dx"] = FU._pull(xs[b], r["dx"], nx, dt)
        r["dfns"] = [FU._pull(fns_ps[b][i], r["dfns"][i], nf, dt) for i in range(len(r["dfns"]))]
    return res, grads


def reference_cfg(cfg, nx, nf, opts, params, xs, thetas, fns_ps, Gs, steps=0, groups=None):
    """reference() for any raw configuration `cfg` and Fourier orders nx / nf"""
    opts = _check(opts)
    nx, nf = _orders(opts, nx, nf, cfg["n_input_functions"])
    wide = wide_cfg(cfg, nx, nf)
    if groups is None:
        groups = [[b] for b in range(len(xs)) if len(xs[b]) > 0]
    masks = None
    if "drop" in opts:
        # masked_port counts one mask per reference call: one B = 1 call per sample
        assert all(len(g) == 1 for g in groups), "with dropout every reference call holds one sample"
        masks = DU.site_masks(wide, [len(x) for x in xs], steps, order=[g[0] for g in groups])
    passes = []
    for dt in ("float64", "float32"):
        with port(opts, masks) as calls:              # a fresh counter per pass
            if "fourier" in opts:
                passes.append(embedded_pass(wide, nx, nf, params, xs, thetas, fns_ps, Gs, groups, dt))
            else:
                passes.append(GU._port_pass(wide, params, xs, thetas, fns_ps, Gs, groups, dt))
        if masks is not None:
            assert calls[0] == len(masks), (calls[0], len(masks))
    return GU._port_compare(wide, xs, thetas, fns_ps, Gs, *passes)


def reference(case, opts, params, xs, thetas, fns_ps, Gs, steps=0, groups=None):
    """golden_util.port_reference of model(case, opts): (samples, grads, e32) as check_parity_per_sample takes
    them, dx / dfns at the raw widths, e32 the float32 composed port's own distance from the float64 one.  steps:
    the dropout step of the packed forward (or steps[b] per sample)."""
    c = CASES[case]
    return reference_cfg(cfg_of(case), c["nx"], c["nf"], opts, params, xs, thetas, fns_ps, Gs, steps, groups)


def as_fx(ref):
    return DU.as_fx(ref)


run_gpu = PU.run_gpu
