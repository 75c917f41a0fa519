"""Trained-scale activations: the model against float64 where GELU saturates and the softmaxes are peaked.

Every other model-level test builds its weights at nn.Linear's default init, where no GELU pre-activation
leaves [-2, 2] and no softmax sees a logit spread above 0.5: there `__expf(h - m)` without the `- m`, a max
over the wrong lanes or over a pad column, and a GELU tail that is wrong beyond 3 all pass 1e-4.  A trained
GNOT does not stay there.  golden_util.scaled_params multiplies three groups of parameters (a: the MLP
weights, b: the attention query / key projections, c: the gating MLP) and reaches five regimes in which the
float64 reference stays well conditioned (golden_util.REGIMES):

  regime     (a, b, c)       max |h|   share |h| > 3   largest softmax spread
  moderate   (1.6,  8, 3)    >= 6      >= 0.5 %        >= 8
  sharp      (2.0, 16, 4)    >= 10     >= 0.5 %        >= 30
  saturated  (2.2, 30, 5)    >= 16     >= 0.5 %        >= 88  (past fp32 exp's underflow at 87.3)
  qk_only    (1.0, 60, 1)    -         -               >= 15
  overflow   (2.0, 100, 4)   >= 10     >= 0.5 %        >= 30, and a q / k logit >= 95

`overflow` exists because exp(h) / sum exp(h) is the same function with and without the max subtracted until
exp(h) itself overflows at h = 88.72: a scratch build of softmax_heads without the `- m` passed the four other
regimes (their logits spread by up to 100 around zero and stay below 88) and fails this one.

Families, one per softmax / GELU code path (L = 1 and two-layer MLPs unless noted):
  A    d = 64,  4 heads,  3 experts, 2 input functions   chain.hip / linear.hip, dh = 16
  A4   d = 16,  4 heads,  2 experts, 1                   softmax_heads' dh = 4 branch
  A8   d = 64,  8 heads,  2 experts, 1                   its dh = 8 branch
  A12  d = 96,  8 heads,  3 experts, 1                   dh = 12: the butterfly branch, heads straddle tiles
  Ap   d = 100, 4 heads,  2 experts, 1                   dh 25 -> 28: the -INFINITY mask of padded heads
  W    d = 128, 1 head,   2 experts, 1                   dh = 128, the wide attention forms
  B    d = 256, 8 heads,  3 experts, 1                   chain2.hip / linear2.hip
  B'   d = 256, 8 heads,  3 experts, 0, L = 2            fused q|k|v softmax, self-attention only
  B1   d = 256, 1 head,   3 experts, 1                   dh = 256, linear2's wide softmax heads
  D    d = 320, 10 heads, 2 experts, 1                   chainw.hip, its gate softmax and cw_gelu* kernels

Each case is one packed batch of Ns = [161, 3, 1, 64], Ms = [65, 2, 1, 64] (a second input function takes Ms
reversed): a partial 64-point chunk, a whole one, a one-point sample, more than kMinSplitPoints.  Inputs: x and
the input functions in [-1, 1), theta in [0, 1).

Before anything touches the GPU a case must meet golden_util.value_range_conditions on its reference alone:
the regime's ranges are really reached (measured inside the port's float64 pass), and SLACK * e32 stays at most
0.5 of the RTOL term per sample and 1.5 per output row, also with the fp32 pass's denormals flushed -- fp32
with flushed denormals can do these cases to about 1e-6, so a miss on the GPU is the kernels'.
tests/test_oracle.py runs the same conditions for all 50 cases without a GPU.

Every case prints one "RANGE" line; profiles/value_range_parity.txt is that output on the MI355X.
"""
import functools

import numpy as np
import pytest

from golden_util import (REGIMES, check_parity_per_sample, per_sample_errors, port_bf16_emulated,
                         port_reference_ranges, port_stages, reference_sharpness, rel, scaled_params,
                         value_range_conditions, worst_relative, RTOL, SLACK)
from test_gpu_geometry import _run, _same_bits
from test_gpu_parity import attn_path, build_model  # noqa: F401

pytestmark = pytest.mark.gpu


def _cfg(d, H, E, I, L=1):
    return dict(input_dim=2, theta_dim=1, input_func_dim=3, out_dim=2, n_attn_layers=L, d=d, n_mlp_num_layers=2,
                n_expert=E, n_head=H, n_input_functions=I)


FAMILIES = {"A": _cfg(64, 4, 3, 2), "A4": _cfg(16, 4, 2, 1), "A8": _cfg(64, 8, 2, 1), "A12": _cfg(96, 8, 3, 1),
            "Ap": _cfg(100, 4, 2, 1), "W": _cfg(128, 1, 2, 1), "B": _cfg(256, 8, 3, 1), "Bs": _cfg(256, 8, 3, 0, L=2),
            "B1": _cfg(256, 1, 3, 1), "D": _cfg(320, 10, 2, 1)}          # Bs: the docstring's B'
NS, MS = [161, 3, 1, 64], [65, 2, 1, 64]
CASES = [(f, r) for f in FAMILIES for r in REGIMES]

# a case whose reference misses a condition at seed 17 and the regime's factors gets another seed or other
# factors here (never a wider rule): (family, regime) -> dict(seed=..., abc=(a, b, c))
OVERRIDES = {
    # narrow heads spread their logits less: at the regime's own b the reference reaches a spread of 7.5
    # (A4 moderate), 83 and max |h| 15.6 (A4 saturated), 82 (A8 saturated), 29.4 (Ap sharp), 74 (Ap saturated)
    ("A4", "moderate"): dict(abc=(1.6, 10.0, 3.0)),
    ("A4", "saturated"): dict(abc=(2.4, 30.0, 5.5)),      # at d = 16 the largest |h| is the gating MLP's
    ("A8", "saturated"): dict(abc=(2.2, 36.0, 5.0)),
    ("Ap", "sharp"): dict(abc=(2.0, 18.0, 4.0)),
    ("Ap", "saturated"): dict(abc=(2.2, 40.0, 5.0)),
    # at b = 100 the fp32 reference pass with denormals flushed loses a 1 / (q . sum k) of family A12 (3759 times
    # the RTOL term on one sample); b = 72 still reaches a logit of 113
    ("A12", "overflow"): dict(abc=(2.0, 72.0, 4.0)),
}


@functools.lru_cache(maxsize=None)
def _case(family, regime):
    """one reference per (family, regime), shared by both attention paths and the bf16 / recompute / stage runs"""
    cfg = FAMILIES[family]
    I = cfg["n_input_functions"]
    over = OVERRIDES.get((family, regime), {})
    seed, abc = over.get("seed", 17), over.get("abc", REGIMES[regime]["abc"])
    Ms = [MS, MS[::-1]][:I]
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(-1.0, 1.0, (n, cfg["input_dim"])) for n in NS]
    thetas = [rng.random(cfg["theta_dim"]) for _ in NS]
    fns_ps = [[rng.uniform(-1.0, 1.0, (Ms[i][b], cfg["input_func_dim"])) for i in range(I)] for b in range(len(NS))]
    Gs = [rng.standard_normal((n, cfg["out_dim"])) for n in NS]
    params = scaled_params(cfg, seed, *abc)
    samples, grads, e32, probe, flushed = port_reference_ranges(cfg, params, xs, thetas, fns_ps, Gs)
    off = lambda L: np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    return dict(cfg=cfg, params=params, samples=samples, grads=grads, e32=e32, probe=probe, flushed=flushed,
                xs=xs, thetas=thetas, fns_ps=fns_ps, Gs=Gs, abc=abc, seed=seed,
                x=np.concatenate(xs), x_off=off(NS), theta=np.stack(thetas),
                fns=[np.concatenate([fns_ps[b][i] for b in range(len(NS))]) for i in range(I)],
                fn_offs=[off(Ms[i]) for i in range(I)],
                G=np.concatenate(Gs), out=np.concatenate([s["out"] for s in samples]))


def _ranges(fx):
    p = fx["probe"]
    return f"max|h| {p.max_h:.2f} share>3 {100 * p.share:.2f}% spread {p.spread:.1f} q/k logit {p.head_logit:.1f}"


def _all_grads(fx, grads):
    keys = sorted(fx["grads"])
    return np.concatenate([np.ravel(grads[k]) for k in keys])


def _log(kind, family, regime, path, got, fx):
    figs = per_sample_errors(got, fx)
    ws, ws_at, wr, wr_at = worst_relative(figs)
    es, er = reference_sharpness(fx["samples"])
    e_all = rel(_all_grads(fx, got["grads"]), _all_grads(fx, fx["grads"]))
    print(f"\nRANGE {kind} {family}/{regime} {path}: {_ranges(fx)} | out {rel(got['out'], fx['out']):.2e} "
          f"all-grad {e_all:.2e} worst-sample {ws:.2e} ({ws_at}) worst-row {wr:.2e} ({wr_at}) | reference e32: "
          f"per sample {es * RTOL / SLACK:.1e} per row {er * RTOL / SLACK:.1e} (of the RTOL term: {es:.2f}, {er:.2f})")


def _assert_finite(got):
    arrays = [got["out"], got["dx"], got["dtheta"], *got["dfns"], *got["grads"].values()]
    assert all(np.isfinite(a).all() for a in arrays), "non-finite result"


@pytest.mark.parametrize("family,regime", CASES)
def test_value_range_parity(family, regime, attn_path):
    fx = _case(family, regime)
    missed = value_range_conditions(fx, regime)
    assert not missed, missed
    m = build_model(fx["params"], fx["cfg"])
    plain = _run(m, fx, want=False)
    got = _run(m, fx)
    again = _run(m, fx)
    _log("fp32", family, regime, attn_path, got, fx)
    _assert_finite(got)
    assert not _same_bits(plain, got), "asking for input gradients changed the output or a parameter gradient"
    assert not _same_bits(got, again), "a second run gave other bits"
    errs = check_parity_per_sample(got, fx)
    assert not errs, errs


@pytest.mark.parametrize("regime", ["sharp", "saturated"])
@pytest.mark.parametrize("family", ["A", "B", "D"])
def test_value_range_stages(family, regime):
    """The gate softmax ("scores") and the trunk MLP's output ("query0") against the port's float64
    intermediates, row by row: ||err|| <= RTOL max(||row||, sample rms) + SLACK (the row's fp32-port error);
    every scores row sums to 1 within 4 ulp of 1."""
    fx = _case(family, regime)
    assert not value_range_conditions(fx, regime)
    cfg = fx["cfg"]
    m = build_model(fx["params"], cfg)
    _run(m, fx, want=False)
    P = len(fx["x"])
    stages = port_stages(cfg, fx["params"], fx["xs"], fx["thetas"])
    bad = []
    for name, cols in (("scores", cfg["n_expert"]), ("query0", cfg["d"])):
        st = stages[name]
        got = m.engine().debug_tensor(name, P, cols).double().cpu().numpy()
        err = np.linalg.norm(got - st["ref"], axis=1)
        lim = RTOL * st["floor"] + SLACK * st["e32"]
        w = int(np.argmax(np.where(np.isfinite(err), err / lim, np.inf)))
        print(f"\nRANGE stage {family}/{regime} {name}: worst row {w}: |err| {err[w]:.2e} bound {lim[w]:.2e} "
              f"(row norm {np.linalg.norm(st['ref'][w]):.2e}, fp32-port error {st['e32'][w]:.1e})")
        if not (err <= lim).all():
            bad.append(f"{name}: {int((~(err <= lim)).sum())} rows off, worst row {w}: {err[w]:.3e} > {lim[w]:.3e}")
        if name == "scores":
            dev = np.abs(got.sum(axis=1) - 1.0)
            print(f"RANGE stage {family}/{regime} scores: worst |row sum - 1| {dev.max() / 2.0 ** -23:.2f} ulp")
            if not (dev <= 4 * 2.0 ** -23).all():
                bad.append(f"scores: a row sums to 1 {dev.max():+.3e}")
    assert not bad, bad


@pytest.mark.parametrize("family", ["B", "D"])
def test_value_range_moe_recompute_bitwise(family, attn_path):
    """MoE recompute re-evaluates GELU in the backward: bitwise the saved-activation run at `sharp`"""
    fx = _case(family, "sharp")
    m = build_model(fx["params"], fx["cfg"])
    saved = _run(m, fx)
    m.set_moe_recompute(True)
    rec = _run(m, fx)
    _assert_finite(rec)
    assert not _same_bits(saved, rec)


@functools.lru_cache(maxsize=None)
def _bf16_emulated(family, regime):
    """whole-batch (output, all-gradient) error of the float64 port with bf16-rounded Linear operands"""
    fx = _case(family, regime)
    out, grads = port_bf16_emulated(fx["cfg"], fx["params"], fx["xs"], fx["thetas"], fx["fns_ps"], fx["Gs"])
    return rel(out, fx["out"]), rel(_all_grads(fx, grads), _all_grads(fx, fx["grads"]))


@pytest.mark.parametrize("regime", ["moderate", "sharp"])
@pytest.mark.parametrize("family", ["A", "B"])
def test_value_range_bf16_mode(family, regime, attn_path):
    """bf16 mode away from init scale: finite, other bits than fp32, and the whole-batch output and all-gradient
    errors at most max(1e-2, 4 x the emulated error) -- the float64 port with the weight and the input of every
    Linear rounded to bf16 (golden_util.port_bf16_emulated); the factor 4 covers what the emulation leaves out:
    the bf16 storage of the soft-MoE chains and of the saved gelu', and the accumulation order."""
    fx = _case(family, regime)
    m = build_model(fx["params"], fx["cfg"])
    fp32 = _run(m, fx)
    m.set_precision("bf16")
    got = _run(m, fx)
    _assert_finite(got)
    assert _same_bits(fp32, got), "bf16 mode gave the fp32 bits"
    em_out, em_grad = _bf16_emulated(family, regime)
    e_out = rel(got["out"], fx["out"])
    e_grad = rel(_all_grads(fx, got["grads"]), _all_grads(fx, fx["grads"]))
    print(f"\nRANGE bf16 {family}/{regime} {attn_path}: {_ranges(fx)} | out {e_out:.2e} (emulated {em_out:.2e}) "
          f"all-grad {e_grad:.2e} (emulated {em_grad:.2e})")
    assert e_out <= max(1e-2, 4 * em_out), (e_out, em_out)
    assert e_grad <= max(1e-2, 4 * em_grad), (e_grad, em_grad)
