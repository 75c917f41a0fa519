"""Fixture loading + the parity tolerance rule shared by the CPU and GPU tests."""
import contextlib
import glob
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_names():
    """the model fixtures: every archive with a "meta" entry (train_step_bits.npz, which has none, belongs to
    test_gpu_train_bits.py)"""
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz"))
                  if "meta" in np.load(f).files)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))   # allow_pickle=False (default)
    meta = json.loads(str(z["meta"]))
    cfg = dict(meta["cfg"])
    I = cfg["n_input_functions"]
    fx = dict(
        meta=meta, cfg=cfg,
        params={k[2:]: z[k] for k in z.files if k.startswith("p.")},
        grads={k[2:]: z[k] for k in z.files if k.startswith("g.")},
        e32={k[4:]: float(z[k]) for k in z.files if k.startswith("e32.")},
        x=z["x"], x_off=z["x_off"], theta=z["theta"], G=z["G"], out=z["out"],
        fns=[z[f"fn{i}"] for i in range(I)], fn_offs=[z[f"fn{i}_off"] for i in range(I)],
    )
    return fx


def model_args(cfg):
    d = cfg["d"]
    return (cfg["input_dim"], cfg["theta_dim"], cfg["input_func_dim"], cfg["out_dim"], cfg["n_attn_layers"],
            d, cfg["n_mlp_num_layers"], d, d, cfg["n_expert"], cfg["n_head"], cfg["n_input_functions"])


# Parity rule (fp32 vs the reference's float64 result):
#   * whole-model: ||out - ref|| / ||ref|| <= RTOL and, over all parameter gradients concatenated,
#     ||g - ref|| / ||ref|| <= RTOL  (north_star: "within 1e-4 relative in fp32", norm-wise as
#     SURVEY.md §6 prescribes)
#   * per tensor: ||g - ref|| <= RTOL * ||ref|| + SLACK * e32, where e32 is the reference's OWN
#     fp32-vs-fp64 error on that tensor (stored in the fixture).  Some gradients are pure
#     cancellation at nn.Linear's default init (e.g. key-projection grads ~1e-13 while their fp32
#     noise is ~1e-10); e32 bounds what any fp32 implementation can achieve on them.
RTOL = 1e-4
SLACK = 20.0


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check_parity(out, grads, fx, rtol=RTOL, slack=SLACK):
    errs = []
    # every comparison is written `not (err <= bound)`: a NaN error (a non-finite output or gradient) fails
    e_out = rel(out, fx["out"])
    if not e_out <= rtol:
        errs.append(f"output rel err {e_out:.3e} > {rtol}")
    if grads is not None:
        keys = sorted(fx["grads"])
        g = np.concatenate([np.ravel(grads[k]) for k in keys])
        r = np.concatenate([np.ravel(fx["grads"][k]) for k in keys])
        e_all = rel(g, r)
        if not e_all <= rtol:
            errs.append(f"all-grad rel err {e_all:.3e} > {rtol}")
        for k in keys:
            d = float(np.linalg.norm(np.asarray(grads[k], np.float64) - fx["grads"][k]))
            lim = rtol * float(np.linalg.norm(fx["grads"][k])) + slack * fx["e32"].get(k, 0.0)
            if not d <= lim:
                errs.append(f"{k}: |err| {d:.3e} > {lim:.3e}")
    return errs


# ---------------------------------------------------------------------------------------------------------
# Per-sample reference and parity rule (tests/test_gpu_geometry.py).  The packed ABI defines a packed batch
# as independent B = 1 reference calls, so the reference is the stock-torch port (oracle/torch_port.py) in
# float64, one call per non-empty sample: that sample's output rows, its dx / dtheta / dfns, and its share
# of every parameter gradient.  A second pass in float32 gives the reference's OWN fp32 error (e32), per
# parameter tensor as above and also per sample and per output row.
def _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, dtype):
    import torch
    dt = getattr(torch, dtype)
    from oracle import torch_port
    I = cfg["n_input_functions"]
    p = {k: torch.tensor(np.asarray(v), dtype=dt).requires_grad_(True) for k, v in params.items()}
    res = [None] * len(xs)
    for grp in groups:
        x = torch.tensor(np.stack([xs[b] for b in grp]), dtype=dt).requires_grad_(True)
        t = torch.tensor(np.stack([thetas[b] for b in grp]), dtype=dt).requires_grad_(True)
        fs = [torch.tensor(np.stack([fns_ps[b][i] for b in grp]), dtype=dt).requires_grad_(True) for i in range(I)]
        out = torch_port.gnot_forward(p, cfg, x, t, fs)
        (out * torch.tensor(np.stack([Gs[b] for b in grp]), dtype=dt)).sum().backward()   # param grads accumulate
        f64 = lambda a: a.detach().double().numpy().copy()
        # an input the output does not depend on has no .grad: zeros of its shape, as for the parameters below
        gx, gt, gf = [torch.zeros_like(v) if v.grad is None else v.grad for v in (x, t)] + \
                     [[torch.zeros_like(f) if f.grad is None else f.grad for f in fs]]
        for k, b in enumerate(grp):
            res[b] = dict(out=f64(out[k]), dx=f64(gx[k]), dtheta=f64(gt[k]), dfns=[f64(g[k]) for g in gf])
    grads = {k: (np.zeros(v.shape) if v.grad is None else v.grad.double().numpy().copy()) for k, v in p.items()}
    return res, grads


def port_reference(cfg, params, xs, thetas, fns_ps, Gs, groups=None):
    """The per-sample reference of a batch: xs[b] [N_b, in], thetas[b] [th], fns_ps[b][i] [M_ib, F], Gs[b]
    [N_b, out] (the output cotangent).  A sample with N_b = 0 contributes no rows and a zero gradient: it is
    left out of the reference calls, its dtheta row and dfns rows are exactly zero.  groups: lists of sample
    indices run as ONE padded reference call each (equal shapes); default one B = 1 call per non-empty sample.

    Returns (samples, grads, e32): samples[b] = dict(N, M, out, dx, dtheta, dfns, e32=dict(out, dx, dtheta, dfns,
    rows)) with the float64 values and the norms of the reference's fp32-minus-fp64 differences (rows: one
    norm per output row); grads / e32: parameter gradients summed over samples and their fp32 error norms,
    the form check_parity takes."""
    if groups is None:
        groups = [[b] for b in range(len(xs)) if len(xs[b]) > 0]
    p64 = _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float64")
    p32 = _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float32")
    return _port_compare(cfg, xs, thetas, fns_ps, Gs, p64, p32)


def _port_compare(cfg, xs, thetas, fns_ps, Gs, p64, p32):
    """port_reference's result from a float64 pass and a float32 pass of _port_pass"""
    B, I = len(xs), cfg["n_input_functions"]
    (r64, g64), (r32, g32) = p64, p32
    nrm = lambda a, b: float(np.linalg.norm(a - b))
    samples = []
    for b in range(B):
        M = [len(fns_ps[b][i]) for i in range(I)]
        if r64[b] is None:       # empty sample: no rows, exact-zero input gradients
            z = dict(out=np.zeros((0, np.shape(Gs[b])[1])), dx=np.zeros((0, np.shape(xs[b])[1])),
                     dtheta=np.zeros(np.shape(thetas[b])), dfns=[np.zeros(np.shape(fns_ps[b][i])) for i in range(I)])
            samples.append(dict(z, N=0, M=M, e32=dict(out=0.0, dx=0.0, dtheta=0.0, dfns=[0.0] * I, rows=np.zeros(0))))
            continue
        a, c = r64[b], r32[b]
        e = dict(out=nrm(c["out"], a["out"]), dx=nrm(c["dx"], a["dx"]), dtheta=nrm(c["dtheta"], a["dtheta"]),
                 dfns=[nrm(c["dfns"][i], a["dfns"][i]) for i in range(I)],
                 rows=np.linalg.norm(c["out"] - a["out"], axis=1))
        samples.append(dict(a, N=len(xs[b]), M=M, e32=e))
    return samples, g64, {k: nrm(g32[k], g64[k]) for k in g64}


def split_samples(got, samples):
    """Cut packed GPU results (out [P, out], dx [P, in], dtheta [B, th], dfns[i] [Q_i, F]) into the per-sample
    pieces of port_reference's `samples`."""
    pieces, p0 = [], 0
    q0 = [0] * len(got["dfns"])
    for b, s in enumerate(samples):
        pc = dict(out=np.asarray(got["out"][p0:p0 + s["N"]], np.float64), dx=np.asarray(got["dx"][p0:p0 + s["N"]], np.float64),
                  dtheta=np.asarray(got["dtheta"][b], np.float64),
                  dfns=[np.asarray(got["dfns"][i][q0[i]:q0[i] + s["M"][i]], np.float64) for i in range(len(q0))])
        p0 += s["N"]
        q0 = [q + m for q, m in zip(q0, s["M"])]
        pieces.append(pc)
    return pieces


SEG = 64    # points per attention chunk (engine.cpp kSeg): failure texts place a row within its chunk


def per_sample_errors(got, fx):
    """The figures of the per-sample rule, before any bound: for every non-empty sample b a dict with the
    error norm, the reference norm and e32 of its output rows / dx rows / dtheta row / each dfns segment, and
    per output row the arrays err, ref, e32 plus the sample's rms row norm."""
    figs = []
    for b, (s, g) in enumerate(zip(fx["samples"], split_samples(got, fx["samples"]))):
        if s["N"] == 0:
            figs.append(None)
            continue
        parts = [("out", g["out"], s["out"], s["e32"]["out"]), ("dx", g["dx"], s["dx"], s["e32"]["dx"]),
                 ("dtheta", g["dtheta"], s["dtheta"], s["e32"]["dtheta"])]
        parts += [(f"dfn{i}", g["dfns"][i], s["dfns"][i], s["e32"]["dfns"][i]) for i in range(len(s["dfns"]))]
        f = {name: dict(err=float(np.linalg.norm(a - r)), ref=float(np.linalg.norm(r)), e32=float(e))
             for name, a, r, e in parts}
        rown = np.linalg.norm(s["out"], axis=1)
        f["rows"] = dict(err=np.linalg.norm(g["out"] - s["out"], axis=1), ref=rown, e32=np.asarray(s["e32"]["rows"]),
                         rms=float(np.sqrt(np.mean(rown ** 2))))
        figs.append(f)
    return figs


def worst_relative(figs):
    """(worst per-sample err / ref over every checked piece, "piece@sample" it was found at, worst per-row
    err / max(row norm, sample rms), "row@sample"): what a log line carries.  A NaN counts as the worst."""
    ws, wr = (-1.0, "-"), (-1.0, "-")
    key = lambda v: np.inf if np.isnan(v) else v
    for b, f in enumerate(figs):
        if f is None:
            continue
        for k, v in f.items():
            if k != "rows":
                ws = max(ws, (v["err"] / max(v["ref"], 1e-300), f"{k}@{b}"), key=lambda t: key(t[0]))
        r = f["rows"]
        q = r["err"] / np.maximum(np.maximum(r["ref"], r["rms"]), 1e-300)
        w = int(np.argmax(np.where(np.isnan(q), np.inf, q)))
        wr = max(wr, (float(q[w]), f"row{w}@{b}"), key=lambda t: key(t[0]))
    return ws[0], ws[1], wr[0], wr[1]


def check_parity_per_sample(got, fx, rtol=RTOL, slack=SLACK):
    """The parity rule (rtol * ||ref|| + slack * e32, `not (err <= bound)` so a NaN fails) applied
      * to the whole batch: output and parameter gradients, check_parity unchanged;
      * to every non-empty sample on its own: its output rows, its dx rows, its dtheta row and each of its
        dfns segments -- a few per cent of error confined to a 1-point sample is 1e-4 of nothing in a
        whole-batch norm;
      * to every output row: ||err_row|| <= rtol * max(||ref_row||, rms row norm of its sample) + slack * e32_row.
    got: dict(out, grads, dx, dtheta, dfns) of packed arrays; fx: a case with "samples" (port_reference).  A
    failure names the sample, its (N_b, M_b) and the worst row's place in the sample and in its 64-point
    attention chunk, so that it points at a tile edge."""
    errs = check_parity(got["out"], got["grads"], fx, rtol, slack)
    for b, f in enumerate(per_sample_errors(got, fx)):
        if f is None:
            continue
        s = fx["samples"][b]
        tag = f"sample {b} (N={s['N']}, M={s['M']})"
        rows = f["rows"]
        lim_r = rtol * np.maximum(rows["ref"], rows["rms"]) + slack * rows["e32"]
        bad = ~(rows["err"] <= lim_r)
        with np.errstate(invalid="ignore"):
            ratio = np.where(np.isfinite(rows["err"]), rows["err"] / lim_r, np.inf)
        w = int(np.argmax(ratio))
        where = f"worst row {w} of {s['N']} (point {w % SEG} of a {min(SEG, s['N'] - w // SEG * SEG)}-point chunk {w // SEG})"
        for name, v in f.items():
            if name == "rows":
                continue
            lim = rtol * v["ref"] + slack * v["e32"]
            if not v["err"] <= lim:
                errs.append(f"{tag} {name}: |err| {v['err']:.3e} > {lim:.3e} (ref {v['ref']:.3e})"
                            + (f"; {where}" if name == "out" else ""))
        if bad.any():
            errs.append(f"{tag}: {int(bad.sum())} output rows off, {where}: |err| {rows['err'][w]:.3e} > {lim_r[w]:.3e}")
    return errs


# ---------------------------------------------------------------------------------------------------------
# Trained-scale value ranges (tests/test_gpu_value_range.py).  At nn.Linear's default init no GELU
# pre-activation leaves [-2, 2] and no softmax sees a logit spread above 0.5; scaling three groups of
# parameters reaches the ranges of a trained model while the float64 reference stays well conditioned.
_QK = re.compile(r"\.(query|key)(\.\d+)?\.(weight|bias)$")

# regime: (a, b, c) and the ranges its reference must reach: max |GELU pre-activation|, largest softmax
# logit spread, share of pre-activations beyond 3, largest logit inside a q / k head softmax.
# `overflow` is `sharp` with q / k logits past ln(FLT_MAX) = 88.72: softmax(h) = exp(h) / sum exp(h) is the same
# function with and without the max subtracted until exp(h) itself overflows, so only a logit up there tells
# `__expf(h - m)` from `__expf(h)` (a spread of 100 around zero does not).
REGIMES = {
    "moderate": dict(abc=(1.6, 8.0, 3.0), max_h=6.0, spread=8.0, share=0.005, head_logit=0.0),
    "sharp": dict(abc=(2.0, 16.0, 4.0), max_h=10.0, spread=30.0, share=0.005, head_logit=0.0),
    "saturated": dict(abc=(2.2, 30.0, 5.0), max_h=16.0, spread=88.0, share=0.005, head_logit=0.0),
    "qk_only": dict(abc=(1.0, 60.0, 1.0), max_h=0.0, spread=15.0, share=0.0, head_logit=0.0),
    "overflow": dict(abc=(2.0, 100.0, 4.0), max_h=10.0, spread=30.0, share=0.005, head_logit=95.0),
}


def param_group(key):
    """'a': the weight of an MLP Linear outside the gating MLP; 'b': weight or bias of an attention query / key
    projection; 'c': any gating tensor; None: everything else (MLP biases, value projections, fc_out)"""
    if key.startswith("gating."):
        return "c"
    if _QK.search(key):
        return "b"
    if ".layers." in key and key.endswith("weight"):
        return "a"
    return None


def scaled_params(cfg, seed, a, b, c):
    """float64 state-dict of GNOT(*model_args(cfg)) under torch.manual_seed(seed) with the groups of
    param_group multiplied by a, b and c"""
    import torch
    from gnot_amd import GNOT
    torch.manual_seed(seed)
    f = {"a": a, "b": b, "c": c, None: 1.0}
    return {k: v.double().numpy() * f[param_group(k)] for k, v in GNOT(*model_args(cfg)).state_dict().items()}


class _Shim:
    """a module with some attributes replaced"""
    def __init__(self, base, **over):
        self._base = base
        self.__dict__.update(over)

    def __getattr__(self, name):
        return getattr(self._base, name)


@contextlib.contextmanager
def port_hooks(gelu=None, softmax=None, linear=None):
    """Inside the context oracle.torch_port calls these in place of F.gelu / torch.softmax / F.linear.  Only
    the names the port's own module looks up are replaced (torch itself is untouched) and both are restored
    on exit, so the port's arithmetic outside the context cannot change."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_port
    pick = lambda **kw: {k: v for k, v in kw.items() if v is not None}
    saved = torch_port.F, torch_port.torch
    torch_port.F = _Shim(F, **pick(gelu=gelu, linear=linear))
    torch_port.torch = _Shim(torch, **pick(softmax=softmax))
    try:
        yield
    finally:
        torch_port.F, torch_port.torch = saved


class RangeProbe:
    """What the port's float64 pass really reaches: max |GELU pre-activation|, the share of pre-activations
    beyond 3, the largest (max - min) logit inside any softmax (feature softmax of q / k, expert gate), and the
    largest logit inside a q / k head softmax."""
    def __init__(self):
        self.max_h, self.n_h, self.n_big, self.spread, self.head_logit = 0.0, 0, 0, 0.0, 0.0

    @property
    def share(self):
        return self.n_big / max(self.n_h, 1)

    def hooks(self):
        import torch
        import torch.nn.functional as F

        def gelu(h):
            if h.dtype == torch.float64 and h.numel():
                a = h.detach().abs()
                self.max_h = max(self.max_h, float(a.max()))
                self.n_h += a.numel()
                self.n_big += int((a > 3.0).sum())
            return F.gelu(h)

        def softmax(t, dim):
            if t.dtype == torch.float64 and t.numel():
                d = t.detach()
                self.spread = max(self.spread, float((d.max(dim).values - d.min(dim).values).max()))
                if d.dim() == 4:            # [B, H, L, dh]: a feature softmax over a head of q or k
                    self.head_logit = max(self.head_logit, float(d.max()))
            return torch.softmax(t, dim)

        return port_hooks(gelu=gelu, softmax=softmax)


def port_reference_ranges(cfg, params, xs, thetas, fns_ps, Gs):
    """port_reference plus what its float64 pass reached and a second fp32 pass with denormals flushed.
    Returns (samples, grads, e32, probe, flushed): flushed = (samples, e32) measured with the fp32 pass under
    torch.set_flush_denormal(True), or None where the machine cannot flush."""
    import torch
    groups = [[b] for b in range(len(xs)) if len(xs[b]) > 0]
    probe = RangeProbe()
    with probe.hooks():
        p64 = _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float64")
    p32 = _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float32")
    samples, grads, e32 = _port_compare(cfg, xs, thetas, fns_ps, Gs, p64, p32)
    flushed = None
    if torch.set_flush_denormal(True):
        try:
            pf = _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float32")
        finally:
            torch.set_flush_denormal(False)
        sf, _, ef = _port_compare(cfg, xs, thetas, fns_ps, Gs, p64, pf)
        flushed = (sf, ef)
    return samples, grads, e32, probe, flushed


def reference_sharpness(samples):
    """(worst SLACK * e32 / (RTOL * ||out||) over the non-empty samples, the same per output row with the
    floor max(row norm, sample rms) of check_parity_per_sample)"""
    ws, wr = 0.0, 0.0
    for s in samples:
        if s["N"] == 0:
            continue
        ws = max(ws, SLACK * s["e32"]["out"] / (RTOL * float(np.linalg.norm(s["out"]))))
        rown = np.linalg.norm(s["out"], axis=1)
        floor = np.maximum(rown, np.sqrt(np.mean(rown ** 2)))
        wr = max(wr, float((SLACK * np.asarray(s["e32"]["rows"]) / (RTOL * floor)).max()))
    return ws, wr


def value_range_conditions(fx, regime):
    """The conditions a value-range case must meet on its reference alone (fx: samples, probe, flushed of
    port_reference_ranges); a list of what is missed.  The regime is really reached; the reference is sharp
    (SLACK * e32 at most 0.5 of the RTOL term per sample, 1.5 per row); the same with denormals flushed."""
    R, pr = REGIMES[regime], fx["probe"]
    bad = []
    if not pr.max_h >= R["max_h"]:
        bad.append(f"max |h| {pr.max_h:.2f} < {R['max_h']}")
    if not pr.spread >= R["spread"]:
        bad.append(f"softmax spread {pr.spread:.2f} < {R['spread']}")
    if not pr.share >= R["share"]:
        bad.append(f"share of |h| > 3 {pr.share:.4f} < {R['share']}")
    if not pr.head_logit >= R["head_logit"]:
        bad.append(f"largest q / k softmax logit {pr.head_logit:.1f} < {R['head_logit']}")
    passes = [("", fx["samples"])] + ([(" (denormals flushed)", fx["flushed"][0])] if fx["flushed"] else [])
    for tag, samples in passes:
        ws, wr = reference_sharpness(samples)
        if not ws <= 0.5:
            bad.append(f"reference e32 term per sample{tag}: {ws:.2f} of the RTOL term > 0.5")
        if not wr <= 1.5:
            bad.append(f"reference e32 term per row{tag}: {wr:.2f} of the RTOL term > 1.5")
    return bad


def port_stages(cfg, params, xs, thetas):
    """The port's intermediates the engine exposes, per packed row: name -> dict(ref [P, cols] float64, e32
    [P] the row norms of the port's fp32-minus-fp64 difference, floor [P] max(row norm, its sample's rms row
    norm)).  "scores": the expert-gate softmax; "query0": the trunk MLP's output."""
    import torch
    from oracle import torch_port
    n_lin = max(cfg["n_mlp_num_layers"], 1) + 1

    def run(dt):
        p = {k: torch.tensor(np.asarray(v), dtype=dt) for k, v in params.items()}
        sc, q0 = [], []
        for x, th in zip(xs, thetas):
            x, th = torch.tensor(np.asarray(x), dtype=dt)[None], torch.tensor(np.asarray(th), dtype=dt)[None]
            sc.append(torch.softmax(torch_port._mlp(p, "gating", x, n_lin), -1)[0].double().numpy())
            xin = torch.cat([x, th[:, None, :].expand(-1, x.shape[1], -1)], -1)
            q0.append(torch_port._mlp(p, "x", xin, n_lin)[0].double().numpy())
        return dict(scores=sc, query0=q0)

    r64, r32 = run(torch.float64), run(torch.float32)
    res = {}
    for name in r64:
        floor = []
        for a in r64[name]:
            rown = np.linalg.norm(a, axis=1)
            floor.append(np.maximum(rown, np.sqrt(np.mean(rown ** 2))))
        ref = np.concatenate(r64[name])
        res[name] = dict(ref=ref, e32=np.linalg.norm(np.concatenate(r32[name]) - ref, axis=1), floor=np.concatenate(floor))
    return res


def port_bf16_emulated(cfg, params, xs, thetas, fns_ps, Gs):
    """(out [P, out], grads) of the float64 port with the weight and the input of every Linear rounded to bf16
    (round to nearest even) before each F.linear, accumulation in float64: what one bf16 operand piece per
    MFMA costs, without the bf16 storage of saved activations and the fp32 accumulation order."""
    import torch
    import torch.nn.functional as F
    bf = lambda t: t.to(torch.bfloat16).to(t.dtype)
    groups = [[b] for b in range(len(xs)) if len(xs[b]) > 0]
    with port_hooks(linear=lambda x, w, b=None: F.linear(bf(x), bf(w), b)):
        res, grads = _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float64")
    return np.concatenate([r["out"] for r in res if r is not None]), grads


# ---------------------------------------------------------------------------------------------------------
# The device GELU's formula (csrc/gnot_common.h gelu_tail / gelu / gelu_grad) on the CPU: in float64, and
# operation by operation in float32 with correctly rounded 1/x and exp2 (tests/test_gpu_gelu.py).
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def gelu_exact64(x):
    """(gelu(x), gelu'(x)) with the exact erf, float64"""
    import torch
    x = np.asarray(x, np.float64)
    Phi = 0.5 * (1.0 + torch.special.erf(torch.from_numpy(x / np.sqrt(2.0))).numpy())
    phi = np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)
    # x Phi(x) for x < 0 from the complementary function: 1 + erf cancels there
    tail = 0.5 * torch.special.erfc(torch.from_numpy(np.abs(x) / np.sqrt(2.0))).numpy()
    Phi = np.where(x < 0, tail, Phi)
    return x * Phi, Phi + x * phi


def gelu_formula64(x):
    """the kernels' Abramowitz-Stegun 7.1.26 form in float64: (gelu, gelu')"""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    t = 1.0 / (1.0 + AS_P * ax / np.sqrt(2.0))
    P = np.zeros_like(x)
    for c in AS_A[::-1]:
        P = P * t + 0.5 * c
    e = np.exp(-0.5 * x * x)
    q = P * t * e
    Phi = 0.5 + np.copysign(0.5 - q, x)
    return np.maximum(x, 0.0) - ax * q, Phi + x * e / np.sqrt(2.0 * np.pi)


def gelu_formula32(x):
    """gnot_common.h's operation sequence in numpy float32: every constant as the compiler folds it, every fmaf
    as one rounding (its exact float64 product plus the addend, rounded once more to float32), 1/x and exp2
    correctly rounded where the device's v_rcp_f32 / v_exp_f32 are 1-ulp approximations: (gelu, gelu')"""
    f32 = np.float32
    x = np.asarray(x, f32)
    f64 = lambda v: np.asarray(v, np.float64)
    fma = lambda a, b, c: (f64(a) * f64(b) + f64(c)).astype(f32)
    ax = np.abs(x)
    k = f32(f32(AS_P) * f32(0.70710678118654752440))
    t = (f32(1.0) / fma(ax, k, f32(1.0))).astype(f32)
    h = [f32(f32(0.5) * f32(c)) for c in AS_A]
    P = fma(t, h[4], h[3])
    P = fma(t, P, h[2])
    P = fma(t, P, h[1])
    P = fma(t, P, h[0])
    arg = (x * (x * f32(-0.72134752044448170368))).astype(f32)
    e = np.exp2(arg.astype(np.float64)).astype(f32)
    q = ((P * t).astype(f32) * e).astype(f32)
    y = fma(-ax, q, np.maximum(x, f32(0.0)))
    Phi = (f32(0.5) + np.copysign((f32(0.5) - q).astype(f32), x)).astype(f32)
    dy = fma((x * f32(0.39894228040143267794)).astype(f32), e, Phi)
    return y, dy


def ulp32(v):
    """the float32 ulp at |v| (of the smallest normal below it)"""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), float(np.finfo(np.float32).tiny))
    return np.exp2(np.floor(np.log2(a)) - 23.0)


def gelu_test_inputs():
    """float32 inputs of the pointwise GELU tests: a grid of 2^20 + 3 points on [-12, 12] (the odd count leaves
    a grid-stride tail), +-0, +-1e-30, +-1e-40 (a denormal), +-2^k for k = -20 .. 5, and the 200 float32
    neighbours on each side of +-3.0834 and +-2.4639, where the formula's error peaks"""
    f32 = np.float32
    parts = [np.linspace(-12.0, 12.0, 2 ** 20 + 3).astype(f32)]
    sp = [0.0, 1e-30, 1e-40] + [2.0 ** k for k in range(-20, 6)]
    parts.append(np.array(sp + [-v for v in sp], f32))
    for c in (3.0834, 2.4639):
        bits = int(np.array(c, f32).view(np.int32))
        nb = (bits + np.arange(-200, 201, dtype=np.int64)).astype(np.int32).view(f32)
        parts += [nb, -nb]
    return np.concatenate(parts)
