"""Fixture loading + the parity tolerance rule shared by the CPU and GPU tests."""
import glob
import json
import os

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
        for k, b in enumerate(grp):
            res[b] = dict(out=f64(out[k]), dx=f64(x.grad[k]), dtheta=f64(t.grad[k]), dfns=[f64(f.grad[k]) for f in fs])
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
    B, I = len(xs), cfg["n_input_functions"]
    if groups is None:
        groups = [[b] for b in range(B) if len(xs[b]) > 0]
    r64, g64 = _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float64")
    r32, g32 = _port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, "float32")
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
