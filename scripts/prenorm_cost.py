#!/usr/bin/env python3
"""What GNOT(..., pre_norm=True) adds to a step, measured in one process, alternating:
  * the two row kernels of csrc/norm.hip on their own at 262,144 x 256 (the configs[2] residual stream), timed with
    device events; GB/s from the algorithmic bytes, 2 C 4 per row forward (read x, write y; the 4-byte rstd
    not counted) and 4 C 4 + 4 backward with accumulate (read y, dy, dx and rstd, write dx);
  * an eager training step (pack + forward + RelL2 + backward + FlatAdamW) of the configs[2] model (bench.py
    cfg3: d = 256, 8 heads, 8 experts, 4 blocks, one 805-point input function, one 262,144-point mesh) with and
    without the option.

    python scripts/prenorm_cost.py [--points 262144] [--reps 20] [--steps 6] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnot-replication_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gnot_amd import GNOT, train  # noqa: E402
from gnot_amd.norm import layer_norm_rows, layer_norm_rows_bwd  # noqa: E402

CFG3 = dict(input_dim=3, theta_dim=1, input_func_dim=3, out_dim=1, n_attn_layers=4, n_attn_hidden_dim=256,
            n_mlp_num_layers=4, n_mlp_hidden_dim=256, n_input_hidden_dim=256, n_expert=8, n_head=8,
            n_input_functions=1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)        # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=262144)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    P, C = args.points, args.width
    gen = torch.Generator(device=dev).manual_seed(0)
    x, dy, dx = (torch.randn(P, C, device=dev, generator=gen) for _ in range(3))
    y, rstd = layer_norm_rows(x)
    src, dst = torch.empty(P * C, device=dev), torch.empty(P * C, device=dev)
    runs = {
        "norm_fwd": lambda: layer_norm_rows(x, out=y),
        "norm_bwd_accumulate": lambda: layer_norm_rows_bwd(y, rstd, dy, dx=dx, accumulate=True),
        "copy_fwd_bytes": lambda: dst.copy_(src),        # reads and writes P C floats: the forward's bytes
    }
    t = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for k, fn in runs.items():                       # interleaved: every repetition times all of them
            ms = timed(fn)
            if rep >= args.warmup:
                t[k].append(ms * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    fwd_bytes, bwd_bytes = P * 2 * C * 4, P * (4 * C * 4 + 4)
    out = {"points": P, "C": C, "reps": args.reps, "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
           "us_median": {k: round(v, 1) for k, v in med.items()},
           "us_min": {k: round(min(v), 1) for k, v in t.items()},
           "us_max": {k: round(max(v), 1) for k, v in t.items()},
           "fwd_GBps": round(fwd_bytes / med["norm_fwd"] * 1e-3, 1),
           "bwd_GBps": round(bwd_bytes / med["norm_bwd_accumulate"] * 1e-3, 1),
           "copy_GBps": round(fwd_bytes / med["copy_fwd_bytes"] * 1e-3, 1)}
    del x, dy, dx, y, rstd, src, dst

    # the training step, with and without the option: the same weights and data, eager, alternating
    xs = torch.rand(P, 3, device=dev, generator=gen)
    theta = torch.rand(1, 1, device=dev, generator=gen)
    fn = torch.rand(805, 3, device=dev, generator=gen)
    tgt = torch.randn(P, 1, device=dev, generator=gen)
    x_off, fn_off = [0, P], [0, 805]
    loss_fn = train.RelL2Loss()
    steps = {}
    for name, on in (("plain", False), ("pre_norm", True)):
        torch.manual_seed(0)
        m = GNOT(**CFG3, pre_norm=on).to(dev)
        opt = train.FlatAdamW(train.flatten_parameters(m), lr=1e-3)
        m.engine().param_grads = False

        def step(m=m, opt=opt):
            pred = m.forward_packed(xs, x_off, theta, [fn], [fn_off])
            loss_fn(x_off, pred, tgt).backward()
            opt.step(m.engine().grad_flat)
        steps[name] = step
    ts = {k: [] for k in steps}
    for rep in range(args.warmup + args.steps):
        for k, fn_ in steps.items():
            ms = timed(fn_)
            if rep >= args.warmup:
                ts[k].append(ms)
    smed = {k: statistics.median(v) for k, v in ts.items()}
    out["step_ms_median"] = {k: round(v, 2) for k, v in smed.items()}
    out["step_ms_min"] = {k: round(min(v), 2) for k, v in ts.items()}
    out["step_ms_max"] = {k: round(max(v), 2) for k, v in ts.items()}
    out["step_pre_norm_over_plain"] = round(smed["pre_norm"] / smed["plain"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
