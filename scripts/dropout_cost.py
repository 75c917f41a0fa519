#!/usr/bin/env python3
"""What GNOT(..., attn_dropout=p) adds to a step, measured in one process, alternating:
  * the row kernel of csrc/dropout.hip on its own at 262,144 x 256 (the configs[2] attention output), timed with
    device events; GB/s from the algorithmic bytes, 2 C 4 per row (read and write x in place), beside a copy of
    the same bytes.  Philox4x32-10 costs 20 high and 20 low 32-bit multiplies per quad, so the pass may be bound
    by the VALU and not by HBM: the figure says which;
  * an eager training step (pack + forward + RelL2 + backward + FlatAdamW) of the configs[2] model (bench.py
    cfg3: d = 256, 8 heads, 8 experts, 4 blocks, one 805-point input function, one 262,144-point mesh) and of the
    configs[1] model (cfg2: d = 128, 4 experts, 2 input functions, 10,000 points) at p = 0 and p = 0.1.
p = 0 launches nothing and carries no table: it is the step of a model without the keyword.

    python scripts/dropout_cost.py [--points 262144] [--reps 20] [--steps 6] [--out FILE]
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
from gnot_amd.dropout import as_int32, dropout_rows, key_words  # noqa: E402

CFG3 = dict(input_dim=3, theta_dim=1, input_func_dim=3, out_dim=1, n_attn_layers=4, n_attn_hidden_dim=256,
            n_mlp_num_layers=4, n_mlp_hidden_dim=256, n_input_hidden_dim=256, n_expert=8, n_head=8,
            n_input_functions=1)
CFG2 = dict(input_dim=2, theta_dim=1, input_func_dim=3, out_dim=1, n_attn_layers=4, n_attn_hidden_dim=128,
            n_mlp_num_layers=4, n_mlp_hidden_dim=128, n_input_hidden_dim=128, n_expert=4, n_head=8,
            n_input_functions=2)
P_ON = 0.1


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)        # ms


def step_times(cfg, P, dev, gen, warmup, steps):
    """median / min / max ms of the eager training step at p = 0 and p = P_ON: the same weights and data, alternating"""
    I = cfg["n_input_functions"]
    xs = torch.rand(P, cfg["input_dim"], device=dev, generator=gen)
    theta = torch.rand(1, 1, device=dev, generator=gen)
    fns = [torch.rand(805, 3, device=dev, generator=gen) for _ in range(I)]
    tgt = torch.randn(P, 1, device=dev, generator=gen)
    x_off, fn_offs = [0, P], [[0, 805]] * I
    loss_fn = train.RelL2Loss()
    runs = {}
    for name, p in (("p0", 0.0), ("p0.1", P_ON)):
        torch.manual_seed(0)
        m = GNOT(**cfg, attn_dropout=p).to(dev)
        opt = train.FlatAdamW(train.flatten_parameters(m), lr=1e-3)
        m.engine().param_grads = False

        def step(m=m, opt=opt):
            pred = m.forward_packed(xs, x_off, theta, fns, fn_offs)
            loss_fn(x_off, pred, tgt).backward()
            opt.step(m.engine().grad_flat)
        runs[name] = step
    ts = {k: [] for k in runs}
    for rep in range(warmup + steps):
        for k, fn_ in runs.items():
            ms = timed(fn_)
            if rep >= warmup:
                ts[k].append(ms)
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(min(v), 3) for k, v in ts.items()},
            "ms_max": {k: round(max(v), 3) for k, v in ts.items()}, "p0.1_over_p0": round(med["p0.1"] / med["p0"], 4)}


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
    x = torch.randn(P, C, device=dev, generator=gen)
    off = torch.tensor([0, P], dtype=torch.int64, device=dev)
    glo = torch.zeros(1, dtype=torch.int64, device=dev)
    key = torch.tensor(as_int32(key_words(1234, 1)), dtype=torch.int32, device=dev)
    src, dst = torch.empty(P * C, device=dev), torch.empty(P * C, device=dev)
    runs = {
        "dropout_rows": lambda: dropout_rows(x, C, off, glo, key, 0, P_ON),
        "copy_same_bytes": lambda: dst.copy_(src),       # reads and writes P C floats
    }
    t = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for k, fn in runs.items():                       # interleaved: every repetition times all of them
            ms = timed(fn)
            if rep >= args.warmup:
                t[k].append(ms * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = P * 2 * C * 4
    out = {"points": P, "C": C, "reps": args.reps, "p": P_ON, "bytes": nbytes,
           "us_median": {k: round(v, 1) for k, v in med.items()},
           "us_min": {k: round(min(v), 1) for k, v in t.items()},
           "us_max": {k: round(max(v), 1) for k, v in t.items()},
           "dropout_GBps": round(nbytes / med["dropout_rows"] * 1e-3, 1),
           "copy_GBps": round(nbytes / med["copy_same_bytes"] * 1e-3, 1)}
    del x, src, dst
    out["configs2_step"] = step_times(CFG3, P, dev, gen, args.warmup, args.steps)
    out["configs1_step"] = step_times(CFG2, 10000, dev, gen, args.warmup, max(args.steps, 20))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
