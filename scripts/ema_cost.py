#!/usr/bin/env python3
"""What the weight EMA adds to the native step at the configs[2] arena size: the plain update
(gnot_adamw_step), the update with the average fused in (gnot_adamw_step_ema) and the plain update followed
by the stand-alone pass (gnot_ema_update), then the same three behind the non-finite guard, timed with
device events in one process, interleaved, after a warm-up.
AdamW reads 4n and writes 3n floats (28 B per parameter); the fused average adds a read and a write (36 B),
a pass of its own reads the parameter once more (40 B).  Every ratio is taken inside this one run.

    python scripts/ema_cost.py [--reps 50] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnot-replication_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gnot_amd import GNOT, _lib, train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import bench
    dev = torch.device("cuda", 0)
    model = GNOT(**bench.WORKLOADS["cfg3"]["model"]).to(dev)      # configs[2]'s constructor arguments
    n = train.flatten_parameters(model).numel()      # the arena: engine().grad_flat has the same layout and size
    del model
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    param, grad = (torch.randn(n, device=dev, generator=gen) * s for s in (0.1, 1e-2))
    m, v, ema = torch.zeros(n, device=dev), torch.zeros(n, device=dev), param.clone()
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 1e-3, 1.0, 1e-3], device=dev)   # hyper[8]: the EMA weight
    clip = torch.zeros(2, device=dev)
    guard = torch.zeros(2, dtype=torch.int32, device=dev)
    work = torch.empty(lib.gnot_grad_clip_work_floats(n), device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: t.data_ptr()
    _lib.check(lib.gnot_grad_norm(P(grad), n, P(hyper), P(work), P(clip), s))       # a finite norm for the guard
    a = (P(param), P(grad), P(m), P(v))
    ema_pass = lambda: lib.gnot_ema_update(P(ema), P(param), n, P(hyper) + 32, s)
    runs = {
        "adamw": lambda: lib.gnot_adamw_step(*a, n, P(hyper), s),
        "adamw_ema": lambda: lib.gnot_adamw_step_ema(*a, P(ema), n, P(hyper), None, None, s),
        "adamw+ema_update": lambda: lib.gnot_adamw_step(*a, n, P(hyper), s) or ema_pass(),
        "adamw_guarded": lambda: lib.gnot_adamw_step_guarded(*a, n, P(hyper), P(clip), P(guard), s),
        "adamw_ema_guarded": lambda: lib.gnot_adamw_step_ema(*a, P(ema), n, P(hyper), P(clip), P(guard), s),
        "adamw_guarded+ema_update": lambda: lib.gnot_adamw_step_guarded(*a, n, P(hyper), P(clip), P(guard), s)
        or ema_pass(),
    }
    times = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for k, fn in runs.items():                   # interleaved: every repetition times all of them
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(fn())
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(t) for k, t in times.items()}
    out = {"arena_floats": n, "reps": args.reps, "skipped": int(guard[0]),
           "us_median": {k: round(x, 2) for k, x in med.items()},
           "us_min": {k: round(min(t), 2) for k, t in times.items()},
           "us_max": {k: round(max(t), 2) for k, t in times.items()},
           "fused_over_plain": round(med["adamw_ema"] / med["adamw"], 3),
           "fused_over_pair": round(med["adamw_ema"] / med["adamw+ema_update"], 3),
           "guarded_fused_over_plain": round(med["adamw_ema_guarded"] / med["adamw_guarded"], 3),
           "guarded_fused_over_pair": round(med["adamw_ema_guarded"] / med["adamw_guarded+ema_update"], 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
