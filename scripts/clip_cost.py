#!/usr/bin/env python3
"""What gradient clipping adds to the native step at the configs[2] arena size: the two norm kernels
(gnot_grad_clip) against the AdamW kernel (gnot_adamw_step), and the clipped update
(gnot_adamw_step_clipped), and what the non-finite guard adds to that: the norm alone (gnot_grad_norm) and
the guarded update (gnot_adamw_step_guarded), timed with device events in one process, interleaved, after a
warm-up.
The norm pass reads n floats, AdamW reads 4n and writes 3n, so the clip must cost less than the update.

    python scripts/clip_cost.py [--reps 50]
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
    args = ap.parse_args()
    import bench
    dev = torch.device("cuda", 0)
    model = GNOT(**bench.WORKLOADS["cfg3"]["model"]).to(dev)      # configs[2]'s constructor arguments
    n = train.flatten_parameters(model).numel()      # the arena: engine().grad_flat has the same layout and size
    del model
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    param, grad = (torch.randn(n, device=dev, generator=gen) * s for s in (0.1, 1e-2))
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 1e-3, 1.0], device=dev)
    clip = torch.zeros(2, device=dev)
    guard = torch.zeros(2, dtype=torch.int32, device=dev)
    work = torch.empty(lib.gnot_grad_clip_work_floats(n), device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: t.data_ptr()
    runs = {
        "adamw": lambda: lib.gnot_adamw_step(P(param), P(grad), P(m), P(v), n, P(hyper), s),
        "grad_clip": lambda: lib.gnot_grad_clip(P(grad), n, P(hyper), 1.0, P(work), P(clip), s),
        "adamw_clipped": lambda: lib.gnot_adamw_step_clipped(P(param), P(grad), P(m), P(v), n, P(hyper), P(clip), s),
        "grad_norm": lambda: lib.gnot_grad_norm(P(grad), n, P(hyper), P(work), P(clip), s),
        "adamw_guarded": lambda: lib.gnot_adamw_step_guarded(P(param), P(grad), P(m), P(v), n, P(hyper), P(clip),
                                                             P(guard), s),
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
    out = {"arena_floats": n, "reps": args.reps, "norm": float(clip[0]), "skipped": int(guard[0]),
           "us_median": {k: round(statistics.median(t), 2) for k, t in times.items()},
           "us_min": {k: round(min(t), 2) for k, t in times.items()},
           "us_max": {k: round(max(t), 2) for k, t in times.items()}}
    print(json.dumps(out))
    assert out["us_median"]["grad_clip"] <= out["us_median"]["adamw"], "the clip kernels cost more than AdamW"


if __name__ == "__main__":
    main()
