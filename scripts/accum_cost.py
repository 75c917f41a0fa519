#!/usr/bin/env python3
"""What gradient accumulation costs at configs[1] size (bench.py --workload cfg2: d = 128, 4 experts,
4 blocks, two 805-point input functions, 10,000-point meshes): one optimizer step on ONE plan over two
meshes against the same step as an accumulated group of two one-mesh micro-batches (overwrite, then
accumulate into a caller-owned arena, one FlatAdamW step per group).  Both through the product path
(forward_packed, native RelL2, autograd backward, FlatAdamW), wall time per step between device
synchronisations, interleaved in one process after a warm-up; and the split-K finish alone, overwrite
against accumulate, as device time of one whole backward each.

    python scripts/accum_cost.py [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnot-replication_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gnot_amd import GNOT, train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import bench
    w = bench.WORKLOADS["cfg2"]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = GNOT(**w["model"]).to(dev)
    flat = train.flatten_parameters(model)
    opt = train.FlatAdamW(flat, lr=1e-4)
    model.set_grad_arena(torch.empty(model.grad_numel(), device=dev))
    eng = model.engine()
    eng.param_grads = False
    loss_fn = train.RelL2Loss()
    N, M, I = w["N"], w["M"], w["model"]["n_input_functions"]
    g = torch.Generator(device="cpu").manual_seed(1)
    mesh = lambda: dict(x=torch.rand(N, 2, generator=g).to(dev), theta=torch.rand(1, 1, generator=g).to(dev),
                        fns=[torch.rand(M, 3, generator=g).to(dev) for _ in range(I)],
                        y=(torch.randn(N, 1, generator=g) + 2).to(dev))
    a, b = mesh(), mesh()
    both = dict(x=torch.cat([a["x"], b["x"]]), theta=torch.cat([a["theta"], b["theta"]]),
                fns=[torch.cat([a["fns"][i], b["fns"][i]]) for i in range(I)], y=torch.cat([a["y"], b["y"]]))

    def fwd_bwd(d, B, weight, accumulate):
        off = [N * k for k in range(B + 1)]
        out = model.forward_packed(d["x"], off, d["theta"], d["fns"], [[M * k for k in range(B + 1)]] * I)
        loss = loss_fn(off, out, d["y"])
        with model.backward_options(accumulate=accumulate):
            (loss * weight).backward()

    def one_plan():
        fwd_bwd(both, 2, 1.0, False)
        opt.step(eng.grad_flat)

    def accumulated():
        fwd_bwd(a, 1, 0.5, False)
        fwd_bwd(b, 1, 0.5, True)
        opt.step(eng.grad_flat)

    def bwd_only(accumulate):            # device time of one one-mesh backward, overwrite or accumulate
        off = [0, N]
        out = model.forward_packed(a["x"], off, a["theta"], a["fns"], [[0, M]] * I)
        loss = loss_fn(off, out, a["y"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with model.backward_options(accumulate=accumulate):
            e0.record()
            loss.backward()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {"one_plan_two_meshes": [], "two_accumulated_micro_batches": [], "backward_overwrite": [],
             "backward_accumulate": []}
    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # interleaved in blocks of 5 steps per form: the two forms have different geometries, so the first step
    # of a block re-plans and re-binds the engine and is not timed (an accumulated group itself keeps one
    # geometry here; what a geometry change costs is bench.py --vary-geometry's subject)
    for block in range(-1, (args.reps + 4) // 5):          # block -1: warm-up
        for k, fn in (("one_plan_two_meshes", one_plan), ("two_accumulated_micro_batches", accumulated)):
            fn()
            for _ in range(args.warmup if block < 0 else 5):
                t = timed(fn)
                if block >= 0:
                    times[k].append(t)
        for _ in range(5):
            for k, acc in (("backward_overwrite", False), ("backward_accumulate", True)):
                t = bwd_only(acc)
                if block >= 0:
                    times[k].append(t)
    out = {"workload": "cfg2 widths, 10,000-point meshes", "arena_floats": model.grad_numel(), "reps": args.reps,
           "ms_median": {k: round(statistics.median(t), 4) for k, t in times.items()},
           "ms_min": {k: round(min(t), 4) for k, t in times.items()},
           "ms_max": {k: round(max(t), 4) for k, t in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
