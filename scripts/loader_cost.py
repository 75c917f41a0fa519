#!/usr/bin/env python3
"""What the data path costs an epoch of train.fit at configs[1]'s model: 32 synthetic meshes of 10,000 points
(two 805-point input functions), batch 4, so 8 optimizer steps an epoch.  Arms:

    parent_host    fit over a CPU DataLoader (collate_packed, pageable copies) on a checkout of the parent commit
                   (--parent DIR, a tree with its library built; left out when not given)
    host           the same loader on this tree (the loss is read back once per epoch instead of per step)
    device         fit over a DeviceLoader on this tree (the dataset in device memory, batches gathered there)
    device_sub     the same with points_per_mesh (--points-per-mesh, default 2500)
    device_norm    `device` with unit-Gaussian normalisation: Normalizer.fit over the dataset (before the warm-up
                   epoch), DeviceLoader(normalizer=) and RelL2Loss(normalizer=)

Every arm runs in a process of its own (one warm-up epoch, then --epochs timed ones, wall time from one
epoch's end to the next, each behind a device synchronise); the arms are interleaved and the round repeated
--reps times, so every arm shows its own spread.  Prints one JSON line.

    python scripts/loader_cost.py [--parent DIR] [--epochs 20] [--reps 3] [--arms device,device_norm] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES, POINTS, FN_POINTS, BATCH = 32, 10000, (805, 805), 4


def child(args):
    """one arm in this process, on the package and the bench.py of args.tree: prints {"epoch_ms": [...], "lib": path}"""
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch

    import bench
    from gnot_amd import GNOT, _lib, data, train

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = GNOT(**bench.WORKLOADS["cfg2"]["model"]).to(dev)          # configs[1]'s constructor arguments
    rng = np.random.default_rng(0)
    samples = [data.synthetic_sample(rng, POINTS, fn_points=FN_POINTS) for _ in range(MESHES)]
    gen = torch.Generator().manual_seed(1)
    kw = {}
    if args.child.startswith("device"):
        ds = data.DeviceDataset(samples, dev)
        if args.child == "device_norm":
            kw["normalizer"] = data.Normalizer.fit(ds)
            kw["loss_fn"] = train.RelL2Loss(kw["normalizer"])
        loader = data.DeviceLoader(ds, BATCH, shuffle=True, generator=gen, normalizer=kw.get("normalizer"),
                                   points_per_mesh=args.points_per_mesh if args.child == "device_sub" else None)
    else:
        loader = torch.utils.data.DataLoader(data.NS2dData(samples), batch_size=BATCH, shuffle=True, generator=gen,
                                             collate_fn=data.collate_packed)
    stamps = []

    def log(msg):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())

    train.fit(model, loader, None, epochs=1 + args.epochs, per_epoch_schedule=False, log=log, **kw)
    print(json.dumps({"epoch_ms": [round((b - a) * 1e3, 3) for a, b in zip(stamps, stamps[1:])], "lib": _lib.LIB_PATH}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--epochs", type=int, default=20, help="timed epochs per process, after one warm-up epoch")
    ap.add_argument("--reps", type=int, default=3, help="processes per arm")
    ap.add_argument("--points-per-mesh", type=int, default=2500)
    ap.add_argument("--arms", default=None, help="comma-separated arms to run (default: all)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    arms = ([("parent_host", "host", os.path.abspath(args.parent))] if args.parent else []) + \
        [("host", "host", ROOT), ("device", "device", ROOT), ("device_sub", "device_sub", ROOT),
         ("device_norm", "device_norm", ROOT)]
    if args.arms:
        arms = [a for a in arms if a[0] in args.arms.split(",")]
    runs = {name: [] for name, _, _ in arms}
    for _ in range(args.reps):
        for name, kind, tree in arms:                # interleaved: every round runs all of them
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--tree", tree, "--epochs", str(args.epochs),
                   "--points-per-mesh", str(args.points_per_mesh)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if res.returncode != 0:
                sys.exit(f"{name} failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
            got = json.loads(res.stdout.strip().splitlines()[-1])
            assert os.path.abspath(got["lib"]).startswith(tree + os.sep), (name, got["lib"])     # the tree it names
            runs[name].append(got["epoch_ms"])
    med = {k: [round(statistics.median(r), 3) for r in v] for k, v in runs.items()}
    out = {"meshes": MESHES, "points": POINTS, "batch": BATCH, "steps_per_epoch": MESHES // BATCH,
           "epochs": args.epochs, "reps": args.reps, "points_per_mesh": args.points_per_mesh,
           "epoch_ms_median_per_process": med,
           "epoch_ms_median": {k: round(statistics.median(v), 3) for k, v in med.items()},
           "epoch_ms_min": {k: round(min(min(r) for r in v), 3) for k, v in runs.items()},
           "epoch_ms_max": {k: round(max(max(r) for r in v), 3) for k, v in runs.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
