#!/usr/bin/env python3
"""What the entries of the loss family cost: gnot_rel_l2_loss, gnot_mse_loss, gnot_lp_loss(rel2) and
gnot_lp_loss(rel1, component weights), the last two with and without the per-sample terms, each with the gradient,
on 262,144 packed rows (4 samples of 65,536) with C = 1 and C = 3 output channels.  --parent-lib names a
libgnot_hip.so built from the parent commit, whose gnot_rel_l2_loss and gnot_mse_loss, and whose gnot_lp_loss for rel2
and mse with the terms, are then timed in the same process.
Every variant is timed in blocks of --calls back-to-back calls between two device events (one call is a few
microseconds of kernels: a single one would time the events); the blocks of all variants are interleaved, repetition
after repetition, after a warm-up, and the medians per call are reported.  gnot_rel_l2_loss / gnot_mse_loss are
gnot_lp_loss(rel2) / (mse) without weights and terms, so each pair should sit inside the spread of repeated blocks
(us_min .. us_max), and under the same kind with the terms (the same kernels and one more store).

    python scripts/lp_loss_cost.py [--parent-lib PATH] [--reps 30] [--calls 200] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnot-replication_amd"))

import torch  # noqa: E402

from gnot_amd import _lib  # noqa: E402

ROWS, B = 262144, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a libgnot_hip.so of the parent commit, timed beside this tree's")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed block")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--weighted", action="store_true",
                    help="also time gnot_lp_loss_weighted (rel2, mse; weights of ones and with a quarter zeros)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.gnot_rel_l2_loss.argtypes = lib.gnot_rel_l2_loss.argtypes
        parent.gnot_mse_loss.argtypes = lib.gnot_mse_loss.argtypes
        parent.gnot_lp_loss.argtypes = lib.gnot_lp_loss.argtypes
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: None if t is None else t.data_ptr()
    off = [b * (ROWS // B) for b in range(B + 1)]
    oh = (ctypes.c_int64 * (B + 1))(*off)
    off_dev = torch.tensor(off, dtype=torch.int64, device=dev)
    out = {"rows": ROWS, "samples": B, "reps": args.reps, "calls_per_block": args.calls}
    for C in (1, 3):
        gen = torch.Generator(device=dev).manual_seed(C)
        pred = torch.randn(ROWS, C, device=dev, generator=gen)
        tgt = torch.randn(ROWS, C, device=dev, generator=gen) + 0.5
        w = torch.tensor([1.0, 0.0, 3.0][:C], device=dev)
        work = torch.empty(lib.gnot_lp_loss_work_floats(oh, B, C), device=dev)
        loss, terms, dpred = torch.empty((), device=dev), torch.empty(B, C, device=dev), torch.empty_like(pred)
        head = (P(pred), P(tgt), P(off_dev), oh, B, C)
        lp = lambda kind, wt, tm, of=lib: (lambda: of.gnot_lp_loss(*head, _lib.LP_KINDS[kind], P(wt), None, P(work),
                                                                   P(loss), P(tm), P(dpred), s))
        tail = (P(work), P(loss), P(dpred), s)
        runs = {}
        if parent is not None:
            runs.update({"parent_rel_l2": lambda: parent.gnot_rel_l2_loss(*head, *tail),
                         "parent_mse": lambda: parent.gnot_mse_loss(*head, *tail),
                         "parent_lp_rel2_terms": lp("rel2", None, terms, parent),
                         "parent_lp_mse_terms": lp("mse", None, terms, parent)})
        runs.update({"rel_l2": lambda: lib.gnot_rel_l2_loss(*head, *tail),
                     "mse": lambda: lib.gnot_mse_loss(*head, *tail),
                     "lp_rel2": lp("rel2", None, None), "lp_rel2_terms": lp("rel2", None, terms),
                     "lp_rel1_w": lp("rel1", w, None), "lp_rel1_w_terms": lp("rel1", w, terms)})
        if args.weighted:      # gnot_lp_loss_weighted beside the unweighted entry of the same kind: one more float a row
            pw = torch.rand(ROWS, device=dev, generator=gen) * 2.9 + 0.1
            pw[torch.rand(ROWS, device=dev, generator=gen) < 0.25] = 0.0
            ones = torch.ones(ROWS, device=dev)
            work_w = torch.empty(lib.gnot_lp_loss_weighted_work_floats(oh, B, C), device=dev)
            lpw = lambda kind, pts: (lambda: lib.gnot_lp_loss_weighted(
                P(pred), P(tgt), P(pts), P(off_dev), oh, B, C, _lib.LP_KINDS[kind], None, None, P(work_w), P(loss), None,
                P(dpred), s))
            runs.update({"lp_mse": lp("mse", None, None), "weighted_rel2_ones": lpw("rel2", ones),
                         "weighted_rel2_quarter_zeros": lpw("rel2", pw), "weighted_mse_ones": lpw("mse", ones),
                         "weighted_mse_quarter_zeros": lpw("mse", pw)})
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):
            for k, fn in runs.items():               # interleaved: every repetition times a block of each
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    if fn() != 0:
                        raise RuntimeError(f"{k}: a call failed")
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        med = {k: statistics.median(t) for k, t in times.items()}
        base = med.get("parent_rel_l2", med["rel_l2"])
        out[f"C{C}"] = {"us_median": {k: round(x, 2) for k, x in med.items()},
                        "us_min": {k: round(min(t), 2) for k, t in times.items()},
                        "us_max": {k: round(max(t), 2) for k, t in times.items()},
                        "over_" + ("parent_rel_l2" if parent is not None else "rel_l2"):
                            {k: round(x / base, 3) for k, x in med.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
