#!/usr/bin/env python3
"""What the Fourier embedding adds to a step: the two passes of csrc/fourier.hip at 262,144 points with
input_dim 3 and x_fourier = 3 (45 embedded columns, staged at a row pitch of 48 floats), each beside a device
copy that moves the same bytes, timed with device events in one process, interleaved, after a warm-up.
The forward reads C and writes ld floats per point ((3 + 48) * 4 = 204 B); the backward of the engine reads the
embedded row and two gradient sources and writes C floats ((3 * 48 + 3) * 4 = 588 B).  One thread per output
element evaluates one sinf or cosf; the backward has no trigonometry.

    python scripts/fourier_cost.py [--points 262144] [--reps 50] [--out FILE]
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

from gnot_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    P, C, n = args.points, 3, 3
    W = 4 * n + 3
    ld = (C * W + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(P, C, device=dev, generator=gen) * 2 - 1
    emb = torch.empty(P, ld, device=dev)
    ga, gb = (torch.randn(P, ld, device=dev, generator=gen) for _ in range(2))
    dx = torch.empty(P, C, device=dev)
    fwd_bytes, bwd_bytes = P * (C + ld) * 4, P * (3 * ld + C) * 4
    # a copy moves its size twice (read + write): half the pass's bytes per side
    cf_src, cb_src = torch.empty(fwd_bytes // 8, device=dev), torch.empty(bwd_bytes // 8, device=dev)
    cf_dst, cb_dst = torch.empty_like(cf_src), torch.empty_like(cb_src)
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: t.data_ptr()
    runs = {
        "embed_fwd": lambda: lib.gnot_fourier_embed(p(x), P, C, n, p(emb), ld, s),
        "copy_fwd_bytes": lambda: cf_dst.copy_(cf_src) is None,
        "embed_bwd": lambda: lib.gnot_fourier_embed_bwd(p(emb), ld, p(ga), ld, p(gb), ld, P, C, n, p(dx), s),
        "copy_bwd_bytes": lambda: cb_dst.copy_(cb_src) is None,
    }
    times = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for k, fn in runs.items():                   # interleaved: every repetition times all of them
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(int(fn()))
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(t) for k, t in times.items()}
    out = {"points": P, "C": C, "order": n, "ld": ld, "reps": args.reps, "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
           "us_median": {k: round(v, 2) for k, v in med.items()},
           "us_min": {k: round(min(t), 2) for k, t in times.items()},
           "us_max": {k: round(max(t), 2) for k, t in times.items()},
           "fwd_over_copy": round(med["embed_fwd"] / med["copy_fwd_bytes"], 2),
           "bwd_over_copy": round(med["embed_bwd"] / med["copy_bwd_bytes"], 2),
           "fwd_GBps": round(fwd_bytes / med["embed_fwd"] * 1e-3, 1),
           "bwd_GBps": round(bwd_bytes / med["embed_bwd"] * 1e-3, 1)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
