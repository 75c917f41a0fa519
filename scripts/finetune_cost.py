#!/usr/bin/env python3
"""What fine-tuning costs at the configs[1] and configs[2] shapes, for the set-ups train.param_groups resolves --

    all           everything trainable, one group (the plain optimizer entries)
    no_decay      everything trainable, the biases in a group without weight decay
    last_block    blocks.<L-1>.* and out.* trainable, the rest frozen
    decoder       out.* trainable, the rest frozen

1. The eager training step (forward + RelL2 + backward + FlatAdamW) of one model whose requires_grad flags are
   switched between the arms, in rounds: every round runs every arm (one untimed step after the switch, which
   re-plans, then `--steps` timed ones), so the arms alternate in one process; medians over all rounds, with
   `forward_loss` (the training forward and the loss alone) beside them.  The expectation: `decoder` approaches
   `forward_loss` plus the decoder's backward, and `no_decay` costs what `all` costs.
2. The optimizer entries alone at the same arena layouts: the slice-table update (gnot_adamw_step_groups) and norm
   (gnot_grad_norm_groups) against the plain entries (gnot_adamw_step, gnot_grad_norm), device events around
   each launch, the arms interleaved; `cover` is one group over every tensor.  The expectation: the covering table
   costs what the plain update costs plus noise, and a frozen tensor costs nothing (it has no slice).

    python scripts/finetune_cost.py [--reps 50] [--rounds 3] [--steps 4]
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


def arms(model):
    """{name: param_groups' answer} of the set-ups above"""
    last = model._cfg["n_attn_layers"] - 1
    names = [n for n, _ in train.arena_layout(model)]
    rest = lambda keep: sorted({n.split(".")[0] + ".*" if not n.startswith("blocks.") else ".".join(n.split(".")[:2]) + ".*"
                                for n in names if not n.startswith(keep)})
    return {"cover": train.param_groups(model),
            "no_decay": train.param_groups(model, no_decay=["*.bias"]),
            "last_block": train.param_groups(model, freeze=rest((f"blocks.{last}.", "out."))),
            "decoder": train.param_groups(model, freeze=rest(("out.",)))}


def measure(cfg, reps, warmup, dev):
    import bench
    model = GNOT(**bench.WORKLOADS[cfg]["model"]).to(dev)
    layout = train.arena_layout(model)
    n = train.flatten_parameters(model).numel()
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    param, grad = (torch.randn(n, device=dev, generator=gen) * s for s in (0.1, 1e-2))
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 1e-3, 1.0], device=dev)
    clip = torch.zeros(2, device=dev)
    work = torch.empty(lib.gnot_grad_clip_work_floats(n), device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: t.data_ptr()
    runs = {"adamw": lambda: lib.gnot_adamw_step(P(param), P(grad), P(m), P(v), n, P(hyper), s),
            "grad_norm": lambda: lib.gnot_grad_norm(P(grad), n, P(hyper), P(work), P(clip), s)}
    info = {}
    for name, groups in arms(model).items():
        opt = train.FlatAdamW(param, groups=groups, layout=layout, skip_nonfinite=True)     # builds the tables
        table = (P(opt._slices), opt._slices_host, opt._slices.shape[0])
        info[name] = {"slices": table[2], "groups": opt._ngroups,
                      "trainable_floats": int(opt._slices[:, 1].sum())}
        runs["adamw_" + name] = (lambda o=opt, t=table: lib.gnot_adamw_step_groups(
            P(param), P(grad), P(m), P(v), None, n, P(hyper), P(o._ghyper), o._ngroups, *t, None, None, s))
        runs["grad_norm_" + name] = (lambda o=opt, t=table: lib.gnot_grad_norm_groups(
            P(grad), n, P(hyper), *t, P(o._clip_work), P(clip), s))
    del model
    times = {k: [] for k in runs}
    for rep in range(warmup + reps):
        for k, fn in runs.items():                   # interleaved: every repetition times all of them
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(fn())
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return {"workload": cfg, "arena_floats": n, "reps": reps, "tables": info,
            "us_median": {k: round(statistics.median(t), 2) for k, t in times.items()},
            "us_min": {k: round(min(t), 2) for k, t in times.items()},
            "us_max": {k: round(max(t), 2) for k, t in times.items()}}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)        # ms


def step_times(cfg, P, rounds, steps, dev):
    """ms of the eager training step per arm (median / min / max over rounds x steps) and of forward + loss alone"""
    import bench
    mc = bench.WORKLOADS[cfg]["model"]
    I = mc["n_input_functions"]
    gen = torch.Generator(device=dev).manual_seed(0)
    xs = torch.rand(P, mc["input_dim"], device=dev, generator=gen)
    theta = torch.rand(1, mc["theta_dim"], device=dev, generator=gen)
    fns = [torch.rand(805, mc["input_func_dim"], device=dev, generator=gen) for _ in range(I)]
    tgt = torch.randn(P, mc["out_dim"], device=dev, generator=gen)
    x_off, fn_offs = [0, P], [[0, 805]] * I
    loss_fn = train.RelL2Loss()
    torch.manual_seed(0)
    m = GNOT(**mc).to(dev)
    layout = train.arena_layout(m)
    flat = train.flatten_parameters(m)
    m.engine().param_grads = False
    sets = arms(m)
    sets["all"] = sets.pop("cover")
    opts, frozen = {}, {}
    for name, groups in sets.items():
        opts[name] = train.FlatAdamW(flat, lr=1e-5) if name == "all" else \
            train.FlatAdamW(flat, lr=1e-5, groups=groups, layout=layout)
        frozen[name] = {n for g in groups if g["frozen"] for n in g["tensors"]}

    def step(opt):
        pred = m.forward_packed(xs, x_off, theta, fns, fn_offs)
        loss_fn(x_off, pred, tgt).backward()
        opt.step(m.engine().grad_flat)

    def forward_loss():
        loss_fn(x_off, m.forward_packed(xs, x_off, theta, fns, fn_offs), tgt)      # the graph is dropped: no backward

    ts = {k: [] for k in list(sets) + ["forward_loss"]}
    plans = {}
    for _ in range(rounds):
        for name in sets:
            for n, p in m.named_parameters():
                p.requires_grad_(n not in frozen[name])
            step(opts[name])                             # untimed: the switch re-plans
            torch.cuda.synchronize()
            plans[name] = m.engine().backward_plan()
            ts[name] += [timed(lambda: step(opts[name])) for _ in range(steps)]
        ts["forward_loss"] += [timed(forward_loss) for _ in range(steps)]
    return {"workload": cfg, "points": P, "rounds": rounds, "steps": steps,
            "backward_plan": {k: list(v) for k, v in plans.items()},
            "ms_median": {k: round(statistics.median(v), 3) for k, v in ts.items()},
            "ms_min": {k: round(min(v), 3) for k, v in ts.items()},
            "ms_max": {k: round(max(v), 3) for k, v in ts.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for cfg, P, steps in (("cfg2", 10000, max(args.steps, 20)), ("cfg3", 262144, args.steps)):   # configs[1], configs[2]
        print(json.dumps(step_times(cfg, P, args.rounds, steps, dev)))
        torch.cuda.empty_cache()
    for cfg in ("cfg2", "cfg3"):
        print(json.dumps(measure(cfg, args.reps, args.warmup, dev)))


if __name__ == "__main__":
    main()
