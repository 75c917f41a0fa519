#!/usr/bin/env python3
"""Bitwise A/B of two builds of libgnot_hip.so on the same inputs (a refactor must not change one bit).

    GNOT_LIB=<a.so> python scripts/diag_bitwise_ab.py dump gpurun_out/a.npz
    GNOT_LIB=<b.so> python scripts/diag_bitwise_ab.py dump gpurun_out/b.npz
    python scripts/diag_bitwise_ab.py compare gpurun_out/a.npz gpurun_out/b.npz
    GNOT_LIB=<a.so> python scripts/diag_bitwise_ab.py record tests/golden/train_step_bits.npz
    GNOT_LIB=<a.so> python scripts/diag_bitwise_ab.py record-family tests/golden/train_family_bits.npz
    GNOT_LIB=<a.so> python scripts/diag_bitwise_ab.py record-attn tests/golden/attn_call_bits.npz
    GNOT_LIB=<a.so> python scripts/diag_bitwise_ab.py time-eager [case]

Each case runs one training forward + backward (sum(out * G)) and stores the output and the flat gradient
arena: d = 256 / E = 8 (configs[2]'s widths) in fp32, bf16 mode and with MoE recompute, d = 128 / E = 4 /
two input functions (configs[1]'s) in fp32 and bf16 mode, d = 64 (chain.hip; once more with x.requires_grad_(),
storing x.grad), and five widths of tests/test_gpu_widths.py (WIDTH_CASES).  Every case also stores the packed
weight images and biases as they lie in the workspace (layout and content).  Then the shapes of an attention call
(tests/attn_call_util.py CASES, "attn.*"): with and without input functions, plain, with pre-norm, with dropout, with
input gradients, with the encoders and block 0 frozen, three blocks at an internal width of 640, padded heads and
d = 256, all on a packed batch with empty samples; `record-attn` writes those but the widest as the fixture of
tests/test_gpu_attn_call_bits.py.  Then the training step
(tests/train_step_util.py step_replay): every AdamW entry, both norm entries and both losses at n = 1, 257, 8195
and 524291, and the loss family and the slice-table update (loss_replay): RelL2Loss, MSELoss and every LpLoss kind,
raw and with a normalizer, with and without component weights, and gnot_adamw_step_groups behind the slice-table
norm entries.  `record` writes the inputs and results of the first three sizes, `record-family` those of
loss_replay, as the two fixtures of tests/test_gpu_train_bits.py; a fixture is recorded from the build BEFORE a
change, which then has to reproduce it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnot-replication_amd"), os.path.join(ROOT, "tests")]

CASES = [
    # name, (input, theta, fn, out, L, d, nl, E, H, I), P, precision, recompute
    ("d256_fp32", (3, 1, 3, 1, 2, 256, 4, 8, 8, 1), 20000, "fp32", False),
    ("d256_bf16", (3, 1, 3, 1, 2, 256, 4, 8, 8, 1), 20000, "bf16", False),
    ("d256_recompute", (3, 1, 3, 1, 2, 256, 4, 8, 8, 1), 20000, "fp32", True),
    ("d128_fp32", (2, 1, 3, 1, 2, 128, 4, 4, 8, 2), 10000, "fp32", False),
    ("d128_bf16", (2, 1, 3, 1, 2, 128, 4, 4, 8, 2), 10000, "bf16", False),
    ("d64_fp32", (2, 1, 3, 2, 2, 64, 3, 3, 4, 1), 3000, "fp32", False),
    ("d64_xgrad", (2, 1, 3, 2, 2, 64, 3, 3, 4, 1), 3000, "fp32", False),   # x.requires_grad_(): x.grad is stored too
]
# tests/test_gpu_widths.py CASES at that file's point counts: the narrowest width, no input functions, padded
# heads, chainw.hip and the K-split tables
WIDTH_CASES = ["d16_h4", "d80_h5", "d100_h4", "d320_h10", "d576_h9"]
WIDTH_POINTS, WIDTH_FN_POINTS = [300, 173], [[120, 77], [64, 31]]


def _offsets(counts):
    return [0] + [sum(counts[: k + 1]) for k in range(len(counts))]


def _cases():
    """name, model arguments, x offsets, offsets per input function, precision, recompute"""
    for name, args, P, prec, rec in CASES:
        yield name, args, [0, P // 3, P], [[0, 200, 500]] * args[-1], prec, rec
    from test_gpu_widths import CASES as W
    for name in WIDTH_CASES:
        c = W[name]
        args = (c["input_dim"], c["theta_dim"], c["input_func_dim"], c["out_dim"], c["n_attn_layers"], c["d"],
                c["n_mlp_num_layers"], c["n_expert"], c["n_head"], c["n_input_functions"])
        yield name, args, _offsets(WIDTH_POINTS), [_offsets(m) for m in WIDTH_FN_POINTS[: args[-1]]], "fp32", False


def dump(path):
    import torch
    from gnot_amd import GNOT
    dev = torch.device("cuda")
    res = {}
    for name, (i, t, f, o, L, d, nl, E, H, I), x_off, fn_offs, prec, rec in _cases():
        torch.manual_seed(5)
        m = GNOT(i, t, f, o, L, d, nl, d, d, E, H, I).to(dev)
        m.set_precision(prec)
        m.set_moe_recompute(rec)
        g = torch.Generator(device="cpu").manual_seed(6)
        P = x_off[-1]
        x = torch.rand(P, i, generator=g).to(dev)
        if name.endswith("_xgrad"):
            x.requires_grad_()
        th = torch.rand(len(x_off) - 1, t, generator=g).to(dev)
        fns = [torch.rand(fo[-1], f, generator=g).to(dev) for fo in fn_offs]
        G = torch.randn(P, o, generator=g).to(dev)
        out = m.forward_packed(x, x_off, th, fns, fn_offs)
        (out * G).sum().backward()
        torch.cuda.synchronize()
        res[name + ".out"] = out.detach().cpu().numpy()
        res[name + ".grad"] = m.engine().grad_flat.detach().cpu().numpy()
        if x.grad is not None:
            res[name + ".xgrad"] = x.grad.cpu().numpy()
        # the packed weight images and biases: the workspace from buffer "packed" up to "grads"
        eng = m.engine()
        lo, hi = (eng.debug_ptr(n)[0] - eng.ws.data_ptr() for n in ("packed", "grads"))
        res[name + ".packed"] = eng.ws[lo:hi].view(torch.float32).cpu().numpy()
        print(name, "done", flush=True)
    import attn_call_util as A
    for name in A.CASES:
        for k, v in A.run(name, dev).items():
            res[f"attn.{name}.{k}"] = np.asarray(v)
        print("attn." + name, "done", flush=True)
    import train_step_util as U
    res.update({"step." + k: v for k, v in U.step_replay(U.step_inputs(U.NS)).items()})
    res.update({"family." + k: v for k, v in U.loss_replay(U.loss_inputs()).items()})
    np.savez(path, **res)


def time_eager(name="d128_fp32", steps=30, warmup=5):
    """ms per eager training step (forward + backward, no graph) of one dump case, by a host clock around a device
    synchronise: the figure that host-side planning and launch code can move"""
    import time
    import torch
    from gnot_amd import GNOT
    dev = torch.device("cuda")
    (i, t, f, o, L, d, nl, E, H, I), x_off, fn_offs = next((c[1], c[2], c[3]) for c in _cases() if c[0] == name)
    torch.manual_seed(5)
    m = GNOT(i, t, f, o, L, d, nl, d, d, E, H, I).to(dev)
    g = torch.Generator(device="cpu").manual_seed(6)
    x = torch.rand(x_off[-1], i, generator=g).to(dev)
    th = torch.rand(len(x_off) - 1, t, generator=g).to(dev)
    fns = [torch.rand(fo[-1], f, generator=g).to(dev) for fo in fn_offs]
    G = torch.randn(x_off[-1], o, generator=g).to(dev)
    for k in range(warmup + steps):
        if k == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        m.zero_grad(set_to_none=True)
        (m.forward_packed(x, x_off, th, fns, fn_offs) * G).sum().backward()
    torch.cuda.synchronize()
    print(f"{name} eager ms/step {(time.perf_counter() - t0) * 1e3 / steps:.4f}")


def record(path):
    import train_step_util as U
    inp = U.step_inputs(U.NS[:3])
    out = U.step_replay(inp)
    np.savez(path, **{"in." + k: v for k, v in inp.items()}, **{"out." + k: v for k, v in out.items()})


def record_family(path):
    import train_step_util as U
    inp = U.loss_inputs()
    out = U.loss_replay(inp)
    np.savez_compressed(path, **{"in." + k: v for k, v in inp.items()}, **{"out." + k: v for k, v in out.items()})
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{path}: {size} bytes, more than a committed file may have"
    print(f"{path}: {len(inp)} inputs, {len(out)} results, {size} bytes")


def record_attn(path):
    import torch
    import attn_call_util as A
    res = {}
    for name in A.FIXTURE_CASES:
        r = A.run(name, torch.device("cuda"))
        assert r["out"].shape == (A.ROWS, A.OUT)
        for k, v in r.items():           # the output in full, every gradient as its SHA-256
            res[f"{name}.{k}"] = np.asarray(A.digest(v) if k == "grad" or k.startswith("d") else v)
        print(name, r["forms"], r["plan"].tolist(), flush=True)
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{path}: {size} bytes, more than a committed file may have"
    print(f"{path}: {len(A.FIXTURE_CASES)} cases, {len(res)} entries, {size} bytes")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    assert sorted(A.files) == sorted(B.files)
    for k in A.files:
        same = A[k].tobytes() == B[k].tobytes()      # bits: a NaN equals itself
        if not same or not k.startswith(("step.", "family.")):
            print(f"{k:24s} {'bitwise equal' if same else 'DIFFERS in %d elements' % (A[k] != B[k]).sum()}")
        bad += not same
    print(f"{len(A.files)} arrays, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    modes = {"dump": dump, "record": record, "record-family": record_family, "record-attn": record_attn}
    if sys.argv[1] == "time-eager":
        time_eager(*sys.argv[2:3])
    elif sys.argv[1] in modes:
        modes[sys.argv[1]](sys.argv[2])
    else:
        compare(sys.argv[2], sys.argv[3])
