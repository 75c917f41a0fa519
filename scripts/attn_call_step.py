#!/usr/bin/env python3
"""Eager training steps (forward, backward, FlatAdamW) of one tests/attn_call_util.py case, for a kernel trace:
    rocprofv3 --kernel-trace ... -- python scripts/attn_call_step.py [case, default d32_i2_prenorm] [steps, default 3]
scripts/launch_list.py <trace> step then lists the last step's launches."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnot-replication_amd"), os.path.join(ROOT, "tests")]

import torch

import attn_call_util as A
from gnot_amd.train import FlatAdamW, flatten_parameters

name = sys.argv[1] if len(sys.argv) > 1 else "d32_i2_prenorm"
m, x, theta, fns, G, _ = A.build(name, torch.device("cuda"))
opt = FlatAdamW(flatten_parameters(m), lr=1e-4)
for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 3):
    out = m.forward_packed(x, A.offsets(A.NS), theta, fns, [A.offsets(A.MS)] * len(fns))
    (out * G).sum().backward()
    opt.step(m.engine().grad_flat)
    m.zero_grad(set_to_none=True)
torch.cuda.synchronize()
print(name, "steps done", float(out.abs().sum()))
