"""The cases of the attention-call fixture (tests/golden/attn_call_bits.npz, tests/test_gpu_attn_call_bits.py) and of
the attention part of scripts/diag_bitwise_ab.py: one training forward + backward (sum(out * G)) per case on the
packed batch NS / MS -- empty samples, a one-point sample and a sample that ends on a 64-point segment edge, the
same points for every input function.

Weights and inputs come from numpy.random.RandomState(SEED + the case's index), a frozen stream, not from torch's
initialiser: weights N(0, 1) / sqrt(fan-in) and biases U(-1, 1) / sqrt(fan-in) in canonical Linear order, then x,
theta, the input functions (all U(0, 1)) and the output gradient G (N(0, 1)), all float32."""
import hashlib

import numpy as np

NS = [65, 0, 1, 0, 128]
MS = [17, 5, 1, 0, 64]
ROWS = sum(NS)
SEED = 20240
P_DROP, DROP_SEED, DROP_STEP = 0.25, 1234, 7
IN, THETA, FN, OUT = 2, 1, 3, 2

# name -> d, heads, blocks, input functions, MLP layers, experts, option ("" | prenorm | drop | igrad | frozen)
CASES = {}
for _i in (2, 0):
    for _opt in ("", "prenorm", "drop", "igrad"):
        CASES[f"d32_i{_i}" + ("_" + _opt if _opt else "")] = (32, 4, 2, _i, 2, 2, _opt)
CASES["d32_i2_frozen"] = (32, 4, 2, 2, 2, 2, "frozen")
CASES["d640_l3"] = (640, 10, 3, 2, 1, 2, "")          # d(fn) jobs in one launch of K-halves
CASES["d30_h2_i1"] = (30, 2, 2, 1, 2, 2, "")          # padded heads
CASES["d256_h8_l1_i1"] = (256, 8, 1, 1, 2, 2, "")
# the committed fixture: every case but the wide one (its gradients alone would fill the file's budget)
FIXTURE_CASES = [n for n in CASES if n != "d640_l3"]


def offsets(counts):
    return [0] + [int(v) for v in np.cumsum(counts)]


def generate(name):
    """(weights [(W, b)] in canonical order, x, theta, fns, G, sha256 hex of all of them) of a case"""
    d, H, L, I, nl, E, _ = CASES[name]
    rs = np.random.RandomState(SEED + list(CASES).index(name))
    NLin = max(nl, 1) + 1
    mlp = lambda i, o: [(o if j == NLin - 1 else d, i if j == 0 else d) for j in range(NLin)]   # (out, in)
    shapes = mlp(IN + THETA, d) + mlp(IN, E)
    for _ in range(I):
        shapes += mlp(FN, d)
    for _ in range(L):
        shapes += [(d, d)] * (2 + 2 * max(I, 1) + 4)
        for _ in range(2 * E):
            shapes += mlp(d, d)
    shapes += mlp(d, OUT)
    f32 = np.float32
    weights = [((rs.standard_normal((o, i)) / np.sqrt(i)).astype(f32), (rs.uniform(-1, 1, o) / np.sqrt(i)).astype(f32))
               for o, i in shapes]
    x = rs.rand(ROWS, IN).astype(f32)
    theta = rs.rand(len(NS), THETA).astype(f32)
    fns = [rs.rand(sum(MS), FN).astype(f32) for _ in range(I)]
    G = rs.standard_normal((ROWS, OUT)).astype(f32)
    h = hashlib.sha256()
    for a in [t for wb in weights for t in wb] + [x, theta] + fns + [G]:
        h.update(np.ascontiguousarray(a).tobytes())
    return weights, x, theta, fns, G, h.hexdigest()


def build(name, dev):
    """(model, x, theta, fns, G as tensors on `dev`, the inputs' sha256) of a case, its options applied"""
    import torch
    from gnot_amd import GNOT
    d, H, L, I, nl, E, opt = CASES[name]
    weights, x, theta, fns, G, sha = generate(name)
    kw = {}
    if opt == "prenorm":
        kw["pre_norm"] = True
    if opt == "drop":
        kw.update(attn_dropout=P_DROP, dropout_seed=DROP_SEED)
    m = GNOT(IN, THETA, FN, OUT, L, d, nl, d, d, E, H, I, **kw)
    lins = m.linears()
    assert [tuple(l.weight.shape) for l in lins] == [w.shape for w, _ in weights], "the generator's Linear order"
    with torch.no_grad():
        for l, (w, b) in zip(lins, weights):
            l.weight.copy_(torch.from_numpy(w))
            l.bias.copy_(torch.from_numpy(b))
    m = m.to(dev).train()
    if opt == "frozen":                      # the encoders and all of block 0
        for mod in [m.x, m.gating, *m.input_func_mlps, m.blocks[0]]:
            for p in mod.parameters():
                p.requires_grad_(False)
    if opt == "drop":
        m.set_dropout_step(DROP_STEP)
    tx, tt = torch.from_numpy(x).to(dev), torch.from_numpy(theta).to(dev)
    tf = [torch.from_numpy(f).to(dev) for f in fns]
    if opt == "igrad":
        for t in [tx, tt] + tf:
            t.requires_grad_()
    return m, tx, tt, tf, torch.from_numpy(G).to(dev), sha


def run(name, dev):
    """One training step of a case on `dev`: {"in_sha", "out", "grad" (the gradients of the trainable parameters in
    named_parameters() order, flat), "dx" / "dtheta" / "dfn{i}" (the igrad cases), "forms" (the
    gnot_debug_kernel_forms text, keys sorted), "plan" (gnot_debug_backward_plan's pair)}"""
    import torch
    I, opt = CASES[name][3], CASES[name][6]
    m, tx, tt, tf, G, sha = build(name, dev)
    out = m.forward_packed(tx, offsets(NS), tt, tf, [offsets(MS)] * I)
    (out * G).sum().backward()
    torch.cuda.synchronize()
    eng = m.engine()
    res = {"in_sha": sha, "out": out.detach().cpu().numpy(),
           "grad": torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.grad is not None]).cpu().numpy(),
           "forms": " ".join(f"{k}={v}" for k, v in sorted(eng.kernel_forms().items())),
           "plan": np.array(eng.backward_plan(), dtype=np.int64)}
    if opt == "igrad":
        res["dx"], res["dtheta"] = tx.grad.cpu().numpy(), tt.grad.cpu().numpy()
        for i, f in enumerate(tf):
            res[f"dfn{i}"] = f.grad.cpu().numpy()
    return res


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
