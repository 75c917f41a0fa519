"""The optional parts of the native training step on the GPU: MSELoss (reference loss.py:4-12) and its
gradient vs float64, the device-side global gradient norm / clip coefficient (gnot_grad_clip) vs float64,
FlatAdamW(max_grad_norm=...) vs torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, its hipGraph capture,
train.fit with MSE and clipping vs a stock-torch replica, and the unclipped default left bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

import train_step_util as U
from gnot_amd import train
from train_step_util import SMALL

pytestmark = pytest.mark.gpu

TCFG = dict(n_mlp_num_layers=2, n_expert=2, n_head=4, n_attn_layers=1, n_input_functions=1)


# ------------------------------------------------------------------ MSELoss
def _mse_formula(pred, tgt, off):
    """loss.py:4-12 with dgl AvgPooling = per-sample mean over points, then the mean."""
    return torch.stack([((pred[s:e] - tgt[s:e]) ** 2).mean(0) for s, e in zip(off[:-1], off[1:])]).mean()


@pytest.mark.parametrize("sizes,C", [([10000], 1), ([37, 1, 5000, 2049], 3), ([4097, 4096], 2)])
def test_native_mse_loss_and_grad(sizes, C):
    rng = np.random.default_rng(0)
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    pred = rng.standard_normal((off[-1], C))
    tgt = rng.standard_normal((off[-1], C))
    dev = torch.device("cuda")
    p64 = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    ref = _mse_formula(p64, torch.tensor(tgt, dtype=torch.float64), off)
    ref.backward()
    ref = float(ref.detach())
    r = p64.grad.numpy()
    loss_fn = train.MSELoss()
    got = []
    for _ in range(2):
        pt = torch.tensor(pred, dtype=torch.float32, device=dev, requires_grad=True)
        loss = loss_fn(off, pt, torch.tensor(tgt, dtype=torch.float32, device=dev))
        loss.backward()
        got.append((loss.detach().cpu(), pt.grad.cpu()))
    loss, g = float(got[0][0]), got[0][1].double().numpy()
    print(f"mse {sizes} C={C}: loss rel err {abs(loss - ref) / ref:.2e}, "
          f"grad rel err {np.linalg.norm(g - r) / np.linalg.norm(r):.2e}")
    assert abs(loss - ref) <= 1e-5 * ref
    assert np.linalg.norm(g - r) <= 1e-5 * np.linalg.norm(r)
    # deterministic: a second call gives the same bits
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ------------------------------------------------------------------ norm and coefficient
def _grad_clip(g, h7, max_norm):
    """gnot_grad_clip on the device tensor g (any view); returns clip [2] on the host (U.norm checks the
    elements behind the declared sizes of work and clip)"""
    return U.norm(g, U.hyper(h7), max_norm).cpu()


def _check_clip(g, h7):
    norm = abs(h7) * float(g.double().pow(2).sum().sqrt())
    for max_norm, clipping in ((2.0 * norm, False), (0.5 * norm, True)):
        c = _grad_clip(g, h7, max_norm)
        coef = min(1.0, max_norm / (norm + 1e-6))
        print(f"n={g.numel()} h7={h7} max={max_norm:.4g}: norm rel err {abs(float(c[0]) - norm) / norm:.2e}, "
              f"coef {float(c[1])!r} vs {coef!r}")
        assert abs(float(c[0]) - norm) <= 1e-5 * norm
        assert abs(float(c[1]) - coef) <= 1e-5 * coef
        assert clipping == (float(c[1]) < 1.0)
        if not clipping:
            assert float(c[1]) == 1.0                      # exactly 1.0f
        assert torch.equal(c, _grad_clip(g, h7, max_norm))  # bitwise on a repeat call


@pytest.mark.parametrize("h7", [1.0, 0.5])
@pytest.mark.parametrize("n", [1, 255, 257, 524291])
def test_grad_norm_and_coefficient(n, h7):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()
    _check_clip(g, h7)


@pytest.mark.parametrize("h7", [1.0, 0.5])
def test_grad_norm_misaligned_base(h7):
    """The same data through a view one element into a larger buffer: a base that is 4- but not 16-byte
    aligned.  The bytes around the view stay as they were."""
    n = 524291
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()
    buf = torch.full((n + 6,), 1e30, dtype=torch.float32, device="cuda")     # a stray read would wreck the norm
    assert buf.data_ptr() % 16 == 0
    buf[1:1 + n].copy_(g)
    before = buf.clone()
    view = buf[1:1 + n]
    assert view.data_ptr() % 16 == 4
    _check_clip(view, h7)
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))


# ------------------------------------------------------------------ clipped AdamW against torch
def test_clipped_flat_adamw_matches_torch_clip_grad_norm():
    from gnot_amd import GNOT
    dev = torch.device("cuda")
    torch.manual_seed(0)
    a = GNOT(*SMALL).to(dev)
    b = GNOT(*SMALL).to(dev)
    b.load_state_dict(a.state_dict())
    flat = train.flatten_parameters(b)
    opt_a = torch.optim.AdamW(a.parameters(), lr=1e-3, foreach=False)
    sch_a = torch.optim.lr_scheduler.OneCycleLR(opt_a, max_lr=1e-3, steps_per_epoch=4, epochs=3)
    opt_b = train.FlatAdamW(flat, lr=1e-3, schedule=train.OneCycle(1e-3, 3, 4), max_grad_norm=1.0)
    lin_names = []
    for l in b.linears():
        for p in (l.weight, l.bias):
            lin_names.append(next(n for n, q in b.named_parameters() if q is p))
    g = torch.Generator(device="cpu").manual_seed(1)
    for step in range(10):
        scale = 1e-3 if step % 2 == 0 else 1.0
        grads = [torch.randn(p.shape, generator=g).to(dev) * scale for p in a.parameters()]
        # the flat gradient in the arena layout, taken before torch scales .grad in place
        gmap = {n: gr for (n, _), gr in zip(a.named_parameters(), grads)}
        gflat = torch.cat([gmap[n].reshape(-1) for n in lin_names])
        for p, gr in zip(a.parameters(), grads):
            p.grad = gr.clone()
        norm = float(torch.nn.utils.clip_grad_norm_(list(a.parameters()), 1.0))
        # both branches with margin: no clip on the small steps, a clip on the large ones
        assert norm < 0.5 if step % 2 == 0 else norm > 2.0, (step, norm)
        opt_a.step()
        sch_a.step()
        keep = gflat.clone()
        opt_b.step(gflat)
        opt_b.schedule.step()
        assert opt_b.grad_norm.dim() == 0
        assert abs(float(opt_b.grad_norm) - norm) <= 1e-5 * norm, (step, float(opt_b.grad_norm), norm)
        assert torch.equal(gflat, keep)               # the gradient buffer itself is left unclipped
    torch.cuda.synchronize()
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        err = (pa - pb).abs().max().item()
        assert err <= 1e-6 * max(1.0, pa.abs().max().item()), (n, err)


# ------------------------------------------------------------------ capture
def test_clipped_launch_replays_with_the_coefficient_of_each_replay():
    """One torch.cuda.graph over launch(): norm stage 1 -> stage 2 -> clipped update, a linear chain.  The
    coefficient is read from device memory when the graph runs, so a replay on a small gradient does not
    clip and one on a large gradient does, each bitwise equal to an eager optimiser."""
    dev = torch.device("cuda")
    n = 70001
    gen = torch.Generator().manual_seed(5)
    flat0 = torch.randn(n, generator=gen).to(dev)
    opt_g = train.FlatAdamW(flat0.clone(), max_grad_norm=1.0)
    opt_e = train.FlatAdamW(flat0.clone(), max_grad_norm=1.0)
    g_static = torch.zeros(n, device=dev)
    g0 = torch.randn(n, generator=gen).to(dev) * 1e-2
    g_static.copy_(g0)
    opt_g.step(g_static)                 # one eager step on both first (loads the kernels)
    opt_e.step(g0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.launch(g_static)
    for scale, clipped in ((1.0, True), (1e-4, False)):
        gk = torch.randn(n, generator=gen).to(dev) * scale
        g_static.copy_(gk)
        opt_g.prepare()
        graph.replay()
        opt_e.step(gk)
        torch.cuda.synchronize()
        assert (float(opt_g.grad_norm) > 1.0) == clipped
        assert torch.equal(opt_g.grad_norm, opt_e.grad_norm)
        for x, y in ((opt_g.flat, opt_e.flat), (opt_g.m, opt_e.m), (opt_g.v, opt_e.v)):
            assert torch.equal(x, y)


# ------------------------------------------------------------------ defaults unchanged
def test_coefficient_one_leaves_the_plain_step_bit_for_bit():
    dev = torch.device("cuda")
    n = 524291
    gen = torch.Generator().manual_seed(9)
    flat0 = torch.randn(n, generator=gen).to(dev)
    plain = train.FlatAdamW(flat0.clone(), schedule=train.OneCycle(1e-3, 3, 4))
    huge = train.FlatAdamW(flat0.clone(), schedule=train.OneCycle(1e-3, 3, 4), max_grad_norm=1e30)
    assert plain.grad_norm is None
    for _ in range(3):
        gr = torch.randn(n, generator=gen).to(dev)
        plain.step(gr)
        huge.step(gr)
        plain.schedule.step()
        huge.schedule.step()
    torch.cuda.synchronize()
    assert float(huge._clip[1]) == 1.0
    for x, y in ((plain.flat, huge.flat), (plain.m, huge.m), (plain.v, huge.v)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------ fit with MSE and clipping
def _replica_out(torch_port, p, b, dev):
    """reference forward of one packed batch: one unpadded B=1 call per sample."""
    outs = []
    for i in range(len(b["x_off"]) - 1):
        s, e = b["x_off"][i], b["x_off"][i + 1]
        fo = b["fn_offs"][0]
        outs.append(torch_port.gnot_forward(p, TCFG, b["x"][s:e][None].to(dev), b["theta"][i:i + 1].to(dev),
                                            [b["fns"][0][fo[i]:fo[i + 1]][None].to(dev)])[0])
    return torch.cat(outs), b["x_off"]


def _rel_l2(out, y, off):
    tot = [(((out[s:e] - y[s:e]) ** 2).sum(0) / (y[s:e] ** 2).sum(0)).sqrt() for s, e in zip(off[:-1], off[1:])]
    return torch.stack(tot).mean()


def _replica(init, train_loader, test_loader, epochs, dev, max_norm):
    """Stock torch: MSE (loss.py:4-12) -> backward -> clip_grad_norm_ -> AdamW, OneCycleLR per epoch, RelL2
    test metric.  max_norm None: one forward/backward only, returning the first step's gradient norm."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import torch_port
    p = {k: v.clone().requires_grad_(True) for k, v in init.items()}
    opt = torch.optim.AdamW(list(p.values()), lr=1e-3, foreach=False)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, steps_per_epoch=len(train_loader), epochs=epochs)
    hist_train, hist_test, norms = [], [], []
    for _ in range(epochs):
        losses = []
        for b in train_loader:
            opt.zero_grad()
            out, off = _replica_out(torch_port, p, b, dev)
            loss = _mse_formula(out, b["y"].to(dev), off)
            loss.backward()
            if max_norm is None:
                return float(torch.nn.utils.clip_grad_norm_(list(p.values()), float("inf")))
            norms.append(float(torch.nn.utils.clip_grad_norm_(list(p.values()), max_norm)))
            opt.step()
            losses.append(float(loss))
        sched.step()
        hist_train.append(np.mean(losses))
        with torch.no_grad():
            vals = []
            for b in test_loader:
                out, off = _replica_out(torch_port, p, b, dev)
                vals.append(float(_rel_l2(out, b["y"].to(dev), off)))
        hist_test.append(np.mean(vals))
    return hist_train, hist_test, norms, {k: v.detach().clone() for k, v in p.items()}


def test_fit_with_mse_and_clipping_matches_torch_reference():
    from gnot_amd import GNOT
    dev = torch.device("cuda")
    train_loader, test_loader = U.batches(6)
    torch.manual_seed(0)
    model = GNOT(*SMALL).to(dev)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    epochs = 2
    max_norm = 0.5 * _replica(init, train_loader, test_loader, epochs, dev, None)
    ref_train, ref_test, norms, ref_final = _replica(init, train_loader, test_loader, epochs, dev, max_norm)
    assert sum(nm > max_norm for nm in norms) >= 1, (norms, max_norm)       # the clip was active

    got_train, got_test = train.fit(model, train_loader, test_loader, epochs=epochs, log=lambda msg: None,
                                    loss_fn=train.MSELoss(), max_grad_norm=max_norm)
    print("train", got_train, ref_train, "test", got_test, ref_test, "norms", norms, "max", max_norm)
    assert np.allclose(got_train, ref_train, rtol=1e-4, atol=0), (got_train, ref_train)
    assert np.allclose(got_test, ref_test, rtol=1e-4, atol=0), (got_test, ref_test)       # RelL2 metric
    sd = model.state_dict()
    assert list(sd.keys()) == list(init.keys())
    for k in sd:
        r = ref_final[k]
        assert float((sd[k] - r).norm() / r.norm().clamp_min(1e-12)) < 1e-3, k
