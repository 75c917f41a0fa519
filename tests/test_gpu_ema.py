"""The weight EMA on the GPU.  Every comparison is bitwise unless stated.

C ABI: gnot_ema_update against float64; gnot_adamw_step_ema leaves param / exp_avg / exp_avg_sq as the
existing entry of its kind (plain, clipped, guarded) and ema as gnot_ema_update after that entry; behind the
guard a NaN / +inf / -inf gradient writes nothing but the guard, the average included.  Sizes: n = 1 (one
thread), 257 (a partial block), 8195 (two norm partials, an unaligned tail) and 524291 (the update's
grid-stride wrap past 2048 blocks), with the ema and gradient bases on a 16-byte boundary and one float off,
and a sentinel behind (and, for those two, in front of) every array.
FlatAdamW(ema_decay=...): one captured graph replayed on a NaN and on a finite gradient with the weight of each
replay, and its state keys.  WeightEMA.swapped() under a model.  train.fit(ema_decay=...): the training
trajectory of the run without it, the test metric and checkpoint of the averaged weights, and a resumed run."""
import math
import os

import pytest
import torch

import train_step_util as U
from gnot_amd import train
from train_step_util import BAD, NS, PAD, bits

pytestmark = pytest.mark.gpu

WEIGHTS = [1 - 0.999, 9 / 11, 1.0]


# ------------------------------------------------------------------ 1. the stand-alone pass against float64
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_ema_update_against_float64(n, offset):
    start = U.Arrays(n, offset)
    for w in WEIGHTS:
        weight = torch.tensor([w, PAD], dtype=torch.float32).cuda()
        w32 = float(weight[0])                       # the fp32 value the kernel reads
        got = start.copy()
        got.ema_update(weight)
        assert got.differing(start) == ["e"]         # param is only read
        p, e = start.p.double(), start.e.double()
        ref64 = e + w32 * (p - e)
        # two roundings (the difference, the fused multiply-add), each within 2^-24 of operands no larger than
        # |p| + |ema|, and one in hand
        bound = 3 * 2.0 ** -24 * (p.abs() + e.abs())
        err = (got.e.double() - ref64).abs()
        print(f"n={n} offset={offset} w={w32!r}: max err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (n, offset, w, float((err / bound).max()))


# ------------------------------------------------------------------ 2. fused equals unfused
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_fused_step_is_the_existing_step_then_ema_update(n, offset):
    g, start = U.grad(n, offset), U.Arrays(n, offset)
    norm = float(g.double().pow(2).sum().sqrt())
    for w in WEIGHTS[:2]:
        hyper = U.hyper(w=w)
        weight = hyper[8:]
        for kind, max_norm in (("plain", None), ("clipped", 0.5 * norm), ("clipped", 2.0 * norm),
                               ("guarded", None), ("guarded", 0.5 * norm)):
            clip = None if kind == "plain" else U.norm(g, hyper, max_norm)
            if clip is not None:
                assert math.isfinite(float(clip[0]))
                assert float(clip[1]) < 1.0 if max_norm == 0.5 * norm else float(clip[1]) == 1.0
            ref, got = start.copy(), start.copy()
            ref_guard, got_guard = (U.guard(), U.guard()) if kind == "guarded" else (None, None)
            ref.step(g, hyper, clip, ref_guard)
            assert ref.differing(start) == ["p", "m", "v"]
            ref.ema_update(weight)
            got.step_ema(g, hyper, clip, got_guard)
            assert got.differing(ref) == [], (n, offset, w, kind, max_norm)
            assert ref.differing(start) == ["p", "m", "v", "e"]
            if kind == "guarded":
                assert got_guard.tolist() == ref_guard.tolist() == [0, 0, 0]


# ------------------------------------------------------------------ 3. a non-finite gradient: nothing but the guard
@pytest.mark.parametrize("where", ["first", "last", "tail", "head"])
@pytest.mark.parametrize("n", NS)
def test_guarded_ema_step_skips_a_nonfinite_gradient(n, where):
    offset = 1 if where == "head" else 0
    g, hyper, start = U.grad(n, offset), U.hyper(w=9 / 11), U.Arrays(n, offset)
    good = g.clone()
    for k, bad in enumerate(BAD):
        g.copy_(good)
        g[U.bad_index(n, where)] = bad
        clip = U.norm(g, hyper, None if k % 2 == 0 else 1.0)
        assert not math.isfinite(float(clip[0])), (n, where, bad, float(clip[0]))
        got, guard = start.copy(), U.guard()
        got.step_ema(g, hyper, clip, guard)
        assert got.differing(start) == [], (n, where, bad)       # the average in particular
        assert guard.tolist() == [1, 1, 0]
        # a following finite launch equals the unguarded reference and keeps the count
        clip = U.norm(good, hyper)
        ref = start.copy()
        ref.step(good, hyper, clip)
        ref.ema_update(hyper[8:])
        got.step_ema(good, hyper, clip, guard)
        assert got.differing(ref) == [] and got.differing(start) == ["p", "m", "v", "e"]
        assert guard.tolist() == [1, 0, 0]


# ------------------------------------------------------------------ 4. FlatAdamW: capture
@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["norm", "clip"])
def test_ema_launch_replays_with_the_weight_and_decision_of_each_replay(max_norm):
    """One torch.cuda.graph over launch(): norm stage 1 -> stage 2 -> guarded EMA update, a linear chain.  The
    replay on a NaN gradient changes nothing, the average included; the one on a finite gradient is an eager
    optimizer's step without the option and WeightEMA.update by hand.  The weight differs between the two
    replays (warm-up), so it is read from device memory."""
    n = 70001
    gen = torch.Generator().manual_seed(5)
    flat0 = torch.randn(n, generator=gen).cuda()
    opt_g = train.FlatAdamW(flat0.clone(), max_grad_norm=max_norm, skip_nonfinite=True, ema_decay=0.99)
    opt_e = train.FlatAdamW(flat0.clone(), max_grad_norm=max_norm)
    ema_e = train.WeightEMA(opt_e.flat, 0.99)
    assert opt_e.ema is None and opt_g.ema.ema.data_ptr() != opt_g.flat.data_ptr()
    assert torch.equal(bits(opt_g.ema.ema), bits(flat0))
    g_static = torch.zeros(n, device="cuda")
    g0 = torch.randn(n, generator=gen).cuda()
    g_static.copy_(g0)
    opt_g.step(g_static)                 # one eager step on both first (loads the kernels)
    opt_e.step(g0)
    ema_e.update(opt_e.t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.launch(g_static)
    same = lambda: all(torch.equal(bits(x), bits(y)) for x, y in ((opt_g.flat, opt_e.flat), (opt_g.m, opt_e.m),
                                                                  (opt_g.v, opt_e.v), (opt_g.ema.ema, ema_e.ema)))
    assert same() and int(opt_g.skipped_steps) == 0
    assert not torch.equal(opt_g.ema.ema, opt_g.flat) and not torch.equal(opt_g.ema.ema, flat0)
    # replay 1: a NaN in the gradient -- the step number is consumed, nothing else moves
    gk = torch.randn(n, generator=gen).cuda()
    g_static.copy_(gk)
    g_static[n // 2] = float("nan")
    before = opt_g.ema.ema.clone()
    opt_g.prepare()
    graph.replay()
    opt_e.prepare()
    torch.cuda.synchronize()
    w1 = float(opt_g.hyper[8])
    assert same() and torch.equal(bits(opt_g.ema.ema), bits(before))
    assert int(opt_g.skipped_steps) == 1 and int(opt_g.last_skipped) == 1 and math.isnan(float(opt_g.grad_norm))
    # replay 2: finite
    g_static.copy_(gk)
    opt_g.prepare()
    graph.replay()
    opt_e.step(gk)
    ema_e.update(opt_e.t)
    torch.cuda.synchronize()
    w2 = float(opt_g.hyper[8])
    assert same() and not torch.equal(opt_g.ema.ema, before)
    assert int(opt_g.skipped_steps) == 1 and int(opt_g.last_skipped) == 0
    assert opt_g.t == opt_e.t == 3
    assert w1 == ema_e.weight(2) and w2 == ema_e.weight(3) and w1 != w2


# ------------------------------------------------------------------ 8. the option off
def test_flat_adamw_without_the_option_is_unchanged():
    flat = torch.randn(257, generator=torch.Generator().manual_seed(1)).cuda()
    opt = train.FlatAdamW(flat)
    assert opt.ema is None and opt.hyper.numel() == 8 and all(h.numel() == 8 for h in opt._ring)
    assert list(opt.state_dict().keys()) == ["exp_avg", "exp_avg_sq", "t", "skipped", "numel", "lr", "beta1", "beta2",
                                             "eps", "weight_decay", "max_grad_norm", "skip_nonfinite"]
    on = train.FlatAdamW(flat.clone(), ema_decay=0.999, ema_warmup=False)
    assert on.hyper.numel() == 9 and all(h.numel() == 9 for h in on._ring) and on.ema.warmup is False
    state = on.state_dict()
    assert list(state.keys()) == list(opt.state_dict().keys()) + ["ema"]
    assert set(state["ema"]) == {"ema", "decay", "warmup", "numel"}
    # the two kinds of state do not load into each other
    with pytest.raises(ValueError, match="ema_decay"):
        opt.load_state_dict(state)
    with pytest.raises(ValueError, match="ema_decay"):
        on.load_state_dict(opt.state_dict())


# ------------------------------------------------------------------ model-level helpers
def _averaged_state_dict(model, flat, ema):
    """the module's state_dict with every parameter of the flat arena replaced by its slice of `ema`"""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    covered = 0
    for name, p in model.named_parameters():
        o = (p.data_ptr() - flat.data_ptr()) // 4
        assert 0 <= o and o + p.numel() <= flat.numel(), name
        sd[name] = ema[o:o + p.numel()].view(p.shape).clone()
        covered += p.numel()
    assert covered == flat.numel()
    return sd


def _same_state_dict(a, b):
    return list(a.keys()) == list(b.keys()) and all(torch.equal(bits(a[k].cpu()), bits(b[k].cpu())) for k in a)


# ------------------------------------------------------------------ 5. swapped()
def test_swapped_makes_the_average_the_modules_parameters():
    dev = torch.device("cuda")
    model, batch = U.model(), U.batches()[1][0]
    flat = train.flatten_parameters(model)
    ema = train.WeightEMA(flat, 0.9)
    ema.ema.add_(0.01 * torch.randn(flat.numel(), generator=torch.Generator().manual_seed(9)).cuda())
    flat0, ema0 = flat.clone(), ema.ema.clone()
    flat_ptr = flat.data_ptr()
    fresh = U.model(seed=7)
    fresh.load_state_dict(_averaged_state_dict(model, flat, ema.ema))
    with torch.no_grad():
        ref = train._forward_batch(fresh, batch, dev)[0].clone()
        raw = train._forward_batch(model, batch, dev)[0].clone()
        with ema.swapped() as inside:
            assert inside is ema
            assert torch.equal(bits(flat), bits(ema0)) and torch.equal(bits(ema.ema), bits(flat0))
            got = train._forward_batch(model, batch, dev)[0].clone()
        assert torch.equal(bits(got), bits(ref))
        assert not torch.equal(got, raw)
        assert torch.equal(bits(flat), bits(flat0)) and torch.equal(bits(ema.ema), bits(ema0))
        assert torch.equal(bits(train._forward_batch(model, batch, dev)[0]), bits(raw))
        with pytest.raises(U.Stop):
            with ema.swapped():
                raise U.Stop
        assert torch.equal(bits(flat), bits(flat0)) and torch.equal(bits(ema.ema), bits(ema0))
    assert flat.data_ptr() == flat_ptr and model.linears()[0].weight.data_ptr() == flat_ptr       # in place


# ------------------------------------------------------------------ 6. fit
def test_fit_evaluates_and_checkpoints_the_average(tmp_path):
    tr, te = U.batches()
    dev = torch.device("cuda")
    quiet = lambda msg: None
    plain = U.model()
    plain_hist = train.fit(plain, tr, te, epochs=2, log=quiet)
    ckpt = os.path.join(tmp_path, "best_model.pth")
    model, lines = U.model(), []
    hist = train.fit(model, tr, te, epochs=2, checkpoint=ckpt, ema_decay=0.9, ema_warmup=False, log=lines.append)
    assert [l.split(":")[0] for l in lines] == ["Epoch 0, Loss", "Epoch 0, Test Metric", "Epoch 1, Loss",
                                                "Epoch 1, Test Metric"]
    # the training trajectory is the run's without the option; the metric is not
    assert hist[0] == plain_hist[0]
    assert torch.equal(bits(U.flat_params(model)), bits(U.flat_params(plain)))
    assert all(a != b for a, b in zip(hist[1], plain_hist[1]))

    # by hand over the public pieces
    ref = U.model()
    flat = train.flatten_parameters(ref)
    sched = train.OneCycle(1e-3, 2, len(tr))
    opt = train.FlatAdamW(flat, lr=1e-3, schedule=sched)
    ema = train.WeightEMA(flat, 0.9, warmup=False)
    eng = ref.engine()
    eng.param_grads = False
    loss_fn, ref_test, best, best_sd = train.RelL2Loss(), [], float("inf"), None
    for _ in range(2):
        for batch in tr:
            pred, off, y = train._forward_batch(ref, batch, dev)
            loss_fn(off, pred, y).backward()
            opt.step(eng.grad_flat)
            ema.update(opt.t)
        sched.step()
        with ema.swapped():
            ref_test.append(train.evaluate(ref, te, loss_fn))
            if ref_test[-1] < best:
                best, best_sd = ref_test[-1], {k: v.detach().clone() for k, v in ref.state_dict().items()}
    assert torch.equal(bits(flat), bits(U.flat_params(model)))
    assert hist[1] == ref_test, (hist[1], ref_test)
    # the checkpoint holds the averaged weights of the best epoch, not the raw ones
    loaded = train.load_checkpoint(U.model(seed=3), ckpt)
    assert _same_state_dict(loaded.state_dict(), best_sd)
    assert not _same_state_dict(loaded.state_dict(), model.state_dict())


# ------------------------------------------------------------------ 7. resume
def test_resumed_fit_continues_the_average_bitwise(tmp_path):
    tr, te = U.batches()
    quiet = lambda msg: None
    kw = dict(accum_steps=2, max_grad_norm=0.5 * U.first_grad_norm(), ema_decay=0.9)
    p, q = os.path.join(tmp_path, "p.pt"), os.path.join(tmp_path, "q.pt")
    model = U.model()
    ref_hist = train.fit(model, tr, te, epochs=4, state_path=p, log=quiet, **kw)
    ref_flat = U.flat_params(model).clone()

    lines = []

    def log(msg):
        lines.append(msg)
        if sum("Test Metric" in l for l in lines) == 2:
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(U.model(), tr, te, epochs=4, state_path=q, log=log, **kw)
    first = train.load_training_state(q)["next_epoch"]
    assert 1 <= first <= 2                                  # what was on disk when the run died
    model = U.model(seed=123)                                # a fresh module with other weights
    lines.clear()
    hist = train.fit(model, tr, te, epochs=4, state_path=q, resume=True, log=lines.append, **kw)
    assert lines[0].startswith(f"Epoch {first}, Loss") and len(lines) == 2 * (4 - first)

    assert hist == ref_hist and len(hist[0]) == 4 and len(hist[1]) == 4
    assert torch.equal(bits(U.flat_params(model)), bits(ref_flat))
    a, b = train.load_training_state(p), train.load_training_state(q)
    assert a["ema_args"] == b["ema_args"] == {"ema_decay": 0.9, "ema_warmup": True}
    assert "ema_decay" not in a["args"] and set(a["args"]) == set(train.TRAJECTORY_ARGS)
    assert a["next_epoch"] == b["next_epoch"] == 4 and a["optimizer"]["t"] == b["optimizer"]["t"] == 8
    for k in ("exp_avg", "exp_avg_sq"):
        assert float(a["optimizer"][k].abs().max()) > 0
        assert torch.equal(bits(a["optimizer"][k]), bits(b["optimizer"][k])), k
    ea, eb = a["optimizer"]["ema"], b["optimizer"]["ema"]
    assert ea["decay"] == eb["decay"] == 0.9 and ea["warmup"] is True and eb["warmup"] is True
    assert torch.equal(bits(ea["ema"]), bits(eb["ema"]))
    for k in a["model"]:
        assert torch.equal(bits(a["model"][k]), bits(b["model"][k])), k
    assert a["hist_test"] == b["hist_test"] and a["best"] == b["best"]
    # the file keeps the raw weights; the average is another array
    assert _same_state_dict(a["model"], model.state_dict())
    assert ea["ema"].numel() == ref_flat.numel() and not torch.equal(ea["ema"], ref_flat.cpu())

    # another decay, another warm-up, a dropped and an added average are refused by name
    with pytest.raises(ValueError, match="ema_decay"):
        train.fit(U.model(), tr, te, epochs=4, state_path=p, resume=True, log=quiet, **dict(kw, ema_decay=0.99))
    with pytest.raises(ValueError, match="ema_warmup"):
        train.fit(U.model(), tr, te, epochs=4, state_path=p, resume=True, log=quiet, ema_warmup=False, **kw)
    dropped = {k: v for k, v in kw.items() if k != "ema_decay"}
    with pytest.raises(ValueError, match="ema_decay"):
        train.fit(U.model(), tr, te, epochs=4, state_path=p, resume=True, log=quiet, **dropped)
    r = os.path.join(tmp_path, "r.pt")
    train.fit(U.model(), tr, te, epochs=1, state_path=r, log=quiet, **dropped)
    assert train.load_training_state(r).get("ema_args") is None
    with pytest.raises(ValueError, match="ema_decay"):
        train.fit(U.model(), tr, te, epochs=1, state_path=r, resume=True, log=quiet, **kw)
