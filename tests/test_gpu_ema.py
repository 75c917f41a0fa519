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
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gnot_amd import _lib, train

pytestmark = pytest.mark.gpu

SMALL = (2, 1, 3, 1, 1, 32, 2, 32, 32, 2, 4, 1)      # the model of test_gpu_train_state.py
NS = [1, 257, 8195, 524291]
PAD = -7.0                                            # around every array's declared size
BAD = [float("nan"), float("inf"), float("-inf")]
WEIGHTS = [1 - 0.999, 9 / 11, 1.0]

bits = lambda t: t.view(torch.int32)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _based(src, offset=0):
    """src on the device, its base `offset` floats behind a 16-byte boundary, PAD elements all around it:
    (the view of src's size, the allocation)"""
    n = src.numel()
    buf = torch.full((offset + n + 3,), PAD, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n]
    view.copy_(src)
    assert view.data_ptr() % 16 == 4 * offset
    return view, buf


def _intact(view, buf):
    """the PAD elements in front of and behind the view are untouched"""
    k = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:k] == PAD).all()) and bool((buf[k + view.numel():] == PAD).all())


def _hyper(w, h7=1.0, t=3):
    """the 9 floats of gnot_adamw_step_ema; the first 8 are gnot_adamw_step's"""
    return torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 1 - 0.9 ** t, 1 - 0.999 ** t, h7, w], dtype=torch.float32).cuda()


def _grad(n, offset, seed=0):
    g, buf = _based(torch.randn(n, generator=torch.Generator().manual_seed(1000 * seed + n)), offset)
    buf[:offset] = 1e30                  # a stray read wrecks the norm
    buf[offset + n:] = 1e30
    return g


def _norm(g, hyper, max_norm=None):
    """clip [2] (device) of gnot_grad_clip (max_norm given) or gnot_grad_norm"""
    lib, n = _lib.load(), g.numel()
    work = torch.empty(lib.gnot_grad_clip_work_floats(n), dtype=torch.float32, device="cuda")
    clip = torch.zeros(2, dtype=torch.float32, device="cuda")
    if max_norm is None:
        _lib.check(lib.gnot_grad_norm(g.data_ptr(), n, hyper.data_ptr(), work.data_ptr(), clip.data_ptr(), _stream()))
    else:
        _lib.check(lib.gnot_grad_clip(g.data_ptr(), n, hyper.data_ptr(), max_norm, work.data_ptr(), clip.data_ptr(),
                                      _stream()))
    return clip


class _Arrays:
    """param / exp_avg / exp_avg_sq / ema of n elements in the middle of a run, PAD elements around each; the
    ema base is `offset` floats behind a 16-byte boundary"""

    NAMES = ("p", "m", "v", "e")

    def __init__(self, n, offset):
        gen = torch.Generator().manual_seed(n)
        p = torch.randn(n, generator=gen)
        self.n, self.offset = n, offset
        self._set(p, 0.1 * torch.randn(n, generator=gen), 0.01 * torch.rand(n, generator=gen),
                  p + 0.05 * torch.randn(n, generator=gen))

    def _set(self, p, m, v, e):
        (self.p, self.pb), (self.m, self.mb), (self.v, self.vb), (self.e, self.eb) = (
            _based(p), _based(m), _based(v), _based(e, self.offset))

    def copy(self):
        c = _Arrays.__new__(_Arrays)
        c.n, c.offset = self.n, self.offset
        c._set(self.p, self.m, self.v, self.e)
        return c

    def differing(self, other):
        """names of the arrays (allocations, sentinels included) whose bits differ"""
        return [k for k in self.NAMES if not torch.equal(bits(getattr(self, k + "b")), bits(getattr(other, k + "b")))]

    def _check_pads(self):
        for k in self.NAMES:
            assert _intact(getattr(self, k), getattr(self, k + "b")), k

    def step(self, g, hyper, clip=None, guard=None):
        """the existing entry of the kind: plain, clipped or guarded"""
        lib = _lib.load()
        a = (self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, hyper.data_ptr())
        if guard is not None:
            _lib.check(lib.gnot_adamw_step_guarded(*a, clip.data_ptr(), guard.data_ptr(), _stream()))
        elif clip is not None:
            _lib.check(lib.gnot_adamw_step_clipped(*a, clip.data_ptr(), _stream()))
        else:
            _lib.check(lib.gnot_adamw_step(*a, _stream()))
        self._check_pads()

    def ema_update(self, weight):
        _lib.check(_lib.load().gnot_ema_update(self.e.data_ptr(), self.p.data_ptr(), self.n, weight.data_ptr(),
                                               _stream()))
        self._check_pads()

    def step_ema(self, g, hyper, clip=None, guard=None):
        _lib.check(_lib.load().gnot_adamw_step_ema(
            self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.e.data_ptr(), self.n,
            hyper.data_ptr(), None if clip is None else clip.data_ptr(), None if guard is None else guard.data_ptr(),
            _stream()))
        self._check_pads()


def _guard():
    return torch.zeros(3, dtype=torch.int32, device="cuda")      # {skipped, skipped now} and an element behind


# ------------------------------------------------------------------ 1. the stand-alone pass against float64
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_ema_update_against_float64(n, offset):
    start = _Arrays(n, offset)
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
    g, start = _grad(n, offset), _Arrays(n, offset)
    norm = float(g.double().pow(2).sum().sqrt())
    for w in WEIGHTS[:2]:
        hyper = _hyper(w)
        weight = hyper[8:]
        for kind, max_norm in (("plain", None), ("clipped", 0.5 * norm), ("clipped", 2.0 * norm),
                               ("guarded", None), ("guarded", 0.5 * norm)):
            clip = None if kind == "plain" else _norm(g, hyper, max_norm)
            if clip is not None:
                assert math.isfinite(float(clip[0]))
                assert float(clip[1]) < 1.0 if max_norm == 0.5 * norm else float(clip[1]) == 1.0
            ref, got = start.copy(), start.copy()
            ref_guard, got_guard = (_guard(), _guard()) if kind == "guarded" else (None, None)
            ref.step(g, hyper, clip, ref_guard)
            assert ref.differing(start) == ["p", "m", "v"]
            ref.ema_update(weight)
            got.step_ema(g, hyper, clip, got_guard)
            assert got.differing(ref) == [], (n, offset, w, kind, max_norm)
            assert ref.differing(start) == ["p", "m", "v", "e"]
            if kind == "guarded":
                assert got_guard.tolist() == ref_guard.tolist() == [0, 0, 0]


# ------------------------------------------------------------------ 3. a non-finite gradient: nothing but the guard
def _bad_index(n, where):
    """first / last element; "tail": inside the 1 to 3 elements behind the last 16-byte load of an aligned
    base (n % 4 of them); "head": inside the up to 3 elements in front of the first one of a base a float off"""
    return {"first": 0, "last": n - 1, "tail": n - 1 - (n % 4) // 2, "head": min(1, n - 1)}[where]


@pytest.mark.parametrize("where", ["first", "last", "tail", "head"])
@pytest.mark.parametrize("n", NS)
def test_guarded_ema_step_skips_a_nonfinite_gradient(n, where):
    offset = 1 if where == "head" else 0
    g, hyper, start = _grad(n, offset), _hyper(9 / 11), _Arrays(n, offset)
    good = g.clone()
    for k, bad in enumerate(BAD):
        g.copy_(good)
        g[_bad_index(n, where)] = bad
        clip = _norm(g, hyper, None if k % 2 == 0 else 1.0)
        assert not math.isfinite(float(clip[0])), (n, where, bad, float(clip[0]))
        got, guard = start.copy(), _guard()
        got.step_ema(g, hyper, clip, guard)
        assert got.differing(start) == [], (n, where, bad)       # the average in particular
        assert guard.tolist() == [1, 1, 0]
        # a following finite launch equals the unguarded reference and keeps the count
        clip = _norm(good, hyper)
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
class _Stop(Exception):
    pass


_BATCHES = None


def _batches():
    """list-of-batches loaders: four train and two test batches of two meshes of 40 to 120 points"""
    global _BATCHES
    if _BATCHES is None:
        from gnot_amd import data
        rng = np.random.default_rng(3)
        mk_s = lambda k: [data.synthetic_sample(rng, int(rng.integers(40, 120)), fn_points=(int(rng.integers(10, 30)),))
                          for _ in range(k)]
        mk = lambda s: list(torch.utils.data.DataLoader(data.NS2dData(s), batch_size=2, shuffle=False,
                                                        collate_fn=data.collate_packed))
        _BATCHES = mk(mk_s(8)), mk(mk_s(4))
    return _BATCHES


def _model(seed=0):
    from gnot_amd import GNOT
    torch.manual_seed(seed)
    return GNOT(*SMALL).cuda()


def _flat_params(model):
    return torch.cat([t.detach().reshape(-1) for l in model.linears() for t in (l.weight, l.bias)])


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
    model, batch = _model(), _batches()[1][0]
    flat = train.flatten_parameters(model)
    ema = train.WeightEMA(flat, 0.9)
    ema.ema.add_(0.01 * torch.randn(flat.numel(), generator=torch.Generator().manual_seed(9)).cuda())
    flat0, ema0 = flat.clone(), ema.ema.clone()
    flat_ptr = flat.data_ptr()
    fresh = _model(seed=7)
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
        with pytest.raises(_Stop):
            with ema.swapped():
                raise _Stop
        assert torch.equal(bits(flat), bits(flat0)) and torch.equal(bits(ema.ema), bits(ema0))
    assert flat.data_ptr() == flat_ptr and model.linears()[0].weight.data_ptr() == flat_ptr       # in place


# ------------------------------------------------------------------ 6. fit
def test_fit_evaluates_and_checkpoints_the_average(tmp_path):
    tr, te = _batches()
    dev = torch.device("cuda")
    quiet = lambda msg: None
    plain = _model()
    plain_hist = train.fit(plain, tr, te, epochs=2, log=quiet)
    ckpt = os.path.join(tmp_path, "best_model.pth")
    model, lines = _model(), []
    hist = train.fit(model, tr, te, epochs=2, checkpoint=ckpt, ema_decay=0.9, ema_warmup=False, log=lines.append)
    assert [l.split(":")[0] for l in lines] == ["Epoch 0, Loss", "Epoch 0, Test Metric", "Epoch 1, Loss",
                                                "Epoch 1, Test Metric"]
    # the training trajectory is the run's without the option; the metric is not
    assert hist[0] == plain_hist[0]
    assert torch.equal(bits(_flat_params(model)), bits(_flat_params(plain)))
    assert all(a != b for a, b in zip(hist[1], plain_hist[1]))

    # by hand over the public pieces
    ref = _model()
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
    assert torch.equal(bits(flat), bits(_flat_params(model)))
    assert hist[1] == ref_test, (hist[1], ref_test)
    # the checkpoint holds the averaged weights of the best epoch, not the raw ones
    loaded = train.load_checkpoint(_model(seed=3), ckpt)
    assert _same_state_dict(loaded.state_dict(), best_sd)
    assert not _same_state_dict(loaded.state_dict(), model.state_dict())


# ------------------------------------------------------------------ 7. resume
def _first_grad_norm():
    """the gradient norm of the first train batch at the initial weights (sizes max_grad_norm)"""
    model, (tr, _) = _model(), _batches()
    eng = model.engine()
    eng.param_grads = False
    pred, off, y = train._forward_batch(model, tr[0], torch.device("cuda"))
    train.RelL2Loss()(off, pred, y).backward()
    return float(eng.grad_flat.norm())


def test_resumed_fit_continues_the_average_bitwise(tmp_path):
    tr, te = _batches()
    quiet = lambda msg: None
    kw = dict(accum_steps=2, max_grad_norm=0.5 * _first_grad_norm(), ema_decay=0.9)
    p, q = os.path.join(tmp_path, "p.pt"), os.path.join(tmp_path, "q.pt")
    model = _model()
    ref_hist = train.fit(model, tr, te, epochs=4, state_path=p, log=quiet, **kw)
    ref_flat = _flat_params(model).clone()

    lines = []

    def log(msg):
        lines.append(msg)
        if sum("Test Metric" in l for l in lines) == 2:
            raise _Stop

    with pytest.raises(_Stop):
        train.fit(_model(), tr, te, epochs=4, state_path=q, log=log, **kw)
    first = train.load_training_state(q)["next_epoch"]
    assert 1 <= first <= 2                                  # what was on disk when the run died
    model = _model(seed=123)                                # a fresh module with other weights
    lines.clear()
    hist = train.fit(model, tr, te, epochs=4, state_path=q, resume=True, log=lines.append, **kw)
    assert lines[0].startswith(f"Epoch {first}, Loss") and len(lines) == 2 * (4 - first)

    assert hist == ref_hist and len(hist[0]) == 4 and len(hist[1]) == 4
    assert torch.equal(bits(_flat_params(model)), bits(ref_flat))
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
        train.fit(_model(), tr, te, epochs=4, state_path=p, resume=True, log=quiet, **dict(kw, ema_decay=0.99))
    with pytest.raises(ValueError, match="ema_warmup"):
        train.fit(_model(), tr, te, epochs=4, state_path=p, resume=True, log=quiet, ema_warmup=False, **kw)
    dropped = {k: v for k, v in kw.items() if k != "ema_decay"}
    with pytest.raises(ValueError, match="ema_decay"):
        train.fit(_model(), tr, te, epochs=4, state_path=p, resume=True, log=quiet, **dropped)
    r = os.path.join(tmp_path, "r.pt")
    train.fit(_model(), tr, te, epochs=1, state_path=r, log=quiet, **dropped)
    assert train.load_training_state(r).get("ema_args") is None
    with pytest.raises(ValueError, match="ema_decay"):
        train.fit(_model(), tr, te, epochs=1, state_path=r, resume=True, log=quiet, **kw)
