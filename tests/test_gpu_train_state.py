"""The non-finite step guard and the resumable training state on the GPU.  Every comparison is bitwise.

C ABI: gnot_grad_norm carries gnot_grad_clip's norm bits; gnot_adamw_step_guarded equals
gnot_adamw_step_clipped (and, behind gnot_grad_norm, the plain gnot_adamw_step) on a finite gradient and
writes nothing but its guard on a NaN / +inf / -inf one, at n = 1 (one thread), 257 (a partial block), 8195
(two norm partials, an unaligned tail) and 524291 (the update's grid-stride wrap past 2048 blocks), with an
aligned gradient base and one a float off.  FlatAdamW(skip_nonfinite=True): one captured graph replayed on
a NaN and on a finite gradient, and its state_dict.  train.fit: a run stopped in its second epoch and resumed
on a fresh module equals the uninterrupted one, and a NaN batch is skipped."""
import math
import os

import pytest
import torch

import train_step_util as U
from gnot_amd import train
from train_step_util import BAD, NS, bits

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ the norm alone
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_grad_norm_carries_the_bits_of_grad_clip(n, offset):
    g = U.grad(n, offset)
    for h7 in (1.0, 0.5):
        hyper = U.hyper(h7)
        got = U.norm(g, hyper).cpu()
        ref64 = abs(h7) * float(g.double().pow(2).sum().sqrt())
        assert abs(float(got[0]) - ref64) <= 1e-5 * ref64
        assert float(got[1]) == 1.0
        for max_norm in (0.5 * ref64, 2.0 * ref64):
            ref = U.norm(g, hyper, max_norm).cpu()
            assert torch.equal(bits(got[:1]), bits(ref[:1])), (n, offset, h7, float(got[0]), float(ref[0]))


# ------------------------------------------------------------------ a finite gradient: the clipped / plain update
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_guarded_step_on_a_finite_gradient_is_the_unguarded_one(n, offset):
    g, hyper, start = U.grad(n, offset), U.hyper(), U.Arrays(n)
    norm = float(g.double().pow(2).sum().sqrt())
    for max_norm, clipping in ((0.5 * norm, True), (2.0 * norm, False), (None, False)):
        clip = U.norm(g, hyper, max_norm)
        assert math.isfinite(float(clip[0])) and (float(clip[1]) < 1.0) == clipping
        if not clipping:
            assert float(clip[1]) == 1.0
        ref, got, guard = start.copy(), start.copy(), U.guard()
        if max_norm is None:
            ref.step(g, hyper)                         # behind gnot_grad_norm: the plain gnot_adamw_step
        else:
            ref.step(g, hyper, clip)
        got.step(g, hyper, clip, guard)
        assert not ref.same(start)
        assert got.same(ref), (n, offset, max_norm)
        assert guard.tolist() == [0, 0, 0]


# ------------------------------------------------------------------ a non-finite gradient: nothing but the guard
@pytest.mark.parametrize("where", ["first", "last", "tail", "head"])
@pytest.mark.parametrize("n", NS)
def test_guarded_step_skips_a_nonfinite_gradient(n, where):
    g, hyper, start = U.grad(n, 1 if where == "head" else 0), U.hyper(), U.Arrays(n)
    good = g.clone()
    for k, bad in enumerate(BAD):
        g.copy_(good)
        g[U.bad_index(n, where)] = bad
        # the norm through either entry: max_norm / (inf + 1e-6) is a coefficient of 0, NaN stays NaN
        clip = U.norm(g, hyper, None if k % 2 == 0 else 1.0)
        assert not math.isfinite(float(clip[0])), (n, where, bad, float(clip[0]))
        got, guard = start.copy(), U.guard()
        got.step(g, hyper, clip, guard)
        assert got.same(start), (n, where, bad)
        assert guard.tolist() == [1, 1, 0]
        # a following finite launch applies the update and keeps the count
        clip = U.norm(good, hyper)
        ref = start.copy()
        ref.step(good, hyper, clip)
        got.step(good, hyper, clip, guard)
        assert got.same(ref) and not got.same(start)
        assert guard.tolist() == [1, 0, 0]


def test_a_finite_gradient_whose_squared_sum_overflows_is_skipped():
    n = 257
    g = torch.full((n,), 3e19, dtype=torch.float32, device="cuda")       # finite, but 257 * 9e38 > fp32 max
    hyper, start = U.hyper(), U.Arrays(n)
    clip = U.norm(g, hyper)
    assert float(clip[0]) == float("inf")
    got, guard = start.copy(), U.guard()
    got.step(g, hyper, clip, guard)
    assert got.same(start) and guard.tolist() == [1, 1, 0]


# ------------------------------------------------------------------ FlatAdamW: capture, state
@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["norm", "clip"])
def test_guarded_launch_replays_with_the_decision_of_each_replay(max_norm):
    """One torch.cuda.graph over launch(): norm stage 1 -> stage 2 -> guarded update, a linear chain.  The
    norm is read from device memory when the graph runs: the replay on a NaN gradient changes nothing, the
    one on a finite gradient is an eager unguarded optimizer's step."""
    n = 70001
    gen = torch.Generator().manual_seed(5)
    flat0 = torch.randn(n, generator=gen).cuda()
    opt_g = train.FlatAdamW(flat0.clone(), max_grad_norm=max_norm, skip_nonfinite=True)
    opt_e = train.FlatAdamW(flat0.clone(), max_grad_norm=max_norm)
    assert opt_e.skipped_steps is None and opt_e.last_skipped is None
    assert opt_g.skipped_steps.dim() == 0 and opt_g.last_skipped.dim() == 0 and opt_g.grad_norm.dim() == 0
    g_static = torch.zeros(n, device="cuda")
    g0 = torch.randn(n, generator=gen).cuda()
    g_static.copy_(g0)
    opt_g.step(g_static)                 # one eager step on both first (loads the kernels)
    opt_e.step(g0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.launch(g_static)
    same = lambda: all(torch.equal(bits(x), bits(y)) for x, y in ((opt_g.flat, opt_e.flat), (opt_g.m, opt_e.m),
                                                                  (opt_g.v, opt_e.v)))
    assert same() and int(opt_g.skipped_steps) == 0
    # replay 1: a NaN in the gradient -- the step number is consumed, nothing else moves
    gk = torch.randn(n, generator=gen).cuda()
    g_static.copy_(gk)
    g_static[n // 2] = float("nan")
    opt_g.prepare()
    graph.replay()
    opt_e.prepare()
    torch.cuda.synchronize()
    assert same()
    assert int(opt_g.skipped_steps) == 1 and int(opt_g.last_skipped) == 1 and math.isnan(float(opt_g.grad_norm))
    # replay 2: finite
    g_static.copy_(gk)
    opt_g.prepare()
    graph.replay()
    before = opt_e.flat.clone()
    opt_e.step(gk)
    torch.cuda.synchronize()
    assert same() and not torch.equal(opt_e.flat, before)
    assert int(opt_g.skipped_steps) == 1 and int(opt_g.last_skipped) == 0
    assert opt_g.t == opt_e.t == 3


def test_flat_adamw_state_round_trips():
    n = 8195
    gen = torch.Generator().manual_seed(2)
    mk = lambda flat: train.FlatAdamW(flat, schedule=train.OneCycle(1e-3, 2, 4), max_grad_norm=1.0, skip_nonfinite=True)
    a = mk(torch.randn(n, generator=gen).cuda())
    grads = [torch.randn(n, generator=gen).cuda() for _ in range(3)]
    grads[1][17] = float("inf")
    for g in grads:
        a.step(g)
        a.schedule.step()
    state = a.state_dict()
    assert state["t"] == 3 and state["skipped"] == 1 and state["numel"] == n
    assert state["exp_avg"].data_ptr() != a.m.data_ptr()                 # copies, not views
    b = mk(a.flat.clone())
    b.load_state_dict(state)
    b.schedule.load_state_dict(a.schedule.state_dict())
    assert int(b.skipped_steps) == 1 and int(b.last_skipped) == 0 and b.t == 3
    g = torch.randn(n, generator=gen).cuda()
    a.step(g)
    b.step(g)
    for x, y in ((a.flat, b.flat), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(bits(x), bits(y))
    with pytest.raises(ValueError, match="numel"):
        mk(torch.zeros(n + 1, device="cuda")).load_state_dict(state)


# ------------------------------------------------------------------ fit
def _uninterrupted(path, **kw):
    model, (tr, te) = U.model(), U.batches()
    hist = train.fit(model, tr, te, epochs=4, state_path=path, log=lambda msg: None, **kw)
    return hist, U.flat_params(model).clone()


@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """fit(epochs=4, state_path=p), uninterrupted: (p, histories, final flat parameters)"""
    path = os.path.join(tmp_path_factory.mktemp("state"), "p.pt")
    return (path,) + _uninterrupted(path)


def _stopped_and_resumed(path, **kw):
    tr, te = U.batches()
    lines = []

    def log(msg):
        lines.append(msg)
        if sum("Test Metric" in l for l in lines) == 2:
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(U.model(), tr, te, epochs=4, state_path=path, log=log, **kw)
    first = train.load_training_state(path)["next_epoch"]
    assert 1 <= first <= 2                                  # what was on disk when the run died
    model = U.model(seed=123)                                # a fresh module with other weights
    lines.clear()
    hist = train.fit(model, tr, te, epochs=4, state_path=path, resume=True, log=lines.append, **kw)
    assert lines[0].startswith(f"Epoch {first}, Loss") and len(lines) == 2 * (4 - first)
    return hist, U.flat_params(model).clone()


def _assert_same_run(p, q, ref, got):
    (ref_hist, ref_flat), (got_hist, got_flat) = ref, got
    assert got_hist == ref_hist and len(got_hist[0]) == 4 and len(got_hist[1]) == 4
    assert torch.equal(bits(got_flat), bits(ref_flat))
    a, b = train.load_training_state(p), train.load_training_state(q)
    assert a["next_epoch"] == b["next_epoch"] == 4 and a["optimizer"]["t"] == b["optimizer"]["t"]
    for k in ("exp_avg", "exp_avg_sq"):
        assert float(a["optimizer"][k].abs().max()) > 0
        assert torch.equal(bits(a["optimizer"][k]), bits(b["optimizer"][k])), k
    assert list(a["model"].keys()) == list(b["model"].keys())
    for k in a["model"]:
        assert torch.equal(bits(a["model"][k]), bits(b["model"][k])), k
    assert a["schedule"] == b["schedule"] and a["hist_test"] == b["hist_test"] and a["best"] == b["best"]


def test_resumed_fit_is_the_uninterrupted_fit_bitwise(finished, tmp_path):
    p, ref_hist, ref_flat = finished
    q = os.path.join(tmp_path, "q.pt")
    _assert_same_run(p, q, (ref_hist, ref_flat), _stopped_and_resumed(q))


def test_resumed_fit_with_accumulation_and_clipping_bitwise(tmp_path):
    kw = dict(accum_steps=2, max_grad_norm=0.5 * U.first_grad_norm())
    p, q = os.path.join(tmp_path, "p.pt"), os.path.join(tmp_path, "q.pt")
    _assert_same_run(p, q, _uninterrupted(p, **kw), _stopped_and_resumed(q, **kw))


def test_resume_without_a_file_starts_from_scratch(finished, tmp_path):
    _, ref_hist, ref_flat = finished
    model, (tr, te) = U.model(), U.batches()
    q = os.path.join(tmp_path, "none_yet.pt")
    hist = train.fit(model, tr, te, epochs=4, state_path=q, resume=True, log=lambda msg: None)
    assert hist == ref_hist and torch.equal(bits(U.flat_params(model)), bits(ref_flat))
    # ... and a finished run resumes to nothing left to do: the stored histories, the stored weights
    again = U.model(seed=5)
    assert train.fit(again, tr, te, epochs=4, state_path=q, resume=True, log=lambda msg: None) == ref_hist
    assert torch.equal(bits(U.flat_params(again)), bits(ref_flat))


def test_resume_refuses_another_trajectory(finished):
    p = finished[0]
    tr, te = U.batches()
    with pytest.raises(ValueError, match="epochs"):
        train.fit(U.model(), tr, te, epochs=5, state_path=p, resume=True, log=lambda msg: None)
    with pytest.raises(ValueError, match="accum_steps"):
        train.fit(U.model(), tr, te, epochs=4, accum_steps=2, state_path=p, resume=True, log=lambda msg: None)
    with pytest.raises(ValueError, match="state_path"):
        train.fit(U.model(), tr, te, epochs=4, resume=True, log=lambda msg: None)


def test_fit_skips_a_nan_batch():
    tr = [dict(b) for b in U.batches()[0][:3]]
    tr[1]["y"] = tr[1]["y"].clone()
    tr[1]["y"][5] = float("nan")
    dev = torch.device("cuda")

    # by hand over the public pieces: a step for batches 1 and 3, the step number alone for batch 2
    ref = U.model()
    flat = train.flatten_parameters(ref)
    sched = train.OneCycle(1e-3, 1, 3)
    opt = train.FlatAdamW(flat, lr=1e-3, schedule=sched)
    eng = ref.engine()
    eng.param_grads = False
    loss_fn, losses = train.RelL2Loss(), []
    for i, batch in enumerate(tr):
        if i == 1:
            opt.prepare()
            continue
        pred, off, y = train._forward_batch(ref, batch, dev)
        loss = loss_fn(off, pred, y)
        loss.backward()
        opt.step(eng.grad_flat)
        losses.append(float(loss))
    torch.cuda.synchronize()
    assert torch.isfinite(flat).all()

    model, lines = U.model(), []
    hist, _ = train.fit(model, tr, None, epochs=1, skip_nonfinite=True, log=lines.append)
    assert torch.equal(bits(U.flat_params(model)), bits(flat))
    assert hist == [sum(losses) / 2] and math.isfinite(hist[0])
    skipped = [l for l in lines if "Skipped steps" in l]
    assert len(skipped) == 1 and "Skipped steps: 1 " in skipped[0], lines

    # the test bites: without the flag the same loader ends with non-finite parameters
    model = U.model()
    train.fit(model, tr, None, epochs=1, log=lambda msg: None)
    assert not torch.isfinite(U.flat_params(model)).all()
