"""Gradient accumulation over micro-batches on the native path (gnot_backward_ex, GNOT.set_grad_arena,
GNOT.backward_options, train.fit(accum_steps=...)).

Meshes of 300 / 77 / 513 / 129 points with one 40-point input function each: the weight-gradient jobs split
at 128 points, so jobs with several split-K partials and jobs with one both occur, and 77 / 129 / 513 are
no multiple of any tile.  What is checked:
  1. a caller-owned arena changes no bit of a plain backward, and nothing is written behind its size;
  2. forward + backward(overwrite), the same forward + backward(accumulate) leaves exactly 2 g (s + s is
     exact in fp32) -- for every weight-gradient kernel class, forked and serial, with MoE recompute, and
     across a re-bind of a padded plan (whose bind clears the workspace: not the arena);
  3. two micro-batches of different geometry, accumulated, against float64 autograd of the whole batch;
  4. train.fit(accum_steps=2) on batches of 2 against a float64 stock-torch loop on batches of 4;
  5. the deferred gradient collective: two ranks, reduce only with the last micro-batch;
  6. the refusals."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from golden_util import RTOL, SLACK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = (2, 1, 3, 1, 1, 32, 2, 32, 32, 2, 4, 1)          # the model of test_train.py: 128-tile weight gradients
D256 = (2, 1, 3, 1, 1, 256, 2, 256, 256, 2, 8, 1)        # the wide kernels: pgemm_x6w (fp32), pgemm_b16 (bf16 mode)
D100 = (2, 1, 3, 1, 1, 100, 2, 100, 100, 2, 4, 1)        # heads of 25 padded to 28: per-head jobs, padded plan
MODELS = {"small": SMALL, "d256": D256, "d100": D100}
NS, M = [300, 77, 513, 129], 40
GUARD = -12345.0


def _tcfg(args):
    return dict(n_mlp_num_layers=args[6], n_expert=args[9], n_head=args[10], n_attn_layers=args[4],
                n_input_functions=args[11])


_SAMPLES = None


def _samples():
    """the four meshes (float64, host), generated once"""
    global _SAMPLES
    if _SAMPLES is None:
        rng = np.random.default_rng(11)
        _SAMPLES = [dict(x=rng.random((n, 2)), theta=rng.random(1), fn=rng.random((M, 3)),
                         y=rng.standard_normal((n, 1)) + 2.0, G=rng.standard_normal((n, 1))) for n in NS]
    return _SAMPLES


def _batch(idx, dev="cuda"):
    """packed fp32 batch of the samples idx: x, x_off, theta, fns, fn_offs, y, G"""
    S = [_samples()[i] for i in idx]
    cat = lambda k: torch.from_numpy(np.concatenate([s[k] for s in S])).float().to(dev)
    off = np.concatenate([[0], np.cumsum([s["x"].shape[0] for s in S])]).tolist()
    theta = torch.from_numpy(np.stack([s["theta"] for s in S])).float().to(dev)
    return cat("x"), off, theta, [cat("fn")], [[M * b for b in range(len(S) + 1)]], cat("y"), cat("G")


def _model(name, prec="fp32", recompute=False, seed=0):
    from gnot_amd import GNOT
    torch.manual_seed(seed)
    m = GNOT(*MODELS[name]).cuda()
    m.set_precision(prec)
    if recompute:
        m.set_moe_recompute(True)
    m.engine().param_grads = False
    return m


def _arena(m):
    """(the tensor given to set_grad_arena, the allocation behind it): one guard float past the declared size"""
    n = m.grad_numel()
    buf = torch.full((n + 1,), GUARD, dtype=torch.float32, device="cuda")
    return buf[:n], buf


def _step(m, idx, accumulate=False):
    """forward + backward of sum(out * G) on the samples idx; returns the output"""
    x, off, theta, fns, fo, _, G = _batch(idx)
    out = m.forward_packed(x, off, theta, fns, fo)
    with m.backward_options(accumulate=accumulate):
        (out * G).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone()


# ------------------------------------------------------------------ 1. the arena alone
@pytest.mark.parametrize("name", ["small", "d100"])
def test_caller_arena_equals_workspace_arena_bitwise(name):
    m = _model(name)
    eng = m.engine()
    out0 = _step(m, [0, 1, 2, 3])
    assert eng.grad_flat.numel() == m.grad_numel()
    g0 = eng.grad_flat.clone()                            # the workspace arena
    arena, buf = _arena(m)
    m.set_grad_arena(arena)
    out1 = _step(m, [0, 1, 2, 3])
    assert eng.grad_flat.data_ptr() == arena.data_ptr() and eng.grad_arena.data_ptr() == arena.data_ptr()
    assert eng.grad_views[0][0].data_ptr() == arena.data_ptr()
    assert torch.equal(out0, out1)
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    assert torch.equal(arena.view(torch.int32), g0.view(torch.int32))
    assert float(buf[-1]) == GUARD
    # .grad through autograd (param_grads) reads the caller's arena too
    eng.param_grads = True
    m.zero_grad(set_to_none=True)
    _step(m, [0, 1, 2, 3])
    got = torch.cat([t.grad.reshape(-1) for l in m.linears() for t in (l.weight, l.bias)])
    assert torch.equal(got, g0)
    # and back to the workspace arena
    eng.param_grads = False
    m.set_grad_arena(None)
    _step(m, [0, 1, 2, 3])
    assert eng.grad_flat.data_ptr() != arena.data_ptr() and torch.equal(eng.grad_flat, g0)


# ------------------------------------------------------------------ 2. doubling
DOUBLING = [(n, p, o, False) for n, p in (("small", "fp32"), ("d256", "fp32"), ("d256", "bf16"), ("d100", "fp32"))
            for o in ("0", "1")] + [("d256", "fp32", None, True)]


@pytest.mark.parametrize("name,prec,overlap,recompute", DOUBLING,
                         ids=[f"{n}-{p}-overlap{o}" + ("-recompute" if r else "") for n, p, o, r in DOUBLING])
def test_accumulate_doubles_bitwise(name, prec, overlap, recompute, monkeypatch):
    """overwrite then accumulate on the same forward leaves exactly 2 g in the arena.  A state job that
    accumulated would change the second forward's output or gradients; a job class without the flag would
    leave g.  Then across geometries A = all four meshes, B = the 77-point mesh alone (one split): the plan
    is re-bound in between -- a padded plan clears its workspace at bind -- and the sum must be gA + gB."""
    if overlap is None:
        monkeypatch.delenv("GNOT_WGRAD_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("GNOT_WGRAD_OVERLAP", overlap)      # read when the plan is created
    m = _model(name, prec, recompute)
    arena, buf = _arena(m)
    m.set_grad_arena(arena)
    bits = lambda t: t.view(torch.int32)
    A, B = [0, 1, 2, 3], [1]
    outA = _step(m, A)
    gA = arena.clone()
    assert torch.isfinite(gA).all() and int((gA != 0).sum()) > gA.numel() // 2
    out2 = _step(m, A, accumulate=True)                       # the same bound plan: no re-bind
    assert torch.equal(bits(outA), bits(out2))
    bad = (bits(arena) != bits(2 * gA)).nonzero().flatten()
    assert bad.numel() == 0, (bad.numel(), bad[:8].tolist(), arena[bad[:8]].tolist(), gA[bad[:8]].tolist())
    out3 = _step(m, A)                                        # ... and overwrite again after accumulating
    assert torch.equal(bits(outA), bits(out3)) and torch.equal(bits(arena), bits(gA))
    _step(m, B)
    gB = arena.clone()
    assert not torch.equal(gA, gB)
    _step(m, A)
    assert torch.equal(bits(arena), bits(gA))
    _step(m, B, accumulate=True)                              # re-planned and re-bound since the overwrite
    bad = (bits(arena) != bits(gA + gB)).nonzero().flatten()
    assert bad.numel() == 0, (bad.numel(), bad[:8].tolist())
    assert float(buf[-1]) == GUARD


# ------------------------------------------------------------------ 3. across geometries, against float64
def _reference(args, state, dtype):
    """torch_port autograd of the 4-sample RelL2 loss (one unpadded B = 1 call per sample, loss.py:14-23) in
    `dtype` on the host: (loss, {name: gradient})"""
    from oracle import torch_port
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in state.items()}
    t = lambda a: torch.from_numpy(a).float().to(dtype)      # the fp32-rounded inputs the GPU sees
    vals = []
    for s in _samples():
        out = torch_port.gnot_forward(p, _tcfg(args), t(s["x"])[None], t(s["theta"])[None], [t(s["fn"])[None]])[0]
        y = t(s["y"])
        vals.append((((out - y) ** 2).sum(0) / (y ** 2).sum(0)).sqrt())
    loss = torch.stack(vals).mean()
    loss.backward()
    return float(loss.detach()), {k: v.grad.double().numpy() for k, v in p.items()}


def _named_grads(m, flat):
    """{state_dict name: gradient} from a flat arena (Engine.grad_layout order = m.linears())"""
    names = {id(q): n for n, q in m.named_parameters()}
    out, o = {}, 0
    for l in m.linears():
        for q in (l.weight, l.bias):
            out[names[id(q)]] = flat[o:o + q.numel()].view(q.shape).double().cpu().numpy()
            o += q.numel()
    return out


def _check_vs_reference(got, ref, e32, bf16, what):
    """The project's bars.  fp32 (golden_util.check_parity, test_gpu_parity.py): all gradients concatenated
    within 1e-4 norm-wise, and every tensor within 1e-4 ||ref|| + 20 e32, e32 being the reference's OWN
    fp32-vs-fp64 error on that tensor (some gradients are pure cancellation at the default init).  bf16 mode
    (test_gpu_bf16.py): all gradients concatenated within 1e-2 norm-wise."""
    keys = sorted(ref)
    cat = lambda g: np.concatenate([g[k].ravel() for k in keys])
    e_all = float(np.linalg.norm(cat(got) - cat(ref)) / np.linalg.norm(cat(ref)))
    print(f"{what}: all-gradient rel err {e_all:.3e}")
    assert e_all <= (1e-2 if bf16 else RTOL), (what, e_all)
    if not bf16:
        for k in keys:
            d = float(np.linalg.norm(got[k] - ref[k]))
            lim = RTOL * float(np.linalg.norm(ref[k])) + SLACK * e32[k]
            assert d <= lim, (what, k, d, lim)


@pytest.mark.parametrize("name,prec,order", [("small", "fp32", "big_first"), ("small", "fp32", "big_second"),
                                             ("d256", "fp32", "big_second"), ("d256", "bf16", "big_second")])
def test_accumulated_micro_batches_match_float64_whole_batch(name, prec, order):
    from gnot_amd import train
    m = _model(name, prec, seed=1)
    eng = m.engine()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss64, ref = _reference(MODELS[name], state, torch.float64)
    _, g32 = _reference(MODELS[name], state, torch.float32)
    e32 = {k: float(np.linalg.norm(g32[k] - ref[k])) for k in ref}
    loss_fn = train.RelL2Loss()
    bf16 = prec == "bf16"

    # the single plan over all four meshes, on the same inputs
    x, off, theta, fns, fo, y, _ = _batch([0, 1, 2, 3])
    loss = loss_fn(off, m.forward_packed(x, off, theta, fns, fo), y)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - loss64) <= (1e-2 if bf16 else 1e-4) * loss64
    _check_vs_reference(_named_grads(m, eng.grad_flat), ref, e32, bf16, "one plan")

    # two micro-batches of two meshes, weights 1/2 each (both have two samples)
    arena, buf = _arena(m)
    m.set_grad_arena(arena)
    mbs = [[2, 3], [0, 1]] if order == "big_first" else [[0, 1], [2, 3]]
    eng.ws = None                                  # the workspace starts at the first micro-batch's size
    sizes, total = [], 0.0
    for i, idx in enumerate(mbs):
        x, off, theta, fns, fo, y, _ = _batch(idx)
        loss = loss_fn(off, m.forward_packed(x, off, theta, fns, fo), y)
        with m.backward_options(accumulate=i > 0):
            (loss * 0.5).backward()
        total += 0.5 * float(loss.detach())
        sizes.append(eng.ws.numel())
    torch.cuda.synchronize()
    if order == "big_second":
        assert sizes[1] > sizes[0]                 # the workspace had to grow under the accumulated sum
    else:
        assert sizes[1] == sizes[0]
    assert abs(total - loss64) <= (1e-2 if bf16 else 1e-4) * loss64
    _check_vs_reference(_named_grads(m, arena), ref, e32, bf16, f"accumulated {order}")
    assert float(buf[-1]) == GUARD


# ------------------------------------------------------------------ 4. fit
def _fit_loaders():
    from gnot_amd import data
    rng = np.random.default_rng(3)
    samples = [data.synthetic_sample(rng, int(rng.integers(40, 120)), fn_points=(int(rng.integers(10, 30)),))
               for _ in range(8)]
    mk = lambda bs: torch.utils.data.DataLoader(data.NS2dData(samples), batch_size=bs, shuffle=False,
                                                collate_fn=data.collate_packed)
    return mk(2), mk(4)


def _rel_l2(out, y, off):
    tot = [(((out[s:e] - y[s:e]) ** 2).sum(0) / (y[s:e] ** 2).sum(0)).sqrt() for s, e in zip(off[:-1], off[1:])]
    return torch.stack(tot).mean()


def _replica64(init, loader, epochs, max_norm):
    """The stock-torch loop of tests/test_gpu_train_loop.py in float64 on the host: torch_port forward (one
    unpadded B = 1 call per sample) + autograd, RelL2, clip_grad_norm_ when max_norm is set, AdamW,
    OneCycleLR stepped per epoch.  max_norm "probe": the first step's gradient norm only."""
    from oracle import torch_port
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in init.items()}
    opt = torch.optim.AdamW(list(p.values()), lr=1e-3, foreach=False)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, steps_per_epoch=len(loader), epochs=epochs)
    hist, norms = [], []
    for _ in range(epochs):
        losses = []
        for b in loader:
            opt.zero_grad()
            outs = []
            fo = b["fn_offs"][0]
            for i in range(len(b["x_off"]) - 1):
                s, e = b["x_off"][i], b["x_off"][i + 1]
                outs.append(torch_port.gnot_forward(p, _tcfg(SMALL), b["x"][s:e][None].double(),
                                                    b["theta"][i:i + 1].double(),
                                                    [b["fns"][0][fo[i]:fo[i + 1]][None].double()])[0])
            loss = _rel_l2(torch.cat(outs), b["y"].double(), b["x_off"])
            loss.backward()
            if max_norm == "probe":
                return float(torch.nn.utils.clip_grad_norm_(list(p.values()), float("inf")))
            if max_norm is not None:
                norms.append(float(torch.nn.utils.clip_grad_norm_(list(p.values()), max_norm)))
            opt.step()
            losses.append(float(loss.detach()))
        sched.step()
        hist.append(np.mean(losses))
    return hist, norms, {k: v.detach().clone() for k, v in p.items()}


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_fit_accum_steps_matches_float64_loop_on_whole_batches(clip):
    from gnot_amd import GNOT, train
    dev = torch.device("cuda")
    loader2, loader4 = _fit_loaders()
    torch.manual_seed(0)
    model = GNOT(*SMALL).to(dev)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    epochs = 2
    max_norm = 0.5 * _replica64(init, loader4, epochs, "probe") if clip else None
    ref_train, norms, ref_final = _replica64(init, loader4, epochs, max_norm)
    if clip:
        assert sum(nm > max_norm for nm in norms) >= 1, (norms, max_norm)      # the clip was active

    got_train, _ = train.fit(model, loader2, None, epochs=epochs, log=lambda msg: None, max_grad_norm=max_norm,
                             accum_steps=2)
    print("train", got_train, ref_train, "norms", norms, "max", max_norm)
    assert len(got_train) == epochs
    assert np.allclose(got_train, ref_train, rtol=1e-4, atol=0), (got_train, ref_train)
    sd = model.state_dict()
    for k in sd:
        r = ref_final[k]
        assert float((sd[k].double().cpu() - r).norm() / r.norm().clamp_min(1e-12)) < 1e-3, k
    # the arena and the options are restored
    assert model._grad_arena is None and model.engine().user_arena is None and model.engine().param_grads
    assert model.engine().bwd_opts == {"accumulate": False, "reduce": True}


def test_fit_accum_steps_one_is_todays_loop_bitwise():
    from gnot_amd import GNOT, train
    dev = torch.device("cuda")
    loader2, _ = _fit_loaders()
    finals, hists = [], []
    for kw in ({}, {"accum_steps": 1}):
        torch.manual_seed(0)
        model = GNOT(*SMALL).to(dev)
        hists.append(train.fit(model, loader2, None, epochs=1, log=lambda msg: None, **kw)[0])
        assert model._grad_arena is None                       # no arena is installed
        finals.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    assert hists[0] == hists[1]
    for k in finals[0]:
        assert torch.equal(finals[0][k].view(torch.int32), finals[1][k].view(torch.int32)), k


# ------------------------------------------------------------------ 5. the deferred collective
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gnot-replication_amd"), os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gnot_amd import parallel as par

        class Counting(par.PointShardComm):
            calls = 0

            def _allreduce(self, user, buf, count, stream):
                self.calls += 1
                return super()._allreduce(user, buf, count, stream)

        m = _model("small", seed=3)                          # the same weights on every rank
        arena, buf = _arena(m)
        m.set_grad_arena(arena)
        mbs = [[0, 1], [2]] if rank == 0 else [[3], [1, 2]]  # this rank's own micro-batches

        def group(counter=None):
            seen = []
            for i, idx in enumerate(mbs):
                x, off, theta, fns, fo, _, G = _batch(idx)
                out = m.forward_packed(x, off, theta, fns, fo)
                with m.backward_options(accumulate=i > 0, reduce=i == len(mbs) - 1):
                    (out * G).sum().backward()
                torch.cuda.synchronize()
                seen.append(counter.calls if counter is not None else 0)
            return seen

        group()                                              # local sums, then ONE flat all-reduce
        ref = arena.cpu()
        dist.all_reduce(ref)
        comm = Counting(stage_via_host=True)
        m.set_grad_allreduce(comm)
        seen = group(comm)                                   # reduce=False, then reduce=True inside the backward
        got = arena.cpu()
        q.put((rank, bool(torch.equal(got.view(torch.int32), ref.view(torch.int32))), seen,
               bool(torch.isfinite(got).all()), float(buf[-1]) == GUARD))
    except Exception as e:
        q.put((rank, False, repr(e), False, False))
        raise
    finally:
        dist.destroy_process_group()


def test_deferred_grad_allreduce_equals_flat_allreduce_of_local_sums():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=200) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    for rank, equal, seen, finite, guard in res:
        assert equal and finite and guard, (rank, seen)
        assert seen[0] == 0 and seen[1] > 0, (rank, seen)    # no gradient collective in the first backward


def test_grad_hook_runs_only_when_reducing():
    m = _model("small")
    arena, _ = _arena(m)
    m.set_grad_arena(arena)
    calls = []
    m.engine().grad_hook = lambda flat: calls.append(flat.data_ptr())
    x, off, theta, fns, fo, _, G = _batch([1])
    for i, red in enumerate((False, True)):
        out = m.forward_packed(x, off, theta, fns, fo)
        with m.backward_options(accumulate=i > 0, reduce=red):
            (out * G).sum().backward()
        assert len(calls) == (1 if red else 0)
    assert calls == [arena.data_ptr()]


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    from gnot_amd import GNOT
    torch.manual_seed(0)
    m = GNOT(*SMALL).cuda()
    n = m.grad_numel()
    x, off, theta, fns, fo, _, G = _batch([1])
    with pytest.raises(RuntimeError, match="set_grad_arena"):          # no arena
        with m.backward_options(accumulate=True):
            pass
    with pytest.raises(ValueError, match="at least"):                  # too small
        m.set_grad_arena(torch.zeros(n - 1, device="cuda"))
    with pytest.raises(ValueError, match="device"):
        m.set_grad_arena(torch.zeros(n))
    m.set_grad_arena(torch.zeros(n, device="cuda"))
    with pytest.raises(RuntimeError, match="param_grads"):             # autograd still owns .grad
        with m.backward_options(accumulate=True):
            pass
    # the engine refuses as well when the options are set behind the context manager's back
    out = m.forward_packed(x, off, theta, fns, fo)
    m._bwd_opts["accumulate"] = True
    try:
        with pytest.raises(RuntimeError, match="param_grads"):
            (out * G).sum().backward()
    finally:
        m._bwd_opts["accumulate"] = False
