"""GNOT(..., pre_norm=True) through forward_packed on the GPU against the float64 pre-norm reference of
tests/prenorm_util.py (the stock-torch port with its attention inputs layer-normalised), under the project's
parity rule (golden_util.RTOL / SLACK with the e32 of the pre-norm reference; no new tolerance): every kernel
family the option touches, an empty sample, the normalised rows themselves, the bf16 mode, and the bitwise
option checks (MoE recompute, accumulated micro-batches, a captured training step, the unchanged default)."""
import numpy as np
import pytest
import torch

import golden_util as GU
import prenorm_util as PU

pytestmark = pytest.mark.gpu

PARITY_CASES = ["d64", "d40", "d30", "d200", "d256", "d320"]
_FX = {}
bits = lambda t: t.view(torch.int32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


def fixture(case):
    """(CPU model, inputs, reference) of a case, computed once and left unchanged"""
    if case not in _FX:
        _FX[case] = PU.fixture(case)
    return _FX[case]


def gpu_model(case, dev, **kw):
    m0, _, _ = fixture(case)
    m = PU.model(case, **kw)
    m.load_state_dict(m0.state_dict(), strict=False)       # (a model without the option has no pre_norm_eps)
    return m.to(dev)


@pytest.mark.parametrize("case", PARITY_CASES)
def test_parity_with_the_pre_norm_reference(dev, case):
    _, data, fx = fixture(case)
    got = PU.run_gpu(gpu_model(case, dev), data, dev)
    ws, wsw, wr, wrw = GU.worst_relative(GU.per_sample_errors(got, fx))
    print(f"{case}: output {GU.rel(got['out'], fx['out']):.2e}, worst per sample {ws:.2e} ({wsw}), per row {wr:.2e} ({wrw})")
    errs = GU.check_parity_per_sample(got, fx)
    assert not errs, errs


def test_empty_sample(dev):
    """Ns = [129, 0, 64]: no rows and exact-zero dtheta / dfns for the empty sample, as without the option"""
    m0 = PU.model("d64")
    data = PU.inputs("d64", Ns=[129, 0, 64], Ms=[17, 5, 3])
    samples, grads, e32 = PU.reference(PU.cfg_of("d64"), PU.params64(m0), *data)
    fx = dict(samples=samples, grads=grads, e32=e32, out=np.concatenate([s["out"] for s in samples]))
    got = PU.run_gpu(m0.to(dev), data, dev)
    assert got["out"].shape[0] == 129 + 64
    assert (got["dtheta"][1] == 0).all()
    for g in got["dfns"]:
        assert (g[17:22] == 0).all()
    errs = GU.check_parity_per_sample(got, fx)
    assert not errs, errs


def _normalised_rows(case):
    """per sample the (raw, normalised) tensors of the float64 and the float32 pre-norm port, in call order"""
    from oracle import torch_port
    m0, (xs, thetas, fns_ps, _), _ = fixture(case)
    res = {}
    for dt in (torch.float64, torch.float32):
        p = {k: torch.tensor(v, dtype=dt) for k, v in PU.params64(m0).items()}
        t = lambda a: torch.tensor(np.asarray(a), dtype=dt)[None]
        per = []
        for b in range(len(xs)):
            seen = []
            with PU.pre_norm_port(seen=seen):
                torch_port.gnot_forward(p, PU.cfg_of(case), t(xs[b]), t(thetas[b]), [t(f) for f in fns_ps[b]])
            per.append(seen)
        res[dt] = per
    return res[torch.float64], res[torch.float32]


def test_debug_buffers_hold_the_normalised_rows(dev):
    """b0.n1 = LN(query0), b1.n2 = LN(b1.query1), fnn0 = LN(fnenc0): real columns against the float64 norm of the
    reference's rows under the per-row parity rule, pad columns (none at d = 64) and nothing else"""
    case = "d64"
    _, data, _ = fixture(case)
    m = gpu_model(case, dev)
    PU.run_gpu(m, data, dev)
    eng = m.engine()
    s64, s32 = _normalised_rows(case)
    # call order per sample (2 input functions, 2 blocks): [q, enc0, enc1, q1] of block 0, then of block 1
    for name, k, rows in (("b0.n1", 0, sum(PU.NS)), ("b1.n2", 7, sum(PU.NS)), ("fnn0", 1, sum(PU.MS))):
        ptr, ld = eng.debug_ptr(name)
        assert ld == 64
        got = eng.debug_tensor(name, rows, ld).double().cpu().numpy()
        ref = np.concatenate([PU.ln64(s[k][0][0].numpy())[0] for s in s64])
        e32 = np.concatenate([np.linalg.norm(a[k][1][0].double().numpy() - b[k][1][0].numpy(), axis=1) for a, b in zip(s32, s64)])
        rown = np.linalg.norm(ref, axis=1)                        # sqrt(d) for every row but a degenerate one
        lim = GU.RTOL * np.maximum(rown, np.sqrt(np.mean(rown ** 2))) + GU.SLACK * e32
        err = np.linalg.norm(got - ref, axis=1)
        assert (err <= lim).all(), (name, float((err / lim).max()))


def test_pad_columns_of_the_normalised_rows_are_zero(dev):
    """d = 40 runs at an internal width of 48: statistics over 40 columns, columns 40 .. 47 exact zeros"""
    case = "d40"
    _, data, _ = fixture(case)
    m = gpu_model(case, dev)
    PU.run_gpu(m, data, dev)
    for name in ("b0.n1", "b0.n2"):
        ptr, ld = m.engine().debug_ptr(name)
        assert ld == 48
        t = m.engine().debug_tensor(name, sum(PU.NS), ld)
        assert bool((t[:, 40:] == 0).all()) and bool(torch.isfinite(t).all())
        assert float(t[:, :40].mean(1).abs().max()) < 1e-5 and float((t[:, :40].var(1, unbiased=False) - 1).abs().max()) < 1e-2


def test_bf16_mode(dev):
    """the bar and the sanity check of tests/test_gpu_bf16.py: output and concatenated gradients within 1e-2 of
    the float64 pre-norm reference, and more than 1e-6 from the fp32 results"""
    case = "d256"
    _, data, fx = fixture(case)
    m = gpu_model(case, dev)
    g32 = PU.run_gpu(m, data, dev)
    m.set_precision("bf16")
    g16 = PU.run_gpu(m, data, dev)
    keys = sorted(fx["grads"])
    cat = lambda g: np.concatenate([np.ravel(g[k]) for k in keys])
    e_out, e_grad = GU.rel(g16["out"], fx["out"]), GU.rel(cat(g16["grads"]), cat(fx["grads"]))
    print(f"bf16 pre-norm d=256: output {e_out:.2e}, gradients {e_grad:.2e}")
    assert e_out < 1e-2 and e_grad < 1e-2, (e_out, e_grad)
    assert GU.rel(g16["out"], g32["out"]) > 1e-6 and GU.rel(cat(g16["grads"]), cat(g32["grads"])) > 1e-6


def _same(a, b):
    return (np.array_equal(a["out"], b["out"]) and all(np.array_equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
            and np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["dtheta"], b["dtheta"])
            and all(np.array_equal(x, y) for x, y in zip(a["dfns"], b["dfns"])))


@pytest.mark.parametrize("case", ["d64", "d256"])
def test_moe_recompute_is_bitwise_equal(dev, case):
    _, data, _ = fixture(case)
    m = gpu_model(case, dev)
    plain = PU.run_gpu(m, data, dev)
    m.set_moe_recompute(True)
    assert _same(PU.run_gpu(m, data, dev), plain)


def _packed(data, idx, dev):
    xs, thetas, fns_ps, Gs = data
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    off = lambda ls: np.concatenate([[0], np.cumsum(ls)]).tolist()
    I = len(fns_ps[0])
    return (t(np.concatenate([xs[b] for b in idx])), off([len(xs[b]) for b in idx]), t(np.stack([thetas[b] for b in idx])),
            [t(np.concatenate([fns_ps[b][i] for b in idx])) for i in range(I)],
            [off([len(fns_ps[b][i]) for b in idx]) for i in range(I)], t(np.concatenate([Gs[b] for b in idx])))


@pytest.mark.parametrize("case", ["d64", "d256"])
def test_accumulated_micro_batches_are_the_float32_sum(dev, case):
    """two micro-batches through set_grad_arena + backward_options(accumulate=True) leave the element-wise
    float32 sum of the two separate backwards in the arena"""
    _, data, _ = fixture(case)
    m = gpu_model(case, dev)
    m.engine().param_grads = False
    arena = torch.zeros(m.grad_numel(), dtype=torch.float32, device=dev)
    m.set_grad_arena(arena)

    def step(idx, accumulate):
        x, off, theta, fns, fo, G = _packed(data, idx, dev)
        out = m.forward_packed(x, off, theta, fns, fo)
        with m.backward_options(accumulate=accumulate):
            (out * G).sum().backward()
        torch.cuda.synchronize()

    step([0, 2], False)
    gA = arena.clone()
    step([1], False)
    gB = arena.clone()
    assert torch.isfinite(gA).all() and torch.isfinite(gB).all() and not torch.equal(gA, gB)
    step([0, 2], False)
    step([1], True)
    assert torch.equal(bits(arena), bits(gA + gB))


@pytest.mark.parametrize("case", ["d64", "d256"])
def test_captured_training_step_replays_the_eager_step(dev, case):
    """forward + RelL2 + backward + FlatAdamW.launch captured in one hipGraph: its replay leaves the parameters
    of the eager step, bit for bit"""
    from gnot_amd import train
    _, data, _ = fixture(case)
    x, off, theta, fns, fo, y = _packed(data, [0, 1, 2], dev)
    loss_fn = train.RelL2Loss()
    models, opts = [], []
    for _ in range(2):
        m = gpu_model(case, dev)
        opts.append(train.FlatAdamW(train.flatten_parameters(m), lr=1e-3))
        m.engine().param_grads = False
        models.append(m)

    def fwd_bwd_opt(m, opt):
        out = m.forward_packed(x, off, theta, fns, fo)
        loss_fn(off, out, y).backward()
        opt.launch(m.engine().grad_flat)

    for m, opt in zip(models, opts):                 # one eager step each: plans bound, workspaces allocated
        opt.prepare()
        fwd_bwd_opt(m, opt)
    torch.cuda.synchronize()
    assert torch.equal(bits(opts[0].flat), bits(opts[1].flat))
    opts[0].prepare()
    fwd_bwd_opt(models[0], opts[0])                  # the second step, eager ...
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd_bwd_opt(models[1], opts[1])
    opts[1].prepare()
    graph.replay()                                   # ... and as a replay
    torch.cuda.synchronize()
    assert torch.isfinite(opts[0].flat).all()
    assert torch.equal(bits(opts[0].flat), bits(opts[1].flat))


def test_default_is_unchanged(dev):
    """pre_norm=False and no keyword at all: identical bits, and another function than pre_norm=True"""
    _, data, _ = fixture("d64")
    off = PU.run_gpu(gpu_model("d64", dev, pre_norm=False), data, dev)
    from gnot_amd import GNOT
    m = GNOT(*GU.model_args(PU.cfg_of("d64")))
    m.load_state_dict(gpu_model("d64", dev, pre_norm=False).state_dict())
    assert _same(PU.run_gpu(m.to(dev), data, dev), off)
    on = PU.run_gpu(gpu_model("d64", dev), data, dev)
    assert GU.rel(on["out"], off["out"]) > 1e-3
