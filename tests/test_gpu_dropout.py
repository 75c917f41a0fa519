"""GNOT(..., attn_dropout=0.25) through forward_packed on the GPU against the masked float64 reference of
tests/dropout_util.py (the stock-torch port with every attention output multiplied by the numpy mask of its
site), under the project's parity rule (golden_util.RTOL / SLACK with the e32 of the masked port; no new
tolerance): every kernel family downstream of the dropped rows, an empty sample, the dropped rows themselves, the
module flag, the step counter and the pending-backward path, and the bitwise option checks (MoE recompute, input
gradients, accumulated micro-batches, a captured training step, a resumed fit, the unchanged default)."""
import os

import numpy as np
import pytest
import torch

import dropout_util as DU
import golden_util as GU
import prenorm_util as PU

pytestmark = pytest.mark.gpu

bits = lambda t: t.view(torch.int32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


def gpu_model(case, dev, **kw):
    m0, _, _ = DU.fixture(case)
    m = DU.model(case, **kw)
    m.load_state_dict(m0.state_dict())
    return m.to(dev)


def run_at(m, data, dev, step=0):
    m.set_dropout_step(step)
    return PU.run_gpu(m, data, dev)


# d256 twice: forked weight gradients (the default below 65,536 points) and, with GNOT_WGRAD_OVERLAP=0 set before
# the model is built, the serial form with the two direct MoE row streams
@pytest.mark.parametrize("case, serial", [("d64", False), ("d40", False), ("d30", False), ("d256", False),
                                          ("d256", True), ("d320", False)])
def test_parity_with_the_masked_reference(dev, case, serial, monkeypatch):
    if serial:
        monkeypatch.setenv("GNOT_WGRAD_OVERLAP", "0")
    _, data, fx = DU.fixture(case)
    m = gpu_model(case, dev)
    assert m.training
    got = run_at(m, data, dev)
    if case == "d256":
        assert m.engine().kernel_forms()["serial_wgrad"] == ("1" if serial else "0")
    ws, wsw, wr, wrw = GU.worst_relative(GU.per_sample_errors(got, fx))
    print(f"{case}{' serial' if serial else ''}: output {GU.rel(got['out'], fx['out']):.2e}, worst per sample {ws:.2e} "
          f"({wsw}), per row {wr:.2e} ({wrw})")
    errs = GU.check_parity_per_sample(got, fx)
    assert not errs, errs
    assert m.dropout_state()["step"] == 1


def test_empty_sample(dev):
    """Ns = [129, 0, 64]: the sample index of the key counts the empty sample"""
    m0 = DU.model("d64")
    data = PU.inputs("d64", Ns=[129, 0, 64], Ms=[17, 5, 3])
    fx = DU.as_fx(DU.reference(PU.cfg_of("d64"), PU.params64(m0), *data, steps=0))
    got = run_at(m0.to(dev), data, dev)
    assert got["out"].shape[0] == 129 + 64
    assert (got["dtheta"][1] == 0).all()
    for g in got["dfns"]:
        assert (g[17:22] == 0).all()
    errs = GU.check_parity_per_sample(got, fx)
    assert not errs, errs


@pytest.mark.parametrize("case", ["d64", "d40"])
def test_attention_outputs_are_zero_exactly_where_the_mask_is(dev, case):
    _, data, _ = DU.fixture(case)
    m = gpu_model(case, dev)
    run_at(m, data, dev, step=3)
    cfg = PU.cfg_of(case)
    d = cfg["d"]
    for name, site in [("b0.a", 0), ("b0.bb", 1)] + ([("b1.a", 2), ("b1.bb", 3)] if cfg["n_attn_layers"] > 1 else []):
        _, ld = m.engine().debug_ptr(name)
        t = m.engine().debug_tensor(name, sum(PU.NS), ld).cpu().numpy()
        want = DU.mask_scale(PU.NS, [0] * 3, d, DU.SEED, 3, site, DU.P_DROP)
        assert np.array_equal(t[:, :d] == 0, want == 0), name
        assert np.isfinite(t).all() and (t[:, d:] == 0).all()          # pad columns stay exact zeros
        assert 0.2 < (want == 0).mean() < 0.3


def _same(a, b, inputs=True):
    return (np.array_equal(a["out"], b["out"]) and all(np.array_equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
            and (not inputs or (np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["dtheta"], b["dtheta"])
                                and all(np.array_equal(x, y) for x, y in zip(a["dfns"], b["dfns"])))))


def test_default_and_eval_are_unchanged(dev):
    """attn_dropout=0 and no keyword at all: identical bits; eval() with p > 0: the bits of p = 0; training with
    p > 0: another function"""
    from gnot_amd import GNOT
    _, data, _ = DU.fixture("d64")
    off = PU.run_gpu(gpu_model("d64", dev, attn_dropout=0.0), data, dev)
    m = GNOT(*GU.model_args(PU.cfg_of("d64")))
    m.load_state_dict(DU.fixture("d64")[0].state_dict())
    assert _same(PU.run_gpu(m.to(dev), data, dev), off)
    on = gpu_model("d64", dev)
    on.eval()
    assert _same(PU.run_gpu(on, data, dev), off)
    assert on.dropout_state()["step"] == 0                            # an inactive forward takes no step
    on.train()
    assert GU.rel(PU.run_gpu(on, data, dev)["out"], off["out"]) > 1e-3
    assert on.dropout_state()["step"] == 1


def test_no_grad_with_the_training_flag_drops_the_same_elements(dev):
    _, data, _ = DU.fixture("d64")
    m = gpu_model("d64", dev)
    want = run_at(m, data, dev, step=5)["out"]
    x, off, theta, fns, fo, _ = _packed(data, [0, 1, 2], dev)
    m.set_dropout_step(5)
    with torch.no_grad():
        out = m.forward_packed(x, off, theta, fns, fo)
    assert np.array_equal(out.double().cpu().numpy(), want)
    assert m.dropout_state()["step"] == 6
    m.eval()
    with torch.no_grad():
        out = m.forward_packed(x, off, theta, fns, fo)
    assert not np.array_equal(out.double().cpu().numpy(), want) and m.dropout_state()["step"] == 6


def _packed(data, idx, dev):
    xs, thetas, fns_ps, Gs = data
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    off = lambda ls: np.concatenate([[0], np.cumsum(ls)]).tolist()
    I = len(fns_ps[0])
    return (t(np.concatenate([xs[b] for b in idx])), off([len(xs[b]) for b in idx]), t(np.stack([thetas[b] for b in idx])),
            [t(np.concatenate([fns_ps[b][i] for b in idx])) for i in range(I)],
            [off([len(fns_ps[b][i]) for b in idx]) for i in range(I)], t(np.concatenate([Gs[b] for b in idx])))


def test_two_pending_forwards_keep_their_own_masks(dev):
    """two forwards (steps k, k + 1), then ONE backward through both: each engine regenerates its own forward's
    mask.  Outputs and input gradients of each forward against the masked port at its step; the parameter
    gradients against the sum of the two references, with the sum of their e32"""
    case, k = "d64", 7
    m0, data, _ = DU.fixture(case)
    refs = [DU.as_fx(DU.reference(PU.cfg_of(case), PU.params64(m0), *data, steps=s)) for s in (k, k + 1)]
    m = gpu_model(case, dev)
    m.set_dropout_step(k)
    runs = []
    for _ in range(2):
        x, off, theta, fns, fo, G = _packed(data, [0, 1, 2], dev)
        leaves = [x.requires_grad_(True), theta.requires_grad_(True)] + [f.requires_grad_(True) for f in fns]
        runs.append((m.forward_packed(x, off, theta, fns, fo), G, leaves))
    assert m.dropout_state()["step"] == k + 2
    assert not torch.equal(runs[0][0], runs[1][0])
    sum((out * G).sum() for out, G, _ in runs).backward()
    torch.cuda.synchronize()
    f64 = lambda v: v.detach().double().cpu().numpy()
    for (out, _, leaves), fx in zip(runs, refs):
        got = dict(out=f64(out), grads=None, dx=f64(leaves[0].grad), dtheta=f64(leaves[1].grad),
                   dfns=[f64(f.grad) for f in leaves[2:]])
        errs = GU.check_parity_per_sample(got, fx)
        assert not errs, errs
    for name, p in m.named_parameters():
        ref = refs[0]["grads"][name] + refs[1]["grads"][name]
        lim = GU.RTOL * np.linalg.norm(ref) + GU.SLACK * (refs[0]["e32"][name] + refs[1]["e32"][name])
        assert np.linalg.norm(f64(p.grad) - ref) <= lim, name


@pytest.mark.parametrize("case", ["d64", "d256"])
def test_moe_recompute_and_input_gradients_change_no_bit(dev, case):
    _, data, _ = DU.fixture(case)
    m = gpu_model(case, dev)
    plain = run_at(m, data, dev)
    # without input gradients (no leaf requires grad): the parameter gradients are the same bits
    x, off, theta, fns, fo, G = _packed(data, [0, 1, 2], dev)
    for p in m.parameters():
        p.grad = None
    m.set_dropout_step(0)
    out = m.forward_packed(x, off, theta, fns, fo)
    (out * G).sum().backward()
    torch.cuda.synchronize()
    assert not m.engine().input_grads
    noin = dict(out=out.detach().double().cpu().numpy(), grads={k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()})
    assert _same(noin, plain, inputs=False)
    m.set_moe_recompute(True)
    assert _same(run_at(m, data, dev), plain)


def test_bf16_mode(dev):
    """the bar and the sanity check of tests/test_gpu_bf16.py: output and concatenated gradients within 1e-2 of
    the masked float64 reference, and more than 1e-6 from the fp32 results"""
    case = "d256"
    _, data, fx = DU.fixture(case)
    m = gpu_model(case, dev)
    g32 = run_at(m, data, dev)
    m.set_precision("bf16")
    g16 = run_at(m, data, dev)
    keys = sorted(fx["grads"])
    cat = lambda g: np.concatenate([np.ravel(g[k]) for k in keys])
    e_out, e_grad = GU.rel(g16["out"], fx["out"]), GU.rel(cat(g16["grads"]), cat(fx["grads"]))
    print(f"bf16 dropout d=256: output {e_out:.2e}, gradients {e_grad:.2e}")
    assert e_out < 1e-2 and e_grad < 1e-2, (e_out, e_grad)
    assert GU.rel(g16["out"], g32["out"]) > 1e-6 and GU.rel(cat(g16["grads"]), cat(g32["grads"])) > 1e-6


@pytest.mark.parametrize("case", ["d64", "d256"])
def test_accumulated_micro_batches_are_the_float32_sum(dev, case):
    """two micro-batches, each at its own step, through set_grad_arena + backward_options(accumulate=True) leave
    the element-wise float32 sum of the two separate backwards in the arena"""
    _, data, _ = DU.fixture(case)
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

    m.set_dropout_step(3)
    step([0, 2], False)
    gA = arena.clone()
    step([1], False)                                  # step 4
    gB = arena.clone()
    assert torch.isfinite(gA).all() and torch.isfinite(gB).all() and not torch.equal(gA, gB)
    m.set_dropout_step(3)
    step([0, 2], False)
    step([1], True)
    assert m.dropout_state()["step"] == 5
    assert torch.equal(bits(arena), bits(gA + gB))


@pytest.mark.parametrize("case", ["d64", "d256"])
def test_captured_training_step_replays_the_eager_step(dev, case):
    """forward + RelL2 + backward + FlatAdamW.launch captured in one hipGraph: replayed after set_dropout_step(k)
    it leaves the parameters of the eager step k, bit for bit, and after set_dropout_step(k + 1) those of the eager
    step k + 1 (the key is read when the kernels run)"""
    from gnot_amd import train
    _, data, _ = DU.fixture(case)
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

    for m, opt in zip(models, opts):                 # one eager step each (step 0): plans bound, workspaces allocated
        opt.prepare()
        fwd_bwd_opt(m, opt)
    torch.cuda.synchronize()
    assert torch.equal(bits(opts[0].flat), bits(opts[1].flat))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd_bwd_opt(models[1], opts[1])
    assert models[1].dropout_state()["step"] == 1    # a captured forward writes no key and takes no step
    for k in (1, 2):
        opts[0].prepare()
        fwd_bwd_opt(models[0], opts[0])              # step k, eager ...
        opts[1].prepare()
        models[1].set_dropout_step(k)
        graph.replay()                               # ... and as a replay
        torch.cuda.synchronize()
        assert torch.isfinite(opts[0].flat).all()
        assert torch.equal(bits(opts[0].flat), bits(opts[1].flat)), k
    # the same graph at a stale step is another update: the mask does come from the key
    before = opts[1].flat.clone()
    opts[0].prepare()
    fwd_bwd_opt(models[0], opts[0])                  # eager step 3
    opts[1].prepare()
    models[1].set_dropout_step(2)
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(opts[1].flat, before) and not torch.equal(bits(opts[0].flat), bits(opts[1].flat))


# ------------------------------------------------------------------ fit
FIT_ARGS = (2, 1, 3, 1, 1, 64, 2, 64, 64, 2, 4, 1)       # train_step_util.SMALL at d = 64


def _fit_model(seed=0, p=0.25):
    from gnot_amd import GNOT
    torch.manual_seed(seed)
    return GNOT(*FIT_ARGS, attn_dropout=p, dropout_seed=99).cuda()


@pytest.fixture(scope="module")
def loaders():
    """6 synthetic meshes of 150 to 300 points: two train batches and one test batch of two"""
    from gnot_amd import data
    rng = np.random.default_rng(5)
    mk_s = lambda k: [data.synthetic_sample(rng, int(rng.integers(150, 300)), fn_points=(int(rng.integers(10, 30)),))
                      for _ in range(k)]
    mk = lambda s: list(torch.utils.data.DataLoader(data.NS2dData(s), batch_size=2, shuffle=False,
                                                    collate_fn=data.collate_packed))
    return mk(mk_s(4)), mk(mk_s(2))


def test_resumed_fit_is_the_uninterrupted_fit_bitwise(dev, loaders, tmp_path):
    import train_step_util as U
    from gnot_amd import train
    tr, te = loaders
    p, q = (os.path.join(tmp_path, n) for n in ("p.pt", "q.pt"))
    ref = _fit_model()
    ref_hist = train.fit(ref, tr, te, epochs=2, state_path=p, log=lambda msg: None)
    ref_flat = U.flat_params(ref).clone()
    assert all(np.isfinite(v) for h in ref_hist for v in h) and len(ref_hist[0]) == 2
    assert ref.training and ref.dropout_state()["step"] == 4          # 2 epochs x 2 batches; the test pass takes none

    def log(msg):
        if msg.startswith("Epoch 1, Loss"):               # epoch 0's state is on disk, epoch 1's is not
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(_fit_model(), tr, te, epochs=2, state_path=q, log=log)
    state = train.load_training_state(q)
    assert state["next_epoch"] == 1 and state["dropout"] == dict(p=0.25, seed=99, step=2)
    got = _fit_model(seed=123)                            # a fresh module with other weights, its counter at 0
    got_hist = train.fit(got, tr, te, epochs=2, state_path=q, resume=True, log=lambda msg: None)
    assert got_hist == ref_hist
    assert torch.equal(U.bits(U.flat_params(got)), U.bits(ref_flat))
    assert got.dropout_state() == ref.dropout_state()
    # dropout does something: the run without it has another history
    plain_hist = train.fit(_fit_model(p=0.0), tr, te, epochs=2, log=lambda msg: None)
    assert plain_hist != ref_hist
    # a resume under another p, another seed or without dropout is refused
    for other in (_fit_model(p=0.5), _fit_model(p=0.0)):
        with pytest.raises(ValueError, match="dropout"):
            train.fit(other, tr, te, epochs=2, state_path=q, resume=True, log=lambda msg: None)
