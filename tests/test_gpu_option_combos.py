"""Pre-norm, attention dropout and the Fourier embedding TOGETHER through forward_packed on the GPU, against the
composed float64 reference of tests/combo_util.py (the three single-option references nested; guarded on the CPU
by tests/test_option_combos.py), under the project's parity rule (golden_util.RTOL / SLACK with the e32 of the
composed port; the bf16 mode at the 1e-2 bar of tests/test_gpu_bf16.py; no new tolerance).  Every other test file
turns one of these options on at a time, while attn_backward, the shortened backward of frozen Linears,
gnot_input_grads and the workspace carve are shared by all of them: the pairs and the triple at every kernel
family, the dropped and the normalised rows themselves, frozen Linears on top of the triple, the bitwise option
checks, the bf16 mode, a captured fine-tuning step and two point-sharded ranks.

Geometry: Ns = [129, 0, 64, 1], Ms = [17, 5, 3, 1] (combo_util.NS / MS), dropout step 3.  No non-empty sample has
an empty input function: the reference is 0 / 0 there."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import combo_util as CU
import dropout_util as DU
import golden_util as GU
import prenorm_util as PU
import test_gpu_frozen_linears as FL
from test_gpu_prenorm_kernel import C_FWD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 3
ALL = list(range(len(CU.NS)))
PAIRS = [("prenorm", "drop"), ("prenorm", "fourier"), ("drop", "fourier")]
_FX = {}
bits = lambda t: t.view(torch.int32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


def fixture(case, opts=CU.TRIPLE, step=STEP):
    """(inputs, fx) of a case with `opts` on at a dropout step: fx the dict check_parity_per_sample takes.  Computed
    once per process, shared by the tests that need it and left unchanged."""
    key = (case, frozenset(opts), step)
    if key not in _FX:
        data = CU.inputs(case)
        params = {k: v.detach().double().numpy() for k, v in CU.model(case, opts).named_parameters()}
        _FX[key] = (data, CU.as_fx(CU.reference(case, opts, params, *data, steps=step)))
    return _FX[key]


def gpu_model(case, dev, opts=CU.TRIPLE):
    return CU.model(case, opts).to(dev)          # the seed makes the weights: the same for every subset of options


def run_at(m, data, dev, step=STEP):
    if m.attn_dropout:
        m.set_dropout_step(step)
    return CU.run_gpu(m, data, dev)


def _packed(data, idx, dev):
    xs, thetas, fns_ps, Gs = data
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    off = lambda ls: np.concatenate([[0], np.cumsum(ls)]).astype(np.int64).tolist()
    I = len(fns_ps[0])
    return (t(np.concatenate([xs[b] for b in idx])), off([len(xs[b]) for b in idx]), t(np.stack([thetas[b] for b in idx])),
            [t(np.concatenate([fns_ps[b][i] for b in idx])) for i in range(I)],
            [off([len(fns_ps[b][i]) for b in idx]) for i in range(I)], t(np.concatenate([Gs[b] for b in idx])))


def _same(a, b, inputs=True):
    return (np.array_equal(a["out"], b["out"]) and all(np.array_equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
            and (not inputs or (np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["dtheta"], b["dtheta"])
                                and all(np.array_equal(x, y) for x, y in zip(a["dfns"], b["dfns"])))))


# ------------------------------------------------------------------ (a) parity of the combinations
# c256 twice: forked weight gradients (the default below 65,536 points) and, with GNOT_WGRAD_OVERLAP=0 set before
# the model is built, the serial form
PARITY = [("c64", o, False) for o in PAIRS] + [(c, CU.TRIPLE, False) for c in ("c64", "c40", "c30", "c256", "c320")] + \
         [("c256", CU.TRIPLE, True)]


@pytest.mark.parametrize("case, opts, serial", PARITY,
                         ids=[f"{c}-{'+'.join(o)}{'-serial' if s else ''}" for c, o, s in PARITY])
def test_parity_with_the_composed_reference(dev, case, opts, serial, monkeypatch):
    if serial:
        monkeypatch.setenv("GNOT_WGRAD_OVERLAP", "0")
    data, fx = fixture(case, opts)
    m = gpu_model(case, dev, opts)
    assert m.training
    got = run_at(m, data, dev)
    if serial:
        assert m.engine().kernel_forms()["serial_wgrad"] == "1"
    assert got["out"].shape[0] == sum(CU.NS) and got["dx"].shape[1] == CU.IN
    assert (got["dtheta"][1] == 0).all() and all((g[CU.MS[0]:CU.MS[0] + CU.MS[1]] == 0).all() for g in got["dfns"])
    keys = sorted(fx["grads"])
    cat = lambda g: np.concatenate([np.ravel(g[k]) for k in keys])
    ws, wsw, wr, wrw = GU.worst_relative(GU.per_sample_errors(got, fx))
    print(f"{case} {'+'.join(opts)}{' serial' if serial else ''}: output {GU.rel(got['out'], fx['out']):.2e}, gradients "
          f"{GU.rel(cat(got['grads']), cat(fx['grads'])):.2e}, worst per sample {ws:.2e} ({wsw}), per row {wr:.2e} ({wrw})")
    errs = GU.check_parity_per_sample(got, fx)
    assert not errs, errs
    if "drop" in opts:
        assert m.dropout_state()["step"] == STEP + 1


# ------------------------------------------------------------------ (b) the dropped and the normalised rows
def _forward_only(case, dev):
    """a training forward of the triple at STEP whose backward has not run: the engine's rows as the forward left
    them"""
    data, _ = fixture(case)
    m = gpu_model(case, dev)
    x, off, theta, fns, fo, G = _packed(data, ALL, dev)
    m.set_dropout_step(STEP)
    out = m.forward_packed(x, off, theta, fns, fo)
    torch.cuda.synchronize()
    return m, out, G


def test_attention_outputs_are_zero_exactly_where_the_mask_is(dev):
    case = "c64"
    m, out, G = _forward_only(case, dev)
    d, P = CU.CASES[case]["d"], sum(CU.NS)
    for name, site in [("b0.a", 0), ("b0.bb", 1), ("b1.a", 2), ("b1.bb", 3)]:
        _, ld = m.engine().debug_ptr(name)
        t = m.engine().debug_tensor(name, P, ld).cpu().numpy()
        want = DU.mask_scale(CU.NS, [0] * len(CU.NS), d, DU.SEED, STEP, site, DU.P_DROP)
        assert np.array_equal(t[:, :d] == 0, want == 0), name
        assert np.isfinite(t).all() and (t[:, d:] == 0).all()          # pad columns stay exact zeros
        assert 0.2 < (want == 0).mean() < 0.3
    (out * G).sum().backward()


def _port_rows(case):
    """per non-empty sample the (raw, normalised) tensors of the float64 and the float32 composed port at STEP, in
    call order"""
    from gnot_amd import fourier_features
    from oracle import torch_port
    c, (xs, thetas, fns_ps, _) = CU.CASES[case], fixture(case)[0]
    wide = CU.wide_cfg(CU.cfg_of(case), c["nx"], c["nf"])
    params = {k: v.detach().double().numpy() for k, v in CU.model(case, CU.TRIPLE).named_parameters()}
    res = {}
    for dt in (torch.float64, torch.float32):
        p = {k: torch.tensor(v, dtype=dt) for k, v in params.items()}
        t = lambda a: torch.tensor(np.asarray(a), dtype=dt)[None]
        per = []
        for b in [b for b, n in enumerate(CU.NS) if n > 0]:
            seen, masks = [], DU.site_masks(wide, CU.NS, STEP, order=[b])
            with CU.port(CU.TRIPLE, masks, seen=seen) as calls:
                torch_port.gnot_forward(p, wide, fourier_features(t(xs[b]), c["nx"]), t(thetas[b]),
                                        [fourier_features(t(f), c["nf"]) for f in fns_ps[b]])
            assert calls[0] == len(masks)
            per.append(seen)
        res[dt] = per
    return res[torch.float64], res[torch.float32]


def test_debug_buffers_hold_the_normalised_rows(dev):
    """The n1 / n2 rows of both blocks and the fnn{i} rows.  Block 1's and every n2 are taken from rows that come
    out of dropped attention outputs.  (1) Each is the LayerNorm of the raw rows the ENGINE holds, element by
    element within the row kernel's own bound (prenorm_util.fwd_ratios, C_FWD of tests/test_gpu_prenorm_kernel.py).
    (2) Each is the normalised row of the composed reference under the per-row parity rule, as in
    tests/test_gpu_prenorm.py."""
    case = "c64"
    m, out, G = _forward_only(case, dev)
    eng = m.engine()
    P, Q = sum(CU.NS), sum(CU.MS)
    s64, s32 = _port_rows(case)
    # call order per sample (2 input functions, 2 blocks): [q, enc0, enc1, q1] of block 0, then of block 1
    for name, raw, rstd, k, rows in (("b0.n1", "query0", "b0.r1", 0, P), ("b0.n2", "b0.query1", "b0.r2", 3, P),
                                     ("b1.n1", "b0.query2", "b1.r1", 4, P), ("b1.n2", "b1.query1", "b1.r2", 7, P),
                                     ("fnn0", "fnenc0", "fnr0", 1, Q), ("fnn1", "fnenc1", "fnr1", 2, Q)):
        assert eng.debug_ptr(name)[1] == 64
        got = eng.debug_tensor(name, rows, 64).double().cpu().numpy()
        x = eng.debug_tensor(raw, rows, 64).double().cpu().numpy()
        r = eng.debug_tensor(rstd, rows, 1).double().cpu().numpy()[:, 0]
        qf, qr = PU.fwd_ratios(x, got, r)
        assert qf <= C_FWD and qr <= C_FWD, (name, qf, qr)
        if rows == P:            # (the empty sample has no reference call; its 5 input-function rows are normalised too)
            ref = np.concatenate([PU.ln64(s[k][0][0].numpy())[0] for s in s64])
            e32 = np.concatenate([np.linalg.norm(a[k][1][0].double().numpy() - b[k][1][0].numpy(), axis=1) for a, b in zip(s32, s64)])
            rown = np.linalg.norm(ref, axis=1)
            lim = GU.RTOL * np.maximum(rown, np.sqrt(np.mean(rown ** 2))) + GU.SLACK * e32
            err = np.linalg.norm(got - ref, axis=1)
            assert (err <= lim).all(), (name, float((err / lim).max()))
    (out * G).sum().backward()


# ------------------------------------------------------------------ (c) frozen Linears on top of the triple
FROZEN = [("c64", s) for s in FL.SETS] + [("c256", s) for s in FL.SETS if s != "last_block"]


@pytest.mark.parametrize("case, which", FROZEN, ids=[f"{c}-{s}" for c, s in FROZEN])
def test_frozen_set_on_the_triple(dev, case, which):
    patterns, input_grads, stage_of = FL.SETS[which]
    data, fx = fixture(case)
    L = CU.CASES[case]["L"]
    m = gpu_model(case, dev)
    x, off, theta, fns, fo, G = _packed(data, ALL, dev)

    def forward(leaves=False):
        m.set_dropout_step(STEP)
        a = [v.clone().requires_grad_(True) for v in [x, theta] + fns] if leaves else [x, theta] + fns
        return m.forward_packed(a[0], off, a[1], a[2:], fo), a

    # the unfrozen forward (a training forward, whose backward runs: the engine is free again afterwards)
    out0, _ = forward()
    assert m.engine().backward_plan() == (len(m.linears()), -1)
    (out0 * G).sum().backward()
    m.zero_grad(set_to_none=True)

    frozen = FL.frozen_names(m, patterns)
    assert frozen and (which == "all_frozen_input_grads") == (len(frozen) == len(list(m.parameters())))
    for n, p in m.named_parameters():
        p.requires_grad_(n not in frozen)
    arena = FL.sentinel_arena(m)
    out, leaves = forward(input_grads)
    assert torch.equal(bits(out.detach()), bits(out0.detach()))
    live = [l for l in m.linears() if l.weight.requires_grad or l.bias.requires_grad]
    assert m.engine().backward_plan() == (len(live), stage_of(L))
    (out * G).sum().backward()
    torch.cuda.synchronize()
    FL.check_arena(m, arena, frozen, "plain")

    # .grad is None exactly on the frozen parameters; the trainable gradients against the composed reference
    f64 = lambda v: v.detach().double().cpu().numpy()
    grads = {}
    for n, p in m.named_parameters():
        assert (p.grad is None) == (n in frozen), n
        if p.grad is not None:
            grads[n] = f64(p.grad)
    sub = dict(fx, grads={k: fx["grads"][k] for k in grads})
    keys = sorted(grads)
    cat = lambda g: np.concatenate([np.ravel(g[k]) for k in keys])
    line = f"{case} triple, {which}: output {GU.rel(f64(out), fx['out']):.2e}"
    if grads:
        line += f", trainable gradients {GU.rel(cat(grads), cat(sub['grads'])):.2e}"
    if input_grads:
        got = dict(out=f64(out), grads=None, dx=f64(leaves[0].grad), dtheta=f64(leaves[1].grad),
                   dfns=[f64(f.grad) for f in leaves[2:]])
        ws, wsw, wr, wrw = GU.worst_relative(GU.per_sample_errors(got, fx))
        print(line + f", worst per sample {ws:.2e} ({wsw}), per row {wr:.2e} ({wrw})")
        errs = GU.check_parity_per_sample(got, fx)
    else:
        print(line)
        errs = GU.check_parity(f64(out), grads, sub)
    assert not errs, errs

    # an accumulating backward of the same step on top: the trainable ranges hold the float32 sum, the frozen ones
    # keep the sentinel
    if not grads:
        return
    first = arena.clone()
    m.engine().param_grads = False
    out2, _ = forward(input_grads)
    with m.backward_options(accumulate=True):
        (out2 * G).sum().backward()
    torch.cuda.synchronize()
    FL.check_arena(m, arena, frozen, "accumulate")
    for name, (o, n) in FL.arena_ranges(m).items():
        if name not in frozen:
            assert torch.equal(bits(arena[o:o + n]), bits(first[o:o + n] + first[o:o + n])), name


# ------------------------------------------------------------------ (d) bitwise invariants under the triple
@pytest.mark.parametrize("case", ["c64", "c256"])
def test_moe_recompute_and_input_gradients_change_no_bit(dev, case):
    data, _ = fixture(case)
    m = gpu_model(case, dev)
    plain = run_at(m, data, dev)
    # without input gradients (no leaf requires grad): the output and the parameter gradients are the same bits
    x, off, theta, fns, fo, G = _packed(data, ALL, dev)
    for p in m.parameters():
        p.grad = None
    m.set_dropout_step(STEP)
    out = m.forward_packed(x, off, theta, fns, fo)
    (out * G).sum().backward()
    torch.cuda.synchronize()
    assert not m.engine().input_grads
    noin = dict(out=out.detach().double().cpu().numpy(), grads={k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()})
    assert _same(noin, plain, inputs=False)
    m.set_moe_recompute(True)
    assert _same(run_at(m, data, dev), plain)


@pytest.mark.parametrize("case", ["c64", "c256"])
def test_accumulated_micro_batches_are_the_float32_sum(dev, case):
    """two micro-batches at steps k and k + 1 through set_grad_arena + backward_options(accumulate=True) leave the
    element-wise float32 sum of the two separate backwards in the arena"""
    data, _ = fixture(case)
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

    A, B = [0, 1, 3], [2]                             # 129 points, the empty sample and the 1-point sample; 64 points
    m.set_dropout_step(STEP)
    step(A, False)
    gA = arena.clone()
    step(B, False)                                    # step k + 1
    gB = arena.clone()
    assert torch.isfinite(gA).all() and torch.isfinite(gB).all() and not torch.equal(gA, gB)
    m.set_dropout_step(STEP)
    step(A, False)
    step(B, True)
    assert m.dropout_state()["step"] == STEP + 2
    assert torch.equal(bits(arena), bits(gA + gB))


@pytest.mark.parametrize("case", ["c64", "c256"])
def test_eval_is_the_model_without_dropout(dev, case):
    """eval() of the triple: the bits of the pre-norm + Fourier model, and no step taken; training: another function"""
    data, _ = fixture(case)
    off = CU.run_gpu(gpu_model(case, dev, ("prenorm", "fourier")), data, dev)
    on = gpu_model(case, dev)
    on.eval()
    assert _same(CU.run_gpu(on, data, dev), off)
    assert on.dropout_state()["step"] == 0
    on.train()
    assert not np.array_equal(CU.run_gpu(on, data, dev)["out"], off["out"]) and on.dropout_state()["step"] == 1


# ------------------------------------------------------------------ (e) bf16 mode
def test_bf16_mode(dev):
    """the bar and the sanity check of tests/test_gpu_bf16.py: output and concatenated gradients within 1e-2 of
    the composed float64 reference, and more than 1e-6 from the fp32 results"""
    case = "c256"
    data, fx = fixture(case)
    m = gpu_model(case, dev)
    g32 = run_at(m, data, dev)
    m.set_precision("bf16")
    g16 = run_at(m, data, dev)
    keys = sorted(fx["grads"])
    cat = lambda g: np.concatenate([np.ravel(g[k]) for k in keys])
    e_out, e_grad = GU.rel(g16["out"], fx["out"]), GU.rel(cat(g16["grads"]), cat(fx["grads"]))
    print(f"bf16 {case} triple: output {e_out:.2e}, gradients {e_grad:.2e}")
    assert e_out < 1e-2 and e_grad < 1e-2, (e_out, e_grad)
    assert GU.rel(g16["out"], g32["out"]) > 1e-6 and GU.rel(cat(g16["grads"]), cat(g32["grads"])) > 1e-6


# ------------------------------------------------------------------ (f) a captured fine-tuning step
def test_captured_fine_tuning_step_replays_the_eager_step(dev):
    """forward + RelL2 + backward + FlatAdamW.launch of the c64 triple with everything but the decoder frozen,
    captured in one graph: replayed after set_dropout_step(k) it leaves the parameters of the eager step k, bit for
    bit, for k = 1, 2 (the pattern of tests/test_gpu_dropout.py)"""
    from gnot_amd import train
    case = "c64"
    patterns = FL.SETS["decoder_only"][0]
    data, _ = fixture(case)
    x, off, theta, fns, fo, y = _packed(data, ALL, dev)
    loss_off = sorted(set(off))                      # the loss takes no empty sample: the same rows without it
    loss_fn = train.RelL2Loss()
    models, opts = [], []
    for _ in range(2):
        m = gpu_model(case, dev)
        frozen = FL.frozen_names(m, patterns)
        for n, p in m.named_parameters():
            p.requires_grad_(n not in frozen)
        opts.append(train.FlatAdamW(train.flatten_parameters(m), lr=1e-3, groups=train.param_groups(m, freeze=patterns),
                                    layout=train.arena_layout(m)))
        m.engine().param_grads = False
        models.append(m)

    def fwd_bwd_opt(m, opt):
        out = m.forward_packed(x, off, theta, fns, fo)
        loss_fn(loss_off, out, y).backward()
        opt.launch(m.engine().grad_flat)

    for m, opt in zip(models, opts):                 # one eager step each (step 0): plans bound, workspaces allocated
        opt.prepare()
        fwd_bwd_opt(m, opt)
    torch.cuda.synchronize()
    L = CU.CASES[case]["L"]
    assert models[1].engine().backward_plan() == (len(models[1].out.linears()), L)
    assert torch.equal(bits(opts[0].flat), bits(opts[1].flat))
    start = opts[1].flat.clone()
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
    # the decoder moved, the frozen tensors kept their bits
    o = 0
    for name, n in train.arena_layout(models[1]):
        assert torch.equal(bits(opts[1].flat[o:o + n]), bits(start[o:o + n])) == (name in frozen), name
        o += n


# ------------------------------------------------------------------ (g) two ranks, gloo, both on the one GPU
SHARD = "c64s"           # d = 64, 4 heads, one input function, one block


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
        (xs, thetas, fns_ps, Gs), fx = fixture(SHARD)
        Ns = [len(a) for a in xs]
        x_off = np.concatenate([[0], np.cumsum(Ns)])
        dev = torch.device("cuda", 0)
        m = gpu_model(SHARD, dev)
        m.set_point_shard(par.PointShardComm(stage_via_host=True))
        loc_off, ranges = par.shard_offsets(Ns, rank, world)
        rows = np.concatenate([np.arange(x_off[b] + lo, x_off[b] + hi) for b, (lo, hi) in enumerate(ranges)]).astype(np.int64)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
        x = t(np.concatenate(xs)[rows]).requires_grad_(True)
        theta = t(np.stack(thetas)).requires_grad_(True)
        fn = t(np.concatenate([f[0] for f in fns_ps])).requires_grad_(True)
        fn_off = np.concatenate([[0], np.cumsum([len(f[0]) for f in fns_ps])]).tolist()
        m.set_dropout_step(STEP)
        out = m.forward_packed(x, loc_off, theta, [fn], [fn_off], n_global=Ns)
        (out * t(np.concatenate(Gs)[rows])).sum().backward()       # gnot_input_grads sums dtheta / dfns over the ranks
        h = m.engine().grad_flat.cpu()
        dist.all_reduce(h)                                        # parameter gradients: sum over ranks
        m.engine().grad_flat.copy_(h.to(dev))
        torch.cuda.synchronize()
        f64 = lambda v: v.detach().double().cpu().numpy()
        # this rank's dropped rows: zero exactly at the global mask's positions
        a = m.engine().debug_tensor("b0.a", len(rows), 64).cpu().numpy()
        zeros_ok = bool(np.array_equal(a == 0, DU.mask_scale(Ns, [0] * len(Ns), 64, DU.SEED, STEP, 0, DU.P_DROP)[rows] == 0))
        parts = [None] * world
        dist.all_gather_object(parts, (rows, f64(out), f64(x.grad), f64(theta.grad), f64(fn.grad), zeros_ok))
        if rank == 0:
            P = int(x_off[-1])
            got = dict(out=np.zeros((P, CU.OUT)), dx=np.zeros((P, CU.IN)), dtheta=parts[0][3], dfns=[parts[0][4]],
                       grads={k: f64(p.grad) for k, p in m.named_parameters()})
            errs = []
            for r, (r_rows, o, dx, dth, dfn, ok) in enumerate(parts):
                got["out"][r_rows], got["dx"][r_rows] = o, dx
                # the rank sums are the same on every rank
                assert np.array_equal(dth, got["dtheta"]) and np.array_equal(dfn, got["dfns"][0])
                if not ok:
                    errs.append(f"rank {r}: the zeros of b0.a are not at the global mask's positions")
            q.put(errs + GU.check_parity_per_sample(got, fx))
    except Exception as e:  # report instead of hanging the other rank's collectives
        if rank == 0:
            q.put([f"rank0 exception: {e!r}"])
        raise
    finally:
        dist.destroy_process_group()


def test_point_sharded_triple_matches_the_unsharded_reference():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    errs = q.get(timeout=100)
    for p in procs:
        p.join(timeout=30)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert not errs, errs
