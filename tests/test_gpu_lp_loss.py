"""The Lp loss family on the GPU (gnot_lp_loss through train.LpLoss): every kind against the float64 reference of
lp_util at the bar of the existing loss tests (1e-5 relative, test_train.py), rel2 / mse bit for bit RelL2Loss /
MSELoss, determinism, component weights, one graph capture, fit end to end with resume, and evaluate_table.

Sizes (lp_util.CASES): [1, 2049, 300] with three channels -- a one-row sample, a sample one row past the 2048-row
split -- and [4097, 4096] with one channel -- two full splits and a row, and the exact multiple."""
import os

import numpy as np
import pytest
import torch

import lp_util as L
import train_step_util as U
from gnot_amd import GNOT, Normalizer, data, train
from train_step_util import bits

pytestmark = pytest.mark.gpu

WEIGHTS = [1.0, 0.0, 3.0]
_CACHE = {}


def case(i):
    """(offsets, pred, tgt on the device, pred, tgt as numpy) of lp_util.CASES[i], drawn once"""
    if i not in _CACHE:
        sizes, C = L.CASES[i]
        pred, tgt = L.inputs(sizes, C)
        _CACHE[i] = (L.offsets(sizes), torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda(), pred, tgt)
    return _CACHE[i]


def normalizer(C):
    """y statistics that are no powers of two, so pred * std + mean rounds"""
    mean, std = [0.3, -1.7, 0.05][:C], [1.9, 0.6, 3.3][:C]
    return Normalizer.from_stats(([0.0], [1.0]), ([0.0], [1.0]), (mean, std))


def physical(pred, nz):
    """the float64 de-normalisation of a float32 numpy prediction with nz's (fp32) statistics"""
    if nz is None:
        return pred.astype(np.float64)
    y = nz.y.double().numpy()
    return pred.astype(np.float64) * y[1] + y[0]


def run(fn, off, pred, tgt, grad=True, terms=True):
    """(loss, terms or None, dpred or None) of one pass of the LpLoss / RelL2Loss / MSELoss fn"""
    p = pred.clone().requires_grad_(grad)
    if terms:
        loss, e = fn.loss_and_terms(off, p, tgt)
    else:
        loss, e = fn(off, p, tgt), None
    if grad:
        loss.backward()
    return loss.detach(), e, p.grad


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("with_nz", [False, True], ids=["raw", "normalizer"])
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("i", range(len(L.CASES)))
def test_loss_terms_and_gradient_against_float64(i, kind, with_nz):
    off, pred, tgt, pred_np, tgt_np = case(i)
    C = pred.shape[1]
    nz = normalizer(C) if with_nz else None
    p64 = physical(pred_np, nz)
    differentiable = kind in L.DIFFERENTIABLE
    for weights in (None, WEIGHTS[:C]):
        loss, e, dpred = run(train.LpLoss(kind, weights, nz), off, pred, tgt, grad=differentiable)
        ref_e = L.terms(kind, p64, tgt_np, off)
        ref = L.loss(kind, p64, tgt_np, off, weights)
        err_e = float((np.abs(e.double().cpu().numpy() - ref_e) / ref_e).max())
        print(f"case {i} {kind} nz={with_nz} w={weights}: loss {float(loss):.9g} ref {ref:.9g} "
              f"rel {abs(float(loss) - ref) / ref:.2e}, terms rel {err_e:.2e}")
        assert abs(float(loss) - ref) <= 1e-5 * ref
        assert e.shape == (len(off) - 1, C) and err_e <= 1e-5
        if not differentiable:
            assert dpred is None
            continue
        ref_g = L.grad(kind, p64, tgt_np, off, weights)
        if nz is not None:
            ref_g = ref_g * nz.y.double().numpy()[1]
        g = dpred.double().cpu().numpy()
        if kind in ("rel1", "l1"):
            # sign(d) of an fp32 d next to zero may differ from float64's: leave those elements out
            keep = np.abs(p64 - tgt_np) >= 1e-6
            left_out = 1.0 - keep.mean()
            print(f"    left out {left_out:.2e} of the elements")
            assert left_out < 0.01
            g, ref_g = g * keep, ref_g * keep
        err_g = float(np.linalg.norm(g - ref_g) / np.linalg.norm(ref_g))
        print(f"    dpred norm-wise rel {err_g:.2e}")
        assert err_g <= 1e-5


# ------------------------------------------------------------------ the existing classes, bit for bit
@pytest.mark.parametrize("with_nz", [False, True], ids=["raw", "normalizer"])
@pytest.mark.parametrize("kind,cls", [("rel2", train.RelL2Loss), ("mse", train.MSELoss)])
@pytest.mark.parametrize("i", range(len(L.CASES)))
def test_rel2_and_mse_carry_the_bits_of_the_existing_losses(i, kind, cls, with_nz):
    off, pred, tgt, _, _ = case(i)
    nz = normalizer(pred.shape[1]) if with_nz else None
    ref_loss, _, ref_g = run(cls(nz), off, pred, tgt, terms=False)
    assert float(ref_g.abs().max()) > 0
    # without the terms and with them (one set of kernels; the finish kernel then stores the terms too)
    for terms in (False, True):
        loss, e, g = run(train.LpLoss(kind, normalizer=nz), off, pred, tgt, terms=terms)
        assert torch.equal(bits(loss), bits(ref_loss)), (terms, float(loss), float(ref_loss))
        assert torch.equal(bits(g), bits(ref_g)), terms
    # and the loss alone, no gradient asked for
    with torch.no_grad():
        fn = train.LpLoss(kind, normalizer=nz)
        assert torch.equal(bits(fn(off, pred, tgt)), bits(ref_loss))
        assert torch.equal(bits(fn.loss_and_terms(off, pred, tgt)[0]), bits(ref_loss))
        assert torch.equal(bits(fn.terms(off, pred, tgt)), bits(e))


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize("kind", L.KINDS)
def test_two_runs_give_equal_bits(kind):
    for i in range(len(L.CASES)):
        off, pred, tgt, _, _ = case(i)
        w = WEIGHTS[:pred.shape[1]]
        a = run(train.LpLoss(kind, w), off, pred, tgt, grad=kind in L.DIFFERENTIABLE)
        b = run(train.LpLoss(kind, w), off, pred, tgt, grad=kind in L.DIFFERENTIABLE)
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(bits(x), bits(y))


# ------------------------------------------------------------------ weights
@pytest.mark.parametrize("with_nz", [False, True], ids=["raw", "normalizer"])
@pytest.mark.parametrize("kind", L.DIFFERENTIABLE)
def test_component_weights(kind, with_nz):
    off, pred, tgt, _, _ = case(0)
    nz = normalizer(3) if with_nz else None
    loss, e, g = run(train.LpLoss(kind, WEIGHTS, nz), off, pred, tgt)
    _, e0, g0 = run(train.LpLoss(kind, None, nz), off, pred, tgt)
    assert torch.equal(g[:, 1], torch.zeros_like(g[:, 1]))                    # weight 0: exact zeros
    assert float(g0[:, 1].abs().max()) > 0
    assert float(g[:, 0].abs().max()) > 0 and float(g[:, 2].abs().max()) > 0
    assert torch.equal(bits(e), bits(e0))                                     # the terms ignore the weights
    w = np.asarray(WEIGHTS) / sum(WEIGHTS)
    want = float((e.double().cpu().numpy().mean(0) * w).sum())
    assert abs(float(loss) - want) <= 1e-6 * want
    # the weighted gradient is the unweighted one per channel, times C w^_c (fp32 rounding apart)
    for c in (0, 2):
        ratio = (g[:, c].double() / g0[:, c].double())
        assert float((ratio - 3 * w[c]).abs().max()) <= 1e-6 * 3 * w[c]
    # a NaN in the channel of weight zero stays out of the gradient (not out of the loss: 0 * NaN)
    bad = pred.clone()
    bad[5, 1] = float("nan")
    _, _, gb = run(train.LpLoss(kind, WEIGHTS, nz), off, bad, tgt)
    assert torch.equal(gb[:, 1], torch.zeros_like(gb[:, 1])) and torch.equal(bits(gb[:, 0]), bits(g[:, 0]))


def test_metric_kinds_keep_a_nan_and_take_no_gradient():
    off, pred, tgt, _, _ = case(0)
    bad = pred.clone()
    bad[700, 2] = float("nan")                       # sample 1, channel 2
    for kind in ("relinf", "linf"):
        e = train.LpLoss(kind).terms(off, bad, tgt)
        assert bool(torch.isnan(e[1, 2])) and int(torch.isnan(e).sum()) == 1
        with pytest.raises(ValueError, match="metric only"):
            train.LpLoss(kind)(off, pred.clone().requires_grad_(True), tgt)


def test_wrong_weight_count_and_empty_sample_are_refused():
    off, pred, tgt, _, _ = case(0)
    with pytest.raises(ValueError, match="component_weights"):
        train.LpLoss("rel1", [1, 2])(off, pred, tgt)
    with pytest.raises(RuntimeError, match="empty sample"):
        train.LpLoss("rel2")([0, 1, 1, off[-1]], pred, tgt)


# ------------------------------------------------------------------ capture
def test_captured_rel1_with_weights_replays_on_new_predictions():
    off, pred, tgt, _, _ = case(0)
    fn = train.LpLoss("rel1", WEIGHTS)
    static = pred.clone().requires_grad_(True)
    ref0 = run(train.LpLoss("rel1", WEIGHTS), off, pred, tgt, terms=False)
    fn(off, static, tgt).backward()                  # eager once: geometry, weights, kernels
    static.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = fn(off, static, tgt)
        (dpred,) = torch.autograd.grad(loss, static)
    other = torch.from_numpy(L.inputs(*L.CASES[0], seed=7)[0]).cuda()
    assert not torch.equal(other, pred)
    ref1 = run(train.LpLoss("rel1", WEIGHTS), off, other, tgt, terms=False)
    for src, ref in ((pred, ref0), (other, ref1), (pred, ref0)):
        with torch.no_grad():
            static.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(loss.detach()), bits(ref[0])) and torch.equal(bits(dpred), bits(ref[2]))
    assert not torch.equal(bits(ref0[0]), bits(ref1[0]))


# ------------------------------------------------------------------ fit, evaluate_table
MODEL2 = U.SMALL[:3] + (2,) + U.SMALL[4:]            # U.SMALL with two output channels: the weights [1, 2] need two
FIT_WEIGHTS = [1, 2]


def model2(seed=0):
    torch.manual_seed(seed)
    return GNOT(*MODEL2).cuda()


def loaders():
    """four train meshes in two batches; three test meshes in batches of two and one (a short last batch)"""
    if "loaders" not in _CACHE:
        rng = np.random.default_rng(5)
        mk_s = lambda k: [data.synthetic_sample(rng, int(rng.integers(40, 120)), out_dim=2,
                                                fn_points=(int(rng.integers(10, 30)),)) for _ in range(k)]
        mk = lambda s: list(torch.utils.data.DataLoader(data.NS2dData(s), batch_size=2, shuffle=False,
                                                        collate_fn=data.collate_packed))
        _CACHE["loaders"] = mk(mk_s(4)), mk(mk_s(3))
    return _CACHE["loaders"]


@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """fit(LpLoss('rel1', [1, 2]), epochs=2, state_path=p), uninterrupted: (p, histories, final flat parameters)"""
    path = os.path.join(tmp_path_factory.mktemp("lp_state"), "p.pt")
    model, (tr, te) = model2(), loaders()
    hist = train.fit(model, tr, te, epochs=2, loss_fn=train.LpLoss("rel1", FIT_WEIGHTS), state_path=path,
                     log=lambda msg: None)
    return path, hist, U.flat_params(model).clone()


def test_fit_is_the_hand_written_loop_bitwise(finished):
    _, (hist_train, hist_test), flat_fit = finished
    tr, _ = loaders()
    dev = torch.device("cuda")
    ref = model2()
    flat = train.flatten_parameters(ref)
    sched = train.OneCycle(1e-3, 2, len(tr))
    opt = train.FlatAdamW(flat, lr=1e-3, schedule=sched)
    eng = ref.engine()
    eng.param_grads = False
    loss_fn, epochs = train.LpLoss("rel1", FIT_WEIGHTS), []
    for _ in range(2):
        losses = []
        for batch in tr:
            pred, off, y = train._forward_batch(ref, batch, dev)
            loss = loss_fn(off, pred, y)
            loss.backward()
            opt.step(eng.grad_flat)
            losses.append(float(loss.detach()))
        sched.step()
        epochs.append(sum(losses) / len(losses))
    assert hist_train == epochs and len(hist_test) == 2
    assert torch.equal(bits(U.flat_params(ref)), bits(flat_fit))
    assert train.load_training_state(finished[0])["args"]["loss"] == "LpLoss(rel1, w=[1.0, 2.0])"
    # another loss is another run: rel2 with the same weights ends elsewhere
    other = model2()
    train.fit(other, tr, None, epochs=2, loss_fn=train.LpLoss("rel2", FIT_WEIGHTS), log=lambda msg: None)
    assert not torch.equal(bits(U.flat_params(other)), bits(flat_fit))


def test_resume_refuses_another_loss_and_continues_its_own(finished, tmp_path):
    _, ref_hist, ref_flat = finished
    tr, te = loaders()
    q = os.path.join(tmp_path, "q.pt")
    lines = []

    def log(msg):
        lines.append(msg)
        if sum(", Loss" in l for l in lines) == 2:         # in epoch 1: epoch 0's state is on disk
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(model2(), tr, te, epochs=2, loss_fn=train.LpLoss("rel1", FIT_WEIGHTS), state_path=q, log=log)
    assert train.load_training_state(q)["next_epoch"] == 1
    quiet = lambda msg: None
    for other in (train.LpLoss("rel2"), train.LpLoss("rel1"), train.LpLoss("rel1", [2, 1]), train.RelL2Loss()):
        with pytest.raises(ValueError, match="loss="):
            train.fit(model2(), tr, te, epochs=2, loss_fn=other, state_path=q, resume=True, log=quiet)
    model = model2(seed=123)
    hist = train.fit(model, tr, te, epochs=2, loss_fn=train.LpLoss("rel1", FIT_WEIGHTS), state_path=q, resume=True,
                     log=quiet)
    assert hist == ref_hist and torch.equal(bits(U.flat_params(model)), bits(ref_flat))


def test_a_state_file_of_an_existing_loss_still_resumes(tmp_path):
    """RelL2Loss has no trajectory_name: its state files keep the class name and resume as before"""
    tr, te = loaders()
    q = os.path.join(tmp_path, "q.pt")
    quiet = lambda msg: None
    train.fit(model2(), tr, te, epochs=1, state_path=q, log=quiet)
    assert train.load_training_state(q)["args"]["loss"] == "RelL2Loss"
    assert len(train.fit(model2(), tr, te, epochs=1, state_path=q, resume=True, log=quiet)[0]) == 1


def test_evaluate_table_rows_and_fit_log_components():
    tr, te = loaders()
    dev = torch.device("cuda")
    model = model2()
    assert [len(b["x_off"]) - 1 for b in te] == [2, 1]
    for kind in ("rel2", "linf"):
        table = train.evaluate_table(model, te, kind)
        assert table.shape == (3, 2) and table.device.type == "cpu" and table.dtype == torch.float32
        rows = []
        with torch.no_grad():
            for batch in te:
                pred, off, y = train._forward_batch(model, batch, dev)
                rows.append(L.terms(kind, pred.cpu().numpy(), y.cpu().numpy(), off))
        ref = np.concatenate(rows)
        assert len({round(float(v), 6) for v in ref[:, 0]}) == 3               # a swapped row would show
        assert float((np.abs(table.double().numpy() - ref) / ref).max()) <= 1e-5
    # the scalar metric is main.py's mean over batches of batch means, untouched
    table = train.evaluate_table(model, te)
    per_batch = [table[:2].double().mean(), table[2:].double().mean()]
    want = float(sum(per_batch) / 2)
    assert abs(train.evaluate(model, te) - want) <= 1e-6 * want
    # fit(log_components=True): the column means over all samples, from the metric's own forwards
    plain, lines = model2(), []
    hist_plain = train.fit(plain, tr, te, epochs=1, log=lambda msg: None)
    logged = model2()
    hist = train.fit(logged, tr, te, epochs=1, log=lines.append, log_components=True)
    assert hist == hist_plain and torch.equal(bits(U.flat_params(logged)), bits(U.flat_params(plain)))
    means = train.evaluate_table(logged, te).double().mean(0).tolist()
    assert lines == [f"Epoch 0, Loss: {hist[0][0]}", f"Epoch 0, Test Metric: {hist[1][0]}",
                     f"Epoch 0, Test Metric per component: {means}"]
    assert abs(sum(means) / 2 - hist[1][0]) > 0                              # a short last batch: not the scalar metric
    silent = []
    train.fit(model2(), tr, None, epochs=1, log=silent.append, log_components=True)
    assert silent == [f"Epoch 0, Loss: {hist[0][0]}"]                        # no test loader: nothing more
