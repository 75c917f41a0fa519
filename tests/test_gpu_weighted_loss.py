"""Per-point weights on the GPU: gnot_lp_loss_weighted through train.LpLoss(point_weights=) against the float64
reference of weighted_util at the bar of test_gpu_lp_loss.py (1e-5 relative); the three contracts -- all ones give
the unweighted bits, a power-of-two scale changes no bit, a row of weight zero is never read --; determinism and one
graph capture; guard floats; gnot_channel_stats_weighted against float64 at normalize_util's bars; the weights of a
DeviceLoader's batches; and fit end to end.

Sizes: lp_util.CASES.  Weights (weighted_util.weights): about a quarter exact zeros, the rest U(0.1, 3); the
`empty_head` case has rows 0..2047 of the 2049-row sample all zero -- a whole empty split, and a sample whose only
weighted row is its last."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lp_util as L
import train_step_util as U
import weighted_util as W
from gnot_amd import GNOT, Normalizer, _lib, data, train
from normalize_util import stats_bars, stats_inputs
from test_gpu_lp_loss import WEIGHTS, case, normalizer, physical
from train_step_util import bits

pytestmark = pytest.mark.gpu

PAD = U.PAD
# (case of lp_util.CASES, empty_head)
WCASES = [(0, False), (1, False), (0, True)]
_W = {}


def weights(i, empty_head=False):
    """(device, numpy) weights of case i, drawn once"""
    if (i, empty_head) not in _W:
        w = W.weights(L.CASES[i][0], empty_head=empty_head)
        _W[i, empty_head] = (torch.from_numpy(w).cuda(), w)
    return _W[i, empty_head]


def run(fn, off, pred, tgt, w, grad=True, terms=True):
    """(loss, terms or None, dpred or None) of one pass of the LpLoss fn; w None: the unweighted call"""
    kw = {} if w is None else {"point_weights": w}
    p = pred.clone().requires_grad_(grad)
    if terms:
        loss, e = fn.loss_and_terms(off, p, tgt, **kw)
    else:
        loss, e = fn(off, p, tgt, **kw), None
    if grad:
        loss.backward()
    return loss.detach(), e, p.grad


def same(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("with_nz", [False, True], ids=["raw", "normalizer"])
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("i,empty_head", WCASES)
def test_loss_terms_and_gradient_against_float64(i, empty_head, kind, with_nz):
    off, pred, tgt, pred_np, tgt_np = case(i)
    w, w_np = weights(i, empty_head)
    C = pred.shape[1]
    nz = normalizer(C) if with_nz else None
    p64 = physical(pred_np, nz)
    differentiable = kind in L.DIFFERENTIABLE
    for cw in (None, WEIGHTS[:C]):
        loss, e, dpred = run(train.LpLoss(kind, cw, nz), off, pred, tgt, w, grad=differentiable)
        ref_e = W.terms(kind, p64, tgt_np, off, w_np)
        ref = W.loss(kind, p64, tgt_np, off, w_np, cw)
        err_e = float((np.abs(e.double().cpu().numpy() - ref_e) / ref_e).max())
        print(f"case {i} empty_head={empty_head} {kind} nz={with_nz} cw={cw}: loss {float(loss):.9g} ref {ref:.9g} "
              f"rel {abs(float(loss) - ref) / ref:.2e}, terms rel {err_e:.2e}")
        assert abs(float(loss) - ref) <= 1e-5 * ref
        assert e.shape == (len(off) - 1, C) and err_e <= 1e-5
        if not differentiable:
            assert dpred is None
            continue
        ref_g = W.grad(kind, p64, tgt_np, off, w_np, cw)
        if nz is not None:
            ref_g = ref_g * nz.y.double().numpy()[1]
        g = dpred.double().cpu().numpy()
        assert (g[w_np == 0] == 0).all()
        if kind in ("rel1", "l1"):
            # sign(d) of an fp32 d next to zero may differ from float64's: leave those elements out
            on = w_np > 0
            keep = np.abs(p64 - tgt_np) >= 1e-6
            left_out = 1.0 - keep[on].mean()
            print(f"    left out {left_out:.2e} of the weighted elements")
            assert left_out < 0.01
            g, ref_g = g * keep, ref_g * keep
        err_g = float(np.linalg.norm(g - ref_g) / np.linalg.norm(ref_g))
        print(f"    dpred norm-wise rel {err_g:.2e}")
        assert err_g <= 1e-5


# ------------------------------------------------------------------ 2. all ones: the unweighted bits
@pytest.mark.parametrize("with_nz", [False, True], ids=["raw", "normalizer"])
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("i", range(len(L.CASES)))
def test_ones_give_the_bits_of_the_unweighted_call(i, kind, with_nz):
    off, pred, tgt, _, _ = case(i)
    C = pred.shape[1]
    nz = normalizer(C) if with_nz else None
    ones = torch.ones(pred.shape[0], device="cuda")
    grad = kind in L.DIFFERENTIABLE
    for cw in (None, WEIGHTS[:C]):
        ref = run(train.LpLoss(kind, cw, nz), off, pred, tgt, None, grad=grad)
        got = run(train.LpLoss(kind, cw, nz), off, pred, tgt, ones, grad=grad)
        assert same(ref, got), (cw, float(ref[0]), float(got[0]))
        assert same(ref, run(train.LpLoss(kind, cw, nz), off, pred, tgt, ones[:, None], grad=grad))      # [rows, 1]
    # RelL2Loss / MSELoss take the keyword too
    for k, cls in (("rel2", train.RelL2Loss), ("mse", train.MSELoss)):
        if kind == k:
            ref = run(cls(nz), off, pred, tgt, None, terms=False)
            assert same(ref, run(cls(nz), off, pred, tgt, ones, terms=False))
            assert float(ref[2].abs().max()) > 0


# ------------------------------------------------------------------ 3. a power of two per sample: no bit moves
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("i,empty_head", WCASES)
def test_power_of_two_scales_change_no_bit(i, empty_head, kind):
    off, pred, tgt, _, _ = case(i)
    w, _ = weights(i, empty_head)
    C = pred.shape[1]
    grad = kind in L.DIFFERENTIABLE
    factors = [4.0, 0.25, 4.0][:len(off) - 1]
    scaled = w.clone()
    for b, f in enumerate(factors):
        scaled[off[b]:off[b + 1]] *= f
    assert not torch.equal(scaled, w)
    for cw, nz in ((None, None), (WEIGHTS[:C], normalizer(C))):
        ref = run(train.LpLoss(kind, cw, nz), off, pred, tgt, w, grad=grad)
        assert same(ref, run(train.LpLoss(kind, cw, nz), off, pred, tgt, scaled, grad=grad))
        assert same(ref, run(train.LpLoss(kind, cw, nz), off, pred, tgt, w * 0.25, grad=grad))


# ------------------------------------------------------------------ 4. masks
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("i,empty_head", WCASES)
def test_rows_of_weight_zero_are_never_read(i, empty_head, kind):
    off, pred, tgt, _, _ = case(i)
    w, _ = weights(i, empty_head)
    C = pred.shape[1]
    grad = kind in L.DIFFERENTIABLE
    off_rows = w == 0
    assert 0.15 < float(off_rows.float().mean())
    bad_p, bad_t = pred.clone(), tgt.clone()
    idx = torch.nonzero(off_rows).flatten()
    bad_p[idx[0::3]], bad_t[idx[0::3]] = float("nan"), float("inf")
    bad_p[idx[1::3]], bad_t[idx[1::3]] = float("inf"), float("nan")
    bad_p[idx[2::3]], bad_t[idx[2::3]] = float("-inf"), float("nan")
    for cw, nz in ((None, None), (WEIGHTS[:C], normalizer(C))):
        ref = run(train.LpLoss(kind, cw, nz), off, pred, tgt, w, grad=grad)
        got = run(train.LpLoss(kind, cw, nz), off, bad_p, bad_t, w, grad=grad)
        assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[1]).all())
        assert same(ref, got)
        if grad:
            assert torch.equal(got[2][off_rows], torch.zeros_like(got[2][off_rows]))         # exact zeros
            assert not bool(torch.signbit(got[2][off_rows]).any())
            assert float(got[2][~off_rows].abs().max()) > 0


# ------------------------------------------------------------------ 5. determinism, capture
@pytest.mark.parametrize("kind", L.KINDS)
def test_two_runs_give_equal_bits(kind):
    for i, empty_head in WCASES:
        off, pred, tgt, _, _ = case(i)
        w, _ = weights(i, empty_head)
        cw = WEIGHTS[:pred.shape[1]]
        a = run(train.LpLoss(kind, cw), off, pred, tgt, w, grad=kind in L.DIFFERENTIABLE)
        b = run(train.LpLoss(kind, cw), off, pred, tgt, w, grad=kind in L.DIFFERENTIABLE)
        assert same(a, b)


def test_captured_weighted_rel2_replays_to_the_eager_bits():
    off, pred, tgt, _, _ = case(0)
    w, _ = weights(0)
    fn = train.LpLoss("rel2")
    ref = run(train.LpLoss("rel2"), off, pred, tgt, w, terms=False)
    static = pred.clone().requires_grad_(True)
    fn(off, static, tgt, point_weights=w).backward()      # eager once: geometry, kernels
    static.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = fn(off, static, tgt, point_weights=w)
        (dpred,) = torch.autograd.grad(loss, static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(loss.detach()), bits(ref[0])) and torch.equal(bits(dpred), bits(ref[2]))


# ------------------------------------------------------------------ 6. guard floats
@pytest.mark.parametrize("kind", L.KINDS)
def test_nothing_is_written_behind_work_terms_and_dpred(kind):
    lib = _lib.load()
    off, pred, tgt, _, _ = case(0)
    w, _ = weights(0, True)
    B, (rows, C) = len(off) - 1, pred.shape
    oh = (ctypes.c_int64 * (B + 1))(*off)
    off_dev = torch.tensor(off, dtype=torch.int64, device="cuda")
    nw = lib.gnot_lp_loss_weighted_work_floats(oh, B, C)
    full = lambda n: torch.full((n + 1,), PAD, dtype=torch.float32, device="cuda")
    work, terms, dpred, loss = full(nw), full(B * C), full(rows * C), full(1)
    grad = kind in L.DIFFERENTIABLE
    _lib.check(lib.gnot_lp_loss_weighted(pred.data_ptr(), tgt.data_ptr(), w.data_ptr(), off_dev.data_ptr(), oh, B, C,
                                         _lib.LP_KINDS[kind], None, None, work.data_ptr(), loss.data_ptr(),
                                         terms.data_ptr(), dpred.data_ptr() if grad else None, U.stream()))
    torch.cuda.synchronize()
    assert float(work[nw]) == PAD and float(terms[B * C]) == PAD and float(dpred[rows * C]) == PAD
    assert float(loss[1]) == PAD
    ref = run(train.LpLoss(kind), off, pred, tgt, w, grad=grad)
    assert torch.equal(bits(loss[0]), bits(ref[0])) and torch.equal(bits(terms[:B * C].view(B, C)), bits(ref[1]))
    if grad:
        assert torch.equal(bits(dpred[:rows * C].view(rows, C)), bits(ref[2]))
    else:
        assert bool((dpred == PAD).all())


# ------------------------------------------------------------------ 7. weighted statistics
def _stats_weighted(src, w, eps=1e-8):
    lib = _lib.load()
    rows, C = src.shape
    nw = lib.gnot_channel_stats_weighted_work_floats(rows, C)
    work = torch.full((nw + 1,), PAD, dtype=torch.float32, device="cuda")
    stats = torch.full((3 * C + 1,), PAD, dtype=torch.float32, device="cuda")
    _lib.check(lib.gnot_channel_stats_weighted(src.data_ptr(), w.data_ptr(), rows, C, eps, work.data_ptr(),
                                               stats.data_ptr(), U.stream()))
    torch.cuda.synchronize()
    assert float(work[nw]) == PAD and float(stats[3 * C]) == PAD
    return stats[:3 * C].reshape(3, C).cpu()


def _stats_weights(rows, mode):
    rng = np.random.default_rng(7 + rows)
    if mode == "ones":
        return np.ones(rows, np.float32)
    w = (rng.uniform(0.1, 3.0, rows) * (rng.random(rows) >= 0.25)).astype(np.float32)
    w[-1] = 0.7
    if mode == "empty_slice" and rows > 4096:
        w[:4096] = 0.0                     # a first slice without a weighted row: skipped in the merge
    return w


@pytest.mark.parametrize("mode", ["ones", "mixed", "empty_slice"])
@pytest.mark.parametrize("rows", [1, 4097, 70001])
def test_channel_stats_weighted_against_float64(rows, mode):
    x = stats_inputs(rows)
    w = _stats_weights(rows, mode)
    bad = x.copy()
    bad[w == 0] = np.nan                   # rows of weight zero are not read
    got = _stats_weighted(torch.from_numpy(bad).cuda(), torch.from_numpy(w).cuda())
    again = _stats_weighted(torch.from_numpy(bad).cuda(), torch.from_numpy(w).cuda())
    assert torch.equal(bits(got), bits(again))
    got = got.numpy()
    assert np.isfinite(got).all()
    assert got[0, 2] == np.float32(3.7) and got[1, 2] == 0 and got[2, 2] == 1      # the constant channel, exactly
    if int((w > 0).sum()) == 1:
        r = int(np.flatnonzero(w > 0)[0])
        assert (got[0] == x[r]).all() and (got[1] == 0).all() and (got[2] == 1).all()
        return
    mean64, std64 = W.stats_reference(x, w)
    bar_mean, bar_std = stats_bars(mean64, std64)
    live = [0, 1, 3, 4]
    r_mean = np.abs(got[0] - mean64)[live] / bar_mean[live]
    r_std = np.abs(got[1] - std64)[live] / bar_std[live]
    print(f"channel_stats_weighted rows={rows} {mode}: worst |mean - mean64| / bar {r_mean.max():.3f}, "
          f"worst |std - std64| / bar {r_std.max():.3f}")
    assert (r_mean <= 1).all(), r_mean
    assert (r_std <= 1).all(), r_std
    for c in live:
        assert got[2, c] == np.float32(1) / (got[1, c] + np.float32(1e-8))


def test_one_weighted_row_is_a_constant_channel():
    x = stats_inputs(4097)
    w = np.zeros(4097, np.float32)
    w[4096] = 2.5                          # alone in the second slice; the first has no weighted row
    got = _stats_weighted(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()).numpy()
    assert (got[0] == x[4096]).all() and (got[1] == 0).all() and (got[2] == 1).all()


# ------------------------------------------------------------------ 8. the loader carries the rows' weights
def _indexed_samples(with_w=True):
    """six meshes whose x[:, 0] -- and w -- hold the global row index (exact in fp32)"""
    rng = np.random.default_rng(11)
    out, r0 = [], 0
    for _ in range(6):
        s = data.synthetic_sample(rng, int(rng.integers(150, 320)), fn_points=(int(rng.integers(10, 30)),))
        n = len(s[0])
        s[0][:, 0] = np.arange(r0 + 1, r0 + n + 1)
        out.append(s + [np.arange(r0 + 1, r0 + n + 1, dtype=np.float64)] if with_w else s)
        r0 += n
    return out


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("points", [None, 100])
def test_device_loader_batches_carry_the_weights_of_their_rows(points, shuffle):
    ds = data.DeviceDataset(_indexed_samples(), "cuda", point_weights=True)
    assert ds.w_all.shape == (ds.x_all.shape[0],)
    gen = torch.Generator().manual_seed(3)
    loader = data.DeviceLoader(ds, batch_size=4, shuffle=shuffle, points_per_mesh=points, generator=gen)
    seen = 0
    for batch in loader:
        assert batch["w"].shape == (batch["x"].shape[0],) and batch["w"].dtype == torch.float32
        assert torch.equal(bits(batch["w"]), bits(batch["x"][:, 0].contiguous()))
        if points is not None:
            assert batch["x"].shape[0] == 100 * (len(batch["x_off"]) - 1)
        seen += 1
    assert seen == 2
    plain = data.DeviceDataset(_indexed_samples(False), "cuda")
    assert plain.w_all is None
    assert all("w" not in b for b in data.DeviceLoader(plain, batch_size=4))
    # a fifth entry is ignored without the flag
    assert data.DeviceDataset(_indexed_samples(), "cuda").w_all is None


# ------------------------------------------------------------------ 9. fit
def _fit_samples(mode):
    """six synthetic meshes of about 300 points: plain (4 entries), ones, or a 0/1 mask with NaN targets under it"""
    rng = np.random.default_rng(21)
    out = []
    for _ in range(6):
        s = data.synthetic_sample(rng, int(rng.integers(280, 320)), fn_points=(int(rng.integers(10, 30)),))
        keep = rng.random(len(s[0])) >= 0.3
        keep[0] = True
        if mode == "ones":
            s = s + [np.ones(len(s[0]))]
        elif mode == "mask":
            s[1] = np.where(keep[:, None], s[1], np.nan)
            s = s + [keep.astype(np.float64)]
        out.append(s)
    return out


def _model(seed=0):
    torch.manual_seed(seed)
    return GNOT(*U.SMALL).cuda()


def _host_loader(samples, weighted):
    ds = data.NS2dData(samples, point_weights=weighted)
    return list(torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=data.collate_packed))


QUIET = lambda msg: None


def test_fit_with_ones_is_the_unweighted_run_and_a_mask_is_another():
    plain, ones, mask = _model(), _model(), _model()
    h_plain = train.fit(plain, _host_loader(_fit_samples("plain"), False), None, epochs=2, log=QUIET)
    h_ones = train.fit(ones, _host_loader(_fit_samples("ones"), True), None, epochs=2, log=QUIET)
    assert h_ones == h_plain and torch.equal(bits(U.flat_params(ones)), bits(U.flat_params(plain)))
    tr = _host_loader(_fit_samples("mask"), True)
    assert all("w" in b and bool(torch.isnan(b["y"]).any()) for b in tr)
    h_mask = train.fit(mask, tr, tr, epochs=2, log=QUIET)
    assert all(np.isfinite(v) for v in h_mask[0] + h_mask[1])
    assert bool(torch.isfinite(U.flat_params(mask)).all())
    assert not torch.equal(bits(U.flat_params(mask)), bits(U.flat_params(plain)))
    # accumulated micro-batches and a second loss run on the same weighted batches
    acc = _model()
    h_acc = train.fit(acc, tr, None, epochs=2, accum_steps=2, loss_fn=train.LpLoss("l1"), log=QUIET)
    assert all(np.isfinite(v) for v in h_acc[0]) and bool(torch.isfinite(U.flat_params(acc)).all())
    # a loss without the keyword is refused, not run unweighted
    with pytest.raises(TypeError, match="point_weights"):
        train.fit(_model(), tr, None, epochs=1, loss_fn=lambda off, pred, y: pred.sum(), log=QUIET)


def test_fit_on_masked_device_data_with_a_normalizer_and_resume(tmp_path):
    ds = data.DeviceDataset(_fit_samples("mask"), "cuda", point_weights=True)
    assert bool(torch.isnan(ds.y_all).any())
    nz = Normalizer.fit(ds)
    assert all(bool(torch.isfinite(b).all()) for b in nz.blocks().values())
    mean64, std64 = W.stats_reference(ds.y_all.cpu().numpy(), ds.w_all.cpu().numpy())
    bar_mean, bar_std = stats_bars(mean64, std64)
    y = nz.y.cpu().double().numpy()
    assert (np.abs(y[0] - mean64) <= bar_mean).all() and (np.abs(y[1] - std64) <= bar_std).all()
    mk = lambda: data.DeviceLoader(ds, batch_size=2, shuffle=True, points_per_mesh=200, normalizer=nz,
                                   generator=torch.Generator().manual_seed(5))
    test = data.DeviceLoader(ds, batch_size=4, normalizer=nz)
    p = os.path.join(tmp_path, "p.pt")
    model = _model()
    hist = train.fit(model, mk(), test, epochs=2, normalizer=nz, state_path=p, log=QUIET)
    assert all(np.isfinite(v) for v in hist[0] + hist[1])
    # killed in epoch 1 and resumed: the uninterrupted run bit for bit
    q, lines = os.path.join(tmp_path, "q.pt"), []

    def log(msg):
        lines.append(msg)
        if sum(", Loss" in l for l in lines) == 2:
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(_model(), mk(), test, epochs=2, normalizer=nz, state_path=q, log=log)
    assert train.load_training_state(q)["next_epoch"] == 1
    resumed = _model(seed=9)
    loader = mk()
    hist2 = train.fit(resumed, loader, test, epochs=2, normalizer=nz, state_path=q, resume=True, log=QUIET)
    assert hist2 == hist and torch.equal(bits(U.flat_params(resumed)), bits(U.flat_params(model)))


def test_evaluate_table_is_the_weighted_terms():
    te = _host_loader(_fit_samples("mask"), True)
    model, dev = _model(), torch.device("cuda")
    for kind in ("rel2", "linf"):
        table = train.evaluate_table(model, te, kind)
        assert table.shape == (6, 1)
        rows = []
        with torch.no_grad():
            for batch in te:
                pred, off, y = train._forward_batch(model, batch, dev)
                rows.append(W.terms(kind, pred.cpu().numpy(), y.cpu().numpy(), off, batch["w"].numpy()))
        ref = np.concatenate(rows)
        assert np.isfinite(ref).all()
        assert float((np.abs(table.double().numpy() - ref) / ref).max()) <= 1e-5
    table = train.evaluate_table(model, te)
    want = float(sum(table[2 * k:2 * k + 2].double().mean() for k in range(3)) / 3)
    assert abs(train.evaluate(model, te) - want) <= 1e-6 * want
