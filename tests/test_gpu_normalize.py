"""Unit-Gaussian normalisation on the GPU: gnot_channel_stats against numpy float64, gnot_gather_rows_affine and
the _affine losses bitwise against the plain entries around torch's elementwise arithmetic, the autograd path of
RelL2Loss(normalizer=) against float64, and fit(normalizer=) end to end -- either loader, resume, the folded
checkpoint, and the untouched default."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import train_step_util as U
from gnot_amd import GNOT, Normalizer, _lib, data, train
from normalize_util import STATS_ROWS_CASES, stats_bars, stats_inputs, stats_reference
from train_step_util import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = U.PAD


# ------------------------------------------------------------------ gnot_channel_stats
def _channel_stats(src, eps=1e-8):
    """the stats block [3, C] of src (device) on the host; nothing is written behind the declared sizes"""
    lib = _lib.load()
    rows, C = src.shape
    nw = lib.gnot_channel_stats_work_floats(rows, C)
    work = torch.full((nw + 1,), PAD, dtype=torch.float32, device="cuda")
    stats = torch.full((3 * C + 1,), PAD, dtype=torch.float32, device="cuda")
    _lib.check(lib.gnot_channel_stats(src.data_ptr(), rows, C, eps, work.data_ptr(), stats.data_ptr(), U.stream()))
    torch.cuda.synchronize()
    assert float(work[nw]) == PAD and float(stats[3 * C]) == PAD
    return stats[:3 * C].reshape(3, C).cpu()


@pytest.mark.parametrize("rows", STATS_ROWS_CASES)
def test_channel_stats_against_float64(rows):
    x = stats_inputs(rows)
    got = _channel_stats(torch.from_numpy(x).cuda())
    again = _channel_stats(torch.from_numpy(x).cuda())
    assert torch.equal(bits(got), bits(again))                          # the same bits on every run
    got = got.numpy()
    mean64, std64 = stats_reference(x)
    assert got[0, 2] == np.float32(3.7) and got[1, 2] == 0 and got[2, 2] == 1      # the constant channel, exactly
    if rows == 1:
        assert (got[0] == x[0]).all() and (got[1] == 0).all() and (got[2] == 1).all()
        return
    bar_mean, bar_std = stats_bars(mean64, std64)
    live = [0, 1, 3, 4]
    r_mean = np.abs(got[0] - mean64)[live] / bar_mean[live]
    r_std = np.abs(got[1] - std64)[live] / bar_std[live]
    print(f"channel_stats rows={rows}: worst |mean - mean64| / bar {r_mean.max():.3f}, "
          f"worst |std - std64| / bar {r_std.max():.3f} (channels N(0,1), 1e4+N(0,1), U(0,8), 1e-3 N(0,1))")
    assert (r_mean <= 1).all(), r_mean
    assert (r_std <= 1).all(), r_std
    for c in live:
        assert got[2, c] == np.float32(1) / (got[1, c] + np.float32(1e-8))


@pytest.mark.parametrize("rows", [1, 257, 70001])
def test_channel_stats_of_one_channel(rows):
    x = stats_inputs(rows)[:, 1:2].copy()                               # 1e4 + N(0,1) on its own, C = 1
    got = _channel_stats(torch.from_numpy(x).cuda()).numpy()
    if rows == 1:
        assert got[:, 0].tolist() == [float(x[0, 0]), 0.0, 1.0]
        return
    mean64, std64 = stats_reference(x)
    bar_mean, bar_std = stats_bars(mean64, std64)
    assert abs(got[0, 0] - mean64[0]) <= bar_mean[0] and abs(got[1, 0] - std64[0]) <= bar_std[0]
    # the statistics of a channel do not depend on its neighbours
    assert torch.equal(bits(torch.from_numpy(got[:, 0].copy())),
                       bits(_channel_stats(torch.from_numpy(stats_inputs(rows)).cuda())[:, 1].contiguous()))


def test_normalizer_fit_uses_the_kernel_and_honours_the_flags():
    rng = np.random.default_rng(5)
    samples = _meshes(rng, 3)
    ds = data.DeviceDataset(samples, "cuda")
    nz = Normalizer.fit(ds)
    for blk, src in ((nz.x, ds.x_all), (nz.theta, ds.theta), (nz.y, ds.y_all), (nz.fns[0], ds.fn_all[0])):
        assert blk.is_cuda and blk.shape == (3, src.shape[1])
        assert torch.equal(bits(blk.cpu()), bits(_channel_stats(src)))
    part = Normalizer.fit(ds, theta=False, fns=False)
    assert part.mismatch(Normalizer(nz.x, Normalizer.identity(1), nz.y, [Normalizer.identity(3)])) is None


# ------------------------------------------------------------------ gnot_gather_rows_affine
NS = [1, 63, 64, 65, 257, 0, 40]


def _gather(src, table, stats=None):
    lib = _lib.load()
    C = src.shape[1]
    t_host = torch.tensor(table, dtype=torch.int64)
    t_dev = t_host.cuda()
    rows_out = sum(r[3] for r in table)
    dst, buf = U.based(torch.full((rows_out * C,), -1.0), offset=1)
    host = (ctypes.c_int64 * t_host.numel())(*t_host.reshape(-1).tolist())
    if stats is None:
        rc = lib.gnot_gather_rows(src.data_ptr(), C, t_dev.data_ptr(), host, len(table), dst.data_ptr(), U.stream())
    else:
        rc = lib.gnot_gather_rows_affine(src.data_ptr(), C, t_dev.data_ptr(), host, len(table), stats.data_ptr(),
                                         dst.data_ptr(), U.stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    assert U.intact(dst, buf)
    return dst.reshape(rows_out, C).clone()


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("whole", [True, False], ids=["whole", "k40"])
def test_gather_rows_affine_is_the_gather_then_torch(C, whole):
    rng = np.random.default_rng(10 * C + whole)
    table, s0, d0 = [], 0, 0
    for n in NS:
        k = n if whole else min(40, n)
        lo, hi = (int(v) for v in rng.integers(0, 2 ** 32, size=2, dtype=np.uint64))
        table.append([s0, n, d0, k, lo, hi])
        s0, d0 = s0 + n, d0 + k
    scale, shift = np.array([1.0, 8.0, 1e-3])[:C], np.array([104.0, -3.0, 1e4])[:C]
    src = torch.from_numpy((shift + scale * rng.standard_normal((s0, C))).astype(np.float32)).cuda()
    stats = _channel_stats(src).cuda().contiguous()
    plain = _gather(src, table)
    got = _gather(src, table, stats)
    assert torch.equal(bits(got), bits((plain - stats[0]) * stats[2]))
    assert float(got.abs().max()) < 10                                   # it did normalise
    assert torch.equal(bits(_gather(src, table, Normalizer.identity(C, "cuda"))), bits(plain))
    lib = _lib.load()
    host = (ctypes.c_int64 * (6 * len(table)))(*[v for r in table for v in r])
    assert lib.gnot_gather_rows_affine(src.data_ptr(), C, src.data_ptr(), host, len(table), None, got.data_ptr(),
                                       U.stream()) == -1


# ------------------------------------------------------------------ the _affine losses
def _loss_rows():
    src = open(os.path.join(ROOT, "gnot-replication_amd", "csrc", "train.hip")).read()
    return int(re.search(r"constexpr int kLossRows = (\d+);", src).group(1))


def _native_loss(name, pred, tgt, off, stats=None):
    """(loss, dpred) of the entry gnot_<name>_loss (stats None) or gnot_<name>_loss_affine on device tensors"""
    lib = _lib.load()
    B, C = len(off) - 1, pred.shape[1]
    oh = (ctypes.c_int64 * (B + 1))(*off)
    nw = getattr(lib, f"gnot_{name}_work_floats")(oh, B, C)
    work = torch.full((nw + 1,), PAD, dtype=torch.float32, device="cuda")
    loss = torch.full((2,), PAD, dtype=torch.float32, device="cuda")
    dpred, buf = U.based(torch.full((pred.numel(),), PAD), offset=1)
    off_dev = torch.tensor(off, dtype=torch.int64).cuda()
    head = (pred.data_ptr(), tgt.data_ptr(), off_dev.data_ptr(), oh, B, C)
    tail = (work.data_ptr(), loss.data_ptr(), dpred.data_ptr(), U.stream())
    if stats is None:
        _lib.check(getattr(lib, f"gnot_{name}_loss")(*head, *tail))
    else:
        _lib.check(getattr(lib, f"gnot_{name}_loss_affine")(*head, stats.data_ptr(), *tail))
    torch.cuda.synchronize()
    assert U.intact(dpred, buf) and float(work[nw]) == PAD and float(loss[1]) == PAD
    return loss[0].clone(), dpred.reshape(pred.shape).clone()


def _loss_case(C, off, seed):
    rng = np.random.default_rng(seed)
    mean, std = np.array([50.0, -3.0, 0.5])[:C], np.array([3.0, 0.25, 7.0])[:C]
    stats = Normalizer.from_stats(([0.0], [1.0]), ([0.0], [1.0]), (mean, std)).y.cuda().contiguous()
    pred = torch.from_numpy(rng.standard_normal((off[-1], C)).astype(np.float32)).cuda()
    tgt = torch.from_numpy((mean + std * rng.standard_normal((off[-1], C))).astype(np.float32)).cuda()
    return stats, pred, tgt


OFF = [0, 1, 64, 321, 321 + 4097]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name,off", [("rel_l2", OFF), ("mse", OFF), ("rel_l2", OFF[:3] + OFF[2:])],
                         ids=["rel_l2", "mse", "rel_l2_empty_sample"])
def test_affine_losses_are_the_plain_ones_on_the_denormalised_prediction(name, off, C):
    K = _loss_rows()
    assert K < 4097 < 3 * K and 4097 % K                    # the last sample crosses a split boundary
    stats, pred, tgt = _loss_case(C, off, seed=C)
    phys = pred * stats[1] + stats[0]                       # torch: the product and the sum each rounded
    ref_loss, ref_d = _native_loss(name, phys, tgt, off)
    got_loss, got_d = _native_loss(name, pred, tgt, off, stats)
    assert torch.equal(bits(got_loss), bits(ref_loss))
    assert torch.equal(bits(got_d), bits(ref_d * stats[1]))
    if len(off) == len(OFF):
        assert np.isfinite(float(got_loss)) and float(got_d.abs().max()) > 0
    # the identity block: the plain entry's bits
    ident = Normalizer.identity(C, "cuda")
    a, b = _native_loss(name, phys, tgt, off, ident), (ref_loss, ref_d)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def test_affine_mse_refuses_an_empty_sample_as_the_plain_entry_does():
    stats, pred, tgt = _loss_case(1, [0, 5, 5, 9], seed=0)
    with pytest.raises(RuntimeError, match="empty sample"):
        _native_loss("mse", pred, tgt, [0, 5, 5, 9], stats)


def _formula(kind, pred, tgt, off):
    cuts = list(zip(off[:-1], off[1:]))
    if kind == "mse":
        return torch.stack([((pred[s:e] - tgt[s:e]) ** 2).mean(0) for s, e in cuts]).mean()
    return torch.stack([(((pred[s:e] - tgt[s:e]) ** 2).sum(0) / (tgt[s:e] ** 2).sum(0)).sqrt() for s, e in cuts]).mean()


@pytest.mark.parametrize("kind", ["rel_l2", "mse"])
def test_normalised_loss_and_autograd_against_float64(kind):
    """through RelL2Loss / MSELoss(normalizer=) and autograd, against float64 autograd of the same formula on
    pred * std + mean, at the plain losses' tolerance (tests/test_gpu_train_options.py: 1e-5 relative)"""
    C, off = 3, OFF
    stats, pred, tgt = _loss_case(C, off, seed=9)
    nz = Normalizer(Normalizer.identity(2), Normalizer.identity(1), stats.cpu())     # statistics on the host: moved once
    loss_fn = (train.MSELoss if kind == "mse" else train.RelL2Loss)(nz)
    p64 = pred.double().cpu().requires_grad_(True)
    ref = _formula(kind, p64 * stats[1].double().cpu() + stats[0].double().cpu(), tgt.double().cpu(), off)
    ref.backward()
    p = pred.clone().requires_grad_(True)
    loss = loss_fn(off, p, tgt)
    (2 * loss).backward()
    g, r = p.grad.double().cpu() / 2, p64.grad
    loss, ref = float(loss.detach()), float(ref.detach())
    print(f"{kind}(normalizer): loss rel err {abs(loss - ref) / ref:.2e}, "
          f"grad rel err {float((g - r).norm() / r.norm()):.2e}")
    assert abs(loss - ref) <= 1e-5 * ref
    assert float((g - r).norm()) <= 1e-5 * float(r.norm())
    with pytest.raises(ValueError, match="channels"):
        loss_fn(off, pred[:, :2].contiguous(), tgt[:, :2].contiguous())


# ------------------------------------------------------------------ fit, end to end
def _meshes(rng, k):
    """k meshes of 150 to 300 points in NS2d layout with offsets a raw run struggles with: x in [100, 108]^2,
    y = 50 + 3 f(x), theta around 20, one input function of 50 points around 5"""
    out = []
    for _ in range(k):
        n = int(rng.integers(150, 301))
        x = 100 + 8 * rng.random((n, 2))
        theta = 20 + rng.random(1)
        f = np.sin(np.pi * (x - 100).sum(1) / 8) * (theta[0] - 19.5)
        out.append([x, (50 + 3 * f)[:, None], theta, [5 + 2 * rng.random((50, 3))]])
    return out


def _model(seed=0):
    torch.manual_seed(seed)
    return GNOT(2, 1, 3, 1, 1, 64, 2, 64, 64, 2, 4, 1).cuda()            # d=64, H=4, E=2, nl=2, L=1


def _host_loader(samples):
    return torch.utils.data.DataLoader(data.NS2dData(samples), batch_size=2, shuffle=False, collate_fn=data.collate_packed)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the data, its statistics, and the reference run: fit(normalizer=) for 2 epochs over DeviceLoaders"""
    rng = np.random.default_rng(17)
    tr, te = _meshes(rng, 8), _meshes(rng, 2)
    dtr, dte = data.DeviceDataset(tr, "cuda"), data.DeviceDataset(te, "cuda")
    nz = Normalizer.fit(dtr)
    d = tmp_path_factory.mktemp("normalize")
    state, best = os.path.join(d, "state.pt"), os.path.join(d, "best.pt")
    model = _model()
    hist = train.fit(model, data.DeviceLoader(dtr, 2, normalizer=nz), data.DeviceLoader(dte, 2, normalizer=nz), epochs=2,
                     normalizer=nz, state_path=state, checkpoint=best, log=lambda msg: None)
    return dict(tr=tr, te=te, dtr=dtr, dte=dte, nz=nz, hist=hist, flat=U.flat_params(model).clone(), state=state,
                best=best, model=model)


def test_fit_over_either_loader_is_the_same_normalised_run(world):
    w = world
    assert len(w["hist"][0]) == 2 and len(w["hist"][1]) == 2 and all(np.isfinite(w["hist"][0] + w["hist"][1]))
    model = _model()
    hist = train.fit(model, _host_loader(w["tr"]), _host_loader(w["te"]), epochs=2, normalizer=w["nz"],
                     log=lambda msg: None)
    assert hist == w["hist"]
    assert torch.equal(bits(U.flat_params(model)), bits(w["flat"]))
    # the state file holds the statistics and the unfolded weights
    st = train.load_training_state(w["state"])
    assert w["nz"].mismatch(st["normalizer"]) is None
    for k, v in w["model"].state_dict().items():
        assert torch.equal(bits(st["model"][k]), bits(v.cpu())), k


def test_resumed_normalised_fit_is_the_uninterrupted_one(world, tmp_path):
    w = world
    q = os.path.join(tmp_path, "q.pt")
    loaders = lambda: (data.DeviceLoader(w["dtr"], 2, normalizer=w["nz"]), data.DeviceLoader(w["dte"], 2, normalizer=w["nz"]))
    lines = []

    def log(msg):
        lines.append(msg)
        if sum("Test Metric" in l for l in lines) == 2:
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(_model(), *loaders(), epochs=2, normalizer=w["nz"], state_path=q, log=log)
    assert train.load_training_state(q)["next_epoch"] == 1            # killed after epoch 1 ran, epoch 0 on disk
    model = _model(seed=123)
    same = Normalizer.from_state_dict(w["nz"].state_dict(), "cuda")   # a copy of the statistics serves
    hist = train.fit(model, data.DeviceLoader(w["dtr"], 2, normalizer=same), data.DeviceLoader(w["dte"], 2, normalizer=same),
                     epochs=2, normalizer=same, state_path=q, resume=True, log=lambda msg: None)
    assert hist == w["hist"]
    assert torch.equal(bits(U.flat_params(model)), bits(w["flat"]))
    with pytest.raises(ValueError, match="has a normalizer entry"):
        train.fit(_model(), data.DeviceLoader(w["dtr"], 2), data.DeviceLoader(w["dte"], 2), epochs=2, state_path=q,
                  resume=True, log=lambda msg: None)


def test_folded_checkpoint_predicts_physical_outputs_from_raw_inputs(world):
    w = world
    sd = torch.load(w["best"], map_location="cpu", weights_only=True)
    fresh = _model(seed=5)
    assert list(sd) == list(fresh.state_dict())                        # the reference's keys and nothing else
    fresh.load_state_dict(sd)
    got = train.evaluate(fresh, data.DeviceLoader(w["dte"], 2), train.RelL2Loss())       # raw inputs, plain metric
    want = min(w["hist"][1])                                            # the epoch whose weights were kept
    print(f"folded checkpoint: metric {got!r} on raw inputs, {want!r} in the run (rel diff {abs(got - want) / want:.2e})")
    assert abs(got - want) <= 1e-4 * want
    # the unfolded final weights with the normalizer: the run's last entry, bit for bit
    assert train.evaluate(w["model"], data.DeviceLoader(w["dte"], 2, normalizer=w["nz"]), normalizer=w["nz"]) == w["hist"][1][-1]


def test_default_path_is_untouched_and_normalising_helps(world):
    w = world
    runs = []
    for device_side in (True, False):
        if device_side:
            loaders = data.DeviceLoader(w["dtr"], 2), data.DeviceLoader(w["dte"], 2)
        else:
            loaders = _host_loader(w["tr"]), _host_loader(w["te"])
        model = _model()
        runs.append((train.fit(model, *loaders, epochs=2, log=lambda msg: None), U.flat_params(model).clone()))
    (h0, p0), (h1, p1) = runs
    assert h0 == h1 and torch.equal(bits(p0), bits(p1))
    print(f"train loss after 2 epochs: normalised {w['hist'][0][-1]!r}, raw {h0[0][-1]!r}")
    assert w["hist"][0][-1] < h0[0][-1]
