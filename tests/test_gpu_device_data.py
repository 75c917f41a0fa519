"""Device-resident datasets on the GPU.  Every comparison is bitwise.

gnot_gather_rows against the numpy reference of test_device_data.py on an index-valued source (identity and
permuted segments, an empty one, C = 1..3, one mesh of 2^20 + 1 rows whose permutation walks a 2^22 domain),
sentinels around the destination; x and y gathered with one table stay paired; a full-resolution DeviceLoader
yields collate_packed's batches and fit's run over it is the DataLoader's; a subsampled, shuffled run stopped
after its first epoch resumes to the uninterrupted one; and fit reads nothing back per step."""
import ctypes
import os

import numpy as np
import pytest
import torch

import train_step_util as U
from gnot_amd import _lib, data, train
from test_device_data import gather_reference
from train_step_util import bits

pytestmark = pytest.mark.gpu


def _table(ns, ks, seed=0):
    """table rows for segments of ns rows laid out one behind the other in the source, ks of each taken"""
    rng = np.random.default_rng(seed)
    rows, s0, d0 = [], 0, 0
    for n, k in zip(ns, ks):
        lo, hi = (int(v) for v in rng.integers(0, 2 ** 32, size=2, dtype=np.uint64))
        rows.append([s0, n, d0, k, lo, hi])
        s0, d0 = s0 + n, d0 + k
    return rows


TABLES = {"four": ((1, 2, 65, 1000), (1, 1, 17, 1000)),
          "with_empty": ((1, 2, 0, 65, 1000, 0), (1, 1, 0, 17, 1000, 0)),
          "large": ((1048577,), (4096,))}


@pytest.mark.parametrize("name,C", [(n, C) for n in ("four", "with_empty") for C in (1, 2, 3)] + [("large", 1)])
def test_gather_rows_equals_the_reference(name, C):
    ns, ks = TABLES[name]
    table = _table(ns, ks, seed=C)
    rows_in, rows_out = sum(ns), sum(ks)
    assert rows_in <= 2 ** 24                                             # i + c/4 is exact in fp32
    src_np = (np.arange(rows_in, dtype=np.float32)[:, None] + np.arange(C, dtype=np.float32)[None, :] / 4)
    want = gather_reference(src_np, table)
    assert want.shape == (rows_out, C)
    src = torch.from_numpy(src_np).cuda()
    t_host = torch.tensor(table, dtype=torch.int64)
    t_dev = t_host.cuda()
    dst, buf = U.based(torch.full((rows_out * C,), -1.0), offset=1)
    host = (ctypes.c_int64 * t_host.numel())(*t_host.reshape(-1).tolist())
    _lib.check(_lib.load().gnot_gather_rows(src.data_ptr(), C, t_dev.data_ptr(), host, len(table), dst.data_ptr(),
                                            U.stream()))
    torch.cuda.synchronize()
    assert U.intact(dst, buf)
    got = dst.reshape(rows_out, C).cpu().numpy()
    assert np.array_equal(got, want)
    if name != "large":                                                   # a permuted segment is not the identity
        seg = got[2:19, 0]                                                # 17 of the source rows 3 .. 67
        assert len(set(seg.tolist())) == 17 and not np.array_equal(seg, 3 + np.arange(17, dtype=np.float32))


# ------------------------------------------------------------------ the loader
def _samples(k, rng, paired=False):
    """train_step_util.batches' meshes (40 to 120 points, an input function of 10 to 30 points); paired: the
    target's first channel is an exact fp32 function of the coordinates, y = 2 x0 - x1"""
    out = [data.synthetic_sample(rng, int(rng.integers(40, 120)), fn_points=(int(rng.integers(10, 30)),))
           for _ in range(k)]
    if paired:
        for s in out:
            x = s[0].astype(np.float32)
            s[1] = (np.float32(2) * x[:, :1] - x[:, 1:2]).astype(np.float64)
    return out


@pytest.fixture(scope="module")
def sets():
    """(train samples, test samples) drawn as train_step_util.batches draws them"""
    rng = np.random.default_rng(3)
    return _samples(8, rng), _samples(4, rng)


def test_x_and_y_rows_stay_paired():
    samples = _samples(5, np.random.default_rng(11), paired=True)
    ds = data.DeviceDataset(samples, "cuda")
    mk = lambda: data.DeviceLoader(ds, 2, shuffle=True, points_per_mesh=32, generator=torch.Generator().manual_seed(4))
    tables = mk().epoch_tables()
    x_all, y_all = ds.x_all.cpu().numpy(), ds.y_all.cpu().numpy()
    seen = 0
    for batch, t in zip(mk(), tables):
        x, y = batch["x"], batch["y"]
        assert batch["x_off"] == t["x_off"] and x.shape == (t["x_off"][-1], 2) and y.shape == (t["x_off"][-1], 1)
        assert all(b - a == 32 for a, b in zip(t["x_off"], t["x_off"][1:]))
        assert torch.equal(y[:, 0], 2 * x[:, 0] - x[:, 1])                           # row by row
        assert np.array_equal(x.cpu().numpy(), gather_reference(x_all, t["x"]))      # the rows the keys name
        assert np.array_equal(y.cpu().numpy(), gather_reference(y_all, t["x"]))
        for b, s in enumerate(t["samples"]):                                          # whole, and of the right mesh
            assert torch.equal(batch["theta"][b], ds.theta[s])
            assert torch.equal(batch["fns"][0][t["fn_offs"][0][b]:t["fn_offs"][0][b + 1]],
                               ds.fn_all[0][ds.fn_offs[0][s]:ds.fn_offs[0][s + 1]])
            mesh = x[t["x_off"][b]:t["x_off"][b + 1]]
            assert len({tuple(r) for r in mesh.tolist()}) == 32                      # without replacement
        seen += len(t["samples"])
    assert seen == 5


def _host_loader(samples):
    return torch.utils.data.DataLoader(data.NS2dData(samples), batch_size=2, shuffle=False,
                                       collate_fn=data.collate_packed)


def test_full_resolution_batches_are_collate_packed_bitwise(sets):
    tr, _ = sets
    host, dev = list(_host_loader(tr)), list(data.DeviceLoader(data.DeviceDataset(tr, "cuda"), 2))
    assert len(host) == len(dev) == 4
    # the dataset the existing suites train on
    for h, ref in zip(host, U.batches()[0]):
        assert torch.equal(h["x"], ref["x"])
    for h, d in zip(host, dev):
        assert set(h) == set(d)
        assert h["x_off"] == d["x_off"] and h["fn_offs"] == d["fn_offs"]
        for k in ("x", "y", "theta"):
            assert d[k].is_cuda and d[k].dtype == torch.float32 and d[k].shape == h[k].shape
            assert torch.equal(bits(d[k].cpu()), bits(h[k])), k
        assert len(d["fns"]) == len(h["fns"]) == 1
        assert torch.equal(bits(d["fns"][0].cpu()), bits(h["fns"][0]))


def test_fit_over_either_loader_is_the_same_run(sets):
    tr, te = sets
    runs = []
    for device_side in (False, True):
        if device_side:
            loaders = [data.DeviceLoader(data.DeviceDataset(s, "cuda"), 2) for s in (tr, te)]
        else:
            loaders = [_host_loader(s) for s in (tr, te)]
        model = U.model()
        hist = train.fit(model, *loaders, epochs=2, log=lambda msg: None)
        runs.append((hist, U.flat_params(model).clone()))
    (h0, p0), (h1, p1) = runs
    assert h0 == h1 and len(h0[0]) == 2 and len(h0[1]) == 2
    assert torch.equal(bits(p0), bits(p1))


# ------------------------------------------------------------------ resume
def _loaders(sets, seed):
    tr, te = sets
    return (data.DeviceLoader(data.DeviceDataset(tr, "cuda"), 2, shuffle=True, points_per_mesh=32,
                              generator=torch.Generator().manual_seed(seed)),
            data.DeviceLoader(data.DeviceDataset(te, "cuda"), 2))


def test_resumed_subsampled_fit_is_the_uninterrupted_one(sets, tmp_path):
    p, q = os.path.join(tmp_path, "p.pt"), os.path.join(tmp_path, "q.pt")
    model = U.model()
    ref_hist = train.fit(model, *_loaders(sets, 7), epochs=3, state_path=p, log=lambda msg: None)
    ref_flat = U.flat_params(model).clone()

    lines = []

    def log(msg):
        lines.append(msg)
        if sum("Test Metric" in l for l in lines) == 2:
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(U.model(), *_loaders(sets, 7), epochs=3, state_path=q, log=log)
    assert train.load_training_state(q)["next_epoch"] == 1          # stopped after epoch 1 began, epoch 0 on disk
    model = U.model(seed=123)                                        # a fresh module, and a loader seeded otherwise
    hist = train.fit(model, *_loaders(sets, 99), epochs=3, state_path=q, resume=True, log=lambda msg: None)
    assert hist == ref_hist and len(hist[0]) == 3 and len(hist[1]) == 3
    assert torch.equal(bits(U.flat_params(model)), bits(ref_flat))


# ------------------------------------------------------------------ read-backs
def _count_reads(monkeypatch, fn):
    """how many Tensor -> Python conversions of CUDA tensors fn() makes"""
    count = [0]
    for name in ("item", "__float__", "__int__", "__bool__", "tolist", "cpu"):
        orig = getattr(torch.Tensor, name)

        def wrapper(self, *a, _orig=orig, **kw):
            if self.is_cuda:
                count[0] += 1
            return _orig(self, *a, **kw)

        monkeypatch.setattr(torch.Tensor, name, wrapper)
    fn()
    monkeypatch.undo()
    return count[0]


@pytest.mark.parametrize("kw", [{}, {"accum_steps": 2}], ids=["plain", "accum"])
def test_fit_reads_back_once_per_epoch_not_per_step(monkeypatch, kw):
    rng = np.random.default_rng(21)
    te = data.DeviceLoader(data.DeviceDataset(_samples(4, rng), "cuda"), 2)
    counts = []
    for meshes in (4, 12):                                            # 2 and 6 loader batches an epoch
        tr = data.DeviceLoader(data.DeviceDataset(_samples(meshes, rng), "cuda"), 2, shuffle=True, points_per_mesh=32,
                               generator=torch.Generator().manual_seed(1))
        model = U.model()
        counts.append(_count_reads(monkeypatch, lambda: train.fit(model, tr, te, epochs=1, log=lambda msg: None, **kw)))
    assert counts[0] == counts[1], counts
    assert 1 <= counts[0] <= 4, counts                                # the epoch's losses and the evaluation's
