"""Per-point weights without a GPU: the float64 reference of weighted_util against lp_util, the data format with and
without the fifth entry, every refusal the host makes, and the exported symbols."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import lp_util as L
import weighted_util as W
from gnot_amd import _lib, data, train


# ------------------------------------------------------------------ the reference checks itself
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("i", range(len(L.CASES)))
def test_reference_with_ones_is_the_unweighted_reference(i, kind):
    sizes, C = L.CASES[i]
    off = L.offsets(sizes)
    pred, tgt = L.inputs(sizes, C)
    ones = np.ones(sum(sizes), np.float32)
    cw = [1.0, 0.0, 3.0][:C]
    assert np.allclose(W.terms(kind, pred, tgt, off, ones), L.terms(kind, pred, tgt, off), rtol=1e-13, atol=0)
    assert abs(W.loss(kind, pred, tgt, off, ones, cw) - L.loss(kind, pred, tgt, off, cw)) <= 1e-13
    if kind in L.DIFFERENTIABLE:
        assert np.allclose(W.grad(kind, pred, tgt, off, ones, cw), L.grad(kind, pred, tgt, off, cw), rtol=1e-12, atol=0)


@pytest.mark.parametrize("empty_head", [False, True])
@pytest.mark.parametrize("kind", L.KINDS)
def test_reference_zero_rows_equal_the_compacted_arrays(kind, empty_head):
    sizes, C = L.CASES[0]
    off = L.offsets(sizes)
    pred, tgt = L.inputs(sizes, C)
    w = W.weights(sizes, empty_head=empty_head)
    assert 0.15 < float((w == 0).mean()) and (w >= 0).all()
    if empty_head:
        assert (w[1:2049] == 0).all() and w[2049] > 0
    bad_p, bad_t = pred.copy(), tgt.copy()
    bad_p[w == 0], bad_t[w == 0] = np.nan, np.inf          # never read
    cp, ct, coff, cw = W.compact(pred, tgt, off, w)
    e = W.terms(kind, bad_p, bad_t, off, w)
    assert np.isfinite(e).all()
    for b in range(len(sizes)):                             # sample by sample: the compacted arrays, weighted
        s = slice(coff[b], coff[b + 1])
        one = W.terms(kind, cp[s], ct[s], [0, coff[b + 1] - coff[b]], cw[s])
        assert np.allclose(e[b], one[0], rtol=1e-13, atol=0)
    if kind in ("relinf", "linf"):                          # the maxima do not see the weights at all
        assert np.allclose(e, L.terms(kind, cp, ct, coff), rtol=0, atol=0)
    if kind in L.DIFFERENTIABLE:
        g = W.grad(kind, bad_p, bad_t, off, w)
        assert (g[w == 0] == 0).all() and np.isfinite(g).all()
        assert np.allclose(g[w > 0], W.grad(kind, cp, ct, coff, cw), rtol=1e-13, atol=0)
        # the closed form against a central difference of the loss, on one weighted element
        r = int(np.flatnonzero(w > 0)[3])
        h = 1e-6
        up, dn = pred.astype(np.float64), pred.astype(np.float64)
        up[r, 0] += h
        dn[r, 0] -= h
        lu, ld = W.loss(kind, up, tgt, off, w), W.loss(kind, dn, tgt, off, w)
        fd = (lu - ld) / (2 * h)
        # the difference quotient's own float64 rounding: each loss carries a few eps of itself, divided by 2 h
        # (the truncation term, h^2 f''' / 6, is far below that for these smooth or piecewise-linear kinds)
        tol = 8 * np.finfo(np.float64).eps * max(abs(lu), abs(ld)) / (2 * h) + 1e-6 * abs(g[r, 0])
        assert abs(fd - g[r, 0]) <= tol and abs(g[r, 0]) > 100 * tol


def test_weighted_statistics_reference():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((500, 2)) + [3.0, -1.0]
    mean, std = W.stats_reference(x, np.ones(500))
    assert np.allclose(mean, x.mean(0)) and np.allclose(std, x.std(0, ddof=1))          # rows - 1 at w == 1
    w = rng.integers(0, 4, 500).astype(np.float64)                                       # integer weights repeat rows
    rep = np.repeat(x, w.astype(int), axis=0)
    mean, std = W.stats_reference(x, w)
    assert np.allclose(mean, rep.mean(0))
    v1, v2 = w.sum(), (w ** 2).sum()
    assert np.allclose(std ** 2, rep.var(0) * v1 / (v1 - v2 / v1))
    one = np.zeros(500)
    one[7] = 2.5
    mean, std = W.stats_reference(x, one)
    assert np.allclose(mean, x[7]) and (std == 0).all()


# ------------------------------------------------------------------ the data format
def _samples(k=3, with_w=True, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        s = data.synthetic_sample(rng, int(rng.integers(5, 12)), fn_points=(4,))
        if with_w:
            w = rng.uniform(0.1, 3.0, len(s[0])) * (rng.random(len(s[0])) > 0.3)
            w[0] = 1.5
            s = s + [w]
        out.append(s)
    return out


def test_data_round_trip_with_and_without_the_fifth_entry(tmp_path):
    weighted = _samples(with_w=True)
    plain = [s[:4] for s in weighted]
    # four entries: today's bytes and today's items
    p4 = str(tmp_path / "four.pkl")
    data.write_ns2d(p4, plain)
    want = pickle.dumps([[np.asarray(s[0]), np.asarray(s[1]), np.asarray(s[2]), [np.asarray(v) for v in s[3]]]
                         for s in plain], protocol=4)
    assert open(p4, "rb").read() == want
    ds4 = data.NS2dData(p4)
    assert all(len(item) == 4 for item in ds4.items)
    assert "w" not in data.collate_packed([ds4[i] for i in range(3)])
    # five entries: written, ignored without the flag, read with it
    p5 = str(tmp_path / "five.pkl")
    data.write_ns2d(p5, weighted)
    assert all(len(s) == 5 for s in data.safe_load(p5))
    ignoring = data.NS2dData(p5)
    assert all(len(item) == 4 for item in ignoring.items)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(ignoring.items, ds4.items))
    ds5 = data.NS2dData(p5, point_weights=True)
    assert all(len(item) == 5 and item[4].dtype == torch.float32 and item[4].shape == (item[0].shape[0],)
               for item in ds5.items)
    batch = data.collate_packed([ds5[i] for i in range(3)])
    plain_batch = data.collate_packed([ignoring[i] for i in range(3)])
    assert sorted(set(batch) - set(plain_batch)) == ["w"]
    assert batch["w"].shape == (batch["x"].shape[0],)
    assert torch.equal(batch["w"], torch.cat([torch.from_numpy(np.asarray(s[4])).float() for s in weighted]))
    for k in ("x", "y", "theta"):
        assert torch.equal(batch[k], plain_batch[k])
    assert batch["x_off"] == plain_batch["x_off"]
    # a [N, 1] column is taken as [N]
    col = [s[:4] + [np.asarray(s[4])[:, None]] for s in weighted]
    assert torch.equal(data.NS2dData(col, point_weights=True)[0][4], ds5[0][4])


@pytest.mark.parametrize("how,match", [("negative", "negative"), ("nan", "finite"), ("inf", "finite"),
                                        ("short", "shape"), ("zero", "zero"), ("missing", "fifth")])
def test_dataset_refuses_bad_point_weights(how, match):
    samples = _samples()
    w = np.asarray(samples[1][4]).copy()
    if how == "negative":
        w[2] = -0.5
    elif how == "nan":
        w[2] = np.nan
    elif how == "inf":
        w[2] = np.inf
    elif how == "short":
        w = w[:-1]
    elif how == "zero":
        w[:] = 0.0
    samples[1] = samples[1][:4] + ([w] if how != "missing" else [])
    with pytest.raises(ValueError, match=match):
        data.NS2dData(samples, point_weights=True)
    assert len(data.NS2dData(samples)) == 3                  # without the flag the entry is not looked at


def test_collate_padded_refuses_point_weights():
    ds = data.NS2dData(_samples(), point_weights=True)
    with pytest.raises(ValueError, match="point weights"):
        data.collate_padded([ds[0], ds[1]])
    with pytest.raises(ValueError, match="with and without"):
        data.collate_packed([ds[0], ds[1][:4]])
    assert data.collate_padded([ds[0][:4], ds[1][:4]])["x"].dim() == 3


@pytest.mark.parametrize("cls", [train.RelL2Loss, train.MSELoss, lambda: train.LpLoss("l1")])
def test_losses_refuse_a_wrong_point_weights_shape_before_any_gpu_work(cls):
    fn = cls()
    pred, tgt = torch.zeros(10, 2), torch.ones(10, 2)
    for bad in (torch.ones(9), torch.ones(10, 2), torch.ones(1, 10), torch.ones(10, dtype=torch.int64), [1.0] * 10):
        with pytest.raises(ValueError, match="point_weights"):
            fn([0, 4, 10], pred, tgt, point_weights=bad)
    # a good shape on the host gets as far as the no-GPU error of every loss
    for good in (torch.ones(10), torch.ones(10, 1, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            fn([0, 4, 10], pred, tgt, point_weights=good)
    if isinstance(fn, train.LpLoss):
        for call in (fn.loss_and_terms, fn.terms):
            with pytest.raises(ValueError, match="point_weights"):
                call([0, 4, 10], pred, tgt, point_weights=torch.ones(3))


def test_a_loss_without_the_keyword_is_refused_for_weighted_batches():
    plain = lambda off, pred, y: pred.sum()
    batch = {"w": torch.ones(3)}
    with pytest.raises(TypeError, match="point_weights"):
        train._point_weight_args(batch, "cpu", plain)
    assert train._point_weight_args({}, "cpu", plain) == {}
    kw = train._point_weight_args(batch, "cpu", train.RelL2Loss())
    assert list(kw) == ["point_weights"] and torch.equal(kw["point_weights"], batch["w"])


# ------------------------------------------------------------------ the library
def test_new_symbols_are_exported_and_refuse_on_the_host():
    lib = _lib.load()
    for name in ("gnot_lp_loss_weighted_work_floats", "gnot_lp_loss_weighted",
                 "gnot_channel_stats_weighted_work_floats", "gnot_channel_stats_weighted"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for sizes, C in L.CASES:
        B = len(sizes)
        oh = (ctypes.c_int64 * (B + 1))(*L.offsets(sizes))
        nsplit = -(-max(sizes) // 2048)
        assert lib.gnot_lp_loss_weighted_work_floats(oh, B, C) == B * nsplit * 2 * C + B * C
    assert lib.gnot_lp_loss_weighted_work_floats(None, 1, 1) == 0
    ptr = ctypes.c_void_p(4096)          # dummy device pointers: every refusal below returns before a launch
    oh = (ctypes.c_int64 * 3)(0, 4, 10)
    call = lambda pw, off, kind, dpred: lib.gnot_lp_loss_weighted(ptr, ptr, pw, ptr, off, 2, 2, kind, None, None, ptr,
                                                                  ptr, None, dpred, None)
    assert call(None, oh, 0, None) == -1 and b"point_w" in lib.gnot_last_error()
    assert call(ptr, oh, 6, None) == -1 and b"unknown kind" in lib.gnot_last_error()
    assert call(ptr, oh, 5, ptr) == -1 and b"metrics only" in lib.gnot_last_error()
    assert call(ptr, (ctypes.c_int64 * 3)(0, 4, 4), 3, None) == -1 and b"empty sample" in lib.gnot_last_error()
    assert lib.gnot_channel_stats_weighted_work_floats(0, 3) == 0
    assert lib.gnot_channel_stats_weighted_work_floats(4096, 5) == 17
    assert lib.gnot_channel_stats_weighted_work_floats(4097, 5) == 34
    for args in ((None, ptr, 5, 1, 0.0), (ptr, None, 5, 1, 0.0), (ptr, ptr, 0, 1, 0.0), (ptr, ptr, 5, 0, 0.0),
                 (ptr, ptr, 5, 1, -1.0)):
        assert lib.gnot_channel_stats_weighted(*args, ptr, ptr, None) == -1
        assert b"channel_stats_weighted" in lib.gnot_last_error()
