"""Unit-Gaussian normalisation, on the CPU: the new library entries exist and refuse bad arguments before any
launch, Normalizer.fold against the float64 port of the reference model, the state-dict round trip, identity
blocks, the checks of fit / resume (they fire before any GPU work), and the float32 restatement of
gnot_channel_stats' scheme against the bars test_gpu_normalize.py holds the kernel to."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gnot_amd import GNOT, Normalizer, _lib, data, train
from normalize_util import (STATS_ROWS_CASES, stats_bars, stats_inputs, stats_reference, stats_restatement)
from oracle import torch_port

DUMMY = 0x1000      # a non-null "device pointer": the checks must never get as far as using it
E_INVALID = -1      # GNOT_E_INVALID (a launch that failed for want of a GPU would be GNOT_E_HIP)
NEW = ("gnot_channel_stats_work_floats", "gnot_channel_stats", "gnot_gather_rows_affine", "gnot_rel_l2_loss_affine",
       "gnot_mse_loss_affine")


# ------------------------------------------------------------------ the library's new entries
def test_library_exports_the_new_entries():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_channel_stats_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    call = lambda src=DUMMY, rows=10, C=2, eps=1e-8, work=DUMMY, stats=DUMMY: \
        lib.gnot_channel_stats(src, rows, C, eps, work, stats, None)
    for bad in (dict(src=None), dict(work=None), dict(stats=None), dict(rows=0), dict(rows=-3), dict(rows=1 << 31),
                dict(C=0), dict(eps=-1e-8), dict(eps=float("nan")), dict(eps=float("inf"))):
        assert call(**bad) == E_INVALID, bad
        assert b"channel_stats" in lib.gnot_last_error()
    assert lib.gnot_channel_stats_work_floats(0, 3) == 0 and lib.gnot_channel_stats_work_floats(5, 0) == 0
    # one {m, s, q} per slice of 4096 rows and channel
    assert lib.gnot_channel_stats_work_floats(1, 1) == 3
    assert lib.gnot_channel_stats_work_floats(4096, 5) == 15 and lib.gnot_channel_stats_work_floats(4097, 5) == 30
    assert lib.gnot_channel_stats_work_floats((1 << 31) - 1, 2) == 524288 * 6


def test_affine_entries_refuse_null_statistics_and_what_the_plain_ones_refuse():
    lib = _lib.load()
    table = (ctypes.c_int64 * 6)(0, 10, 0, 10, 0, 0)
    assert lib.gnot_gather_rows_affine(DUMMY, 2, DUMMY, table, 1, None, DUMMY, None) == E_INVALID
    assert b"gather_rows_affine" in lib.gnot_last_error()
    assert lib.gnot_gather_rows_affine(DUMMY, 0, DUMMY, table, 1, DUMMY, DUMMY, None) == E_INVALID
    bad = (ctypes.c_int64 * 6)(0, 10, 0, 11, 0, 0)          # k > n
    assert lib.gnot_gather_rows_affine(DUMMY, 2, DUMMY, bad, 1, DUMMY, DUMMY, None) == E_INVALID
    empty = (ctypes.c_int64 * 6)(0, 0, 0, 0, 0, 0)          # nothing to copy: no launch, like the plain entry
    assert lib.gnot_gather_rows_affine(DUMMY, 2, DUMMY, empty, 1, DUMMY, DUMMY, None) == 0
    off = (ctypes.c_int64 * 3)(0, 5, 9)
    for name in ("gnot_rel_l2_loss_affine", "gnot_mse_loss_affine"):
        fn = getattr(lib, name)
        assert fn(DUMMY, DUMMY, DUMMY, off, 2, 3, None, DUMMY, DUMMY, DUMMY, None) == E_INVALID
        assert b"out_stats" in lib.gnot_last_error()
        assert fn(None, DUMMY, DUMMY, off, 2, 3, DUMMY, DUMMY, DUMMY, DUMMY, None) == E_INVALID
        assert fn(DUMMY, DUMMY, DUMMY, (ctypes.c_int64 * 3)(0, 5, 3), 2, 3, DUMMY, DUMMY, DUMMY, DUMMY, None) == E_INVALID
    hole = (ctypes.c_int64 * 3)(0, 5, 5)                   # MSE refuses an empty sample, as the plain entry does
    assert lib.gnot_mse_loss_affine(DUMMY, DUMMY, DUMMY, hole, 2, 3, DUMMY, DUMMY, DUMMY, DUMMY, None) == E_INVALID
    assert b"empty sample" in lib.gnot_last_error()


# ------------------------------------------------------------------ the scheme of gnot_channel_stats, in float32 numpy
@pytest.mark.parametrize("rows", STATS_ROWS_CASES + (4096, 4097, 12289))
def test_stats_scheme_stays_within_a_quarter_of_the_bars(rows):
    """csrc/stats.hip restated operation by operation in float32 (normalize_util.stats_restatement) on the GPU
    test's inputs: a quarter of the bars the kernel is held to, so the bars leave room for nothing but the
    scheme's own rounding.  (Measured: below 0.06 of either bar at every size.)"""
    x = stats_inputs(rows)
    got = stats_restatement(x)
    mean64, std64 = stats_reference(x)
    assert got[1, 2] == 0 and got[2, 2] == 1 and got[0, 2] == np.float32(3.7)       # the constant channel, exactly
    if rows == 1:
        assert (got[1] == 0).all() and (got[2] == 1).all() and (got[0] == x[0]).all()
        return
    bar_mean, bar_std = stats_bars(mean64, std64)
    for c in (0, 1, 3, 4):
        assert abs(got[0, c] - mean64[c]) <= 0.25 * bar_mean[c], (c, got[0, c], mean64[c])
        assert abs(got[1, c] - std64[c]) <= 0.25 * bar_std[c], (c, got[1, c], std64[c])
        assert got[2, c] == np.float32(1) / (got[1, c] + np.float32(1e-8))


def test_raw_moments_would_fail_the_bar():
    """the scheme the kernel must not use: E[x^2] - E[x]^2 of raw fp32 values loses std at mean 1e4"""
    x = stats_inputs(70001)[:, 1]
    m = np.float32(x.sum(dtype=np.float32) / np.float32(len(x)))
    var = np.float32((x * x).sum(dtype=np.float32) / np.float32(len(x))) - m * m
    std64 = x.astype(np.float64).std(ddof=1)
    assert abs(np.sqrt(max(var, 0)) - std64) > 100 * 1e-5 * std64


# ------------------------------------------------------------------ Normalizer on the host
def _stats(rng, C):
    return rng.uniform(1, 10, C) * rng.choice([-1, 1], C), rng.uniform(1, 10, C)


def _normalizer(rng, in_dim, th_dim, out_dim, fn_dims):
    return Normalizer.from_stats(_stats(rng, in_dim), _stats(rng, th_dim), _stats(rng, out_dim),
                                 [_stats(rng, f) for f in fn_dims])


@pytest.mark.parametrize("I,th_dim", [(1, 2), (0, 2), (1, 1), (2, 1)])
def test_fold_equals_decode_of_the_network_on_encoded_inputs_in_float64(I, th_dim):
    """d=32, nl=2, E=2 at default init: the folded weights on raw inputs against decode(port(encode(inputs))) of
    the unfolded ones, both through oracle/torch_port.py in float64, to 1e-12 relative"""
    rng = np.random.default_rng(7 + 10 * I + th_dim)
    in_dim, fn_dim, out_dim, nl = 2, 3, 2, 2
    torch.manual_seed(3)
    model = GNOT(in_dim, th_dim, fn_dim, out_dim, 1, 32, nl, 32, 32, 2, 4, I)
    cfg = model._cfg
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    nz = _normalizer(rng, in_dim, th_dim, out_dim, [fn_dim] * I)
    B, N, M = 2, 23, 11
    raw = lambda blk, *shape: torch.from_numpy(
        blk[0].double().numpy() + blk[1].double().numpy() * rng.standard_normal(shape + (blk.shape[1],)))
    x, theta, fns = raw(nz.x, B, N), raw(nz.theta, B), [raw(b, B, M) for b in nz.fns]
    enc = nz.encode_batch(dict(x=x, theta=theta, fns=fns))
    assert enc["x"].dtype == torch.float64
    ref = nz.decode(torch_port.gnot_forward(sd, cfg, enc["x"], enc["theta"], enc["fns"]))
    folded = nz.fold(sd, nl, dtype=torch.float64)
    assert list(folded) == list(sd) and all(folded[k].shape == sd[k].shape for k in sd)
    got = torch_port.gnot_forward(folded, cfg, x, theta, fns)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12
    # only the first Linear of each encoder and the last of `out` moved; the model is left alone
    moved = {k for k in sd if not torch.equal(folded[k], sd[k])}
    want = {f"{p}.layers.0.{w}" for p in ["x", "gating"] + [f"input_func_mlps.{i}" for i in range(I)]
            for w in ("weight", "bias")} | {f"out.layers.{2 * nl}.weight", f"out.layers.{2 * nl}.bias"}
    assert moved == want
    for k, v in model.state_dict().items():
        assert torch.equal(v.double(), sd[k])
    # the default rounds once to fp32 and loads into the module
    f32 = nz.fold(model.state_dict(), nl)
    assert all(v.dtype == torch.float32 for v in f32.values())
    GNOT(in_dim, th_dim, fn_dim, out_dim, 1, 32, nl, 32, 32, 2, 4, I).load_state_dict(f32)
    k = "x.layers.0.weight"
    assert torch.equal(f32[k], folded[k].float())


def test_fold_refuses_statistics_of_another_width():
    rng = np.random.default_rng(0)
    model = GNOT(2, 1, 3, 1, 1, 32, 2, 32, 32, 2, 4, 1)
    with pytest.raises(ValueError, match="x.layers.0"):
        _normalizer(rng, 3, 1, 1, [3]).fold(model.state_dict(), 2)
    with pytest.raises(ValueError, match="out.layers.4"):
        _normalizer(rng, 2, 1, 2, [3]).fold(model.state_dict(), 2)


def test_from_stats_follows_the_kernel_rules():
    nz = Normalizer.from_stats(([1e4, 3.7, 0.0], [1.0, 0.0, 2.0]), (0.5, 2e-7), (7.0, 3.0), [], eps=1e-8)
    f = np.float32
    assert nz.x[0].tolist() == [1e4, f(3.7), 0.0] and nz.x[1].tolist() == [1.0, 0.0, 2.0]
    assert nz.x[2].tolist() == [float(f(1) / (f(1) + f(1e-8))), 1.0, float(f(1) / (f(2) + f(1e-8)))]
    assert nz.theta[:, 0].tolist() == [0.5, 0.0, 1.0]           # std <= 1e-6 |mean|: a constant channel
    assert nz.y.shape == (3, 1) and nz.fns == []
    with pytest.raises(ValueError):
        Normalizer.from_stats(([1, 2], [1]), (0, 1), (0, 1))


def test_state_dict_round_trip_under_weights_only(tmp_path):
    rng = np.random.default_rng(1)
    nz = _normalizer(rng, 2, 1, 3, [3, 4])
    sd = nz.state_dict()
    assert set(sd) == {"x", "theta", "y", "fns"} and len(sd["fns"]) == 2
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" for t in [sd["x"], sd["theta"], sd["y"]] + sd["fns"])
    assert sd["x"].data_ptr() != nz.x.data_ptr()
    path = os.path.join(tmp_path, "nz.pt")
    torch.save(sd, path)
    back = Normalizer.from_state_dict(torch.load(path, map_location="cpu", weights_only=True), "cpu")
    assert nz.mismatch(back) is None and back.mismatch(sd) is None
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32))
               for a, b in zip(nz.blocks().values(), back.blocks().values()))
    other = Normalizer.from_state_dict(sd)
    other.fns[1][0, 2] += 1
    assert nz.mismatch(other) == "fns.1"
    other = Normalizer.from_state_dict(sd)
    other.theta[1, 0] = torch.nextafter(other.theta[1, 0], torch.tensor(100.0))          # one ulp is another run
    assert nz.mismatch(other) == "theta"
    assert nz.mismatch(Normalizer(nz.x, nz.theta, nz.y, nz.fns[:1])) == "fns"


def _batch(rng, I=1):
    items = [(torch.from_numpy(rng.standard_normal((n, 2))).float() * 50, torch.from_numpy(rng.standard_normal((n, 1))).float(),
              rng.standard_normal(1), [torch.from_numpy(rng.standard_normal((9, 3))).float() for _ in range(I)])
             for n in (5, 1, 12)]
    return data.collate_packed(items)


def test_identity_blocks_are_bitwise_no_ops():
    rng = np.random.default_rng(2)
    ident = Normalizer(Normalizer.identity(2), Normalizer.identity(1), Normalizer.identity(1), [Normalizer.identity(3)])
    assert ident.x.tolist() == [[0, 0], [1, 1], [1, 1]]
    b = _batch(rng)
    e = ident.encode_batch(b)
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(e["x"]), bits(b["x"])) and torch.equal(bits(e["theta"]), bits(b["theta"]))
    assert torch.equal(bits(e["fns"][0]), bits(b["fns"][0]))
    assert e["y"] is b["y"] and e["x_off"] is b["x_off"] and e["fn_offs"] is b["fn_offs"]
    out = torch.from_numpy(rng.standard_normal((18, 1))).float() * 1e3
    assert torch.equal(bits(ident.decode(out)), bits(out))
    # ... and real ones are the kernel's expression, each operation rounded
    nz = _normalizer(rng, 2, 1, 1, [3])
    e = nz.encode_batch(b)
    assert torch.equal(bits(e["x"]), bits((b["x"] - nz.x[0]) * nz.x[2]))
    assert torch.equal(bits(nz.decode(out)), bits(out * nz.y[1] + nz.y[0]))
    with pytest.raises(ValueError, match="packed"):
        nz.encode_batch(dict(b, counts=[5, 1, 12]))


# ------------------------------------------------------------------ fit's checks, before any GPU work
class _Opt:
    def state_dict(self):
        return {"exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3), "t": 3, "skipped": 0, "numel": 3, "lr": 1e-3,
                "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 1e-2, "max_grad_norm": None,
                "skip_nonfinite": False}


ARGS = dict(epochs=4, lr=1e-3, steps_per_epoch=3, accum_steps=1, per_epoch_schedule=True, max_grad_norm=None,
            loss="RelL2Loss", skip_nonfinite=False)


def test_resume_refusals_name_the_normalizer_entry(tmp_path):
    rng = np.random.default_rng(3)
    nz, other = _normalizer(rng, 2, 1, 1, [3]), _normalizer(rng, 2, 1, 1, [3])
    model = GNOT(2, 1, 3, 1, 1, 32, 2, 32, 32, 2, 4, 1)              # on the CPU: reaching the GPU path would raise
    loader = [_batch(rng) for _ in range(3)]
    path = os.path.join(tmp_path, "state.pt")
    save = lambda n: train.save_training_state(path, model, _Opt(), train.OneCycle(1e-3, 4, 3), 1, 0.5, [0.4], [0.5],
                                               ARGS, None, None, n)
    run = lambda n: train.fit(model, loader, epochs=4, state_path=path, resume=True, normalizer=n)
    save(nz)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert nz.mismatch(state["normalizer"]) is None
    with pytest.raises(ValueError, match=r"normalizer entry \('x' differs"):
        run(other)
    with pytest.raises(ValueError, match="has a normalizer entry, this call has no normalizer"):
        run(None)
    save(None)
    assert "normalizer" not in torch.load(path, map_location="cpu", weights_only=True)
    with pytest.raises(ValueError, match="has no normalizer entry, this call has a normalizer"):
        run(nz)


def test_fit_refuses_mismatched_normalizers_before_any_gpu_call(tmp_path):
    rng = np.random.default_rng(4)
    nz, other = _normalizer(rng, 2, 1, 1, [3]), _normalizer(rng, 2, 1, 1, [3])
    model = GNOT(2, 1, 3, 1, 1, 32, 2, 32, 32, 2, 4, 1)
    samples = [data.synthetic_sample(rng, n, fn_points=(7,)) for n in (5, 9)]
    ds = data.DeviceDataset(samples, "cpu")                            # host tensors: nothing here can launch
    plain = [_batch(rng) for _ in range(2)]
    fit = lambda *a, **k: train.fit(model, *a, epochs=1, **k)
    with pytest.raises(ValueError, match="fit: loss_fn holds no normalizer"):
        fit(plain, loss_fn=train.RelL2Loss(), normalizer=nz)
    with pytest.raises(ValueError, match="fit: loss_fn holds a normalizer, this call has none"):
        fit(plain, loss_fn=train.MSELoss(nz))
    with pytest.raises(ValueError, match=r"fit: loss_fn holds a normalizer with other statistics.*'x'"):
        fit(plain, loss_fn=train.RelL2Loss(other), normalizer=nz)
    with pytest.raises(ValueError, match="fit: train_loader holds no normalizer"):
        fit(data.DeviceLoader(ds, 2), normalizer=nz)
    with pytest.raises(ValueError, match="fit: train_loader holds a normalizer, this call has none"):
        fit(data.DeviceLoader(ds, 2, normalizer=nz))
    with pytest.raises(ValueError, match="fit: train_loader holds a normalizer with other statistics"):
        fit(data.DeviceLoader(ds, 2, normalizer=other), normalizer=nz)
    with pytest.raises(ValueError, match="fit: test_loader holds no normalizer"):
        fit(data.DeviceLoader(ds, 2, normalizer=nz), data.DeviceLoader(ds, 2), normalizer=nz)
    with pytest.raises(ValueError, match="evaluate: the loader holds a normalizer with other statistics"):
        train.evaluate(model, data.DeviceLoader(ds, 2, normalizer=other), normalizer=nz)
    with pytest.raises(ValueError, match="evaluate: loss_fn holds no normalizer"):
        train.evaluate(model, plain, train.RelL2Loss(), normalizer=nz)
    # a loader holding an equal COPY of the statistics is accepted: the next stop is the GPU-only loader
    same = Normalizer.from_state_dict(nz.state_dict())
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        train.evaluate(model, data.DeviceLoader(ds, 2, normalizer=same), normalizer=nz)
    with pytest.raises(ValueError, match="channels"):
        data.DeviceLoader(ds, 2, normalizer=_normalizer(rng, 3, 1, 1, [3]))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        Normalizer.fit(ds)
