"""CPU-side checks of the keyed attention dropout (GNOT(..., attn_dropout=p), gnot_plan_set_dropout,
gnot_dropout_rows): the numpy Philox of tests/dropout_util.py against known answers, the threshold arithmetic,
the mask's statistics and key separation, the host-side refusals, the state entry of fit, the restored `training`
flag, and the room the masked float64 reference leaves the parity rule of the GPU cases."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dropout_util as DU
import golden_util as GU
import prenorm_util as PU

ARGS = (2, 1, 3, 2, 2, 64, 2, 64, 64, 3, 4, 2)       # d = 64, two blocks, two input functions
FIT_ARGS = dict(epochs=4, lr=1e-3, steps_per_epoch=3, accum_steps=1, per_epoch_schedule=True, max_grad_norm=None,
                loss="RelL2Loss", skip_nonfinite=False)


class _Opt:
    def state_dict(self):
        return {"exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3), "t": 3, "skipped": 0, "numel": 3, "lr": 1e-3,
                "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 1e-2, "max_grad_norm": None,
                "skip_nonfinite": False}


def test_symbols_are_exported():
    from gnot_amd import _lib, dropout
    lib = _lib.load()
    for name in ("gnot_plan_set_dropout", "gnot_plan_set_dropout_active", "gnot_dropout_rows"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert callable(dropout.dropout_rows) and callable(dropout.threshold)


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = " ".join(f"{int(w):08x}" for w in DU.philox4x32_10(counter, key))
    assert got == want


def test_philox_is_vectorised():
    c0 = np.arange(7, dtype=np.uint64)[:, None]
    c2 = np.arange(3, dtype=np.uint64)[None, :]
    w = DU.philox4x32_10((c0, 5, c2, 9), (11, 13))
    assert w[0].shape == (7, 3)
    for i in (0, 6):
        for j in (0, 2):
            one = DU.philox4x32_10((i, 5, j, 9), (11, 13))
            assert [int(a[i, j]) for a in w] == [int(a) for a in one]


def test_threshold_and_scale():
    from gnot_amd.dropout import threshold
    two32 = 2.0 ** 32
    for p, T in ((0.0, 0), (2.0 ** -33, 1), (0.5, 1 << 31), (1 - 2.0 ** -24, (1 << 32) - 256),
                 (0.1, int(math.floor(float(np.float32(0.1)) * two32 + 0.5)))):
        t, scale = threshold(p)
        assert t == T == DU.threshold(p)[0], p
        assert scale == float(np.float32(two32 / (two32 - T))) == float(DU.threshold(p)[1]), p
    assert threshold(0.1)[0] == 429496736                   # float32(0.1) = 0.100000001490116
    assert threshold(0.0)[1] == 1.0 and threshold(0.5)[1] == 2.0
    for bad in (1.0, -0.1, math.nan, math.inf, 1 - 2.0 ** -30):      # (the last one rounds to float32 1.0)
        with pytest.raises(ValueError):
            threshold(bad)


@pytest.mark.parametrize("p, seed, step", [(0.1, 1234, 1), (0.25, 1234, 0), (0.5, 7, 3)])
def test_keep_rate(p, seed, step):
    """300 points x 64 columns = 19,200 elements: |k / n - (1 - T / 2^32)| <= 5 sqrt(q (1 - q) / n).  The mask is a
    pure function of the key, so this is deterministic"""
    m = DU.mask_scale([300], [0], 64, seed, step, 0, p)
    T, scale = DU.threshold(p)
    q = 1 - T / 2.0 ** 32
    n = m.size
    k = int((m != 0).sum())
    print(f"p={p} seed={seed} step={step}: kept {k / n:.5f} of {n}, expected {q:.5f} (sigma {math.sqrt(q * (1 - q) / n):.4f})")
    assert n >= 19200 and set(np.unique(m)) == {np.float32(0), scale}
    assert abs(k / n - q) <= 5 * math.sqrt(q * (1 - q) / n)


def test_masks_differ_by_site_step_sample_and_seed():
    base = DU.random_words([40, 40], [0, 0], 64, 1234, 0, 0)
    assert np.array_equal(base, DU.random_words([40, 40], [0, 0], 64, 1234, 0, 0))       # equal keys, equal masks
    assert not np.array_equal(base[:40], base[40:])                                     # two samples
    for other in (DU.random_words([40, 40], [0, 0], 64, 1234, 0, 1),                    # two sites
                  DU.random_words([40, 40], [0, 0], 64, 1234, 1, 0),                    # two steps
                  DU.random_words([40, 40], [0, 0], 64, 1235, 0, 0),                    # two seeds
                  DU.random_words([40, 40], [0, 0], 64, 1234 + (1 << 32), 0, 0)):       # the seed's high word
        assert (other != base).mean() > 0.99
    # a rank that holds points 10 .. 39 of sample 0 and 20 .. 39 of sample 1 draws the unsharded run's words
    part = DU.random_words([30, 20], [10, 20], 64, 1234, 0, 0)
    assert np.array_equal(part, np.concatenate([base[10:40], base[60:80]]))
    # columns: a width that is no multiple of 4 is a prefix of the next quad
    assert np.array_equal(DU.random_words([40, 40], [0, 0], 61, 1234, 0, 0), base[:, :61])


def test_constructor_refusals_and_defaults():
    from gnot_amd import GNOT
    torch.manual_seed(0)
    plain = GNOT(*ARGS)
    assert plain.attn_dropout == 0.0 and plain.dropout_seed == 0
    with pytest.raises(TypeError):
        GNOT(*ARGS, 0, 0, False, 0.1)                                 # keyword only
    for bad in (1.0, -0.1, math.nan, 1.5):
        with pytest.raises(ValueError):
            GNOT(*ARGS, attn_dropout=bad)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            GNOT(*ARGS, attn_dropout=0.1, dropout_seed=bad)
    on = GNOT(*ARGS, attn_dropout=0.1, dropout_seed=5)
    ref_keys = [k for k, _ in plain.named_parameters()]
    assert list(on.state_dict()) == ref_keys == list(plain.state_dict())      # no parameter, no buffer
    assert on.dropout_state() == dict(p=0.1, seed=5, step=0)
    assert GNOT(*ARGS, attn_dropout=2.0 ** -40).attn_dropout == 0.0             # a threshold of 0 is off


def test_probe_plan_and_plan_refusals():
    from gnot_amd import GNOT, _lib
    lib = _lib.load()
    cfg = GNOT(*ARGS)._plan_cfg
    _lib.probe_plan(cfg, dropout=0.0)
    _lib.probe_plan(cfg, dropout=0.25)
    for bad in (1.0, -0.1, math.nan):
        with pytest.raises(ValueError, match="dropout"):
            _lib.probe_plan(cfg, dropout=bad)
    c = _lib.GnotConfig(**cfg)
    plan = ctypes.c_void_p()
    _lib.check(lib.gnot_plan_create(ctypes.byref(c), ctypes.byref(plan)))
    try:
        key = (ctypes.c_uint32 * 4)()
        xo = (ctypes.c_int64 * 4)(0, 129, 193, 194)
        fo = (ctypes.c_int64 * 8)(0, 17, 22, 23, 0, 17, 22, 23)
        size = lambda: lib.gnot_plan_workspace_bytes(plan)
        _lib.check(lib.gnot_plan_set_batch(plan, 3, xo, fo, 1))
        plain = size()
        assert plain > 0
        assert lib.gnot_plan_set_dropout(plan, 0.25, None) == -1 and b"key" in lib.gnot_last_error()
        assert lib.gnot_plan_set_dropout(None, 0.25, ctypes.addressof(key)) == -1
        assert lib.gnot_plan_set_dropout(plan, 1.0, ctypes.addressof(key)) == -1
        assert size() == plain                                         # a refused call changes nothing
        _lib.check(lib.gnot_plan_set_dropout(plan, 0.0, None))         # off stays off: the batch stands
        assert size() == plain
        _lib.check(lib.gnot_plan_set_dropout(plan, 0.25, ctypes.addressof(key)))
        assert size() == 0                                             # the batch is invalidated ...
        _lib.check(lib.gnot_plan_set_batch(plan, 3, xo, fo, 1))
        on = size()
        assert plain <= on <= plain + 256                              # one small table, no workspace rows
        _lib.check(lib.gnot_plan_set_dropout_active(plan, 0))          # a launch-time switch: the batch stands
        assert size() == on
        assert lib.gnot_plan_set_dropout_active(None, 0) == -1
        _lib.check(lib.gnot_plan_set_dropout(plan, 0.0, None))
        assert size() == 0
        _lib.check(lib.gnot_plan_set_batch(plan, 3, xo, fo, 1))
        assert size() == plain                                         # on, then off: a plan that never had it
    finally:
        lib.gnot_plan_destroy(plan)


def test_stand_alone_entry_refuses_bad_arguments():
    """every check returns before any launch, so dummy device pointers do"""
    from gnot_amd import _lib
    lib = _lib.load()
    D, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    call = lambda x=D, ld=64, rows=4, C=64, off=D, glo=D, B=1, key=D, site=0, p=0.25: \
        lib.gnot_dropout_rows(x, ld, rows, C, off, glo, B, key, site, p, None)
    bad = [dict(x=None), dict(off=None), dict(glo=None), dict(key=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31),
           dict(C=0), dict(C=1025), dict(ld=60), dict(C=62, ld=62), dict(ld=1 << 31), dict(x=odd), dict(B=0),
           dict(site=1 << 24), dict(p=1.0), dict(p=-0.1), dict(p=math.nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"dropout_rows" in lib.gnot_last_error(), kw


def test_state_entry_round_trip(tmp_path):
    from gnot_amd import GNOT, train
    torch.manual_seed(0)
    m = GNOT(*ARGS, attn_dropout=0.25, dropout_seed=(1 << 40) + 3)
    m.set_dropout_step(17)
    opt, sched = _Opt(), train.OneCycle(1e-3, 4, 3)
    path = str(tmp_path / "state.pt")
    train.save_training_state(path, m, opt, sched, 1, 0.5, [1.0], [2.0], FIT_ARGS, dropout=m.dropout_state())
    state = train.load_training_state(path)
    assert state["dropout"] == dict(p=0.25, seed=(1 << 40) + 3, step=17)
    fresh = GNOT(*ARGS, attn_dropout=0.25, dropout_seed=(1 << 40) + 3)
    fresh.load_dropout_state(state["dropout"])
    assert fresh.dropout_state() == m.dropout_state()
    for other in (GNOT(*ARGS, attn_dropout=0.5, dropout_seed=(1 << 40) + 3), GNOT(*ARGS, attn_dropout=0.25, dropout_seed=3),
                  GNOT(*ARGS)):
        with pytest.raises(ValueError, match="load_dropout_state"):
            other.load_dropout_state(state["dropout"])
    # fit(resume=True) under another p, another seed or without dropout: refused before any GPU work (the models
    # are on the CPU: reaching the GPU path would raise another error)
    loader = [None] * 3
    for other in (GNOT(*ARGS, attn_dropout=0.5, dropout_seed=(1 << 40) + 3), GNOT(*ARGS, attn_dropout=0.25, dropout_seed=3),
                  GNOT(*ARGS)):
        with pytest.raises(ValueError, match="dropout"):
            train.fit(other, loader, epochs=4, state_path=path, resume=True)
    train.save_training_state(path, GNOT(*ARGS), opt, sched, 1, 0.5, [1.0], [2.0], FIT_ARGS)
    assert "dropout" not in train.load_training_state(path)           # a model that does not drop: no entry
    with pytest.raises(ValueError, match="dropout"):
        train.fit(fresh, loader, epochs=4, state_path=path, resume=True)


def test_evaluate_restores_the_training_flag():
    from gnot_amd import GNOT, train
    m = GNOT(*ARGS, attn_dropout=0.25)
    seen = []

    class Loader:
        def __iter__(self):
            seen.append(m.training)         # the flag while the loader is being read
            return iter(())

    for flag in (True, False):
        m.train(flag)
        assert train.evaluate(m, Loader()) == 0
        assert m.training is flag
        assert train.evaluate_table(m, Loader()).numel() == 0
        assert m.training is flag
    assert seen == [False] * 4
    with train._eval_mode(m.train()):
        assert not m.training
    assert m.training
    with pytest.raises(ZeroDivisionError):
        with train._eval_mode(m):
            1 / 0
    assert m.training                                                 # restored on an exception too


def test_wrapper_is_restored_and_masks_the_attention_output():
    from oracle import torch_port
    plain = torch_port._attention
    cfg = PU.cfg_of("d64s")
    m = DU.model("d64s")
    xs, thetas, fns_ps, _ = PU.inputs("d64s")
    p = {k: torch.tensor(v) for k, v in PU.params64(m).items()}
    t = lambda a: torch.tensor(np.asarray(a))[None]
    run = lambda: torch_port.gnot_forward(p, cfg, t(xs[0]), t(thetas[0]), [t(f) for f in fns_ps[0]])
    before = run()
    ones = [np.ones((129, 64)), np.ones((129, 64))]
    with DU.masked_port(ones) as calls:
        assert torch_port._attention is not plain
        assert torch.equal(run(), before) and calls[0] == 2           # one block: a cross and a self call
    assert torch_port._attention is plain
    masks = DU.site_masks(cfg, PU.NS, 0)[:2]
    with DU.masked_port(masks):
        assert not torch.equal(run(), before)
    with DU.masked_port([np.zeros((129, 64))] * 2):                   # everything dropped: the experts see zeros
        dropped = run()
    assert torch.isfinite(dropped).all() and not torch.equal(dropped, before)
    with pytest.raises(ZeroDivisionError):
        with DU.masked_port(ones):
            1 / 0
    assert torch_port._attention is plain and torch.equal(run(), before)


@pytest.mark.parametrize("case", ["d64", "d40", "d30", "d256", "d320"])
def test_gpu_cases_leave_the_rule_room(case):
    """the float32 masked port against the float64 one: its own error leaves the RTOL / SLACK rule of the GPU
    cases room -- the conditions tests/test_prenorm.py asserts for its cases"""
    _, _, fx = DU.fixture(case)
    g = np.concatenate([np.ravel(fx["grads"][k]) for k in sorted(fx["grads"])])
    e = math.sqrt(sum(v * v for v in fx["e32"].values())) / np.linalg.norm(g)
    ws, wr = GU.reference_sharpness(fx["samples"])
    print(f"{case}: all-gradient e32 {e:.2e}, sharpness per sample {ws:.3f} per row {wr:.3f}")
    assert e <= GU.RTOL and ws <= 0.5 and wr <= 1.5
