"""The weight EMA on the CPU: the argument checks of gnot_ema_update and gnot_adamw_step_ema (they return
before any launch, so dummy device pointers are enough), WeightEMA's weight schedule and its argument check,
and the training-state file with an average inside the optimizer state."""
import os

import pytest
import torch

from gnot_amd import _lib, train

DUMMY = 0x1000      # a non-null "device pointer": the checks must never get as far as using it
OTHER = 0x2000      # a second one: ema and param must differ


# ------------------------------------------------------------------ the C entries refuse
@pytest.mark.parametrize("n", [0, -3])
def test_ema_update_refuses_n_below_one(n):
    assert _lib.load().gnot_ema_update(DUMMY, OTHER, n, DUMMY, None) != 0


def test_ema_update_refuses_null_pointers_and_an_alias():
    lib = _lib.load()
    for k in range(3):
        ptrs = [DUMMY, OTHER, DUMMY]
        ptrs[k] = None
        assert lib.gnot_ema_update(ptrs[0], ptrs[1], 16, ptrs[2], None) != 0
    assert lib.gnot_ema_update(DUMMY, DUMMY, 16, DUMMY, None) != 0
    assert b"alias" in lib.gnot_last_error()


def _step_ema(ptrs, n=16):
    """ptrs: param, grad, exp_avg, exp_avg_sq, ema, hyper, clip, guard"""
    return _lib.load().gnot_adamw_step_ema(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], n, ptrs[5], ptrs[6], ptrs[7],
                                           None)


def _ptrs():
    return [OTHER, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY]


@pytest.mark.parametrize("n", [0, -3])
def test_ema_step_refuses_n_below_one(n):
    assert _step_ema(_ptrs(), n) != 0
    for optional in ((6, 7), (7,)):                      # the plain and the clipped form as well
        ptrs = _ptrs()
        for k in optional:
            ptrs[k] = None
        assert _step_ema(ptrs, n) != 0


def test_ema_step_refuses_null_required_pointers():
    for k in range(6):
        for optional in ((), (7,), (6, 7)):              # guarded, clipped, plain
            ptrs = _ptrs()
            ptrs[k] = None
            for j in optional:
                ptrs[j] = None
            assert _step_ema(ptrs) != 0, (k, optional)


def test_ema_step_refuses_a_guard_without_a_clip_and_an_alias():
    lib = _lib.load()
    ptrs = _ptrs()
    ptrs[6] = None
    assert _step_ema(ptrs) != 0
    assert b"guard" in lib.gnot_last_error()
    ptrs = _ptrs()
    ptrs[4] = ptrs[0]
    assert _step_ema(ptrs) != 0
    assert b"alias" in lib.gnot_last_error()


# ------------------------------------------------------------------ WeightEMA on the host
def _f32(x):
    return torch.tensor(x, dtype=torch.float64).to(torch.float32).item()


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_weight_follows_the_closed_form(decay):
    flat = torch.arange(5, dtype=torch.float32)
    warm, cold = train.WeightEMA(flat, decay), train.WeightEMA(flat, decay, warmup=False)
    assert warm.warmup is True and cold.warmup is False and warm.decay == decay
    assert torch.equal(warm.ema, flat) and warm.ema.data_ptr() != flat.data_ptr()        # a copy
    for t in (1, 2, 9, 10, 1000):
        assert warm.weight(t) == _f32(1.0 - min(decay, (1.0 + t) / (10.0 + t))), t
        assert cold.weight(t) == _f32(1.0 - decay), t
    # 2/11, 3/12 and 10/19 lie below either decay; at t = 1000 the decay itself holds for 0.9 and 0.999 alike
    assert warm.weight(1) == _f32(9.0 / 11.0) and warm.weight(9) == _f32(9.0 / 19.0)
    assert warm.weight(1000) == (_f32(1.0 - decay) if decay < 1001.0 / 1010.0 else _f32(9.0 / 1010.0))


@pytest.mark.parametrize("decay", [0, 1, -0.1, 1.5])
def test_a_decay_outside_the_open_unit_interval_raises(decay):
    with pytest.raises(ValueError, match="decay"):
        train.WeightEMA(torch.zeros(3), decay)


def test_weight_ema_state_round_trips_and_refuses_another_average():
    flat = torch.randn(11, generator=torch.Generator().manual_seed(1))
    a = train.WeightEMA(flat, 0.99, warmup=False)
    a.ema.mul_(0.5)
    state = a.state_dict()
    assert state["ema"].data_ptr() != a.ema.data_ptr() and state["decay"] == 0.99 and state["warmup"] is False
    b = train.WeightEMA(flat.clone(), 0.99)
    b.load_state_dict(state)
    assert torch.equal(b.ema, a.ema) and b.warmup is False
    with pytest.raises(ValueError, match="decay"):
        train.WeightEMA(flat.clone(), 0.9).load_state_dict(state)
    with pytest.raises(ValueError, match="numel"):
        train.WeightEMA(torch.zeros(12), 0.99).load_state_dict(state)


# ------------------------------------------------------------------ the training-state file
class _Opt:
    """stands in for FlatAdamW(ema_decay=...) (which needs a GPU): its state_dict() with an "ema" entry"""

    def __init__(self):
        g = torch.Generator().manual_seed(4)
        self.state = {"exp_avg": torch.randn(37, generator=g), "exp_avg_sq": torch.rand(37, generator=g), "t": 9,
                      "skipped": 0, "numel": 37, "lr": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8,
                      "weight_decay": 1e-2, "max_grad_norm": None, "skip_nonfinite": False,
                      "ema": train.WeightEMA(torch.randn(37, generator=g), 0.999).state_dict()}

    def state_dict(self):
        return self.state


ARGS = dict(epochs=4, lr=1e-3, steps_per_epoch=3, accum_steps=1, per_epoch_schedule=True, max_grad_norm=None,
            loss="RelL2Loss", skip_nonfinite=False)


def test_training_state_with_an_average_round_trips_under_weights_only(tmp_path):
    path = os.path.join(tmp_path, "state.pt")
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))
    opt, sched = _Opt(), train.OneCycle(1e-3, 4, 3)
    ema_args = dict(ema_decay=0.999, ema_warmup=True)
    train.save_training_state(path, model, opt, sched, 2, 0.25, [0.5, 0.4], [0.6, 0.3], ARGS, None, ema_args)
    torch.load(path, map_location="cpu", weights_only=True)         # tensors and plain values only
    state = train.load_training_state(path)
    assert state["ema_args"] == ema_args
    assert state["args"] == ARGS and set(ARGS) == set(train.TRAJECTORY_ARGS)         # the two stay apart
    got, ref = state["optimizer"]["ema"], opt.state["ema"]
    assert set(got) == {"ema", "decay", "warmup", "numel"}
    assert torch.equal(got["ema"].view(torch.int32), ref["ema"].view(torch.int32))
    assert got["decay"] == 0.999 and got["warmup"] is True and got["numel"] == 37
    for k, v in model.state_dict().items():
        assert torch.equal(state["model"][k], v)
    # without the option the entry is absent (or None)
    train.save_training_state(path, model, opt, sched, 2, 0.25, [0.5, 0.4], [0.6, 0.3], ARGS)
    assert train.load_training_state(path).get("ema_args") is None
