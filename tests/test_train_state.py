"""The non-finite step guard and the resumable training state, on the CPU: the argument checks of
gnot_grad_norm and gnot_adamw_step_guarded (they return before any launch, so dummy device pointers are
enough), OneCycle's state, the training-state file (weights_only round trip, atomic replacement) and the
host random state behind a shuffling DataLoader."""
import os

import pytest
import torch

from gnot_amd import _lib, train

DUMMY = 0x1000      # a non-null "device pointer": the checks must never get as far as using it


# ------------------------------------------------------------------ the C entries refuse
@pytest.mark.parametrize("n", [0, -3])
def test_grad_norm_refuses_n_below_one(n):
    assert _lib.load().gnot_grad_norm(DUMMY, n, DUMMY, DUMMY, DUMMY, None) != 0


def test_grad_norm_refuses_null_pointers():
    lib = _lib.load()
    for k in range(4):
        ptrs = [DUMMY] * 4
        ptrs[k] = None
        assert lib.gnot_grad_norm(ptrs[0], 16, ptrs[1], ptrs[2], ptrs[3], None) != 0


@pytest.mark.parametrize("n", [0, -3])
def test_guarded_step_refuses_n_below_one(n):
    assert _lib.load().gnot_adamw_step_guarded(DUMMY, DUMMY, DUMMY, DUMMY, n, DUMMY, DUMMY, DUMMY, None) != 0


def test_guarded_step_refuses_null_pointers():
    lib = _lib.load()
    for k in range(7):
        ptrs = [DUMMY] * 7
        ptrs[k] = None
        assert lib.gnot_adamw_step_guarded(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 16, ptrs[4], ptrs[5], ptrs[6],
                                           None) != 0


# ------------------------------------------------------------------ OneCycle
def test_onecycle_state_round_trips():
    a = train.OneCycle(2e-3, 5, 7, pct_start=0.4, div_factor=10.0, final_div_factor=1e3, base_momentum=0.8,
                       max_momentum=0.9)
    for _ in range(11):
        a.step()
    state = a.state_dict()
    assert state["last"] == 11 and state["total"] == 35 and state["max_lr"] == 2e-3
    assert all(type(v) in (int, float) for v in state.values())
    b = train.OneCycle(2e-3, 5, 7)                 # the shape arguments come from the state
    b.load_state_dict(state)
    assert b.last == 11
    for _ in range(24):
        assert a.values() == b.values()            # the same floats, not merely close
        a.step()
        b.step()


def test_onecycle_refuses_another_schedule():
    state = train.OneCycle(1e-3, 4, 3).state_dict()
    with pytest.raises(ValueError, match="total"):
        train.OneCycle(1e-3, 5, 3).load_state_dict(state)
    with pytest.raises(ValueError, match="max_lr"):
        train.OneCycle(2e-3, 4, 3).load_state_dict(state)


# ------------------------------------------------------------------ the training-state file
class _Opt:
    """stands in for FlatAdamW (which needs a GPU): tensors and plain values behind state_dict()"""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.state = {"exp_avg": torch.randn(37, generator=g), "exp_avg_sq": torch.rand(37, generator=g), "t": 9 + seed,
                      "skipped": 2, "numel": 37, "lr": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8,
                      "weight_decay": 1e-2, "max_grad_norm": None, "skip_nonfinite": True}

    def state_dict(self):
        return self.state


ARGS = dict(epochs=4, lr=1e-3, steps_per_epoch=3, accum_steps=1, per_epoch_schedule=True, max_grad_norm=None,
            loss="RelL2Loss", skip_nonfinite=True)


def _save(path, seed, loader=None):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))
    opt, sched = _Opt(seed), train.OneCycle(1e-3, 4, 3)
    sched.step()
    train.save_training_state(path, model, opt, sched, 2, float("inf") if seed == 0 else 0.25, [0.5, 0.4], [0.6, 0.3],
                              ARGS, loader)
    return model, opt, sched


def test_training_state_round_trips_under_weights_only(tmp_path):
    path = os.path.join(tmp_path, "state.pt")
    gen = torch.Generator().manual_seed(7)
    loader = torch.utils.data.DataLoader(list(range(10)), shuffle=True, generator=gen)
    gen_state = gen.get_state().clone()
    model, opt, sched = _save(path, 0, loader)
    rng = torch.get_rng_state()
    assert os.listdir(tmp_path) == ["state.pt"]                     # no temporary file is left
    torch.load(path, map_location="cpu", weights_only=True)         # tensors and plain values only
    state = train.load_training_state(path)
    assert list(state["model"].keys()) == list(model.state_dict().keys())
    for k, v in model.state_dict().items():
        assert torch.equal(state["model"][k], v)
    for k, v in opt.state.items():
        assert torch.equal(state["optimizer"][k], v) if torch.is_tensor(v) else state["optimizer"][k] == v, k
    assert state["schedule"] == sched.state_dict()
    assert state["next_epoch"] == 2 and state["best"] == float("inf")
    assert state["hist_train"] == [0.5, 0.4] and state["hist_test"] == [0.6, 0.3]
    assert state["args"] == ARGS and set(ARGS) == set(train.TRAJECTORY_ARGS)
    assert torch.equal(state["rng"]["torch"], rng) and torch.equal(state["rng"]["loader"], gen_state)
    # a loader without a generator of its own stores none
    _save(path, 0, list(range(3)))
    assert train.load_training_state(path)["rng"]["loader"] is None


class _Killed(Exception):
    pass


def test_interrupted_save_leaves_the_previous_file(tmp_path, monkeypatch):
    path = os.path.join(tmp_path, "state.pt")
    model, _, _ = _save(path, 0)
    real = torch.save

    def dies_midway(obj, f, *a, **kw):
        real(obj, f, *a, **kw)
        with open(f, "r+b") as fh:             # a torn file under the name the writer chose
            fh.truncate(10)
        raise _Killed

    monkeypatch.setattr(torch, "save", dies_midway)
    with pytest.raises(_Killed):
        _save(path, 1)
    monkeypatch.undo()
    state = train.load_training_state(path)                          # still the first save, whole
    assert state["optimizer"]["t"] == 9 and state["best"] == float("inf")
    for k, v in model.state_dict().items():
        assert torch.equal(state["model"][k], v)
    assert os.listdir(tmp_path) == ["state.pt"]


# ------------------------------------------------------------------ the random state behind the shuffle
@pytest.mark.parametrize("own_generator", [False, True], ids=["global_rng", "loader_generator"])
def test_shuffle_order_continues_after_the_saved_rng_state(own_generator):
    def loader():
        gen = torch.Generator().manual_seed(5) if own_generator else None
        return torch.utils.data.DataLoader(list(range(23)), batch_size=4, shuffle=True, generator=gen)

    epoch = lambda dl: [b.tolist() for b in dl]
    torch.manual_seed(11)
    dl = loader()
    first = [epoch(dl), epoch(dl)]
    saved = train.rng_state(dl)
    rest = [epoch(dl), epoch(dl)]                                    # the uninterrupted run
    assert rest[0] != first[0] and rest[0] != rest[1]

    torch.manual_seed(999)                                           # a new process: another state altogether
    dl2 = loader()
    torch.rand(17)
    train.restore_rng_state(saved, dl2)
    assert [epoch(dl2), epoch(dl2)] == rest
