"""Gradient accumulation over micro-batches, the host side (no GPU): the arena size the C ABI reports
(gnot_plan_grad_floats), the argument errors of gnot_plan_set_grad_arena and gnot_backward_ex -- all of
which return before any launch -- and the grouping / weighting arithmetic of train.fit(accum_steps=...)."""
import ctypes

import pytest

from gnot_amd import _lib, train

SMALL = (2, 1, 3, 1, 1, 32, 2, 32, 32, 2, 4, 1)        # the model of test_train.py
PADDED = (2, 1, 3, 1, 1, 100, 2, 100, 100, 2, 4, 1)    # d = 100 / 4 heads: heads of 25 padded to 28

KEYS = ("input_dim", "theta_dim", "input_func_dim", "out_dim", "n_attn_layers", "n_attn_hidden_dim",
        "n_mlp_num_layers", "n_mlp_hidden_dim", "n_input_hidden_dim", "n_expert", "n_head", "n_input_functions")


@pytest.fixture(params=[SMALL, PADDED], ids=["small", "d100_padded_heads"])
def plan(request):
    lib = _lib.load()
    cfg = _lib.GnotConfig(**dict(zip(KEYS, request.param)))
    p = ctypes.c_void_p()
    _lib.check(lib.gnot_plan_create(ctypes.byref(cfg), ctypes.byref(p)))
    yield lib, p
    lib.gnot_plan_destroy(p)


def _grad_floats_from_dims(lib, p):
    n = lib.gnot_plan_num_linears(p)
    dims = (ctypes.c_int32 * (2 * n))()
    _lib.check(lib.gnot_plan_linear_dims(p, dims))
    return sum(dims[2 * k] * dims[2 * k + 1] + dims[2 * k] for k in range(n))


def test_grad_floats_is_the_sum_over_linear_dims(plan):
    lib, p = plan
    want = _grad_floats_from_dims(lib, p)
    assert want > 0
    assert lib.gnot_plan_grad_floats(p) == want          # valid right after create: no batch set yet
    assert lib.gnot_plan_grad_floats(None) == 0


def test_grad_floats_equals_the_modules_parameter_count():
    from gnot_amd import GNOT
    for args in (SMALL, PADDED):
        m = GNOT(*args)
        assert m.grad_numel() == sum(q.numel() for q in m.parameters())


def test_set_grad_arena_and_backward_ex_argument_errors(plan):
    """The pointers are never dereferenced on the host: a host buffer stands in for device memory."""
    lib, p = plan
    n = lib.gnot_plan_grad_floats(p)
    buf = (ctypes.c_float * (n + 8))()
    base = ctypes.addressof(buf)
    base += (-base) % 16                                  # a 16-byte aligned start inside buf
    dout = (ctypes.c_float * 4)()
    INVALID, STATE = _error_codes()
    assert INVALID < 0 and STATE < 0 and INVALID != STATE
    # a short arena, a misaligned pointer
    assert lib.gnot_plan_set_grad_arena(p, base, n - 1) == INVALID
    assert lib.gnot_plan_set_grad_arena(p, base + 4, n) == INVALID
    assert b"16-byte" in lib.gnot_last_error()
    # unknown flag bits, with and without known ones
    assert lib.gnot_backward_ex(p, dout, 4, None) == INVALID
    assert lib.gnot_backward_ex(p, dout, _lib.BWD_ACCUMULATE | 16, None) == INVALID
    # accumulation into the workspace arena is refused, and the message says why
    assert lib.gnot_backward_ex(p, dout, _lib.BWD_ACCUMULATE, None) == STATE
    msg = lib.gnot_last_error().decode()
    assert "geometry" in msg and "gnot_plan_set_grad_arena" in msg
    # a good arena: accepted, invalidates the batch, and the flag then passes validation (the call fails
    # later, as gnot_backward does on a plan with no forward)
    xo = (ctypes.c_int64 * 3)(0, 300, 377)
    fo = (ctypes.c_int64 * 3)(0, 40, 80)
    _lib.check(lib.gnot_plan_set_batch(p, 2, xo, fo, 1))
    ws = lib.gnot_plan_workspace_bytes(p)
    assert ws > 0
    assert lib.gnot_plan_set_grad_arena(p, base, n) == 0
    assert lib.gnot_plan_workspace_bytes(p) == 0           # set_batch + bind again
    _lib.check(lib.gnot_plan_set_batch(p, 2, xo, fo, 1))
    assert lib.gnot_plan_workspace_bytes(p) == ws          # same workspace layout with a caller arena
    assert lib.gnot_backward_ex(p, dout, _lib.BWD_ACCUMULATE | _lib.BWD_SKIP_GRAD_COMM, None) == STATE
    assert "gnot_forward must run" in lib.gnot_last_error().decode()
    assert lib.gnot_backward(p, dout, None) == STATE
    assert lib.gnot_plan_set_grad_arena(p, None, 0) == 0   # back to the workspace arena
    assert lib.gnot_backward_ex(p, dout, _lib.BWD_ACCUMULATE, None) == STATE
    assert "geometry" in lib.gnot_last_error().decode()


def _error_codes():
    """GNOT_E_INVALID / GNOT_E_STATE as the header defines them"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gnot_hip.h")).read()
    val = lambda name: int(re.search(name + r"\s*=\s*(-?\d+)", src).group(1))
    return val("GNOT_E_INVALID"), val("GNOT_E_STATE")


def test_accum_groups_and_weights():
    groups, weights = train.accum_groups([2, 2, 2, 1], 2)
    assert groups == [[2, 2], [2, 1]]
    assert weights[0] == [0.5, 0.5]
    assert weights[1] == pytest.approx([2 / 3, 1 / 3], rel=1e-15)
    assert len(groups) == 2                                # optimizer steps per epoch
    # the schedule is sized by optimizer steps: ceil(batches / accum_steps)
    for nb, k in ((4, 2), (5, 2), (3, 4), (7, 1)):
        assert len(train.accum_groups([1] * nb, k)[0]) == -(-nb // k)
    assert all(abs(sum(w) - 1) < 1e-15 for w in weights)
    # accum_steps = 1: every batch its own group with weight 1
    assert train.accum_groups([3, 1], 1) == ([[3], [1]], [[1.0], [1.0]])
    with pytest.raises(ValueError):
        train.accum_groups([1, 2], 0)


def test_fit_rejects_bad_accum_steps():
    from gnot_amd import GNOT
    with pytest.raises(ValueError):
        train.fit(GNOT(*SMALL), [], epochs=1, accum_steps=0)


def test_refusals_need_no_gpu():
    """backward_options(accumulate=True): refused while autograd still receives .grad copies, and without a
    caller-owned arena; an arena that is too small, of another dtype or not flat is refused by set_grad_arena."""
    import torch
    from gnot_amd import GNOT
    m = GNOT(*SMALL)
    n = m.grad_numel()
    with pytest.raises(ValueError, match="at least"):
        m.set_grad_arena(torch.zeros(n - 1))
    with pytest.raises(ValueError):
        m.set_grad_arena(torch.zeros(n, dtype=torch.float64))
    with pytest.raises(ValueError):
        m.set_grad_arena(torch.zeros(2, n)[:, ::2])
    with pytest.raises(RuntimeError, match="set_grad_arena"):
        with m.backward_options(accumulate=True):
            pass
    m.set_grad_arena(torch.zeros(n))
    assert m.engine().param_grads
    with pytest.raises(RuntimeError, match="param_grads"):
        with m.backward_options(accumulate=True):
            pass
    m.engine().param_grads = False
    with m.backward_options(accumulate=True, reduce=False):
        assert m.engine().bwd_opts == {"accumulate": True, "reduce": False}
    assert m.engine().bwd_opts == {"accumulate": False, "reduce": True}
    m.set_grad_arena(None)
    assert m.engine().user_arena is None
