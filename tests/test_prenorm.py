"""CPU-side checks of the parameter-free pre-norm (GNOT(..., pre_norm=True), gnot_plan_set_pre_norm,
gnot_layer_norm / gnot_layer_norm_bwd): the exported symbols, the host-side refusals, the plan's workspace, the
state_dict rule and the reference helper of the GPU tests (tests/prenorm_util.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import golden_util as GU
import prenorm_util as PU

ARGS = (2, 1, 3, 2, 2, 64, 2, 64, 64, 3, 4, 2)       # d = 64, two blocks, two input functions


def _plan(lib, n_input_functions=2):
    from gnot_amd import _lib
    cfg = _lib.GnotConfig(input_dim=2, theta_dim=1, input_func_dim=3, out_dim=2, n_attn_layers=2,
                          n_attn_hidden_dim=64, n_mlp_num_layers=2, n_mlp_hidden_dim=64, n_input_hidden_dim=64,
                          n_expert=3, n_head=4, n_input_functions=n_input_functions)
    plan = ctypes.c_void_p()
    _lib.check(lib.gnot_plan_create(ctypes.byref(cfg), ctypes.byref(plan)))
    return plan


def _set_batch(lib, plan, training, I=2):
    from gnot_amd import _lib
    xo = (ctypes.c_int64 * 4)(0, 129, 193, 194)
    fo = (ctypes.c_int64 * (4 * max(I, 1)))(*([0, 17, 22, 23] * max(I, 1)))
    _lib.check(lib.gnot_plan_set_batch(plan, 3, xo, fo if I else None, training))
    return lib.gnot_plan_workspace_bytes(plan)


def test_symbols_are_exported():
    from gnot_amd import _lib, norm
    lib = _lib.load()
    for name in ("gnot_plan_set_pre_norm", "gnot_layer_norm", "gnot_layer_norm_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert callable(norm.layer_norm_rows) and callable(norm.layer_norm_rows_bwd)


def test_stand_alone_entries_refuse_bad_arguments():
    """every check returns before any launch, so dummy device pointers do"""
    from gnot_amd import _lib
    lib = _lib.load()
    D, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    fwd = lambda x=D, ldx=64, rows=4, C=64, eps=1e-5, y=D, ldy=64, rstd=D: \
        lib.gnot_layer_norm(x, ldx, rows, C, eps, y, ldy, rstd, None)
    bwd = lambda y=D, ldy=64, rstd=D, dy=D, lddy=64, rows=4, C=64, dx=D, lddx=64, acc=0: \
        lib.gnot_layer_norm_bwd(y, ldy, rstd, dy, lddy, rows, C, dx, lddx, acc, None)
    bad_fwd = [dict(x=None), dict(y=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(C=0), dict(C=1025),
               dict(ldx=60), dict(ldy=60), dict(C=62, ldx=62), dict(C=62, ldx=64, ldy=62), dict(ldx=1 << 31),
               dict(ldy=1 << 31), dict(x=odd), dict(y=odd), dict(rstd=odd), dict(eps=0.0), dict(eps=-1e-5),
               dict(eps=math.nan), dict(eps=math.inf)]
    for kw in bad_fwd:
        assert fwd(**kw) == -1, kw
        assert b"layer_norm" in lib.gnot_last_error(), kw
    bad_bwd = [dict(y=None), dict(rstd=None), dict(dy=None), dict(dx=None), dict(rows=0), dict(rows=1 << 31), dict(C=0),
               dict(C=1025), dict(ldy=60), dict(lddy=60), dict(lddx=60), dict(C=62, ldy=62), dict(C=62, lddy=62),
               dict(C=62, lddx=62), dict(ldy=1 << 31), dict(lddy=1 << 31), dict(lddx=1 << 31), dict(y=odd),
               dict(rstd=odd), dict(dy=odd), dict(dx=odd)]
    for kw in bad_bwd:
        assert bwd(**kw) == -1, kw
        assert b"layer_norm_bwd" in lib.gnot_last_error(), kw


def test_plan_set_pre_norm_checks_and_workspace():
    from gnot_amd import _lib
    lib = _lib.load()
    for training in (1, 0):
        plan, never = _plan(lib), _plan(lib)
        try:
            for eps in (0.0, -1.0, math.nan, math.inf):
                assert lib.gnot_plan_set_pre_norm(plan, 1, eps) == -1
                assert b"eps" in lib.gnot_last_error()
            assert lib.gnot_plan_set_pre_norm(None, 1, 1e-5) == -1
            plain = _set_batch(lib, plan, training)
            assert plain > 0 and plain == _set_batch(lib, never, training)
            assert lib.gnot_plan_set_pre_norm(plan, 1, math.nan) == -1
            assert lib.gnot_plan_workspace_bytes(plan) == plain        # a refused call changes nothing
            _lib.check(lib.gnot_plan_set_pre_norm(plan, 1, 1e-5))
            assert lib.gnot_plan_workspace_bytes(plan) == 0            # the batch is invalidated ...
            on = _set_batch(lib, plan, training)                       # ... until the next set_batch
            # 2 blocks x (n1, n2) [194, 64] + 2 x fnn [23, 64] (+ rstd rows and dnorm in training)
            assert on >= plain + 4 * 194 * 64 * 4 + 2 * 23 * 64 * 4
            if training:
                assert on >= plain + 5 * 194 * 64 * 4 + 2 * 23 * 64 * 4 + 4 * 194 * 4 + 2 * 23 * 4
            _lib.check(lib.gnot_plan_set_pre_norm(plan, 1, 1e-5))      # unchanged: the batch stands
            assert lib.gnot_plan_workspace_bytes(plan) == on
            _lib.check(lib.gnot_plan_set_pre_norm(plan, 0, 1e-5))
            assert lib.gnot_plan_workspace_bytes(plan) == 0
            assert _set_batch(lib, plan, training) == plain            # on, then off: a plan that never had it
        finally:
            lib.gnot_plan_destroy(plan)
            lib.gnot_plan_destroy(never)


def test_state_dict_rule():
    from gnot_amd import GNOT, Normalizer
    torch.manual_seed(0)
    plain, off, on = GNOT(*ARGS), GNOT(*ARGS, pre_norm=False), GNOT(*ARGS, pre_norm=True)
    with pytest.raises(TypeError):
        GNOT(*ARGS, True)                                             # keyword only
    ref_keys = [k for k, _ in plain.named_parameters()]
    assert list(plain.state_dict()) == ref_keys and list(off.state_dict()) == ref_keys
    assert [k for k, _ in on.named_parameters()] == ref_keys          # the parameter list is the reference's
    extra = [k for k in on.state_dict() if k not in ref_keys]
    assert extra == ["pre_norm_eps"] and len(on.state_dict()) == len(ref_keys) + 1
    b = on.state_dict()["pre_norm_eps"]
    assert b.dim() == 0 and b.dtype == torch.float32 and float(b) == float(np.float32(1e-5))
    with pytest.raises(RuntimeError, match="pre_norm_eps"):
        off.load_state_dict(on.state_dict())                          # unexpected key
    with pytest.raises(RuntimeError, match="pre_norm_eps"):
        on.load_state_dict(off.state_dict())                          # missing key
    on.load_state_dict(GNOT(*ARGS, pre_norm=True).state_dict())
    # Normalizer.fold copies the state dict key by key: the buffer comes through
    ident = lambda n: ([0.0] * n, [1.0] * n)
    nz = Normalizer.from_stats(([0.5, 0.5], [0.3, 0.3]), ([0.5], [0.25]), ([2.0, 1.0], [3.0, 2.0]),
                               [ident(3), ident(3)], eps=0.0)
    folded = nz.fold(on.state_dict(), 2)
    assert list(folded) == list(on.state_dict()) and torch.equal(folded["pre_norm_eps"], b)
    on.load_state_dict(folded)


def test_checkpoints_carry_the_buffer(tmp_path):
    from gnot_amd import GNOT, train
    torch.manual_seed(1)
    on, off = GNOT(*ARGS, pre_norm=True), GNOT(*ARGS)
    path = str(tmp_path / "ck.pth")
    train.save_checkpoint(on, path)
    assert "pre_norm_eps" in torch.load(path, weights_only=True)
    train.load_checkpoint(GNOT(*ARGS, pre_norm=True), path)
    with pytest.raises(RuntimeError, match="pre_norm_eps"):
        train.load_checkpoint(off, path)
    train.save_checkpoint(off, path)
    with pytest.raises(RuntimeError, match="pre_norm_eps"):
        train.load_checkpoint(on, path)


def test_model_needs_the_device():
    from gnot_amd import GNOT
    from gnot_amd.norm import layer_norm_rows
    m = GNOT(2, 1, 3, 1, 1, 64, 2, 64, 64, 3, 4, 0, pre_norm=True)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(torch.rand(1, 10, 2), torch.rand(1, 1))
    with pytest.raises(ValueError, match="ROCm"):
        layer_norm_rows(torch.rand(4, 8))


# ------------------------------------------------------------------ the helper's reference
def _port_out(case, dtype=torch.float64):
    from oracle import torch_port
    m = PU.model(case)
    xs, thetas, fns_ps, _ = PU.inputs(case)
    p = {k: torch.tensor(v, dtype=dtype) for k, v in PU.params64(m).items()}
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)[None]
    return torch_port.gnot_forward(p, PU.cfg_of(case), t(xs[0]), t(thetas[0]), [t(f) for f in fns_ps[0]])


def test_wrapper_is_restored():
    from oracle import torch_port
    plain = torch_port._attention
    before = _port_out("d64")
    with PU.pre_norm_port():
        assert torch_port._attention is not plain
        inside = _port_out("d64")
    assert torch_port._attention is plain
    assert torch.equal(_port_out("d64"), before)                      # bit-identical outside the wrapper
    assert not torch.equal(inside, before)                            # and it is another function inside
    with pytest.raises(ZeroDivisionError):
        with PU.pre_norm_port():
            1 / 0
    assert torch_port._attention is plain                             # restored on an exception too


def test_wrapper_normalises_query_and_sources():
    """one block, one input function: cross attention normalises (query, enc_0), self attention (query1)"""
    from oracle import torch_port
    seen = []
    with PU.pre_norm_port(seen=seen):
        _port_out("d64s")
    assert len(seen) == 3
    for raw, y in seen:
        want, _ = PU.ln64(raw.numpy())
        assert np.abs(y.numpy() - want).max() <= 1e-12
        assert np.abs(y.numpy().mean(-1)).max() <= 1e-12
    assert seen[0][0].shape[1] == 129 and seen[1][0].shape[1] == 17 and seen[2][0].shape[1] == 129


def test_wrapper_normalises_the_source_without_input_functions():
    """I == 0: the cross branch reads key and value from the query argument (model.py:88-104), so its source is
    normalised too -- one LN per attention call, and the plain attention sees the normalised rows on both sides"""
    from oracle import torch_port
    seen, calls = [], []
    plain = torch_port._attention
    spy = lambda p, prefix, query, srcs, *a: calls.append((prefix, query, srcs)) or plain(p, prefix, query, srcs, *a)
    torch_port._attention = spy
    try:
        with PU.pre_norm_port(seen=seen):
            _port_out("d40")
    finally:
        torch_port._attention = plain
    assert len(seen) == 2 and [c[0] for c in calls] == ["blocks.0.cross_attention", "blocks.0.self_attention"]
    for (raw, y), (_, q, srcs) in zip(seen, calls):
        want, _ = PU.ln64(raw.numpy())
        assert len(srcs) == 1 and srcs[0] is q
        assert np.abs(q.numpy() - want).max() <= 1e-12


def test_formula_backward_is_the_derivative():
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.standard_normal((5, 40)), requires_grad=True)
    g = rng.standard_normal((5, 40))
    y = torch.nn.functional.layer_norm(x, (40,), eps=PU.EPS)
    y.backward(torch.tensor(g))
    y64, r64 = PU.ln64(x.detach().numpy())
    assert np.abs(y64 - y.detach().numpy()).max() <= 1e-13
    assert np.abs(PU.ln64_bwd(y64, r64, g) - x.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("case", ["d64", "d40", "d30", "d200", "d256", "d320"])
def test_gpu_cases_leave_the_rule_room(case):
    """the float32 pre-norm port against the float64 one: its own error leaves the RTOL / SLACK rule of the GPU
    cases room (parameter gradients within RTOL themselves, sharpness far below 1)"""
    _, _, fx = PU.fixture(case)
    g = np.concatenate([np.ravel(fx["grads"][k]) for k in sorted(fx["grads"])])
    e = math.sqrt(sum(v * v for v in fx["e32"].values())) / np.linalg.norm(g)
    ws, wr = GU.reference_sharpness(fx["samples"])
    print(f"{case}: all-gradient e32 {e:.2e}, sharpness per sample {ws:.3f} per row {wr:.3f}")
    assert e <= GU.RTOL and ws <= 0.5 and wr <= 1.5
