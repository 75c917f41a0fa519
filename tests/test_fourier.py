"""CPU-side checks of the Fourier-feature embedding (gnot_amd.fourier, GNOT(..., x_fourier=, fn_fourier=)):
the torch map against the formula, the module's parameter layout, the refusals, the checkpoint rule, the C
ABI's host-side checks, and the conditioning of the cases tests/test_gpu_fourier.py runs."""
import ctypes

import numpy as np
import pytest
import torch

import fourier_util as FU


@pytest.mark.parametrize("n", [1, 3, 8])
def test_fourier_features_match_the_formula(n):
    from gnot_amd import fourier_features
    rng = np.random.default_rng(n)
    v = rng.uniform(-4, 4, (7, 5, 3))
    got = fourier_features(torch.tensor(v), n).numpy()
    W = 4 * n + 3
    assert got.shape == (7, 5, 3 * W)
    assert np.abs(got - FU.formula64(v, n)).max() <= 1e-15
    # the layout, column by column: channel-major, the raw value first, then cos, then sin
    for c in range(3):
        assert np.array_equal(got[..., c * W], v[..., c])
        for k in range(2 * n + 1):
            f = 2.0 ** (k - n)
            assert np.abs(got[..., c * W + 1 + k] - np.cos(f * v[..., c])).max() <= 1e-15
            assert np.abs(got[..., c * W + 2 * n + 2 + k] - np.sin(f * v[..., c])).max() <= 1e-15
    # float32 in, float32 out, same layout
    g32 = fourier_features(torch.tensor(v, dtype=torch.float32), n)
    assert g32.dtype == torch.float32 and np.abs(g32.double().numpy() - got).max() < 1e-3


def test_fourier_features_order_zero_is_the_identity():
    from gnot_amd import fourier_features
    t = torch.rand(4, 3)
    assert fourier_features(t, 0) is t
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 8\]"):
            fourier_features(t, bad)


def test_fourier_features_gradcheck():
    from gnot_amd import fourier_features
    t = torch.tensor(np.random.default_rng(0).uniform(-2, 2, (5, 2)), requires_grad=True)
    assert torch.autograd.gradcheck(lambda a: fourier_features(a, 2), (t,))
    # and the closed form: dv = g_0 + sum_k f_k (cos g_sin - sin g_cos)
    g = np.random.default_rng(1).standard_normal((5, 2 * 11))
    fourier_features(t, 2).backward(torch.tensor(g))
    want, _ = FU.formula64_bwd(t.detach().numpy(), g, 2)
    assert np.abs(t.grad.numpy() - want).max() <= 1e-14


def test_state_dict_is_the_wide_reference_models():
    from gnot_amd import GNOT
    A = GNOT(2, 1, 3, 1, 1, 64, 2, 64, 64, 3, 4, 1, x_fourier=3, fn_fourier=2)
    B = GNOT(30, 1, 33, 1, 1, 64, 2, 64, 64, 3, 4, 1)
    sa, sb = A.state_dict(), B.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    assert A.x.layers[0].weight.shape == (64, 31) and A.gating.layers[0].weight.shape == (64, 30)
    assert A.input_func_mlps[0].layers[0].weight.shape == (64, 33)
    B.load_state_dict(sa)
    assert A._cfg["input_dim"] == 2 and A._cfg["input_func_dim"] == 3       # the caller's widths
    # the defaults are the model it always was
    C = GNOT(2, 1, 3, 1, 1, 64, 2, 64, 64, 3, 4, 1)
    assert C.x_fourier == 0 and C.fn_fourier == 0 and C.x.layers[0].weight.shape == (64, 3)


def test_constructor_refuses_bad_orders_and_widths():
    from gnot_amd import GNOT
    args = (2, 1, 3, 1, 1, 64, 2, 64, 64, 3, 4, 1)
    for kw in (dict(x_fourier=-1), dict(x_fourier=9), dict(fn_fourier=-2), dict(fn_fourier=9), dict(x_fourier=1.5)):
        with pytest.raises(ValueError, match=r"\[0, 8\]"):
            GNOT(*args, **kw)
    with pytest.raises(TypeError):
        GNOT(*args, 3)                                    # keyword only
    # 2 * 35 + 1 = 71 columns do not fit a hidden width of 64: the engine's message, at construction
    with pytest.raises(ValueError, match="hidden width"):
        GNOT(*args, x_fourier=8)
    GNOT(2, 1, 3, 1, 1, 256, 2, 256, 256, 3, 8, 1, x_fourier=8, fn_fourier=8)


def test_forward_checks_the_raw_widths_before_the_device():
    from gnot_amd import GNOT
    m = GNOT(2, 1, 3, 1, 1, 64, 2, 64, 64, 3, 4, 0, x_fourier=3)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(torch.rand(1, 10, 2), torch.rand(1, 1))


def test_plan_set_fourier_checks():
    """gnot_plan_set_fourier: orders 0 .. 8, embedded widths that are multiples of 4 n + 3, and a changed order
    invalidates the batch (host only)."""
    from gnot_amd import _lib
    lib = _lib.load()
    for name in ("gnot_plan_set_fourier", "gnot_fourier_embed", "gnot_fourier_embed_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    cfg = _lib.GnotConfig(input_dim=30, theta_dim=1, input_func_dim=33, out_dim=1, n_attn_layers=1,
                          n_attn_hidden_dim=64, n_mlp_num_layers=2, n_mlp_hidden_dim=64, n_input_hidden_dim=64,
                          n_expert=3, n_head=4, n_input_functions=1)
    plan = ctypes.c_void_p()
    _lib.check(lib.gnot_plan_create(ctypes.byref(cfg), ctypes.byref(plan)))
    try:
        for nx, nf in ((-1, 0), (9, 0), (0, -1), (0, 9)):
            assert lib.gnot_plan_set_fourier(plan, nx, nf) == -1
            assert b"[0, 8]" in lib.gnot_last_error()
        assert lib.gnot_plan_set_fourier(plan, 2, 0) == -1             # 30 is no multiple of 11
        assert b"input_dim" in lib.gnot_last_error()
        assert lib.gnot_plan_set_fourier(plan, 3, 3) == -1             # 33 is no multiple of 15
        assert b"input_func_dim" in lib.gnot_last_error()
        xo, fo = (ctypes.c_int64 * 2)(0, 50), (ctypes.c_int64 * 2)(0, 7)
        _lib.check(lib.gnot_plan_set_batch(plan, 1, xo, fo, 1))
        plain = lib.gnot_plan_workspace_bytes(plan)
        assert plain > 0
        _lib.check(lib.gnot_plan_set_fourier(plan, 0, 0))              # unchanged: the batch stands
        assert lib.gnot_plan_workspace_bytes(plan) == plain
        _lib.check(lib.gnot_plan_set_fourier(plan, 3, 2))
        assert lib.gnot_plan_workspace_bytes(plan) == 0                # batch invalidated
        _lib.check(lib.gnot_plan_set_batch(plan, 1, xo, fo, 1))
        assert lib.gnot_plan_workspace_bytes(plan) == plain            # the workspace holds the embedded rows as before
        assert lib.gnot_plan_set_fourier(plan, 7, 0) == -1             # 30 is no multiple of 31 either
        assert lib.gnot_plan_workspace_bytes(plan) == plain            # a refused call changes nothing
    finally:
        lib.gnot_plan_destroy(plan)


def test_stand_alone_entries_refuse_bad_arguments():
    """the checks return before any launch, so dummy device pointers do"""
    from gnot_amd import _lib
    lib = _lib.load()
    D = ctypes.c_void_p(4096)
    assert lib.gnot_fourier_embed(None, 4, 2, 3, D, 30, None) == -1
    assert lib.gnot_fourier_embed(D, 4, 2, 3, None, 30, None) == -1
    assert lib.gnot_fourier_embed(D, 0, 2, 3, D, 30, None) == -1
    assert lib.gnot_fourier_embed(D, 4, 0, 3, D, 30, None) == -1
    for n in (0, 9, -1):
        assert lib.gnot_fourier_embed(D, 4, 2, n, D, 100, None) == -1
        assert b"[1, 8]" in lib.gnot_last_error()
    assert lib.gnot_fourier_embed(D, 4, 2, 3, D, 29, None) == -1       # ld < C W
    assert b"ld" in lib.gnot_last_error()
    assert lib.gnot_fourier_embed(D, 4, 2, 3, D, 1 << 31, None) == -1  # 32-bit column indices
    assert lib.gnot_fourier_embed_bwd(D, 1 << 40, D, 1 << 40, None, 0, 4, 1 << 28, 3, D, None) == -1
    assert lib.gnot_fourier_embed_bwd(None, 30, D, 30, None, 0, 4, 2, 3, D, None) == -1
    assert lib.gnot_fourier_embed_bwd(D, 30, None, 30, None, 0, 4, 2, 3, D, None) == -1
    assert lib.gnot_fourier_embed_bwd(D, 30, D, 30, None, 0, 4, 2, 3, None, None) == -1
    assert lib.gnot_fourier_embed_bwd(D, 30, D, 30, None, 0, 4, 2, 9, D, None) == -1
    assert lib.gnot_fourier_embed_bwd(D, 29, D, 30, None, 0, 4, 2, 3, D, None) == -1
    assert lib.gnot_fourier_embed_bwd(D, 30, D, 29, None, 0, 4, 2, 3, D, None) == -1
    assert lib.gnot_fourier_embed_bwd(D, 30, D, 30, D, 29, 4, 2, 3, D, None) == -1
    assert b"pitch" in lib.gnot_last_error()


def test_fourier_embed_needs_the_device():
    from gnot_amd import fourier_embed
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        fourier_embed(torch.rand(4, 2), 3)


def _normalizer(x=None, fn=None):
    from gnot_amd import Normalizer
    ident = ([0.0, 0.0], [1.0, 1.0])
    return Normalizer.from_stats(x or ident, ([0.5], [0.25]), ([2.0], [3.0]),
                                 [fn or ([0.0] * 3, [1.0] * 3)], eps=0.0)


def test_checkpoint_refuses_statistics_of_an_embedded_block(tmp_path):
    from gnot_amd import GNOT, train
    torch.manual_seed(0)
    A = GNOT(2, 1, 3, 1, 1, 64, 2, 64, 64, 3, 4, 1, x_fourier=3, fn_fourier=2)
    path = str(tmp_path / "ck.pth")
    with pytest.raises(ValueError, match=r"statistics for x \(x_fourier=3\).*dataset.*--normalize"):
        train.save_checkpoint(A, path, _normalizer(x=([0.5, 0.5], [0.3, 0.3])))
    with pytest.raises(ValueError, match=r"fns\.0 \(fn_fourier=2\)"):
        train.save_checkpoint(A, path, _normalizer(fn=([0.1] * 3, [2.0] * 3)))
    # theta / y statistics alone fold as before: the x columns and the input functions' Linear untouched
    train.save_checkpoint(A, path, _normalizer())
    sd, raw = torch.load(path, weights_only=True), A.state_dict()
    assert list(sd.keys()) == list(raw.keys())
    W, W0 = sd["x.layers.0.weight"].double(), raw["x.layers.0.weight"].double()
    assert torch.equal(W[:, :30], W0[:, :30])
    assert torch.allclose(W[:, 30], W0[:, 30] * 4.0, rtol=1e-6, atol=0)            # rstd = 1 / 0.25
    assert torch.allclose(sd["x.layers.0.bias"].double(), raw["x.layers.0.bias"].double() - W[:, 30] * 0.5,
                          rtol=1e-6, atol=1e-7)
    for k in ("gating.layers.0.weight", "gating.layers.0.bias", "input_func_mlps.0.layers.0.weight",
              "input_func_mlps.0.layers.0.bias"):
        assert torch.equal(sd[k], raw[k]), k
    assert torch.allclose(sd["out.layers.4.weight"], raw["out.layers.4.weight"] * 3.0)
    # a model that embeds x only keeps folding the input functions' statistics
    Ax = GNOT(2, 1, 3, 1, 1, 64, 2, 64, 64, 3, 4, 1, x_fourier=3)
    train.save_checkpoint(Ax, path, _normalizer(fn=([0.1] * 3, [2.0] * 3)))
    sd = torch.load(path, weights_only=True)
    assert torch.allclose(sd["input_func_mlps.0.layers.0.weight"], Ax.state_dict()["input_func_mlps.0.layers.0.weight"] / 2)
    # and a model without an embedding is what it was
    P = GNOT(2, 1, 3, 1, 1, 64, 2, 64, 64, 3, 4, 1)
    train.save_checkpoint(P, path, _normalizer(x=([0.5, 0.5], [0.3, 0.3])))


# ------------------------------------------------------------------ conditioning of the GPU cases
@pytest.mark.parametrize("case", list(FU.CASES))
def test_gpu_cases_are_well_conditioned(case):
    """The float32 port against the float64 port, both on fourier_features of the inputs, per sample: below
    2.5e-6 (a fortieth of the 1e-4 bar) on the output and on dx, so the reference's own arithmetic never decides
    a GPU case.  Relative, norm-wise per sample."""
    A, _ = FU.models(case)
    xs, thetas, fns_ps, Gs = FU.inputs(case)
    samples, grads, e32 = FU.reference(case, FU.params64(A), xs, thetas, fns_ps, Gs)
    for b, s in enumerate(samples):
        e_out = s["e32"]["out"] / np.linalg.norm(s["out"])
        e_dx = s["e32"]["dx"] / np.linalg.norm(s["dx"])
        print(f"{case} sample {b} (N={s['N']}): output e32 {e_out:.2e}, dx e32 {e_dx:.2e}")
        assert e_out < 2.5e-6 and e_dx < 2.5e-6, (case, b, e_out, e_dx)
        assert s["dx"].shape == (s["N"], FU.IN)
        assert all(g.shape == (m, FU.F) for g, m in zip(s["dfns"], s["M"]))
