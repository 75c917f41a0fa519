"""The Lp loss family without a GPU: the exported symbols, the refusals gnot_lp_loss makes on the host before any
launch, train.LpLoss's argument checks and trajectory name, the float64 reference's own closed forms, and the
training script's command line."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import lp_util as L
from gnot_amd import _lib, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ("gnot_lp_loss_work_floats", "gnot_lp_loss"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert list(_lib.LP_KINDS) == list(L.KINDS) and list(_lib.LP_KINDS.values()) == list(range(6))
    import gnot_amd
    assert gnot_amd.LpLoss is train.LpLoss and gnot_amd.evaluate_table is train.evaluate_table


def test_work_size_covers_two_norms_per_split_and_the_scales():
    lib = _lib.load()
    for sizes, C in L.CASES + [([2048], 2), ([1], 4)]:
        off = L.offsets(sizes)
        B = len(sizes)
        oh = (ctypes.c_int64 * (B + 1))(*off)
        nsplit = -(-max(sizes) // 2048)
        assert lib.gnot_lp_loss_work_floats(oh, B, C) == B * nsplit * 2 * C + B * C
    assert lib.gnot_lp_loss_work_floats(None, 1, 1) == 0


def _call(off, C, kind, dpred=None, ptr=ctypes.c_void_p(4096)):
    """gnot_lp_loss on dummy device pointers: every refusal tested here returns before a launch"""
    B = len(off) - 1
    oh = (ctypes.c_int64 * (B + 1))(*off)
    lib = _lib.load()
    rc = lib.gnot_lp_loss(ptr, ptr, ptr, oh, B, C, kind, None, None, ptr, ptr, None, dpred, None)
    return rc, lib.gnot_last_error().decode()


def test_abi_refuses_on_the_host():
    D = ctypes.c_void_p(4096)
    rc, msg = _call([0, 5, 5, 9], 2, _lib.LP_KINDS["rel1"])
    assert rc == -1 and "empty sample" in msg
    for kind in L.KINDS:                                   # every kind, rel2 included (gnot_rel_l2_loss takes one)
        assert _call([0, 0], 1, _lib.LP_KINDS[kind])[0] == -1
    for bad in (-1, 6, 99):
        rc, msg = _call([0, 5], 1, bad)
        assert rc == -1 and "unknown kind" in msg
    for kind in ("relinf", "linf"):
        rc, msg = _call([0, 5], 1, _lib.LP_KINDS[kind], dpred=D)
        assert rc == -1 and "no gradient" in msg
    rc, msg = _call([0, 5, 3], 1, 0)
    assert rc == -1 and "non-decreasing" in msg
    assert _call([0, 5], 0, 0)[0] == -1 and _call([0, 5], 1, 0, ptr=None)[0] == -1


@pytest.mark.parametrize("weights,match", [([1.0, -0.5], "negative"), ([0.0, 0.0], "positive"), ([], "empty"),
                                           ([1.0, float("nan")], "finite"), ([float("inf"), 1.0], "finite"),
                                           ([3e38, 3e38], "positive")])
def test_lp_loss_refuses_bad_weights(weights, match):
    with pytest.raises(ValueError, match=match):
        train.LpLoss("rel1", weights)


def test_lp_loss_argument_checks_come_before_any_gpu_work():
    with pytest.raises(ValueError, match="unknown kind"):
        train.LpLoss("rel3")
    off, pred, tgt = [0, 4], torch.zeros(4, 3), torch.ones(4, 3)
    # wrong length: known at the call, refused on the host (the tensors here are not even on a device)
    with pytest.raises(ValueError, match="2 component_weights, the prediction has 3"):
        train.LpLoss("l1", [1, 2])(off, pred, tgt)
    for kind in ("relinf", "linf"):
        with pytest.raises(ValueError, match="metric only"):
            train.LpLoss(kind)(off, pred.clone().requires_grad_(True), tgt)
        with pytest.raises(ValueError, match="metric only"):
            train.LpLoss(kind).loss_and_terms(off, pred.clone().requires_grad_(True), tgt)
    # everything the host can check passes: what is left is the device
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        train.LpLoss("linf")(off, pred, tgt)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        train.LpLoss("rel1", [1, 0, 3]).terms(off, pred.clone().requires_grad_(True), tgt)


def test_trajectory_name():
    assert train.LpLoss().trajectory_name() == "LpLoss(rel2)"
    assert train.LpLoss("rel1", [1, 0, 3]).trajectory_name() == "LpLoss(rel1, w=[1.0, 0.0, 3.0])"
    assert train.LpLoss("l1", (0.5,)).trajectory_name() == "LpLoss(l1, w=[0.5])"
    names = {train.LpLoss(k, w).trajectory_name() for k in L.KINDS for w in (None, [1, 2], [2, 1])}
    assert len(names) == 18
    # the classes that existed keep the name fit stores for them
    assert not hasattr(train.RelL2Loss(), "trajectory_name") and not hasattr(train.MSELoss(), "trajectory_name")
    assert train.LpLoss("mse").kind == "mse" and train.LpLoss("mse").component_weights is None


def test_reference_closed_forms_agree_with_autograd():
    """lp_util.grad (what the GPU gradients are held against) is the float64 autograd gradient of lp_util's loss"""
    sizes, C = [1, 7, 30], 3
    off = L.offsets(sizes)
    pred, tgt = L.inputs(sizes, C)
    for weights in (None, [1, 0, 3]):
        w = torch.tensor(L.norm_weights(weights, C))
        for kind in L.DIFFERENTIABLE:
            p = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
            t = torch.tensor(tgt, dtype=torch.float64)
            total = 0
            for b in range(len(sizes)):
                d, tb = p[off[b]:off[b + 1]] - t[off[b]:off[b + 1]], t[off[b]:off[b + 1]]
                e = {"rel2": lambda: ((d ** 2).sum(0) / (tb ** 2).sum(0)).sqrt(),
                     "rel1": lambda: d.abs().sum(0) / tb.abs().sum(0),
                     "mse": lambda: (d ** 2).mean(0), "l1": lambda: d.abs().mean(0)}[kind]()
                total = total + (w * e).sum()
            total = total / len(sizes)
            total.backward()
            assert abs(total.item() - L.loss(kind, pred, tgt, off, weights)) <= 1e-12 * abs(total.item())
            np.testing.assert_allclose(L.grad(kind, pred, tgt, off, weights), p.grad.numpy(), rtol=1e-12, atol=1e-300)
    e = L.terms("linf", pred, tgt, off)
    assert e.shape == (3, 3) and e[0, 1] == abs(np.float64(pred[0, 1]) - np.float64(tgt[0, 1]))


def _script():
    spec = importlib.util.spec_from_file_location("train_ns2d", os.path.join(ROOT, "scripts", "train_ns2d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_arguments():
    s = _script()
    a = s.parse_args(["--synthetic", "8"])
    assert a.loss == "rel_l2" and a.component_weights is None and a.log_components is False
    assert type(s.training_loss(a)) is train.RelL2Loss
    assert type(s.training_loss(s.parse_args(["--loss", "mse"]))) is train.MSELoss
    for flag, kind in (("rel_l1", "rel1"), ("l1", "l1")):
        loss = s.training_loss(s.parse_args(["--loss", flag]))
        assert type(loss) is train.LpLoss and loss.kind == kind and loss.component_weights is None
    a = s.parse_args(["--loss", "rel_l1", "--component-weights", "1,0,3", "--log-components"])
    assert a.component_weights == [1.0, 0.0, 3.0] and a.log_components is True
    assert s.training_loss(a).trajectory_name() == "LpLoss(rel1, w=[1.0, 0.0, 3.0])"
    # weights on the two losses that had a class of their own: the same kinds through LpLoss
    assert s.training_loss(s.parse_args(["--component-weights", "2,1"])).trajectory_name() == "LpLoss(rel2, w=[2.0, 1.0])"
    assert s.training_loss(s.parse_args(["--loss", "mse", "--component-weights", "1"])).kind == "mse"
    for bad in (["--component-weights", "1,-1"], ["--component-weights", "0,0"], ["--component-weights", "a,b"],
                ["--component-weights", ""], ["--loss", "linf"], ["--loss", "rel_linf"]):
        with pytest.raises(SystemExit):
            s.parse_args(bad)
