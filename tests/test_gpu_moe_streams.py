"""The two row streams a fp32 d = 256 soft-MoE call does without.

Training forward: no [E, P, d] stage -- the combine forms s_e y_e from the saved expert outputs and the scores
(misc.hip moe_combine_scaled).  Backward, where a call's weight gradients run on the caller's stream right
after its chain backward (GNOT_WGRAD_OVERLAP=0 here; plans of >= 65,536 points by default): no stored
dz_{NL-1} = s_e dq -- the last Linear's weight-gradient jobs read dquery and scale it by the expert's score
column (wgrad.hip, WgradJob::scale).  GNOT_MOE_STORED_STREAMS=1 restores both stored streams.

Model: d = 256, 8 heads, one block, n_mlp_num_layers 1 and 4, 2 and 8 experts, one input function, fp32.
Point counts: the last 128-point chain block, the last 16-point wave and the last 16-point weight-gradient
stage are partial in each; 77 + 123 puts a sample boundary inside a block; 2,064 points make the balanced
split-K ranges end inside a job (10 or 40 soft-MoE jobs over 256 workgroups at >= 128 points per range).

Checks per case:
  1. float64 (the stock-torch port, one B = 1 call per sample): golden_util.check_parity at its 1e-4 bars on
     the output and every parameter gradient, for the serial (direct) form;
  2. bitwise, direct forms against GNOT_MOE_STORED_STREAMS=1: output, loss, every parameter gradient and the
     input gradients; and against the default (forked) choice of a small plan, which keeps the stored dz;
  3. bitwise: training forward = no_grad forward = training with set_moe_recompute(True), gradients included.
"""
import functools

import numpy as np
import pytest
import torch

from golden_util import check_parity, model_args, port_reference
from test_gpu_geometry import _run, _same_bits
from test_gpu_parity import build_model

pytestmark = pytest.mark.gpu

GEOMS = {"two_samples": [77, 123], "one_block_plus_one": [129], "split_in_job": [2064]}
M_FN = 33          # input-function points per sample


def _cfg(nl, E):
    return dict(input_dim=2, theta_dim=1, input_func_dim=3, out_dim=2, n_attn_layers=1, d=256, n_mlp_num_layers=nl,
                n_expert=E, n_head=8, n_input_functions=1)


@functools.lru_cache(maxsize=None)
def _case(nl, E, geom):
    """one float64 reference per case, shared by every check"""
    from gnot_amd import GNOT
    cfg = _cfg(nl, E)
    Ns = GEOMS[geom]
    torch.manual_seed(31)
    params = {k: v.double().numpy() for k, v in GNOT(*model_args(cfg)).state_dict().items()}
    rng = np.random.default_rng(31)
    xs = [rng.random((n, cfg["input_dim"])) for n in Ns]
    thetas = [rng.random(cfg["theta_dim"]) for _ in Ns]
    fns_ps = [[rng.random((M_FN, cfg["input_func_dim"]))] for _ in Ns]
    Gs = [rng.standard_normal((n, cfg["out_dim"])) for n in Ns]
    samples, grads, e32 = port_reference(cfg, params, xs, thetas, fns_ps, Gs)
    off = lambda L: np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    return dict(cfg=cfg, params=params, samples=samples, grads=grads, e32=e32, x=np.concatenate(xs),
                x_off=off(Ns), theta=np.stack(thetas), fns=[np.concatenate([f[0] for f in fns_ps])],
                fn_offs=[off([M_FN] * len(Ns))], G=np.concatenate(Gs), out=np.concatenate([s["out"] for s in samples]))


def _fresh_run(fx, monkeypatch, overlap, stored, recompute=False):
    """a new model (the switches are read when its plan is created), one forward + backward with input grads"""
    for name, val in (("GNOT_WGRAD_OVERLAP", overlap), ("GNOT_MOE_STORED_STREAMS", stored)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    m = build_model(fx["params"], fx["cfg"])
    if recompute:
        m.set_moe_recompute(True)
    got = _run(m, fx)
    got["loss"] = np.float64((got["out"] * fx["G"]).sum())
    return m, got


def _no_grad_out(m, fx):
    dev = torch.device("cuda")
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    with torch.no_grad():
        out = m.forward_packed(t(fx["x"]), fx["x_off"].tolist(), t(fx["theta"]), [t(f) for f in fx["fns"]],
                               [o.tolist() for o in fx["fn_offs"]])
    torch.cuda.synchronize()
    return out.double().cpu().numpy()


KEYS = ("out", "loss", "dx", "dtheta")


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("E", [2, 8])
@pytest.mark.parametrize("nl", [1, 4])
def test_moe_streams(nl, E, geom, monkeypatch):
    fx = _case(nl, E, geom)
    # serial weight gradients: both direct forms
    m, direct = _fresh_run(fx, monkeypatch, "0", None)
    errs = check_parity(direct["out"], direct["grads"], fx)
    print(f"\nMOE_STREAMS nl={nl} E={E} {geom}: parity errors {errs}")
    assert not errs, errs
    assert all(np.isfinite(a).all() for a in (direct["dx"], direct["dtheta"], *direct["dfns"]))
    # the inference forward keeps the stage path: the same bits
    assert np.array_equal(_no_grad_out(m, fx), direct["out"]), "no_grad forward differs from the training forward"
    # both stored streams restored
    _, stored = _fresh_run(fx, monkeypatch, "0", "1")
    assert not _same_bits(direct, stored, KEYS), "direct forms differ from the stored streams"
    # the default choice of a small plan: forked weight gradients, which keep the stored dz
    _, forked = _fresh_run(fx, monkeypatch, None, None)
    assert not _same_bits(direct, forked, KEYS), "forked plan differs from the serial one"
    _, forked_stored = _fresh_run(fx, monkeypatch, None, "1")
    assert not _same_bits(direct, forked_stored, KEYS), "forked plan with stored streams differs"
    # MoE recompute: its forward keeps no saves (the stage path), its backward re-runs the experts
    _, rec = _fresh_run(fx, monkeypatch, "0", None, recompute=True)
    assert not _same_bits(direct, rec, KEYS), "MoE recompute differs"
