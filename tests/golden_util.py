"""Fixture loading + the parity tolerance rule shared by the CPU and GPU tests."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_names():
    """the model fixtures: every archive with a "meta" entry (train_step_bits.npz, which has none, belongs to
    test_gpu_train_bits.py)"""
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz"))
                  if "meta" in np.load(f).files)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))   # allow_pickle=False (default)
    meta = json.loads(str(z["meta"]))
    cfg = dict(meta["cfg"])
    I = cfg["n_input_functions"]
    fx = dict(
        meta=meta, cfg=cfg,
        params={k[2:]: z[k] for k in z.files if k.startswith("p.")},
        grads={k[2:]: z[k] for k in z.files if k.startswith("g.")},
        e32={k[4:]: float(z[k]) for k in z.files if k.startswith("e32.")},
        x=z["x"], x_off=z["x_off"], theta=z["theta"], G=z["G"], out=z["out"],
        fns=[z[f"fn{i}"] for i in range(I)], fn_offs=[z[f"fn{i}_off"] for i in range(I)],
    )
    return fx


def model_args(cfg):
    d = cfg["d"]
    return (cfg["input_dim"], cfg["theta_dim"], cfg["input_func_dim"], cfg["out_dim"], cfg["n_attn_layers"],
            d, cfg["n_mlp_num_layers"], d, d, cfg["n_expert"], cfg["n_head"], cfg["n_input_functions"])


# Parity rule (fp32 vs the reference's float64 result):
#   * whole-model: ||out - ref|| / ||ref|| <= RTOL and, over all parameter gradients concatenated,
#     ||g - ref|| / ||ref|| <= RTOL  (north_star: "within 1e-4 relative in fp32", norm-wise as
#     SURVEY.md §6 prescribes)
#   * per tensor: ||g - ref|| <= RTOL * ||ref|| + SLACK * e32, where e32 is the reference's OWN
#     fp32-vs-fp64 error on that tensor (stored in the fixture).  Some gradients are pure
#     cancellation at nn.Linear's default init (e.g. key-projection grads ~1e-13 while their fp32
#     noise is ~1e-10); e32 bounds what any fp32 implementation can achieve on them.
RTOL = 1e-4
SLACK = 20.0


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check_parity(out, grads, fx, rtol=RTOL, slack=SLACK):
    errs = []
    # every comparison is written `not (err <= bound)`: a NaN error (a non-finite output or gradient) fails
    e_out = rel(out, fx["out"])
    if not e_out <= rtol:
        errs.append(f"output rel err {e_out:.3e} > {rtol}")
    if grads is not None:
        keys = sorted(fx["grads"])
        g = np.concatenate([np.ravel(grads[k]) for k in keys])
        r = np.concatenate([np.ravel(fx["grads"][k]) for k in keys])
        e_all = rel(g, r)
        if not e_all <= rtol:
            errs.append(f"all-grad rel err {e_all:.3e} > {rtol}")
        for k in keys:
            d = float(np.linalg.norm(np.asarray(grads[k], np.float64) - fx["grads"][k]))
            lim = rtol * float(np.linalg.norm(fx["grads"][k])) + slack * fx["e32"].get(k, 0.0)
            if not d <= lim:
                errs.append(f"{k}: |err| {d:.3e} > {lim:.3e}")
    return errs
