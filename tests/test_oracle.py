"""The CPU oracle (oracle/gnot_oracle.py) against the reference's golden fixtures."""
import numpy as np
import pytest

from golden_util import check_parity, fixture_names, load
from oracle import gnot_oracle as O


@pytest.mark.parametrize("name", fixture_names())
def test_oracle_fp64_matches_reference(name):
    fx = load(name)
    out, grads = O.gnot_forward_backward(fx["params"], fx["cfg"], fx["x"], fx["x_off"], fx["theta"], fx["fns"],
                                         fx["fn_offs"], G=fx["G"], dtype=np.float64)
    assert np.abs(out - fx["out"]).max() <= 1e-12 * max(1.0, np.abs(fx["out"]).max())
    errs = check_parity(out, grads, fx, rtol=1e-9, slack=0.0)
    # cancellation-only tensors (see golden_util) are exempt at this tolerance, not the rest
    errs = [e for e in errs if not any(t in e for t in ("key", "query"))]
    assert not errs, errs


@pytest.mark.parametrize("name", ["cross1_sharp", "main_pad_h8"])
def test_oracle_fp32_within_reference_tolerance(name):
    fx = load(name)
    out, grads = O.gnot_forward_backward(fx["params"], fx["cfg"], fx["x"], fx["x_off"], fx["theta"], fx["fns"],
                                         fx["fn_offs"], G=fx["G"], dtype=np.float32)
    assert not check_parity(out, grads, fx)


def test_padded_equals_per_sample():
    """A zero-padded batch is per-sample computation on the padded rows."""
    fx = load("main_pad_h8")
    out, _ = O.gnot_forward_backward(fx["params"], fx["cfg"], fx["x"], fx["x_off"], fx["theta"], fx["fns"],
                                     fx["fn_offs"])
    outs = []
    for b in range(len(fx["x_off"]) - 1):
        s, e = fx["x_off"][b], fx["x_off"][b + 1]
        fs = [f[o[b]:o[b + 1]] for f, o in zip(fx["fns"], fx["fn_offs"])]
        fo = [np.array([0, o[b + 1] - o[b]]) for o in fx["fn_offs"]]
        ob, _ = O.gnot_forward_backward(fx["params"], fx["cfg"], fx["x"][s:e], np.array([0, e - s]),
                                        fx["theta"][b:b + 1], fs, fo)
        outs.append(ob)
    assert np.allclose(np.concatenate(outs), out, rtol=0, atol=1e-14)


def test_padding_changes_real_outputs():
    """The reference does not mask padding: real-point outputs depend on the pad rows."""
    fx = load("cross2_packed")
    b0 = slice(fx["x_off"][0], fx["x_off"][1])
    fs = [f[o[0]:o[1]] for f, o in zip(fx["fns"], fx["fn_offs"])]
    fo = [np.array([0, o[1] - o[0]]) for o in fx["fn_offs"]]
    n = fx["x_off"][1]
    out0, _ = O.gnot_forward_backward(fx["params"], fx["cfg"], fx["x"][b0], np.array([0, n]), fx["theta"][:1], fs, fo)
    xp = np.concatenate([fx["x"][b0], np.zeros((9, fx["x"].shape[1]))])
    outp, _ = O.gnot_forward_backward(fx["params"], fx["cfg"], xp, np.array([0, n + 9]), fx["theta"][:1], fs, fo)
    assert np.abs(outp[:n] - out0).max() > 1e-10


@pytest.mark.parametrize("name", ["cross1_sharp", "self_only_pad", "cross2_packed"])
def test_torch_port_matches_fixtures(name):
    """The stock-torch CPU port timed as bench.py's cpu_baseline computes the reference's numbers."""
    import torch
    from oracle import torch_port
    fx = load(name)
    cfg = fx["cfg"]
    p = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in fx["params"].items()}
    outs = []
    for b in range(len(fx["x_off"]) - 1):
        s, e = fx["x_off"][b], fx["x_off"][b + 1]
        x = torch.from_numpy(fx["x"][s:e])[None]
        fns = [torch.from_numpy(f[o[b]:o[b + 1]])[None] for f, o in zip(fx["fns"], fx["fn_offs"])]
        o = torch_port.gnot_forward(p, cfg, x, torch.from_numpy(fx["theta"][b:b + 1]), fns)[0]
        (o * torch.from_numpy(fx["G"][s:e])).sum().backward()
        outs.append(o.detach().numpy())
    grads = {k: v.grad.numpy() for k, v in p.items()}
    errs = check_parity(np.concatenate(outs), grads, fx, rtol=1e-9, slack=0.0)
    errs = [e for e in errs if not any(t in e for t in ("key", "query"))]
    assert not errs, errs


def _split(fx):
    B = len(fx["x_off"]) - 1
    cut = lambda a, o: [a[o[b]:o[b + 1]] for b in range(B)]
    fns_ps = [[f[o[b]:o[b + 1]] for f, o in zip(fx["fns"], fx["fn_offs"])] for b in range(B)]
    return cut(fx["x"], fx["x_off"]), list(fx["theta"]), fns_ps, cut(fx["G"], fx["x_off"])


def test_port_reference_matches_fixture():
    """golden_util.port_reference (the per-sample float64 reference of tests/test_gpu_geometry.py: one B = 1
    port call per sample, parameter gradients summed over the samples) reproduces the reference's packed
    fixture: output rows per sample and every parameter gradient."""
    from golden_util import port_reference
    fx = load("cross2_packed")
    samples, grads, e32 = port_reference(fx["cfg"], fx["params"], *_split(fx))
    out = np.concatenate([s["out"] for s in samples])
    errs = check_parity(out, grads, fx, rtol=1e-9, slack=0.0)
    errs = [e for e in errs if not any(t in e for t in ("key", "query"))]
    assert not errs, errs
    assert [s["N"] for s in samples] == np.diff(fx["x_off"]).tolist()
    assert all(0 < e32[k] < 1e-3 * max(np.linalg.norm(grads[k]), 1e-6) for k in grads)


def test_per_sample_rule_sees_what_the_whole_batch_norm_misses():
    """check_parity_per_sample on the geometry suite's `empties` batch (Ns = [65, 0, 1, 0, 128]): the
    reference itself passes; 0.05 % of error confined to the 1-point sample passes the whole-batch rule and
    fails the per-sample one, naming the sample and the row; an error in one sample's dtheta row or a NaN in
    a dfns segment fails; the empty samples' reference rows are exact zeros."""
    from golden_util import check_parity_per_sample
    from test_gpu_geometry import _case
    fx = _case("A", "empties")
    S = fx["samples"]

    def got():
        return dict(out=fx["out"].copy(), grads=fx["grads"], dx=np.concatenate([s["dx"] for s in S]),
                    dtheta=np.stack([s["dtheta"] for s in S]),
                    dfns=[np.concatenate([s["dfns"][i] for s in S]) for i in range(len(fx["fns"]))])

    assert not check_parity_per_sample(got(), fx)
    assert [s["N"] for s in S] == [65, 0, 1, 0, 128]
    for b in (1, 3):
        assert not S[b]["dtheta"].any() and not any(f.any() for f in S[b]["dfns"])
    g = got()
    g["out"][65] *= 1.0005                      # the 1-point sample's only row
    assert not check_parity(g["out"], g["grads"], fx)
    errs = check_parity_per_sample(g, fx)
    assert errs and all("sample 2 (N=1, M=[1, 1])" in e for e in errs) and "worst row 0 of 1" in errs[0], errs
    g = got()
    g["out"][66 + 127] *= 1.002                 # the last row of the last sample's last (full) chunk
    errs = check_parity_per_sample(g, fx)
    assert any("worst row 127 of 128 (point 63 of a 64-point chunk 1)" in e for e in errs), errs
    g = got()
    g["dtheta"][0] *= 1.001
    assert any("sample 0" in e and "dtheta" in e for e in check_parity_per_sample(g, fx))
    g = got()
    g["dfns"][1][0] = np.nan
    assert any("dfn1" in e for e in check_parity_per_sample(g, fx))
