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


# ---------------------------------------------------------------- trained-scale value ranges (test_gpu_value_range.py)
def test_scaled_params_scales_exactly_the_three_groups():
    """a: the weights of every MLP Linear outside the gating MLP; b: weight and bias of every attention query /
    key projection; c: every gating tensor; nothing else -- key by key, with and without input functions"""
    import torch
    from gnot_amd import GNOT
    from golden_util import model_args, scaled_params
    from test_gpu_value_range import FAMILIES
    a, b, c = 2.0, 16.0, 4.0
    for fam in ("A", "Bs"):                       # I = 2 (indexed key / value projections) and I = 0
        cfg = FAMILIES[fam]
        torch.manual_seed(5)
        base = {k: v.double().numpy() for k, v in GNOT(*model_args(cfg)).state_dict().items()}
        got = scaled_params(cfg, 5, a, b, c)
        assert list(got) == list(base)
        seen = {a: 0, b: 0, c: 0, 1.0: 0}
        for k, v in base.items():
            mlp_w = ".layers." in k and k.endswith(".weight")
            qk = any(f".{n}." in k for n in ("query", "key")) and "attention" in k
            want = c if k.startswith("gating.") else b if qk else a if mlp_w else 1.0
            assert got[k].dtype == np.float64 and np.array_equal(got[k], v * want), k
            seen[want] += 1
        assert all(seen.values()), seen
        # what must stay: MLP biases, value projections, fc_out
        assert all(np.array_equal(got[k], base[k]) for k in base
                   if ".value" in k or ".fc_out." in k or (k.endswith(".bias") and ".layers." in k and not k.startswith("gating.")))
        I = cfg["n_input_functions"]
        nkeys = sum(1 for k in base if ".key" in k)
        assert nkeys == cfg["n_attn_layers"] * 2 * (max(I, 1) + 1)


def test_port_hooks_restore_the_port():
    import torch
    import torch.nn.functional as F
    from golden_util import RangeProbe, port_hooks
    from oracle import torch_port
    with pytest.raises(ZeroDivisionError):
        with port_hooks(gelu=lambda h: 1 / 0):
            assert torch_port.F is not F
            torch_port._mlp({"m.layers.0.weight": torch.ones(2, 2), "m.layers.0.bias": torch.zeros(2),
                             "m.layers.2.weight": torch.ones(2, 2), "m.layers.2.bias": torch.zeros(2)}, "m", torch.ones(1, 2), 2)
    assert torch_port.F is F and torch_port.torch is torch
    probe = RangeProbe()
    with probe.hooks():
        h = torch.tensor([[-4.0, 1.0, 2.5]], dtype=torch.float64)
        assert torch.equal(torch_port.F.gelu(h), F.gelu(h))
        assert torch.equal(torch_port.torch.softmax(h, -1), torch.softmax(h, -1))
        torch_port.F.gelu(h.float() * 10)         # the fp32 pass is not recorded
    assert (probe.max_h, probe.n_h, probe.n_big, probe.spread) == (4.0, 3, 1, 6.5)


def test_range_probe_family_A():
    """the ranges family A's reference reaches in each regime (guards against a drift of torch's init), beside
    what the suite's other cases see: at default init nothing leaves |h| < 3 and no softmax spreads by 1"""
    from golden_util import REGIMES, port_reference_ranges, scaled_params
    from test_gpu_value_range import _case
    got = {}
    for regime, R in REGIMES.items():
        pr = _case("A", regime)["probe"]
        assert pr.max_h >= R["max_h"] and pr.spread >= R["spread"] and pr.share >= R["share"], (regime, vars(pr))
        got[regime] = pr
    assert got["moderate"].max_h < got["sharp"].max_h < got["saturated"].max_h < 30
    assert got["moderate"].spread < got["sharp"].spread < got["saturated"].spread < 150
    assert got["qk_only"].max_h < 3 and got["qk_only"].share == 0
    # only `overflow` puts a q / k logit past ln(FLT_MAX), where exp(h) needs the max subtracted
    assert all((pr.head_logit >= 95) == (regime == "overflow") and (pr.head_logit < 88 or regime == "overflow")
               for regime, pr in got.items()), {r: pr.head_logit for r, pr in got.items()}
    fx = _case("A", "moderate")
    init = port_reference_ranges(fx["cfg"], scaled_params(fx["cfg"], 17, 1, 1, 1), fx["xs"][:1], fx["thetas"][:1],
                                 fx["fns_ps"][:1], fx["Gs"][:1])[3]
    assert init.max_h < 3 and init.share == 0 and init.spread < 1, vars(init)


def _value_range_cases():
    from test_gpu_value_range import CASES
    return CASES


@pytest.mark.parametrize("family,regime", _value_range_cases())
def test_value_range_reference_conditions(family, regime):
    """what every value-range GPU case asserts before it touches the GPU: the regime is reached, the reference
    is sharp, and stays so with the fp32 pass's denormals flushed"""
    from golden_util import value_range_conditions
    from test_gpu_value_range import NS, _case
    fx = _case(family, regime)
    assert [s["N"] for s in fx["samples"]] == NS
    missed = value_range_conditions(fx, regime)
    assert not missed, missed


def test_gelu_formula_float64_and_float32():
    """the kernels' A&S form: in float64 within 2.2e-7 of exact GELU and 7.5e-8 |x| everywhere (the derivative
    within 7.5e-8); its float32 restatement follows the float64 one to fp32 rounding and keeps the pointwise
    properties tests/test_gpu_gelu.py asks of the device"""
    from golden_util import gelu_exact64, gelu_formula32, gelu_formula64, gelu_test_inputs, ulp32
    x = gelu_test_inputs()
    assert x.size == 2 ** 20 + 3 + 58 + 4 * 401 and np.isfinite(x).all()
    assert (x == 0).sum() == 3 and np.signbit(x[x == 0]).sum() == 1        # the grid's midpoint, +0 and -0
    x64 = x.astype(np.float64)
    r, dr = gelu_exact64(x64)
    f, df = gelu_formula64(x64)
    assert np.abs(f - r).max() <= 2.2e-7
    assert (np.abs(f - r) <= 7.5e-8 * np.abs(x64)).all()
    assert np.abs(df - dr).max() <= 7.5e-8
    y, dy = gelu_formula32(x)
    assert y.dtype == np.float32 and dy.dtype == np.float32
    assert (np.abs(y - f) <= 200 * ulp32(r)).all() and np.abs(dy - df).max() <= 4e-7
    assert (y[x < 0] <= 0).all() and (y[x > 0] >= 0).all() and (y[x == 0] == 0).all()
    assert (y[x >= 6] == x[x >= 6]).all() and (np.abs(y[x <= -6]) <= 1e-7).all()


def test_bf16_emulated_port():
    from golden_util import port_bf16_emulated, rel
    from test_gpu_value_range import _all_grads, _case
    fx = _case("A", "moderate")
    out, grads = port_bf16_emulated(fx["cfg"], fx["params"], fx["xs"], fx["thetas"], fx["fns_ps"], fx["Gs"])
    e_out, e_grad = rel(out, fx["out"]), rel(_all_grads(fx, grads), _all_grads(fx, fx["grads"]))
    assert 1e-5 < e_out < 1e-2 and 1e-5 < e_grad < 1e-2, (e_out, e_grad)
