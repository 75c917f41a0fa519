"""The composed float64 reference of tests/combo_util.py (pre-norm, attention dropout and the Fourier embedding in
any combination), checked on the CPU before any GPU test relies on it: with one option on it is the reference
of that option's own utility bit for bit, its wrappers leave oracle/torch_port.py as they found it, and with all
three on it is far from every reference that has lost one option -- so a GPU path that silently drops an option
in combination cannot pass the 1e-4 parity rule.

Route: these tests build their parameter dictionaries without the HIP library (combo_util.params64: the plain
torch module of the embedded widths, whose constructor probes no plan).  Only
test_the_models_hold_these_parameters_and_the_largest_orders constructs GNOT with a Fourier order, which loads the
built library as tests/test_fourier.py does."""
import numpy as np
import pytest
import torch

import combo_util as CU
import dropout_util as DU
import fourier_util as FU
import golden_util as GU
import prenorm_util as PU

STEP = 3
_REF = {}


def same(a, b):
    """two (samples, grads, e32) results, bit for bit"""
    (sa, ga, ea), (sb, gb, eb) = a, b
    eq = np.array_equal
    assert len(sa) == len(sb) and sorted(ga) == sorted(gb) and ea == eb
    for x, y in zip(sa, sb):
        assert x["N"] == y["N"] and x["M"] == y["M"]
        assert all(eq(x[k], y[k]) for k in ("out", "dx", "dtheta")) and all(eq(p, q) for p, q in zip(x["dfns"], y["dfns"]))
        assert all(x["e32"][k] == y["e32"][k] for k in ("out", "dx", "dtheta", "dfns")) and eq(x["e32"]["rows"], y["e32"]["rows"])
    assert all(eq(ga[k], gb[k]) for k in ga)


def triple(step=STEP, opts=CU.TRIPLE):
    """the c64 reference with `opts` on at a dropout step, on the triple's parameters and inputs; computed once"""
    key = (step, frozenset(opts))
    if key not in _REF:
        _REF[key] = CU.reference("c64", opts, CU.params64("c64", CU.TRIPLE), *CU.inputs("c64"), steps=step)
    return _REF[key]


def test_pre_norm_alone_is_prenorm_util():
    params, data = CU.params64("c64", ["prenorm"]), CU.inputs("c64")
    same(CU.reference("c64", ["prenorm"], params, *data), PU.reference(CU.cfg_of("c64"), params, *data))


def test_dropout_alone_is_dropout_util():
    params, data = CU.params64("c64", ["drop"]), CU.inputs("c64")
    same(CU.reference("c64", ["drop"], params, *data, steps=STEP),
         DU.reference(CU.cfg_of("c64"), params, *data, steps=STEP))


def test_fourier_alone_is_fourier_util():
    """fourier_util's reference is written per fourier_util.CASES entry: its d64 (2 input functions, orders 3 / 2,
    one block, out_dim 1) through reference_cfg, on this file's geometry"""
    case = "d64"
    c = FU.CASES[case]
    wide = FU.wide_cfg(case)
    raw = dict(wide, input_dim=FU.IN, input_func_dim=FU.F)
    from gnot_amd import GNOT
    torch.manual_seed(5)
    params = {k: v.detach().double().numpy() for k, v in GNOT(*GU.model_args(wide)).named_parameters()}
    data = FU.inputs(case, Ns=CU.NS, Ms=CU.MS)
    same(CU.reference_cfg(raw, c["nx"], c["nf"], ["fourier"], params, *data), FU.reference(case, params, *data))


def test_no_option_is_the_plain_port():
    params, data = CU.params64("c64", []), CU.inputs("c64")
    same(CU.reference("c64", [], params, *data), GU.port_reference(CU.cfg_of("c64"), params, *data))


def test_wrappers_count_their_calls_and_restore_the_port():
    from oracle import torch_port
    plain = torch_port._attention
    case = "c64"
    cfg, c = CU.cfg_of(case), CU.CASES[case]
    wide = CU.wide_cfg(cfg, c["nx"], c["nf"])
    data = CU.inputs(case)
    groups = [[b] for b, n in enumerate(CU.NS) if n > 0]
    masks = DU.site_masks(wide, CU.NS, STEP)
    assert len(masks) == 2 * c["L"] * len(groups)                   # two sites per block, the empty sample has no call
    with CU.port(CU.TRIPLE, masks) as calls:
        assert torch_port._attention is not plain
        res, _ = CU.embedded_pass(wide, c["nx"], c["nf"], CU.params64(case, CU.TRIPLE), *data, groups, "float64")
    assert calls[0] == len(masks) and torch_port._attention is plain
    assert res[1] is None and all(np.isfinite(res[b]["out"]).all() for b in (0, 2, 3))
    with pytest.raises(RuntimeError, match="the body raises"):
        with CU.port(CU.TRIPLE, masks):
            raise RuntimeError("the body raises")
    assert torch_port._attention is plain
    with pytest.raises(IndexError):                                  # one call more than there are masks
        with CU.port(CU.TRIPLE, masks[:1]):
            CU.embedded_pass(wide, c["nx"], c["nf"], CU.params64(case, CU.TRIPLE), *data, groups, "float64")
    assert torch_port._attention is plain


@pytest.mark.parametrize("lost, opts, step", [("pre-norm", ("drop", "fourier"), STEP), ("dropout", ("prenorm", "fourier"), STEP),
                                              ("the step", CU.TRIPLE, STEP + 1)])
def test_losing_an_option_moves_the_reference_far_beyond_the_parity_bar(lost, opts, step):
    """a condition on the reference, not a tolerance on the code under test: the float64 output of the full
    reference is more than 100 x RTOL (relative, norm-wise) from the reference without pre-norm, without dropout,
    and with the mask of the next step"""
    out = lambda ref: np.concatenate([s["out"] for s in ref[0]])
    keys = sorted(triple()[1])
    cat = lambda ref: np.concatenate([np.ravel(ref[1][k]) for k in keys])
    e_out, e_grad = GU.rel(out(triple(step, opts)), out(triple())), GU.rel(cat(triple(step, opts)), cat(triple()))
    print(f"without {lost}: output {e_out:.2e}, gradients {e_grad:.2e}")
    assert np.isfinite(out(triple())).all() and np.isfinite(cat(triple())).all()
    assert e_out > 1e-2 >= 100 * GU.RTOL and e_grad > 1e-2


def test_the_models_hold_these_parameters_and_the_largest_orders():
    """model(case, opts) has params64(case, opts) bit for bit; at c30 and c40 a plan refuses the next order"""
    from gnot_amd import GNOT
    for case in CU.CASES:
        for opts in ([], ["prenorm", "drop"], CU.TRIPLE):
            m, p = CU.model(case, opts), CU.params64(case, opts)
            got = dict(m.named_parameters())
            assert list(got) == list(p)
            assert all(np.array_equal(got[k].detach().double().numpy(), p[k]) for k in p), (case, opts)
    for case, more in (("c30", dict(x_fourier=3)), ("c30", dict(fn_fourier=2)), ("c40", dict(x_fourier=5))):
        c = CU.CASES[case]
        with pytest.raises(ValueError, match="hidden width"):
            GNOT(*GU.model_args(CU.cfg_of(case)), **dict(dict(x_fourier=c["nx"], fn_fourier=c["nf"]), **more))
