"""The device GELU (csrc/gnot_common.h gelu / gelu_and_grad / gelu_grad) point by point against float64.

The model-level rule is norm-wise: a GELU that is 10 % wrong on [-5, -3] moves a whole-batch norm by about
1e-4, because those outputs are small.  gnot_debug_gelu evaluates the same device functions that every chain
epilogue and weight-gradient loader inlines, one launch over golden_util.gelu_test_inputs(): 2^20 + 3 grid
points on [-12, 12], +-0, +-1e-30, +-1e-40 (a denormal), +-2^k for k = -20 .. 5 and the 200 float32 neighbours
on each side of +-3.0834 and +-2.4639.

References: R64, exact GELU and its derivative in float64 (erf / erfc); F64, the kernels' Abramowitz-Stegun
7.1.26 form in float64; F32, that form operation by operation in numpy float32 with correctly rounded 1/x and
exp2 (golden_util.gelu_exact64 / gelu_formula64 / gelu_formula32).

Bounds, for every input:
  |y  - R64 | <= 7.5e-8 |x| + k_y  ulp32(max(|R64 |, tiny))
  |dy - R64'| <= 7.5e-8     + k_dy ulp32(max(|R64'|, tiny))
The first term is the formula's.  A&S 7.1.26 gives erf to 1.5e-7 absolute, so the tail q = Phi(-|x|) =
(1 - erf(|x| / sqrt 2)) / 2 to 7.5e-8, and gelu(x) = max(x, 0) - |x| q inherits 7.5e-8 |x| (measured on these
inputs: 2.11e-7 at x = 3.083, 0.93 of the term).  The derivative is evaluated as Phi(x) + x phi(x) with
Phi(x) = 1/2 + sign(x) (1/2 - q) and phi(x) = e^{-x^2 / 2} / sqrt(2 pi) exact: only Phi carries the
approximation, so the term is 7.5e-8 (1 + |x| * 0) -- the derivative of the A&S error never enters, because
the kernels do not differentiate the approximation (measured: 6.97e-8 at x = -0.064).
The second term is fp32 evaluation.  k is not chosen: it is twice the worst ulp error of F32 against F64 over
the same inputs, computed here (k_y about 250; k_dy about 1e6, all of it on [-12, -4], where 1/2 - q rounds
at the ulp of 1/2 while gelu' itself is 1e-6 .. 1e-30); the factor two is for v_rcp_f32 and v_exp_f32, 1-ulp
approximations where numpy's are correctly rounded.  Because an ulp count that large bounds little where
gelu' is of order one, the derivative is also held to the same rule in absolute terms:
  |dy - R64'| <= 7.5e-8 + 2 max |F32' - F64'|        (about 5.6e-7).

What the code gives on non-finite input (read from gnot_common.h, not asserted): x = +inf has t = 0, e = 0,
q = 0 and fmaf(-inf, 0, inf) = NaN where torch gives inf; x = -inf gives fmaf(-inf, 0, 0) = NaN; gelu' of
either is (x / sqrt(2 pi)) * 0 = NaN; a NaN input gives NaN from all three functions (q is NaN).
"""
import functools

import numpy as np
import pytest
import torch

from golden_util import gelu_exact64, gelu_formula32, gelu_formula64, gelu_test_inputs, ulp32
from train_step_util import stream

pytestmark = pytest.mark.gpu

AS_TAIL = 7.5e-8      # |A&S 7.1.26 error| / 2


def device_gelu(x):
    """(y, dy, y2, dy2) of gnot_debug_gelu over a float32 array"""
    from gnot_amd import _lib
    n = x.size
    d = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = torch.full((4, n + 64), 7.0, dtype=torch.float32, device="cuda")     # 64 guard floats behind each row
    _lib.check(_lib.load().gnot_debug_gelu(d.data_ptr(), *[out[i].data_ptr() for i in range(4)], n, stream()))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, n:] == 7.0).all(), "wrote past n"
    return tuple(host[i, :n].copy() for i in range(4))


@functools.lru_cache(maxsize=None)
def _figures():
    x = gelu_test_inputs()
    x64 = x.astype(np.float64)
    r, dr = gelu_exact64(x64)
    f, df = gelu_formula64(x64)
    y32, dy32 = gelu_formula32(x)
    y, dy, y2, dy2 = device_gelu(x)
    return dict(x=x, x64=x64, r=r, dr=dr, f=f, df=df, y32=y32.astype(np.float64), dy32=dy32.astype(np.float64),
                y=y, dy=dy, y2=y2, dy2=dy2)


def test_fused_form_is_bitwise_the_plain_one():
    F = _figures()
    assert np.array_equal(F["y"].view(np.int32), F["y2"].view(np.int32)), "gelu_and_grad's value differs from gelu's"
    assert np.array_equal(F["dy"].view(np.int32), F["dy2"].view(np.int32)), "gelu_and_grad's derivative differs from gelu_grad's"


def test_gelu_within_formula_and_rounding_bounds():
    F = _figures()
    x64 = F["x64"]
    assert np.isfinite(F["y"]).all() and np.isfinite(F["dy"]).all()
    bad = []
    for name, got, ref, form, emu, tail in (("gelu", F["y"], F["r"], F["f"], F["y32"], AS_TAIL * np.abs(x64)),
                                            ("gelu'", F["dy"], F["dr"], F["df"], F["dy32"], AS_TAIL)):
        u = ulp32(ref)
        k = 2.0 * float((np.abs(emu - form) / u).max())
        dev_ulp = np.abs(got - form) / u
        w = int(dev_ulp.argmax())
        err = np.abs(got - ref)
        excess = err - tail
        we = int(excess.argmax())
        print(f"\nGELU {name}: k {k:.1f} ulp (twice the float32 formula's worst against float64); device worst "
              f"{dev_ulp[w]:.1f} ulp at x = {x64[w]:.6g}; worst |device - exact| {err.max():.3e} at x = {x64[int(err.argmax())]:.6g}; "
              f"worst excess over the formula term {excess[we]:.3e} at x = {x64[we]:.6g} (allowed {k * u[we]:.3e})")
        lim = tail + k * u
        miss = ~(err <= lim)
        if miss.any():
            i = int(np.argmax(np.where(miss, excess / (k * u), -np.inf)))
            bad.append(f"{name}: {int(miss.sum())} points off, worst x = {x64[i]:.9g}: |err| {err[i]:.3e} > {lim[i]:.3e}")
    a = 2.0 * float(np.abs(F["dy32"] - F["df"]).max())
    err = np.abs(F["dy"] - F["dr"])
    print(f"GELU gelu' absolute: allowed {AS_TAIL + a:.3e}, device worst {err.max():.3e} at x = {x64[int(err.argmax())]:.6g}")
    if not (err <= AS_TAIL + a).all():
        bad.append(f"gelu' absolute: {err.max():.3e} > {AS_TAIL + a:.3e}")
    assert not bad, bad


def test_gelu_signs_zeros_and_far_tails():
    F = _figures()
    x, y = F["x"], F["y"]
    assert (y[x < 0] <= 0).all(), "gelu(x) > 0 for a negative x"
    assert (y[x > 0] >= 0).all(), "gelu(x) < 0 for a positive x"
    z = y[x == 0]
    assert z.size == 3 and (z == 0).all()                       # the grid's midpoint and +-0 -> +-0 or +0
    assert not np.signbit(y[(x == 0) & ~np.signbit(x)]).any(), "gelu(+0) = -0"
    far = x >= 6
    assert (np.abs(y[far].astype(np.float64) - F["x64"][far]) <= ulp32(F["x64"][far])).all()
    assert (np.abs(y[x <= -6]) <= 1e-7).all()
