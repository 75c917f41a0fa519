"""The parameter-free LayerNorm row kernels on their own (gnot_layer_norm / gnot_layer_norm_bwd through
gnot_amd.norm), element by element against the float64 formula of tests/prenorm_util.py.

Bounds.  C_FWD and C_BWD are 4 times what torch's own float32 F.layer_norm (CPU) reaches on these same inputs
against float64, in the error scales below (scripts/prenorm_bounds.py, recorded in
profiles/prenorm_kernel_bounds.txt; measured on the CPU, torch 2.10): the kernels' butterfly order differs from
torch's vectorised order and both are logarithmic trees, so more than 4 times points at a serial sum or a
one-pass variance.
  forward   torch 3.483 (1e4 + N(0, 1), C = 257)           -> C_FWD = 13.93, also the relative bound of rstd
  backward  torch 33.5 (N(0, 1), C = 2)                     -> C_BWD = 134.0
            (over all four families torch's backward reaches 9.4e5 on the rows with an offset of 1e4, where its
            dx = a dy + b x + c cancels; the kernel reads y, not x, and is held to 134 on every family)"""
import numpy as np
import pytest
import torch

import prenorm_util as PU

pytestmark = pytest.mark.gpu

C_FWD = 13.93
C_BWD = 134.0
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


def r4(c):
    return (c + 3) // 4 * 4


def _padded(a, ld, dev, fill=NAN):
    """a [rows, C] as the first C columns of a [rows, ld] device buffer whose other columns hold `fill`"""
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=dev)
    buf[:, :a.shape[1]] = torch.tensor(a, device=dev)
    return buf


def _forward(x, ld, dev):
    """(y [rows, ld] with its pad columns, rstd) of the kernel on x [rows, C] at row pitch ld for x and y; the
    input pad columns hold NaN, the output buffer starts as NaN"""
    from gnot_amd.norm import layer_norm_rows
    C = x.shape[1]
    xb = _padded(x, ld, dev)
    yb = torch.full((x.shape[0], ld), NAN, dtype=torch.float32, device=dev)
    _, rstd = layer_norm_rows(xb[:, :C], C, out=yb)
    return yb, rstd


@pytest.mark.parametrize("C", PU.WIDTHS)
def test_rows_against_float64(dev, C):
    from gnot_amd.norm import layer_norm_rows_bwd
    worst = [0.0, 0.0, 0.0]
    for rows in PU.ROWS:
        for ld in (r4(C), r4(C) + 8):
            for fam in PU.FAMILIES:
                tag = (C, rows, ld, fam)
                x, dy = PU.kernel_rows(C, rows, fam)
                yb, rstd = _forward(x, ld, dev)
                y, rs = yb.cpu().numpy(), rstd.cpu().numpy()
                assert np.isfinite(y).all() and np.isfinite(rs).all(), tag      # no NaN leaks from the input pads
                assert (y[:, C:] == 0).all(), tag                                # output pad columns: exact zeros
                qf, qr = PU.fwd_ratios(x, y[:, :C], rs)
                if fam == "constant" or C == 1:
                    assert (y == 0).all(), tag                                   # exact zeros, finite rstd
                # backward from the kernel's own y and rstd: stored, accumulated, and in place
                dyb = _padded(dy, ld, dev)
                dxb = torch.full_like(yb, NAN)
                layer_norm_rows_bwd(yb[:, :C], rstd, dyb[:, :C], C, dx=dxb[:, :C])
                whole = dxb.cpu().numpy()
                assert np.isfinite(whole).all() and (whole[:, C:] == 0).all(), tag
                qb = PU.bwd_ratio(y[:, :C], rs, dy, whole[:, :C])
                old = torch.tensor(np.random.default_rng(7).standard_normal((rows, ld)).astype(np.float32), device=dev)
                acc = old.clone()
                layer_norm_rows_bwd(yb[:, :C], rstd, dyb[:, :C], C, dx=acc[:, :C], accumulate=True)
                want = old.clone()
                want[:, :C] += torch.tensor(whole[:, :C], device=dev)            # one rounded add per element
                assert torch.equal(acc, want), tag                               # (pad columns untouched)
                alias = _padded(dy, ld, dev, fill=0.0)
                layer_norm_rows_bwd(yb[:, :C], rstd, alias[:, :C], C, dx=alias[:, :C])
                assert np.array_equal(alias.cpu().numpy(), whole), tag           # dx aliasing dy: the same bits
                worst = [max(a, b) for a, b in zip(worst, (qf, qr, qb))]
                assert qf <= C_FWD and qr <= C_FWD and qb <= C_BWD, (tag, qf, qr, qb)
    print(f"C={C}: forward {worst[0]:.3f} (bound {C_FWD}), rstd {worst[1]:.3f} (bound {C_FWD}), "
          f"backward {worst[2]:.3f} (bound {C_BWD})")


@pytest.mark.parametrize("C", [5, 64, 257, 1000])
def test_rows_are_deterministic_and_independent_of_the_call(dev, C):
    from gnot_amd.norm import layer_norm_rows, layer_norm_rows_bwd
    x, dy = PU.kernel_rows(C, 257, "normal", seed=1)
    ld = r4(C)
    xb, dyb = _padded(x, ld, dev, 0.0), _padded(dy, ld, dev, 0.0)
    run = lambda a, g: (lambda y, r: (y, r, layer_norm_rows_bwd(y, r, g, C)))(*layer_norm_rows(a, C))
    y, r, dx = run(xb, dyb)
    y2, r2, dx2 = run(xb, dyb)
    assert torch.equal(y, y2) and torch.equal(r, r2) and torch.equal(dx, dx2)    # two runs, the same bits
    for row in (0, 3, 130, 255, 256):                    # every wave slot of a workgroup, first and last workgroup
        y1, r1, dx1 = run(xb[row:row + 1].clone(), dyb[row:row + 1].clone())
        assert torch.equal(y1[0], y[row]) and torch.equal(r1[0], r[row]) and torch.equal(dx1[0], dx[row]), row


def test_inference_form_keeps_no_rstd(dev):
    from gnot_amd.norm import layer_norm_rows
    x, _ = PU.kernel_rows(200, 5, "normal")
    xb = torch.tensor(x, device=dev)
    y, r = layer_norm_rows(xb)
    y0, none = layer_norm_rows(xb, keep_rstd=False)
    assert none is None and torch.equal(y, y0)
