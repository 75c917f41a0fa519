"""The parameter-free LayerNorm row kernels of `GNOT(..., pre_norm=True)` on their own (csrc/norm.hip), as
torch-tensor wrappers on the current stream for row-by-row tests; no autograd (the model differentiates through
the native path).

  layer_norm_rows(x, C, eps)            gnot_layer_norm: y[r, :C] = (x[r, :C] - mean) / sqrt(var + eps), the
                                        columns from C on zeros; returns (y, rstd)
  layer_norm_rows_bwd(y, rstd, dy, C)   gnot_layer_norm_bwd: dx = rstd (dy - mean(dy) - y mean(dy y)), stored
                                        into a new tensor or into / onto `dx`

Every tensor is a 2-d float32 ROCm tensor whose rows are contiguous (stride(1) == 1); the row pitch is
stride(0), so a column slice of a wider buffer is a row array with pad columns.
"""
import ctypes

import torch

from . import _lib

EPS = 1e-5


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _rows(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and
            t.shape[0] >= 1 and t.stride(1) == 1):
        raise ValueError(f"gnot_amd.norm.{what} takes non-empty 2-d float32 ROCm tensors with contiguous rows")
    return t


def layer_norm_rows(x, C=None, eps=EPS, out=None, keep_rstd=True):
    """x [rows, >= C] (pitch x.stride(0)) -> (y, rstd): y = `out` or a new [rows, x.shape[1]] tensor whose
    columns from C on are zeros; rstd [rows], or None with keep_rstd=False (the inference form)."""
    x = _rows(x, "layer_norm_rows")
    rows = x.shape[0]
    C = x.shape[1] if C is None else int(C)
    y = torch.empty((rows, x.shape[1]), dtype=torch.float32, device=x.device) if out is None else _rows(out, "layer_norm_rows")
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if keep_rstd else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().gnot_layer_norm(x.data_ptr(), x.stride(0), rows, C, float(eps), y.data_ptr(), y.stride(0),
                                               None if rstd is None else rstd.data_ptr(), _stream(x)))
    return y, rstd


def layer_norm_rows_bwd(y, rstd, dy, C=None, dx=None, accumulate=False):
    """dx = rstd (dy - mean_C(dy) - y mean_C(dy y)) from layer_norm_rows' y and rstd.  dx: None (a new tensor of
    dy's shape), or the tensor to store into / with accumulate=True to add onto; it may be dy itself."""
    y, dy = _rows(y, "layer_norm_rows_bwd"), _rows(dy, "layer_norm_rows_bwd")
    rows = y.shape[0]
    C = y.shape[1] if C is None else int(C)
    if dx is None:
        if accumulate:
            raise ValueError("gnot_amd.norm.layer_norm_rows_bwd: accumulate needs the tensor to add onto")
        dx = torch.empty((rows, dy.shape[1]), dtype=torch.float32, device=y.device)
    dx = _rows(dx, "layer_norm_rows_bwd")
    if not (rstd.is_cuda and rstd.dtype == torch.float32 and rstd.is_contiguous() and rstd.numel() == rows):
        raise ValueError("gnot_amd.norm.layer_norm_rows_bwd: rstd must be a contiguous float32 ROCm tensor [rows]")
    if dy.shape[0] != rows or dx.shape[0] != rows:
        raise ValueError("gnot_amd.norm.layer_norm_rows_bwd: the row counts differ")
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().gnot_layer_norm_bwd(y.data_ptr(), y.stride(0), rstd.data_ptr(), dy.data_ptr(), dy.stride(0),
                                                   rows, C, dx.data_ptr(), dx.stride(0), int(bool(accumulate)), _stream(y)))
    return dx
