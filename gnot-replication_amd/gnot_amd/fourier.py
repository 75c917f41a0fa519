"""Multi-scale Fourier embedding of coordinates and input functions (the original GNOT code's
`horiz_fourier_dim`; the replicated model.py takes raw inputs).

For an order n >= 1, W = 4 n + 3 and f_k = 2^(k - n), k = 0 .. 2 n, channel c of a row (value v) becomes the W
consecutive columns c W .. c W + W - 1

    [ v, cos(f_0 v) .. cos(f_2n v), sin(f_0 v) .. sin(f_2n v) ]

(channel-major, C W columns in all); n = 0 means no embedding.  `GNOT(..., x_fourier=nx, fn_fourier=nf)` is the
reference GNOT of the embedded widths applied to `fourier_features(x, nx)`, the raw theta and
`fourier_features(fn_i, nf)`; inside the model the embedding runs in libgnot_hip.so (csrc/fourier.hip) as the
inputs are staged.

  fourier_features(t, n)   the map in plain torch: any device and dtype, differentiable -- what feeds a
                           reference or port model of the wide input_dim, and the float64 reference of the tests
  fourier_embed(t, n)      the library's kernel on a float32 ROCm tensor (gnot_fourier_embed), no autograd
  fourier_embed_bwd(...)   the library's backward kernel (gnot_fourier_embed_bwd), for point-by-point tests
"""
import ctypes

import torch

from . import _lib

MAX_ORDER = 8


def check_order(n, name="the Fourier order"):
    """the order as an int; ValueError unless it is an integer in [0, MAX_ORDER]"""
    if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= MAX_ORDER:
        raise ValueError(f"{name} must be an integer in [0, {MAX_ORDER}] (0: no embedding), got {n!r}")
    return int(n)


def width(n):
    """columns per channel: 4 n + 3, or 1 without an embedding"""
    return 4 * n + 3 if n > 0 else 1


def fourier_features(t, n):
    """[..., C] -> [..., C (4 n + 3)] in torch ops on t's device and dtype; n = 0 returns t itself."""
    n = check_order(n)
    if n == 0:
        return t
    f = torch.tensor([2.0 ** (k - n) for k in range(2 * n + 1)], dtype=t.dtype, device=t.device)
    a = t.unsqueeze(-1) * f                          # [..., C, 2n+1]; exact products (powers of two)
    emb = torch.cat([t.unsqueeze(-1), torch.cos(a), torch.sin(a)], dim=-1)
    return emb.reshape(*t.shape[:-1], t.shape[-1] * (4 * n + 3))


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _rows(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(f"gnot_amd.{what} runs on float32 tensors on a ROCm GPU only (libgnot_hip.so); "
                           "fourier_features is the map in plain torch")
    if t.dim() < 1 or t.shape[-1] < 1 or t.numel() == 0:
        raise ValueError(f"gnot_amd.{what}: need a non-empty [..., C] tensor, got {tuple(t.shape)}")
    return t.detach().contiguous().view(-1, t.shape[-1])


def fourier_embed(t, n, ld=None):
    """gnot_fourier_embed on a float32 ROCm tensor [..., C]: [..., C (4 n + 3)], bit for bit what a model with
    that order stages.  ld: row pitch of the result (tests of the zero pad columns); the result is then the
    2-d [rows, ld] buffer.  No autograd (the model differentiates through the native path)."""
    n = check_order(n)
    if n == 0:
        raise ValueError("gnot_amd.fourier_embed: the order must be at least 1 (0 is no embedding)")
    src = _rows(t, "fourier_embed")
    rows, C = src.shape
    cw = C * (4 * n + 3)
    pitch = cw if ld is None else int(ld)
    dst = torch.empty((rows, pitch), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().gnot_fourier_embed(src.data_ptr(), rows, C, n, dst.data_ptr(), pitch, _stream(t)))
    return dst if ld is not None else dst.view(*t.shape[:-1], cw)


def fourier_embed_bwd(emb, g, n, C, g2=None):
    """gnot_fourier_embed_bwd: emb [rows, ld] (fourier_embed's rows), g and g2 [rows, >= C (4 n + 3)] the
    gradient of the embedded rows as a sum of one or two sources -> dv [rows, C]."""
    n = check_order(n)
    ts = [emb, g] + ([g2] if g2 is not None else [])
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()):
            raise ValueError("gnot_amd.fourier_embed_bwd takes contiguous 2-d float32 ROCm tensors")
        if t.shape[0] != emb.shape[0]:
            raise ValueError("gnot_amd.fourier_embed_bwd: the row counts differ")
    rows = emb.shape[0]
    dv = torch.empty((rows, C), dtype=torch.float32, device=emb.device)
    with torch.cuda.device(emb.device):
        _lib.check(_lib.load().gnot_fourier_embed_bwd(
            emb.data_ptr(), emb.shape[1], g.data_ptr(), g.shape[1], None if g2 is None else g2.data_ptr(),
            0 if g2 is None else g2.shape[1], rows, C, n, dv.data_ptr(), _stream(emb)))
    return dv
