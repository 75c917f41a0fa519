"""The keyed dropout of `GNOT(..., attn_dropout=p)` on its own (csrc/dropout.hip, gnot_plan_set_dropout): the
host arithmetic of its threshold and the row kernel as a function of tensors, for tests and measurements.

  threshold(p)                      (T, scale): T = floor(fp32(p) 2^32 + 0.5), scale = fp32(2^32 / (2^32 - T));
                                    ValueError unless fp32(p) is finite and in [0, 1).  T = 0 means off
  key_words(seed, step)             the four uint32 {seed_lo, seed_hi, step, 0} of the device key
  dropout_rows(x, C, off, glo, key, site, p)   gnot_dropout_rows in place on x [rows, ld]

Element (point n of sample b, column c) of call site s is kept iff word c % 4 of
Philox4x32-10((n, b, s << 8 | c // 4, step), (seed_lo, seed_hi)) is at least T, and then scaled; a dropped element
becomes +0.  s = 2 l for block l's cross attention, 2 l + 1 for its self attention."""
import ctypes
import math

import torch

from . import _lib

TWO32 = 1 << 32


def _f32(v):
    return ctypes.c_float(v).value


def threshold(p):
    """(T, scale) of the drop probability p, exactly the library's: p is rounded to float32 first (the C ABI
    takes a float), T in double, scale rounded to float32."""
    try:
        p32 = _f32(float(p))
    except (TypeError, ValueError):
        raise ValueError(f"the dropout probability must be a number in [0, 1), got {p!r}") from None
    if not (math.isfinite(p32) and 0.0 <= p32 < 1.0):
        raise ValueError(f"the dropout probability must be finite and in [0, 1), got {p!r}")
    T = int(math.floor(p32 * TWO32 + 0.5))
    return T, _f32(TWO32 / (TWO32 - T))


def key_words(seed, step):
    """{seed_lo, seed_hi, step mod 2^32, 0} of a seed in [0, 2^64)"""
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"the dropout seed must be in [0, 2^64), got {seed}")
    return [seed & 0xFFFFFFFF, seed >> 32, int(step) & 0xFFFFFFFF, 0]


def as_int32(words):
    """uint32 words as the int32 values with the same bits (torch has no uint32 arithmetic to rely on)"""
    return [w - TWO32 if w >= 1 << 31 else w for w in words]


def dropout_rows(x, C, off, glo, key, site, p):
    """gnot_dropout_rows in place on x [rows, ld] (float32, ROCm, rows contiguous with pitch x.stride(0)): off
    [B + 1] / glo [B] int64 device tensors, key an int32 device tensor of 4 words.  Returns x."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise ValueError("gnot_amd.dropout.dropout_rows: x must be a float32 ROCm tensor [rows, ld] with unit column stride")
    for t, dt, n in ((off, torch.int64, glo.numel() + 1), (glo, torch.int64, glo.numel()), (key, torch.int32, 4)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == n):
            raise ValueError("gnot_amd.dropout.dropout_rows: off [B + 1] / glo [B] int64 and key [4] int32 device tensors")
    with torch.cuda.device(x.device):
        s = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(_lib.load().gnot_dropout_rows(x.data_ptr(), x.stride(0), x.shape[0], int(C), off.data_ptr(),
                                                 glo.data_ptr(), glo.numel(), key.data_ptr(), int(site), float(p), s))
    return x
