"""The optional parts of the training step, on the CPU: the argument checks of gnot_mse_loss and
gnot_grad_clip (they return before any launch, so dummy device pointers are enough), their work sizes,
and a world_size-2 gloo run of the point-sharded MSELoss (loss.py:4-12) against the unsharded formula."""
import ctypes

import pytest
import torch

from gnot_amd import _lib
from gnot_amd import parallel as par
from test_parallel import _run

DUMMY = 0x1000      # a non-null "device pointer": the checks must never get as far as using it


def _off(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _mse(off, B=None, C=2):
    lib = _lib.load()
    B = len(off) - 1 if B is None else B
    return lib.gnot_mse_loss(DUMMY, DUMMY, DUMMY, _off(off), B, C, DUMMY, DUMMY, DUMMY, None)


def test_mse_refuses_an_empty_sample():
    assert _mse([0, 5, 5, 9]) != 0
    assert "empty sample" in _lib.load().gnot_last_error().decode()


def test_mse_refuses_decreasing_offsets():
    assert _mse([0, 5, 3, 9]) != 0


def test_mse_refuses_bad_sizes_and_null_pointers():
    lib = _lib.load()
    assert _mse([1, 5, 9]) != 0                      # off[0] != 0
    assert _mse([0, 5, 9], B=0) != 0
    assert _mse([0, 5, 9], C=0) != 0
    assert lib.gnot_mse_loss(None, DUMMY, DUMMY, _off([0, 5]), 1, 2, DUMMY, DUMMY, DUMMY, None) != 0
    assert lib.gnot_mse_loss(DUMMY, DUMMY, DUMMY, _off([0, 5]), 1, 2, DUMMY, None, DUMMY, None) != 0


@pytest.mark.parametrize("n,max_norm", [(0, 1.0), (-3, 1.0), (16, 0.0), (16, -1.0), (16, float("inf")),
                                        (16, float("nan"))])
def test_grad_clip_refuses(n, max_norm):
    assert _lib.load().gnot_grad_clip(DUMMY, n, DUMMY, max_norm, DUMMY, DUMMY, None) != 0


def test_grad_clip_refuses_null_pointers():
    lib = _lib.load()
    for k in range(4):
        ptrs = [DUMMY] * 4
        ptrs[k] = None
        assert lib.gnot_grad_clip(ptrs[0], 16, ptrs[1], 1.0, ptrs[2], ptrs[3], None) != 0
    assert lib.gnot_adamw_step_clipped(DUMMY, DUMMY, DUMMY, DUMMY, 16, DUMMY, None, None) != 0


def test_work_sizes():
    lib = _lib.load()
    assert lib.gnot_mse_work_floats(_off([0, 37, 38, 5038, 7087]), 4, 3) > 0
    # the longest sample has 5000 rows, three splits: partial sums [B][nsplit][C] and the gradient scales [B][C]
    B, nsplit, C = 4, 3, 3
    assert lib.gnot_mse_work_floats(_off([0, 37, 38, 5038, 7087]), B, C) == B * nsplit * C + B * C
    # one more 2048-row split needs more room
    assert lib.gnot_mse_work_floats(_off([0, 2049]), 1, 1) > lib.gnot_mse_work_floats(_off([0, 2048]), 1, 1)
    sizes = [lib.gnot_grad_clip_work_floats(n) for n in (1, 255, 257, 524291)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert lib.gnot_grad_clip_work_floats(0) == 0


def _sharded_mse(rank, world):
    torch.manual_seed(0)
    ns, C = [11, 7], 2
    B = len(ns)
    off = [0, ns[0], ns[0] + ns[1]]
    out = torch.randn(off[-1], C, dtype=torch.float64, requires_grad=True)
    tgt = torch.randn(off[-1], C, dtype=torch.float64)
    # unsharded reference (loss.py:4-12): per-sample mean over points, then the mean
    ref = torch.stack([((out[s:e] - tgt[s:e]) ** 2).mean(0) for s, e in zip(off[:-1], off[1:])]).mean()
    ref.backward()
    g_ref = out.grad.clone()
    # this rank's slice of every sample
    rng = [par.shard_range(n, rank, world) for n in ns]
    idx = torch.cat([torch.arange(off[b] + lo, off[b] + hi) for b, (lo, hi) in enumerate(rng)])
    seg = torch.cat([torch.full((hi - lo,), b, dtype=torch.int64) for b, (lo, hi) in enumerate(rng)])
    ol = out.detach()[idx].clone().requires_grad_(True)
    loss = par.mse_loss_sharded(ol, tgt[idx], seg, ns)
    loss.backward()
    assert abs(float(loss) - float(ref)) < 1e-12
    assert torch.allclose(ol.grad, g_ref[idx], rtol=0, atol=1e-12)


def test_sharded_mse_loss_gloo():
    _run(2, _sharded_mse)
