"""gnot_dropout_rows (csrc/dropout.hip) on its own against the numpy mask of tests/dropout_util.py, bit for bit:
every width class (one to four quads per lane, widths that are no multiple of 4, the last quad cut), tight and
padded pitches, several workgroups, an empty sample and a non-zero first point; untouched pad columns; dropped
Inf / NaN; refusals before any launch; determinism."""
import numpy as np
import pytest
import torch

import dropout_util as DU

pytestmark = pytest.mark.gpu

NS = [1, 63, 0, 65, 128]                  # 257 rows: 65 workgroups of 4 rows, one empty sample
GLO = [5, 0, 7, 1000, (1 << 31) - 200]    # first points of a rank's shards (the last one near the top of 32 bits)
SEED, STEP, P = (0xDEADBEEF << 32) | 0x12345678, 0x80000001, 0.25
WIDTHS = [1, 3, 4, 5, 63, 64, 65, 200, 256, 257, 1024]
bits = lambda t: t.view(torch.int32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


def tables(dev, seed=SEED, step=STEP):
    from gnot_amd.dropout import as_int32, key_words
    off = torch.tensor(np.concatenate([[0], np.cumsum(NS)]), dtype=torch.int64, device=dev)
    glo = torch.tensor(GLO, dtype=torch.int64, device=dev)
    key = torch.tensor(as_int32(key_words(seed, step)), dtype=torch.int32, device=dev)
    return off, glo, key


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("C", WIDTHS)
def test_ones_give_the_numpy_mask_bit_for_bit(dev, C, pad):
    from gnot_amd.dropout import dropout_rows
    ld = (C + pad + 3) // 4 * 4                                      # tight, or 8 columns more (a pitch is a multiple of 4)
    rows = sum(NS)
    x = torch.ones(rows, ld, device=dev)
    x[:, C:] = 7.0                                                   # pad columns: left as they are
    off, glo, key = tables(dev)
    for site in (0, 5):
        y = dropout_rows(x.clone(), C, off, glo, key, site, P)
        torch.cuda.synchronize()
        want = DU.mask_scale(NS, GLO, C, SEED, STEP, site, P)
        assert np.array_equal(y[:, :C].cpu().numpy().view(np.uint32), want.view(np.uint32)), (C, ld, site)
        assert bool((y[:, C:] == 7.0).all())


def test_dropped_inf_and_nan_become_plus_zero(dev):
    from gnot_amd.dropout import dropout_rows
    C = 64
    x = torch.full((sum(NS), C), float("inf"), device=dev)
    x[::2] = float("nan")
    x[1::4] = -float("inf")
    x[:, ::3] = -2.5
    off, glo, key = tables(dev)
    y = dropout_rows(x.clone(), C, off, glo, key, 1, P)
    torch.cuda.synchronize()
    m = torch.tensor(DU.mask_scale(NS, GLO, C, SEED, STEP, 1, P), device=dev)
    dropped = m == 0
    assert 0.2 < float(dropped.float().mean()) < 0.3
    assert bool((bits(y[dropped]) == 0).all())                       # +0.0f, never NaN or -0
    want = x * m
    kept = ~dropped
    assert torch.equal(torch.isnan(y[kept]), torch.isnan(x[kept]))
    fin = kept & ~torch.isnan(x)
    assert torch.equal(bits(y[fin]), bits(want[fin]))


def test_same_key_same_bits_and_p_zero_is_a_no_op(dev):
    from gnot_amd.dropout import dropout_rows
    torch.manual_seed(0)
    x = torch.randn(sum(NS), 200, device=dev)
    off, glo, key = tables(dev)
    a = dropout_rows(x.clone(), 200, off, glo, key, 2, P)
    b = dropout_rows(x.clone(), 200, off, glo, key, 2, P)
    assert torch.equal(bits(a), bits(b)) and not torch.equal(a, x)
    assert torch.equal(bits(dropout_rows(x.clone(), 200, off, glo, key, 2, 0.0)), bits(x))
    _, _, key2 = tables(dev, step=STEP + 1)
    assert not torch.equal(dropout_rows(x.clone(), 200, off, glo, key2, 2, P), a)
    # the key is read when the kernel runs: rewriting the same tensor changes the mask
    key.copy_(key2)
    assert torch.equal(bits(dropout_rows(x.clone(), 200, off, glo, key, 2, P)),
                       bits(dropout_rows(x.clone(), 200, off, glo, key2, 2, P)))


def test_bad_arguments_are_refused_before_any_launch(dev):
    from gnot_amd.dropout import dropout_rows
    off, glo, key = tables(dev)
    x = torch.ones(sum(NS), 64, device=dev)
    before = x.clone()
    for kw in (dict(C=0), dict(C=65), dict(C=1025), dict(p=1.0), dict(p=-0.5), dict(p=float("nan")), dict(site=1 << 24)):
        args = dict(dict(C=64, site=0, p=P), **kw)
        with pytest.raises(RuntimeError, match="dropout_rows"):
            dropout_rows(x, args["C"], off, glo, key, args["site"], args["p"])
    with pytest.raises(RuntimeError, match="dropout_rows"):
        dropout_rows(x[:, 1:], 60, off, glo, key, 0, P)              # rows that start 4 bytes off a 16-byte boundary
    with pytest.raises(ValueError):
        dropout_rows(x.cpu(), 64, off, glo, key, 0, P)
    with pytest.raises(ValueError):
        dropout_rows(x, 64, off, glo.int(), key, 0, P)
    torch.cuda.synchronize()
    assert torch.equal(x, before)
