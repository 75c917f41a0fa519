"""Device-resident datasets, on the CPU: the keyed permutation gnot_gather_rows draws its subsamples with (a
numpy implementation written from the definition in include/gnot_hip.h: known answers, bijectivity,
uniformity), the argument checks of gnot_gather_rows (they return before any launch, so dummy device pointers
are enough), and the gather tables DeviceLoader builds from its generator alone.
test_gpu_device_data.py imports `perm` and `gather_reference` from here."""
import ctypes

import numpy as np
import pytest
import torch

from gnot_amd import _lib, data

DUMMY = 0x1000      # a non-null "device pointer": the checks must never get as far as using it
E_INVALID = -1      # GNOT_E_INVALID (a launch that failed for want of a GPU would be GNOT_E_HIP)


# ------------------------------------------------------------------ the permutation, from its definition
def fmix32(h):
    h = np.asarray(h, dtype=np.uint32)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def perm(n, key_lo, key_hi, count=None, rounds=6):
    """pi(0), ..., pi(count - 1) for [0, n) under every key: key_lo / key_hi are scalars or arrays [K]; returns
    [count] for scalar keys, [K, count] for arrays.  All arithmetic uint32, mod 2^32."""
    count = n if count is None else count
    scalar = np.ndim(key_lo) == 0
    lo = np.atleast_1d(np.asarray(key_lo, dtype=np.uint64)).astype(np.uint32)[:, None]
    hi = np.atleast_1d(np.asarray(key_hi, dtype=np.uint64)).astype(np.uint32)[:, None]
    x = np.broadcast_to(np.arange(count, dtype=np.uint32), (lo.shape[0], count)).copy()
    if n >= 2:
        h = np.uint32((int(n - 1).bit_length() + 1) // 2)
        mask = np.uint32((1 << int(h)) - 1)
        with np.errstate(over="ignore"):
            rk = [fmix32(lo ^ np.uint32((r * 0x9E3779B9) & 0xFFFFFFFF)) + hi for r in range(rounds)]

            def E(x, sel):
                L, R = x >> h, x & mask
                for r in range(rounds):
                    L, R = R, L ^ (fmix32(R ^ np.broadcast_to(rk[r], sel.shape)[sel]) & mask)
                return (L << h) | R

            todo = np.ones(x.shape, dtype=bool)
            while todo.any():
                x[todo] = E(x[todo], todo)
                todo &= x >= n
    out = x.astype(np.int64)
    return out[0] if scalar else out


def gather_reference(src, table):
    """what gnot_gather_rows writes for src [rows, C] (numpy) and table rows {src_row0, n, dst_row0, k, lo, hi}"""
    parts = [src[:0]]
    for s0, n, _, k, lo, hi in table:
        idx = np.arange(k) if k == n else perm(n, lo, hi, k)
        parts.append(src[s0 + idx])
    return np.concatenate(parts)


KNOWN = [(5, (1, 2), [2, 1, 4, 0, 3]),
         (2, (0, 0), [0, 1]),
         (1000, (0xDEADBEEF, 0x12345678), [295, 93, 789, 425, 835, 187]),
         (65536, (0xFFFFFFFF, 0xFFFFFFFF), [38595, 40549, 16530, 17566]),
         (1048577, (7, 9), [626312, 3652, 36200, 455239])]


@pytest.mark.parametrize("n,key,want", KNOWN, ids=[str(k[0]) for k in KNOWN])
def test_known_answers(n, key, want):
    assert perm(n, key[0], key[1], len(want)).tolist() == want


def test_a_single_element_maps_to_itself():
    assert perm(1, 123, 456).tolist() == [0]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 64, 65, 257, 1000])
def test_bijection(n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 2 ** 32, size=(64, 2), dtype=np.uint64)
    p = perm(n, keys[:, 0], keys[:, 1])
    assert p.shape == (64, n)
    assert (np.sort(p, axis=1) == np.arange(n)).all()


UNIFORM_NS = [2, 3, 5, 16, 17, 37, 64, 65, 257, 1000]
N_KEYS = 8192


@pytest.fixture(scope="module")
def uniform_perms():
    """{n: [8192, n] permutations}; the keys from default_rng(0), a lo and a hi column drawn per n"""
    rng = np.random.default_rng(0)
    out = {}
    for n in UNIFORM_NS:
        lo = rng.integers(0, 2 ** 32, size=N_KEYS, dtype=np.uint64)
        hi = rng.integers(0, 2 ** 32, size=N_KEYS, dtype=np.uint64)
        out[n] = perm(n, lo, hi)
    return out


def _z(counts, p):
    """the largest deviation of binomial(N_KEYS, p) counts from their mean, in standard deviations"""
    return float(np.abs(counts - N_KEYS * p).max() / np.sqrt(N_KEYS * p * (1 - p)))


def test_uniformity(uniform_perms):
    """Every index is among the first k picks, and at position 0, within 5 binomial standard deviations of its
    share of 8192 keys.  Five is a condition, not a measurement: these inputs give 4.48 and 4.48 with the six
    rounds of the definition and 15.3 among the first k with four."""
    worst_in, worst_first = 0.0, 0.0
    for n in UNIFORM_NS:
        p = uniform_perms[n]
        for k in sorted({min(max(k, 1), n - 1) for k in (1, n // 4, n // 2, n - 1)}):
            counts = np.bincount(p[:, :k].reshape(-1), minlength=n)
            worst_in = max(worst_in, _z(counts, k / n))
        worst_first = max(worst_first, _z(np.bincount(p[:, 0], minlength=n), 1 / n))
    print(f"largest deviation: among the first k {worst_in:.2f}, at position 0 {worst_first:.2f} standard deviations")
    assert worst_in <= 5.0 and worst_first <= 5.0


# ------------------------------------------------------------------ gnot_gather_rows: refusals before any launch
def _gather(table, B=None, C=2, src=DUMMY, table_dev=DUMMY, dst=DUMMY, host=True):
    flat = [int(v) for row in table for v in row]
    th = (ctypes.c_int64 * max(len(flat), 1))(*flat) if host else None
    return _lib.load().gnot_gather_rows(src, C, table_dev, th, len(table) if B is None else B, dst, None)


GOOD = [[0, 10, 0, 10, 0, 0], [10, 7, 10, 3, 5, 2 ** 32 - 1]]


def test_gather_refuses_null_pointers_and_bad_sizes():
    assert _gather(GOOD, src=None) == E_INVALID
    assert _gather(GOOD, table_dev=None) == E_INVALID
    assert _gather(GOOD, dst=None) == E_INVALID
    assert _gather(GOOD, host=False) == E_INVALID
    assert _gather(GOOD, B=0) == E_INVALID
    assert _gather(GOOD, B=-1) == E_INVALID
    assert _gather(GOOD, C=0) == E_INVALID
    assert "gather_rows" in _lib.load().gnot_last_error().decode()


@pytest.mark.parametrize("col,value", [(1, -1), (3, -1), (3, 8), (1, 2 ** 31), (4, -1), (4, 2 ** 32), (5, -1),
                                       (5, 2 ** 32)],
                         ids=["n<0", "k<0", "k>n", "n=2^31", "lo<0", "lo=2^32", "hi<0", "hi=2^32"])
def test_gather_refuses_a_bad_segment(col, value):
    table = [list(r) for r in GOOD]
    table[1][col] = value
    if (col, value) == (1, 2 ** 31):
        table[1][3] = 3
    assert _gather(table) == E_INVALID


def test_gather_refuses_a_broken_destination_chain():
    assert _gather([[0, 10, 1, 10, 0, 0]]) == E_INVALID                              # dst_row0[0] != 0
    assert _gather([[0, 10, 0, 10, 0, 0], [10, 7, 9, 3, 0, 0]]) == E_INVALID         # overlaps its predecessor
    assert _gather([[0, 10, 0, 10, 0, 0], [10, 7, 11, 3, 0, 0]]) == E_INVALID        # leaves a hole


def test_gather_of_no_rows_launches_nothing_and_succeeds():
    assert _gather([[0, 0, 0, 0, 0, 0], [0, 9, 0, 0, 1, 2]]) == 0


# ------------------------------------------------------------------ DeviceLoader's tables
def _dataset(n=7):
    rng = np.random.default_rng(5)
    return data.DeviceDataset([data.synthetic_sample(rng, int(rng.integers(40, 120)), fn_points=(int(rng.integers(10, 30)),))
                               for _ in range(n)], "cpu")


def test_tables_come_from_the_generator_alone():
    ds = _dataset()
    mk = lambda seed: data.DeviceLoader(ds, 2, shuffle=True, points_per_mesh=32,
                                        generator=torch.Generator().manual_seed(seed))
    a, b, c = mk(1), mk(1), mk(2)
    torch.manual_seed(0)
    before = torch.get_rng_state()
    ta = [a.epoch_tables(), a.epoch_tables()]
    assert torch.equal(torch.get_rng_state(), before)          # the global generator is not touched
    torch.manual_seed(99)
    tb = [b.epoch_tables(), b.epoch_tables()]
    assert ta == tb
    assert ta[0] != ta[1]                                       # the next epoch draws on
    assert c.epoch_tables() != ta[0]
    # without a generator of its own: torch's global one
    g1, g2 = (data.DeviceLoader(ds, 2, shuffle=True, points_per_mesh=32) for _ in range(2))
    torch.manual_seed(3)
    t1 = g1.epoch_tables()
    torch.manual_seed(3)
    assert g2.epoch_tables() == t1


def test_tables_describe_the_batches():
    ds = _dataset(7)
    assert len(ds) == 7 and ds.x_all.shape == (ds.x_off[-1], 2) and ds.theta.shape == (7, 1)
    loader = data.DeviceLoader(ds, 3, shuffle=True, points_per_mesh=50, generator=torch.Generator().manual_seed(0))
    tables = loader.epoch_tables()
    assert len(tables) == len(loader) == 3
    assert len(data.DeviceLoader(ds, 3, drop_last=True)) == 2 and len(data.DeviceLoader(ds, 3, drop_last=True).epoch_tables()) == 2
    assert sorted(s for t in tables for s in t["samples"]) == list(range(7))
    keys = set()
    for t in tables:
        for b, (s, (s0, n, d0, k, lo, hi)) in enumerate(zip(t["samples"], t["x"])):
            assert (s0, n) == (ds.x_off[s], ds.x_off[s + 1] - ds.x_off[s])
            assert k == min(50, n) and d0 == t["x_off"][b] and t["x_off"][b + 1] == d0 + k
            assert 0 <= lo < 2 ** 32 and 0 <= hi < 2 ** 32
            keys.add((lo, hi))
            assert t["theta"][b] == [s, 1, b, 1, 0, 0]
            f0, fn, fd, fk, _, _ = t["fns"][0][b]                 # input functions are always whole
            assert (f0, fn, fk) == (ds.fn_offs[0][s], ds.fn_offs[0][s + 1] - ds.fn_offs[0][s], fn)
            assert fd == t["fn_offs"][0][b]
    assert len(keys) == 7
    # full resolution in dataset order: identity segments, nothing drawn
    torch.manual_seed(0)
    before = torch.get_rng_state()
    full = data.DeviceLoader(ds, 3).epoch_tables()
    assert torch.equal(torch.get_rng_state(), before)
    assert [t["samples"] for t in full] == [[0, 1, 2], [3, 4, 5], [6]]
    assert all(n == k for t in full for (_, n, _, k, _, _) in t["x"])


def test_loader_refuses_bad_arguments_and_a_host_dataset():
    ds = _dataset(2)
    with pytest.raises(ValueError):
        data.DeviceLoader(ds, 0)
    with pytest.raises(ValueError):
        data.DeviceLoader(ds, 2, points_per_mesh=0)
    with pytest.raises(RuntimeError, match="GPU"):
        next(iter(data.DeviceLoader(ds, 2)))
