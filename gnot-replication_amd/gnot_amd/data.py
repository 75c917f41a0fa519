"""NS2d-format data and batching without dgl.

Reference format (dataset.py:7, 19-36): a pickled list of samples `[X (N x in), Y (N x out), theta
(length theta_dim), [f_1 (M_1 x F), f_2, ...]]` of numpy arrays.  `NS2dData` mirrors
`NS2dDataset.__getitem__` (dataset.py:43-44) with plain tensors instead of a DGLGraph, and reads the
pickle with a restricted unpickler that only rebuilds numpy arrays and plain containers (a pickle
cannot run code through it).  `collate_packed` is the packed-offsets batch the engine consumes
(replacing the padding of main.py:60-82 and utils.py:3-4); `collate_padded` reproduces the
reference's padded tensors exactly, for parity runs.  `synthetic_sample` / `write_ns2d` generate
meshes in the same on-disk format.

`DeviceDataset` / `DeviceLoader` keep the whole dataset in device memory and assemble every packed batch
there with one small kernel per array (libgnot_hip.so gnot_gather_rows), which also draws a per-mesh
subsample of the query points (`points_per_mesh`) as a keyed permutation -- no reference counterpart
(main.py:57-58 batches on the host).
"""
import ctypes
import io
import pickle

import numpy as np
import torch

from . import _lib

_ALLOWED = {
    ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
    ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"),
    ("numpy._core.multiarray", "scalar"), ("builtins", "list"), ("builtins", "tuple"),
}


class _ArrayUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) in _ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"NS2d files may only hold numpy arrays; refusing {module}.{name}")


def safe_load(path):
    with open(path, "rb") as f:
        return _ArrayUnpickler(io.BytesIO(f.read())).load()


def write_ns2d(path, samples):
    """Write samples [[X, Y, theta, [f...]], ...] (numpy) in the reference's pickle format."""
    with open(path, "wb") as f:
        pickle.dump([[np.asarray(s[0]), np.asarray(s[1]), np.asarray(s[2]), [np.asarray(v) for v in s[3]]]
                     for s in samples], f, protocol=4)


def synthetic_sample(rng, n_points, input_dim=2, out_dim=1, theta_dim=1, fn_points=(805,), fn_dim=3):
    """One synthetic mesh in the NS2d layout: coordinates U[0,1]^input_dim, a smooth field as target,
    theta U[0,1], input functions U[0,1]^fn_dim."""
    x = rng.random((n_points, input_dim))
    theta = rng.random(theta_dim)
    y = np.stack([np.sin(np.pi * (c + 1) * x.sum(1)) * (1 + theta[0]) for c in range(out_dim)], 1)
    fns = [rng.random((m, fn_dim)) for m in fn_points]
    return [x.astype(np.float64), y.astype(np.float64), theta, fns]


class NS2dData(torch.utils.data.Dataset):
    """dataset.py:6-44 without dgl: item = (x [N, in], y [N, out], theta, [f_i [M_i, F]])."""

    def __init__(self, path_or_samples):
        self.data = safe_load(path_or_samples) if isinstance(path_or_samples, str) else path_or_samples
        self.items = []
        for s in self.data:
            fns = [torch.from_numpy(np.asarray(f)).float() for f in s[3]] if s[3] else []
            self.items.append((torch.from_numpy(np.asarray(s[0])).float(), torch.from_numpy(np.asarray(s[1])).float(),
                               s[2], fns))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def collate_packed(batch):
    """Packed batch (no padding): x [sum N, in], x_off [B+1], y, theta [B, theta_dim], fns[i] packed with
    fn_offs[i] [B+1].  GNOT.forward_packed(x, x_off, theta, fns, fn_offs) on it equals one unpadded
    B=1 reference call per sample."""
    xs, ys, thetas, fnl = zip(*batch)
    off = [0]
    for x in xs:
        off.append(off[-1] + x.shape[0])
    I = len(fnl[0])
    fns, fn_offs = [], []
    for i in range(I):
        parts = [f[i] for f in fnl]
        o = [0]
        for p in parts:
            o.append(o[-1] + p.shape[0])
        fns.append(torch.cat(parts))
        fn_offs.append(o)
    theta = torch.tensor(np.stack([np.asarray(t, dtype=np.float64) for t in thetas])).float()
    return dict(x=torch.cat(xs), x_off=off, y=torch.cat(ys), theta=theta, fns=fns, fn_offs=fn_offs)


def collate_padded(batch):
    """The reference's batch exactly (main.py:60-82, utils.py:3-4): x zero-padded to the batch max N,
    every input function zero-padded to ONE common max M over all functions and samples, stacked
    [I, B, M, F]; y is returned packed ([sum N, out], main.py:89/93) with the real counts."""
    xs, ys, thetas, fnl = zip(*batch)
    pad = lambda t, L: torch.nn.functional.pad(t, (0, 0, 0, L - t.shape[0]))
    mmax = max((t.shape[0] for arrays in fnl for t in arrays), default=0)
    I = len(fnl[0])
    fns = torch.stack([torch.stack([pad(arrays[i], mmax) for arrays in fnl]) for i in range(I)]) if I else None
    nmax = max(t.shape[0] for t in xs)
    x = torch.stack([pad(t, nmax) for t in xs])
    theta = torch.tensor(np.stack([np.asarray(t, dtype=np.float64) for t in thetas])).float()
    return dict(x=x, theta=theta, fns=fns, y=torch.cat(ys), counts=[t.shape[0] for t in xs])


# ------------------------------------------------------------------ datasets that live on the device
GATHER_COLS = 6      # a gnot_gather_rows table row: {src_row0, n, dst_row0, k, key_lo, key_hi}


def _offsets(sizes):
    off = [0]
    for n in sizes:
        off.append(off[-1] + int(n))
    return off


def _table(src_off, samples, ks=None, keys=None):
    """(rows of a gnot_gather_rows table, packed offsets of the result): segment b is sample samples[b] of an
    array packed by src_off, whole (ks None) or its first ks[b] permuted rows under keys[b] = (lo, hi)"""
    rows, off = [], [0]
    for b, s in enumerate(samples):
        n = src_off[s + 1] - src_off[s]
        k = n if ks is None else ks[b]
        lo, hi = (0, 0) if keys is None else keys[b]
        rows.append([src_off[s], n, off[-1], k, lo, hi])
        off.append(off[-1] + k)
    return rows, off


def gather_tables(x_off, fn_offs, batch_size, shuffle=False, drop_last=False, points_per_mesh=None, generator=None):
    """The gather tables of one epoch over a dataset packed by x_off [S+1] and fn_offs[i] [S+1] (host lists):
    a list with one dict per batch, `samples` (dataset indices), `x` / `fns[i]` / `theta` (table rows, lists
    of GATHER_COLS ints) and the packed offsets `x_off` / `fn_offs` of the batch.  Host arithmetic only.
    The sample order (shuffle) and one 64-bit key per sample (points_per_mesh) are drawn from `generator`
    (None: torch's global CPU generator), the order first, and from nothing else; without shuffle and
    points_per_mesh nothing is drawn."""
    S = len(x_off) - 1
    order = torch.randperm(S, generator=generator).tolist() if shuffle else list(range(S))
    keys = None
    if points_per_mesh is not None:
        if int(points_per_mesh) < 1:
            raise ValueError("points_per_mesh must be at least 1")
        keys = torch.randint(0, 2 ** 32, (S, 2), dtype=torch.int64, generator=generator).tolist()
    theta_off = list(range(S + 1))
    out = []
    for i in range(0, S, batch_size):
        samples = order[i:i + batch_size]
        if drop_last and len(samples) < batch_size:
            break
        ks = bkeys = None
        if keys is not None:     # keys follow the position in the epoch, like the order
            ks = [min(int(points_per_mesh), x_off[s + 1] - x_off[s]) for s in samples]
            bkeys = [tuple(k) for k in keys[i:i + len(samples)]]
        x, off = _table(x_off, samples, ks, bkeys)
        fns = [_table(o, samples) for o in fn_offs]
        out.append(dict(samples=samples, x=x, x_off=off, fns=[t for t, _ in fns], fn_offs=[o for _, o in fns],
                        theta=_table(theta_off, samples)[0]))
    return out


class DeviceDataset:
    """An NS2d-format dataset packed in device memory once: x_all [sum N, in], y_all [sum N, out], theta
    [S, theta_dim], fn_all[i] [sum M_i, F] (fp32) and the host offset lists x_off [S+1], fn_offs[i] [S+1].
    samples_or_data: an NS2dData, or what NS2dData takes (a path or a list of samples).  An MI355X holds
    288 GB; an NS2d training set is a few hundred MB, a few GB at 262k points per mesh."""

    def __init__(self, samples_or_data, device):
        ds = samples_or_data if isinstance(samples_or_data, NS2dData) else NS2dData(samples_or_data)
        if len(ds) == 0:
            raise ValueError("DeviceDataset: no samples")
        xs, ys, thetas, fnl = zip(*ds.items)
        self.device = torch.device(device)
        put = lambda parts: torch.cat(parts).float().contiguous().to(self.device)
        self.x_off = _offsets(x.shape[0] for x in xs)
        self.x_all, self.y_all = put(xs), put(ys)
        # collate_packed's expression, so a gathered row carries the bits of a collated one
        self.theta = torch.tensor(np.stack([np.atleast_1d(np.asarray(t, dtype=np.float64)) for t in thetas])) \
            .float().contiguous().to(self.device)
        self.fn_all = [put([f[i] for f in fnl]) for i in range(len(fnl[0]))]
        self.fn_offs = [_offsets(f[i].shape[0] for f in fnl) for i in range(len(fnl[0]))]

    def __len__(self):
        return len(self.x_off) - 1


class DeviceLoader:
    """A loader of packed batches over a DeviceDataset: iterable, with __len__, yielding collate_packed's dict
    (x, x_off, y, theta, fns, fn_offs; tensors on the device, offsets host lists), every array assembled on the
    device by gnot_gather_rows on the current stream.  train.fit and train.evaluate take it like a DataLoader.
    points_per_mesh=K: x and y of mesh b hold k_b = min(K, N_b) of its points, a uniform subsample without
    replacement and the same rows of both; input functions and theta are always whole.  Every attention
    output is q (K^T V) / (q sum k), a ratio of two sums over points, so a subsample estimates it without any
    rescaling.  None: full meshes in their own order, bit for bit collate_packed's batch.
    The epoch's sample order (shuffle) and every mesh's 64-bit key (points_per_mesh) are drawn when an
    iteration starts, from `generator` (None: torch's global CPU generator) and nothing else
    (gather_tables); the subsample itself is a pure function of (key, N_b), so there is no device random
    state, and train.rng_state / restore_rng_state cover the loader through `.generator`.
    The epoch's tables reach the device as one copy from pinned memory (non_blocking); iterating performs no
    pageable copy and no device-to-host read, and every batch is a fresh allocation of the stream-ordered
    caching allocator, so a step still in flight keeps its batch.
    Padded batches (collate_padded) and slicing a loader over ranks are out of scope: packed batches, one
    process's whole dataset."""

    def __init__(self, dataset, batch_size, shuffle=False, drop_last=False, points_per_mesh=None, generator=None):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        if points_per_mesh is not None and int(points_per_mesh) < 1:
            raise ValueError("points_per_mesh must be at least 1")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.points_per_mesh = None if points_per_mesh is None else int(points_per_mesh)
        self.generator = generator

    def __len__(self):
        S = len(self.dataset)
        return S // self.batch_size if self.drop_last else -(-S // self.batch_size)

    def epoch_tables(self):
        """gather_tables for the next epoch (draws from the generator; needs no GPU)"""
        ds = self.dataset
        return gather_tables(ds.x_off, ds.fn_offs, self.batch_size, self.shuffle, self.drop_last, self.points_per_mesh,
                             self.generator)

    def _gather(self, src, rows, table_dev, rows_out):
        """the [rows_out, C] rows of src that the table selects (host rows `rows`, the same on the device)"""
        dst = torch.empty((rows_out, src.shape[1]), dtype=torch.float32, device=src.device)
        if rows_out:
            host = (ctypes.c_int64 * (len(rows) * GATHER_COLS))(*[v for r in rows for v in r])
            stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
            _lib.check(_lib.load().gnot_gather_rows(src.data_ptr(), src.shape[1], table_dev.data_ptr(), host, len(rows),
                                                    dst.data_ptr(), stream))
        return dst

    def __iter__(self):
        ds = self.dataset
        if not ds.x_all.is_cuda:
            raise RuntimeError("gnot_amd.DeviceLoader assembles batches on a ROCm GPU only (libgnot_hip.so)")
        batches = self.epoch_tables()
        if not batches:
            return
        # every table of the epoch in one pinned tensor and one asynchronous copy; torch's host allocator keeps
        # the pinned block from reuse until the copy has executed
        rows = [r for b in batches for t in [b["x"], b["theta"]] + b["fns"] for r in t]
        pinned = torch.empty((len(rows), GATHER_COLS), dtype=torch.int64, pin_memory=True)
        pinned.copy_(torch.tensor(rows, dtype=torch.int64))
        tables = pinned.to(ds.device, non_blocking=True)
        r0 = 0
        for b in batches:
            B = len(b["samples"])
            dev_table = lambda k: tables[r0 + k * B:r0 + (k + 1) * B]      # the batch's tables: x, theta, fns...
            out = dict(x=self._gather(ds.x_all, b["x"], dev_table(0), b["x_off"][-1]), x_off=b["x_off"],
                       y=self._gather(ds.y_all, b["x"], dev_table(0), b["x_off"][-1]),
                       theta=self._gather(ds.theta, b["theta"], dev_table(1), B),
                       fns=[self._gather(f, t, dev_table(2 + i), o[-1])
                            for i, (f, t, o) in enumerate(zip(ds.fn_all, b["fns"], b["fn_offs"]))],
                       fn_offs=b["fn_offs"])
            r0 += (2 + len(ds.fn_all)) * B
            yield out
