"""NS2d-format data and batching without dgl.

Reference format (dataset.py:7, 19-36): a pickled list of samples `[X (N x in), Y (N x out), theta
(length theta_dim), [f_1 (M_1 x F), f_2, ...]]` of numpy arrays.  `NS2dData` mirrors
`NS2dDataset.__getitem__` (dataset.py:43-44) with plain tensors instead of a DGLGraph, and reads the
pickle with a restricted unpickler that only rebuilds numpy arrays and plain containers (a pickle
cannot run code through it).  `collate_packed` is the packed-offsets batch the engine consumes
(replacing the padding of main.py:60-82 and utils.py:3-4); `collate_padded` reproduces the
reference's padded tensors exactly, for parity runs.  `synthetic_sample` / `write_ns2d` generate
meshes in the same on-disk format.

`Normalizer` holds per-channel statistics of a dataset's arrays (computed on the device, gnot_channel_stats)
and applies unit-Gaussian normalisation in the loader, the losses and the checkpoint.

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
    """Write samples [[X, Y, theta, [f...]], ...] (numpy) in the reference's pickle format.  A sample with a
    fifth entry W [N] (per-point weights, NS2dData(point_weights=True)) is written with it; one without, as
    the reference's four entries."""
    with open(path, "wb") as f:
        pickle.dump([[np.asarray(s[0]), np.asarray(s[1]), np.asarray(s[2]), [np.asarray(v) for v in s[3]]]
                     + ([np.asarray(s[4])] if len(s) > 4 else []) for s in samples], f, protocol=4)


def synthetic_sample(rng, n_points, input_dim=2, out_dim=1, theta_dim=1, fn_points=(805,), fn_dim=3):
    """One synthetic mesh in the NS2d layout: coordinates U[0,1]^input_dim, a smooth field as target,
    theta U[0,1], input functions U[0,1]^fn_dim."""
    x = rng.random((n_points, input_dim))
    theta = rng.random(theta_dim)
    y = np.stack([np.sin(np.pi * (c + 1) * x.sum(1)) * (1 + theta[0]) for c in range(out_dim)], 1)
    fns = [rng.random((m, fn_dim)) for m in fn_points]
    return [x.astype(np.float64), y.astype(np.float64), theta, fns]


def _sample_weights(sample, index, n):
    """the fifth entry of sample `index` as a [n] fp32 tensor, or ValueError (NS2dData(point_weights=True));
    the checks are on the fp32 values the kernels read"""
    if len(sample) < 5:
        raise ValueError(f"NS2dData(point_weights=True): sample {index} has no fifth entry W [N]")
    w = np.asarray(sample[4])
    if not (w.ndim == 1 or (w.ndim == 2 and w.shape[1] == 1)) or w.shape[0] != n:
        raise ValueError(f"NS2dData: the point weights of sample {index} have shape {tuple(w.shape)}, its mesh has "
                         f"{n} points")
    w = torch.from_numpy(np.ascontiguousarray(w.reshape(-1))).float()
    if not bool(torch.isfinite(w).all()):
        raise ValueError(f"NS2dData: the point weights of sample {index} are not all finite")
    if bool((w < 0).any()):
        raise ValueError(f"NS2dData: sample {index} has a negative point weight")
    if not bool((w > 0).any()):
        raise ValueError(f"NS2dData: every point weight of sample {index} is zero")
    return w


class NS2dData(torch.utils.data.Dataset):
    """dataset.py:6-44 without dgl: item = (x [N, in], y [N, out], theta, [f_i [M_i, F]]).
    point_weights: a sample may carry a fifth entry W [N], one weight >= 0 per query point (a quadrature or
    lumped-mass weight, a 0/1 mask, anything else) for the weighted losses and target statistics.  False
    (default): a fifth entry is ignored and the items are the 4-tuples above.  True: every sample must have
    one and the items are 5-tuples (..., w [N] fp32); weights that are not finite, negative, of another length
    than N, or zero on every row of a sample are a ValueError (checked here, on the host)."""

    def __init__(self, path_or_samples, point_weights=False):
        self.data = safe_load(path_or_samples) if isinstance(path_or_samples, str) else path_or_samples
        self.point_weights = bool(point_weights)
        self.items = []
        for i, s in enumerate(self.data):
            fns = [torch.from_numpy(np.asarray(f)).float() for f in s[3]] if s[3] else []
            item = (torch.from_numpy(np.asarray(s[0])).float(), torch.from_numpy(np.asarray(s[1])).float(), s[2], fns)
            if self.point_weights:
                item += (_sample_weights(s, i, item[0].shape[0]),)
            self.items.append(item)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def collate_packed(batch):
    """Packed batch (no padding): x [sum N, in], x_off [B+1], y, theta [B, theta_dim], fns[i] packed with
    fn_offs[i] [B+1].  GNOT.forward_packed(x, x_off, theta, fns, fn_offs) on it equals one unpadded
    B=1 reference call per sample.  Items with point weights (5-tuples, NS2dData(point_weights=True)) add
    w [sum N], packed like y; 4-tuples give the batch above and no such key."""
    if len({len(item) for item in batch}) != 1:
        raise ValueError("collate_packed: items with and without point weights in one batch")
    xs, ys, thetas, fnl, *ws = zip(*batch)
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
    out = dict(x=torch.cat(xs), x_off=off, y=torch.cat(ys), theta=theta, fns=fns, fn_offs=fn_offs)
    if ws:
        out["w"] = torch.cat(ws[0])
    return out


def collate_padded(batch):
    """The reference's batch exactly (main.py:60-82, utils.py:3-4): x zero-padded to the batch max N,
    every input function zero-padded to ONE common max M over all functions and samples, stacked
    [I, B, M, F]; y is returned packed ([sum N, out], main.py:89/93) with the real counts.  Items with point
    weights (5-tuples) are refused: padded batches take none."""
    if any(len(item) != 4 for item in batch):
        raise ValueError("collate_padded takes no point weights (5-tuple items): use collate_packed")
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
    288 GB; an NS2d training set is a few hundred MB, a few GB at 262k points per mesh.
    point_weights: True keeps the samples' per-point weights (NS2dData(point_weights=True); an NS2dData passed
    in must have been built with them) as w_all [sum N], packed like y_all: DeviceLoader then gathers a `w`
    beside every `y`, and Normalizer.fit weighs the target statistics.  False (default): w_all is None."""

    def __init__(self, samples_or_data, device, point_weights=False):
        ds = samples_or_data if isinstance(samples_or_data, NS2dData) else NS2dData(samples_or_data, point_weights)
        if len(ds) == 0:
            raise ValueError("DeviceDataset: no samples")
        if point_weights and not getattr(ds, "point_weights", False):
            raise ValueError("DeviceDataset(point_weights=True): the NS2dData was built without point weights")
        xs, ys, thetas, fnl, *ws = zip(*ds.items)
        self.device = torch.device(device)
        put = lambda parts: torch.cat(parts).float().contiguous().to(self.device)
        self.x_off = _offsets(x.shape[0] for x in xs)
        self.x_all, self.y_all = put(xs), put(ys)
        self.w_all = put(ws[0]) if point_weights else None
        # collate_packed's expression, so a gathered row carries the bits of a collated one
        self.theta = torch.tensor(np.stack([np.atleast_1d(np.asarray(t, dtype=np.float64)) for t in thetas])) \
            .float().contiguous().to(self.device)
        self.fn_all = [put([f[i] for f in fnl]) for i in range(len(fnl[0]))]
        self.fn_offs = [_offsets(f[i].shape[0] for f in fnl) for i in range(len(fnl[0]))]

    def __len__(self):
        return len(self.x_off) - 1


# ------------------------------------------------------------------ unit-Gaussian normalisation
def _block(mean, std, eps):
    """a stats block [3, C] fp32 {mean, std, rstd} from host values, under gnot_channel_stats' rules: a constant
    channel (std <= 1e-6 |mean|) gets std 0 and rstd 1, every other one rstd = 1 / (std + eps) in fp32"""
    mean = torch.as_tensor(np.atleast_1d(np.asarray(mean, dtype=np.float64))).float()
    std = torch.as_tensor(np.atleast_1d(np.asarray(std, dtype=np.float64))).float()
    if mean.shape != std.shape or mean.dim() != 1:
        raise ValueError("Normalizer: mean and std must be vectors of one length")
    const = std <= 1e-6 * mean.abs()
    std = torch.where(const, torch.zeros_like(std), std)
    rstd = torch.where(const, torch.ones_like(std), 1.0 / (std + torch.tensor(eps, dtype=torch.float32)))
    return torch.stack([mean, std, rstd]).contiguous()


class Normalizer:
    """Per-channel unit-Gaussian normalisation of a dataset's inputs and targets, as the original GNOT code
    base's UnitTransformer does it ((v - mean) / (std + 1e-8), metric reported in physical units); the
    replicated main.py trains on raw values.  One stats block per array -- `x`, `theta`, `y` and `fns[i]`, each a
    [3, C] fp32 tensor {mean, std, rstd} on one device, the layout libgnot_hip.so's entries read:
      fit(device_dataset)    the statistics of x_all, theta, every fn_all[i] and y_all, computed where the data
                             lives (gnot_channel_stats: unbiased std, rstd = 1 / (std + eps), a constant channel
                             std 0 / rstd 1); an array whose flag is off gets the identity block (mean 0, std 1,
                             rstd 1), for which both transforms below return their argument's bits (but for the
                             sign of a zero in decode)
      from_stats(...)        the same from host (mean, std) pairs; needs no GPU
      DeviceLoader(normalizer=)   x, theta and the input functions normalised as they are gathered
                             (gnot_gather_rows_affine); y stays raw
      encode_batch(batch)    the same arithmetic, (v - mean) * rstd, in torch ops on a collate_packed batch
                             wherever it lives -- bit for bit the kernel's values
      train.RelL2Loss(normalizer=) / MSELoss(normalizer=)   read the model's output as a normalised prediction
                             and compute loss and metric in physical units (the _affine entries, `y` block)
      decode(out)            out * std_y + mean_y, for inference on normalised weights
      fold(state_dict, n_mlp_num_layers)   the statistics moved into the first and last Linears, so that the
                             checkpoint maps raw inputs to physical outputs with the reference's keys alone
    Out of scope: the point-sharded losses of parallel.py, padded batches (collate_padded), and per-rank
    statistics (every rank fits the same whole dataset and so holds the same blocks)."""

    def __init__(self, x, theta, y, fns=()):
        self.x, self.theta, self.y, self.fns = x, theta, y, list(fns)
        for b in self.blocks().values():
            if b.dim() != 2 or b.shape[0] != 3 or b.dtype != torch.float32:
                raise ValueError("Normalizer: a stats block is a [3, C] fp32 tensor {mean, std, rstd}")

    def blocks(self):
        """{entry name: block} in a fixed order: x, theta, y, fns.0, fns.1, ..."""
        out = {"x": self.x, "theta": self.theta, "y": self.y}
        out.update({f"fns.{i}": b for i, b in enumerate(self.fns)})
        return out

    @staticmethod
    def identity(C, device="cpu"):
        """the block that changes nothing: mean 0, std 1, rstd 1"""
        return torch.tensor([[0.0] * C, [1.0] * C, [1.0] * C], dtype=torch.float32, device=device)

    @classmethod
    def fit(cls, dataset, x=True, theta=True, fns=True, y=True, eps=1e-8):
        """Statistics over a DeviceDataset's arrays on its device (two small kernels per array on the current
        stream, nothing read back).  A dataset with point weights (DeviceDataset(point_weights=True)) gets the
        WEIGHTED statistics of its targets (gnot_channel_stats_weighted: mean = sum w y / sum w, the
        reliability-weights variance, rows of weight zero not read -- a NaN under a mask is harmless); x, theta
        and the input functions are model inputs whatever their weight and stay unweighted."""
        if not dataset.x_all.is_cuda:
            raise RuntimeError("gnot_amd.Normalizer.fit computes on a ROCm GPU only (libgnot_hip.so); "
                               "from_stats builds one from host statistics")
        lib = _lib.load()

        def block(src, on, w=None):
            rows, C = src.shape
            if not on:
                return cls.identity(C, src.device)
            stats = torch.empty((3, C), dtype=torch.float32, device=src.device)
            stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
            if w is None:
                work = torch.empty(lib.gnot_channel_stats_work_floats(rows, C), dtype=torch.float32, device=src.device)
                _lib.check(lib.gnot_channel_stats(src.data_ptr(), rows, C, eps, work.data_ptr(), stats.data_ptr(),
                                                  stream))
            else:
                work = torch.empty(lib.gnot_channel_stats_weighted_work_floats(rows, C), dtype=torch.float32,
                                   device=src.device)
                _lib.check(lib.gnot_channel_stats_weighted(src.data_ptr(), w.data_ptr(), rows, C, eps, work.data_ptr(),
                                                           stats.data_ptr(), stream))
            return stats

        return cls(block(dataset.x_all, x), block(dataset.theta, theta),
                   block(dataset.y_all, y, getattr(dataset, "w_all", None)), [block(f, fns) for f in dataset.fn_all])

    @classmethod
    def from_stats(cls, x, theta, y, fns=(), eps=1e-8, device="cpu"):
        """From host statistics: every argument a (mean, std) pair of vectors (numpy, lists or numbers; float64
        is rounded to fp32 once), fns a list of such pairs.  Needs no GPU."""
        mk = lambda ms: _block(ms[0], ms[1], eps).to(device)
        return cls(mk(x), mk(theta), mk(y), [mk(f) for f in fns])

    def to(self, device):
        """the same statistics on `device` (self if they are there already)"""
        device = torch.device(device)
        if all(b.device == device for b in self.blocks().values()):
            return self
        return Normalizer(self.x.to(device), self.theta.to(device), self.y.to(device), [f.to(device) for f in self.fns])

    def state_dict(self):
        """plain CPU fp32 tensors (copies): {"x", "theta", "y": [3, C], "fns": [[3, F], ...]}; loadable with
        weights_only=True"""
        cp = lambda b: b.detach().cpu().clone()
        return {"x": cp(self.x), "theta": cp(self.theta), "y": cp(self.y), "fns": [cp(f) for f in self.fns]}

    @classmethod
    def from_state_dict(cls, sd, device="cpu"):
        mv = lambda b: b.detach().clone().float().to(device)
        return cls(mv(sd["x"]), mv(sd["theta"]), mv(sd["y"]), [mv(f) for f in sd["fns"]])

    def mismatch(self, other):
        """the first entry (blocks' names) whose statistics differ bitwise from `other`'s -- a Normalizer or a
        state_dict() -- or "fns" for another number of input functions; None: equal.  Compared on the host."""
        a = self.state_dict()
        b = other.state_dict() if isinstance(other, Normalizer) else other
        if len(a["fns"]) != len(b["fns"]):
            return "fns"
        pairs = [(k, a[k], b[k]) for k in ("x", "theta", "y")] + \
                [(f"fns.{i}", p, q) for i, (p, q) in enumerate(zip(a["fns"], b["fns"]))]
        for name, p, q in pairs:
            if p.shape != q.shape or not torch.equal(p.view(torch.int32), q.float().view(torch.int32)):
                return name
        return None

    @staticmethod
    def _encode(v, block):
        b = block.to(device=v.device, dtype=v.dtype)
        return (v - b[0]) * b[2]

    def encode_batch(self, batch):
        """A collate_packed batch with x, theta and every input function normalised, (v - mean) * rstd in torch
        ops on the tensors' own device and dtype (fp32: gnot_gather_rows_affine's bits); y and the offsets are
        passed through.  A padded batch (collate_padded) is refused: its pad rows would stop being zeros."""
        if "counts" in batch:
            raise ValueError("Normalizer.encode_batch takes packed batches (collate_packed) only")
        if len(batch["fns"]) != len(self.fns):
            raise ValueError(f"Normalizer.encode_batch: {len(batch['fns'])} input functions in the batch, "
                             f"{len(self.fns)} in the statistics")
        return dict(batch, x=self._encode(batch["x"], self.x), theta=self._encode(batch["theta"], self.theta),
                    fns=[self._encode(f, b) for f, b in zip(batch["fns"], self.fns)])

    def decode(self, out):
        """a normalised prediction [..., out_dim] in physical units: out * std_y + mean_y"""
        b = self.y.to(device=out.device, dtype=out.dtype)
        return out * b[1] + b[0]

    def fold(self, state_dict, n_mlp_num_layers, dtype=torch.float32):
        """A new state dict (the model and `state_dict` are left alone) whose network takes raw inputs and
        returns physical outputs, with the keys of `state_dict` (the reference's; every entry the fold does not
        name, such as a pre-norm model's `pre_norm_eps` buffer, is copied as it is):
          first Linear of each encoder, W' = W diag(r), b' = b - W' m, with (m, r) = (mean, rstd) of
            x.layers.0                     the x and theta blocks concatenated (the encoder's input is [x, theta])
            gating.layers.0                the x block
            input_func_mlps.i.layers.0     input function i's block
          last Linear of out (out.layers.{2 n_mlp_num_layers}): W' = diag(std_y) W, b' = std_y b + mean_y.
        Computed in float64 on the host and rounded to `dtype` once.  In exact arithmetic the folded network on
        raw inputs IS decode(network(encode(inputs))); in fp32 the first pre-activation now takes W' v - W' m
        as a difference of two numbers |mean| / std times larger than itself, so folding costs about
        (|mean| / std) 2^-24 relative there (x in [100, 108]: 3e-6).  Evaluate with the unfolded weights and
        the normalizer where that matters."""
        sd = {k: v.detach().cpu().clone() for k, v in state_dict.items()}
        f64 = lambda t: t.detach().cpu().double()

        def first(prefix, blocks):
            m = torch.cat([f64(b[0]) for b in blocks])
            r = torch.cat([f64(b[2]) for b in blocks])
            W = f64(sd[prefix + ".layers.0.weight"])
            if W.shape[1] != m.numel():
                raise ValueError(f"Normalizer.fold: {prefix}.layers.0 takes {W.shape[1]} channels, the statistics "
                                 f"hold {m.numel()}")
            W2 = W * r[None, :]
            sd[prefix + ".layers.0.weight"] = W2.to(dtype)
            sd[prefix + ".layers.0.bias"] = (f64(sd[prefix + ".layers.0.bias"]) - W2 @ m).to(dtype)

        first("x", [self.x, self.theta])
        first("gating", [self.x])
        for i, b in enumerate(self.fns):
            first(f"input_func_mlps.{i}", [b])
        last = f"out.layers.{2 * max(int(n_mlp_num_layers), 1)}"
        mean, std = f64(self.y[0]), f64(self.y[1])
        W = f64(sd[last + ".weight"])
        if W.shape[0] != std.numel():
            raise ValueError(f"Normalizer.fold: {last} has {W.shape[0]} outputs, the statistics hold {std.numel()}")
        sd[last + ".weight"] = (std[:, None] * W).to(dtype)
        sd[last + ".bias"] = (std * f64(sd[last + ".bias"]) + mean).to(dtype)
        return sd


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
    normalizer: a Normalizer over this dataset's arrays; x, theta and every input function are then gathered
    through gnot_gather_rows_affine -- normalised in the copy, bit for bit Normalizer.encode_batch of the plain
    batch -- and y stays raw (plain gather), for a loss that holds the same normalizer.  None (default): the
    calls above, unchanged.
    A dataset with point weights (DeviceDataset(point_weights=True)) adds `w` [sum k] to every batch, gathered
    through x's table like y (one more gnot_gather_rows, one channel), so a points_per_mesh subsample carries
    the weights of the rows it drew; the tables are the same.  Without weights a batch has no such key.
    Padded batches (collate_padded) and slicing a loader over ranks are out of scope: packed batches, one
    process's whole dataset."""

    def __init__(self, dataset, batch_size, shuffle=False, drop_last=False, points_per_mesh=None, generator=None,
                 normalizer=None):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        if points_per_mesh is not None and int(points_per_mesh) < 1:
            raise ValueError("points_per_mesh must be at least 1")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.points_per_mesh = None if points_per_mesh is None else int(points_per_mesh)
        self.generator = generator
        self.normalizer = normalizer
        if normalizer is not None:
            have = [b.shape[1] for b in (normalizer.x, normalizer.theta, normalizer.y, *normalizer.fns)]
            need = [t.shape[1] for t in (dataset.x_all, dataset.theta, dataset.y_all, *dataset.fn_all)]
            if have != need:
                raise ValueError(f"DeviceLoader: the normalizer's channels (x, theta, y, fns...) are {have}, "
                                 f"the dataset's {need}")

    def __len__(self):
        S = len(self.dataset)
        return S // self.batch_size if self.drop_last else -(-S // self.batch_size)

    def epoch_tables(self):
        """gather_tables for the next epoch (draws from the generator; needs no GPU)"""
        ds = self.dataset
        return gather_tables(ds.x_off, ds.fn_offs, self.batch_size, self.shuffle, self.drop_last, self.points_per_mesh,
                             self.generator)

    def _gather(self, src, rows, table_dev, rows_out, stats=None):
        """the [rows_out, C] rows of src that the table selects (host rows `rows`, the same on the device);
        stats: a stats block on src's device, the rows are normalised with it as they are copied"""
        dst = torch.empty((rows_out, src.shape[1]), dtype=torch.float32, device=src.device)
        if rows_out:
            host = (ctypes.c_int64 * (len(rows) * GATHER_COLS))(*[v for r in rows for v in r])
            stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
            if stats is None:
                rc = _lib.load().gnot_gather_rows(src.data_ptr(), src.shape[1], table_dev.data_ptr(), host, len(rows),
                                                  dst.data_ptr(), stream)
            else:
                rc = _lib.load().gnot_gather_rows_affine(src.data_ptr(), src.shape[1], table_dev.data_ptr(), host,
                                                         len(rows), stats.data_ptr(), dst.data_ptr(), stream)
            _lib.check(rc)
        return dst

    def __iter__(self):
        ds = self.dataset
        if not ds.x_all.is_cuda:
            raise RuntimeError("gnot_amd.DeviceLoader assembles batches on a ROCm GPU only (libgnot_hip.so)")
        batches = self.epoch_tables()
        if not batches:
            return
        nz = None if self.normalizer is None else self.normalizer.to(ds.device)
        sx, sth, sfn = (None, None, [None] * len(ds.fn_all)) if nz is None else (nz.x, nz.theta, nz.fns)
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
            out = dict(x=self._gather(ds.x_all, b["x"], dev_table(0), b["x_off"][-1], sx), x_off=b["x_off"],
                       y=self._gather(ds.y_all, b["x"], dev_table(0), b["x_off"][-1]),
                       theta=self._gather(ds.theta, b["theta"], dev_table(1), B, sth),
                       fns=[self._gather(f, t, dev_table(2 + i), o[-1], st)
                            for i, (f, t, o, st) in enumerate(zip(ds.fn_all, b["fns"], b["fn_offs"], sfn))],
                       fn_offs=b["fn_offs"])
            if getattr(ds, "w_all", None) is not None:      # the rows y took: x's table, one channel
                out["w"] = self._gather(ds.w_all.view(-1, 1), b["x"], dev_table(0), b["x_off"][-1]).view(-1)
            r0 += (2 + len(ds.fn_all)) * B
            yield out
