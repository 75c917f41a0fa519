"""What the GPU tests of the native training step share (test_gpu_train_options.py, test_gpu_train_state.py,
test_gpu_ema.py, test_gpu_param_groups_kernel.py, test_gpu_train_bits.py): arrays with sentinels around them, the
hyper-parameter vector, the norm entries, the four update entries and the slice-table ones, a small model with
list-of-batches loaders, and the inputs and replays of the two files of recorded bits."""
import ctypes

import numpy as np
import torch

import lp_util as L
from gnot_amd import _lib, train

SMALL = (2, 1, 3, 1, 1, 32, 2, 32, 32, 2, 4, 1)      # the model of test_train.py / test_gpu_train_loop.py
NS = [1, 257, 8195, 524291]
PAD = -7.0                                            # around every array's declared size
BAD = [float("nan"), float("inf"), float("-inf")]

bits = lambda t: t.view(torch.int32)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def based(src, offset=0):
    """src on the device, its base `offset` floats behind a 16-byte boundary, PAD elements all around it:
    (the view of src's size, the allocation)"""
    n = src.numel()
    buf = torch.full((offset + n + 3,), PAD, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n]
    view.copy_(src)
    assert view.data_ptr() % 16 == 4 * offset
    return view, buf


def intact(view, buf):
    """the PAD elements in front of and behind the view are untouched"""
    k = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:k] == PAD).all()) and bool((buf[k + view.numel():] == PAD).all())


def hyper(h7=1.0, t=3, w=None):
    """the 8 floats of gnot_adamw_step; with w, the 9 of gnot_adamw_step_ema"""
    h = [1e-3, 0.9, 0.999, 1e-8, 1e-2, 1 - 0.9 ** t, 1 - 0.999 ** t, h7] + ([] if w is None else [w])
    return torch.tensor(h, dtype=torch.float32).cuda()


def grad(n, offset, seed=0):
    """a gradient of n elements whose base is `offset` floats behind a 16-byte boundary"""
    g, buf = based(torch.randn(n, generator=torch.Generator().manual_seed(1000 * seed + n)), offset)
    buf[:offset] = 1e30                  # a stray read wrecks the norm
    buf[offset + n:] = 1e30
    return g


def norm(g, hyper, max_norm=None):
    """clip [2] (device) of gnot_grad_clip (max_norm given) or gnot_grad_norm; nothing is written behind
    the declared sizes of work and clip"""
    lib, n = _lib.load(), g.numel()
    nw = lib.gnot_grad_clip_work_floats(n)
    work = torch.full((nw + 1,), PAD, dtype=torch.float32, device="cuda")
    clip = torch.full((3,), PAD, dtype=torch.float32, device="cuda")
    if max_norm is None:
        _lib.check(lib.gnot_grad_norm(g.data_ptr(), n, hyper.data_ptr(), work.data_ptr(), clip.data_ptr(), stream()))
    else:
        _lib.check(lib.gnot_grad_clip(g.data_ptr(), n, hyper.data_ptr(), max_norm, work.data_ptr(), clip.data_ptr(),
                                      stream()))
    assert float(work[nw]) == PAD and float(clip[2]) == PAD
    return clip[:2]


class Arrays:
    """param / exp_avg / exp_avg_sq / ema of n elements in the middle of a run, PAD elements around each; the
    ema base is `offset` floats behind a 16-byte boundary"""

    NAMES = ("p", "m", "v", "e")

    def __init__(self, n, offset=0, values=None):
        """values: (p, m, v, e) tensors of n elements; None: drawn from the seed n"""
        if values is None:
            gen = torch.Generator().manual_seed(n)
            p = torch.randn(n, generator=gen)
            values = (p, 0.1 * torch.randn(n, generator=gen), 0.01 * torch.rand(n, generator=gen),
                      p + 0.05 * torch.randn(n, generator=gen))
        self.n, self.offset = n, offset
        (self.p, self.pb), (self.m, self.mb), (self.v, self.vb), (self.e, self.eb) = (
            based(values[0]), based(values[1]), based(values[2]), based(values[3], offset))

    def copy(self):
        return Arrays(self.n, self.offset, (self.p, self.m, self.v, self.e))

    def differing(self, other):
        """names of the arrays (allocations, sentinels included) whose bits differ"""
        return [k for k in self.NAMES if not torch.equal(bits(getattr(self, k + "b")), bits(getattr(other, k + "b")))]

    def same(self, other):
        return self.differing(other) == []

    def _check_pads(self):
        for k in self.NAMES:
            assert intact(getattr(self, k), getattr(self, k + "b")), k

    def step(self, g, hyper, clip=None, guard=None):
        """the entry without the average of the kind: plain, clipped or guarded"""
        lib = _lib.load()
        a = (self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, hyper.data_ptr())
        if guard is not None:
            _lib.check(lib.gnot_adamw_step_guarded(*a, clip.data_ptr(), guard.data_ptr(), stream()))
        elif clip is not None:
            _lib.check(lib.gnot_adamw_step_clipped(*a, clip.data_ptr(), stream()))
        else:
            _lib.check(lib.gnot_adamw_step(*a, stream()))
        self._check_pads()

    def ema_update(self, weight):
        _lib.check(_lib.load().gnot_ema_update(self.e.data_ptr(), self.p.data_ptr(), self.n, weight.data_ptr(),
                                               stream()))
        self._check_pads()

    def step_ema(self, g, hyper, clip=None, guard=None):
        _lib.check(_lib.load().gnot_adamw_step_ema(
            self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.e.data_ptr(), self.n,
            hyper.data_ptr(), None if clip is None else clip.data_ptr(), None if guard is None else guard.data_ptr(),
            stream()))
        self._check_pads()


def guard():
    return torch.zeros(3, dtype=torch.int32, device="cuda")      # {skipped, skipped now} and an element behind


class Table:
    """a slice table on the device and on the host, and the group constants"""

    def __init__(self, rows, ghyper):
        self.n = len(rows)
        self.host = (ctypes.c_int64 * (3 * self.n))(*[v for r in rows for v in r])
        self.dev = torch.tensor(rows, dtype=torch.int64).cuda()
        self.ghyper = torch.tensor(ghyper, dtype=torch.float32).cuda()
        self.G = len(ghyper)


def groups_norm(g, n, hyper, table, max_norm=None):
    """clip [2] of gnot_grad_clip_groups (max_norm given) or gnot_grad_norm_groups; work has nslices floats and
    nothing is written behind them or behind clip"""
    lib = _lib.load()
    work = torch.full((table.n + 1,), PAD, dtype=torch.float32, device="cuda")
    clip = torch.full((3,), PAD, dtype=torch.float32, device="cuda")
    if max_norm is None:
        _lib.check(lib.gnot_grad_norm_groups(g.data_ptr(), n, hyper.data_ptr(), table.dev.data_ptr(), table.host,
                                             table.n, work.data_ptr(), clip.data_ptr(), stream()))
    else:
        _lib.check(lib.gnot_grad_clip_groups(g.data_ptr(), n, hyper.data_ptr(), max_norm, table.dev.data_ptr(),
                                             table.host, table.n, work.data_ptr(), clip.data_ptr(), stream()))
    assert float(work[table.n]) == PAD and float(clip[2]) == PAD
    return clip[:2]


def groups_step(a, g, hyper, table, clip=None, guard=None, ema=False):
    """gnot_adamw_step_groups on the Arrays a; the PAD elements around every array stay"""
    _lib.check(_lib.load().gnot_adamw_step_groups(
        a.p.data_ptr(), g.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), a.e.data_ptr() if ema else None, a.n,
        hyper.data_ptr(), table.ghyper.data_ptr(), table.G, table.dev.data_ptr(), table.host, table.n,
        None if clip is None else clip.data_ptr(), None if guard is None else guard.data_ptr(), stream()))
    a._check_pads()


def bad_index(n, where):
    """first / last element; "tail": inside the 1 to 3 elements behind the last 16-byte load of an aligned
    base (n % 4 of them); "head": inside the up to 3 elements in front of the first one of a base a float off"""
    return {"first": 0, "last": n - 1, "tail": n - 1 - (n % 4) // 2, "head": min(1, n - 1)}[where]


# ------------------------------------------------------------------ model-level helpers
class Stop(Exception):
    pass


_BATCHES = {}


def batches(n_train=8):
    """list-of-batches loaders: n_train / 2 train and two test batches of two meshes of 40 to 120 points"""
    if n_train not in _BATCHES:
        from gnot_amd import data
        rng = np.random.default_rng(3)
        mk_s = lambda k: [data.synthetic_sample(rng, int(rng.integers(40, 120)), fn_points=(int(rng.integers(10, 30)),))
                          for _ in range(k)]
        mk = lambda s: list(torch.utils.data.DataLoader(data.NS2dData(s), batch_size=2, shuffle=False,
                                                        collate_fn=data.collate_packed))
        _BATCHES[n_train] = mk(mk_s(n_train)), mk(mk_s(4))
    return _BATCHES[n_train]


def model(seed=0):
    from gnot_amd import GNOT
    torch.manual_seed(seed)
    return GNOT(*SMALL).cuda()


def flat_params(model):
    return torch.cat([t.detach().reshape(-1) for l in model.linears() for t in (l.weight, l.bias)])


def first_grad_norm():
    """the gradient norm of the first train batch at the initial weights (sizes max_grad_norm)"""
    m, (tr, _) = model(), batches()
    eng = m.engine()
    eng.param_grads = False
    pred, off, y = train._forward_batch(m, tr[0], torch.device("cuda"))
    train.RelL2Loss()(off, pred, y).backward()
    return float(eng.grad_flat.norm())


# ------------------------------------------------------------------ recorded bits (tests/golden/train_step_bits.npz)
# A set of inputs and what one build of the library makes of them through every entry of the training step,
# as plain arrays: test_gpu_train_bits.py replays the inputs of the committed file, which an earlier build wrote
# (scripts/diag_bitwise_ab.py record), and requires its bits; the same script compares two builds on more sizes.
STEP_H7 = (1.0, 0.5, 0.3)                 # 0.3: grad * hyper[7] is inexact, the plain entry fuses it into exp_avg
STEP_KINDS = ("plain", "clip_lt1", "clip_eq1", "guard", "guard_nan")
LOSS_SIZES, LOSS_C = [37, 1, 2049], 3     # two splits and a one-row sample


def step_cases(n):
    """(grad offset, hyper[7], kind, with the average) of every recorded update at size n: all of them at the
    small sizes, a few at the others (each stores up to four arrays of n elements)"""
    if n > 257:
        return [(1, 0.3, "plain", False), (0, 0.3, "plain", True), (1, 0.5, "guard", True)]
    return [(o, h7, kind, ema) for o in (0, 1) for h7 in STEP_H7 for kind in STEP_KINDS for ema in (False, True)]


def step_inputs(ns):
    """the inputs of step_replay for the sizes ns, drawn here once and stored with the results"""
    inp = {"ns": np.array(ns, dtype=np.int64)}
    for n in ns:
        a = Arrays(n)
        g = grad(n, 0)
        for k, t in (("p", a.p), ("m", a.m), ("v", a.v), ("e", a.e), ("g", g)):
            inp[f"n{n}.{k}"] = t.cpu().numpy()
        norm64 = float(g.double().pow(2).sum().sqrt())
        # per hyper[7]: a max_norm that clips and one that does not
        inp[f"n{n}.max_norm"] = np.array([[0.5 * h7 * norm64, 2.0 * h7 * norm64] for h7 in STEP_H7], dtype=np.float32)
    gen = torch.Generator().manual_seed(11)
    rows = sum(LOSS_SIZES)
    inp["loss.pred"] = torch.randn(rows, LOSS_C, generator=gen).numpy()
    inp["loss.tgt"] = torch.randn(rows, LOSS_C, generator=gen).numpy()
    return inp


def _based_on(src, offset):
    """grad()'s layout around given values"""
    g, buf = based(src, offset)
    buf[:offset] = 1e30
    buf[offset + src.numel():] = 1e30
    return g


def step_replay(inp):
    """{name: array of bits} of every update case of step_cases and of both losses on the inputs inp"""
    as_bits = lambda t: t.detach().cpu().contiguous().view(torch.int32).numpy()
    out = {}
    for n in (int(n) for n in inp["ns"]):
        p, m, v, e, g = (torch.from_numpy(np.asarray(inp[f"n{n}.{k}"])) for k in "pmveg")
        g_nan = g.clone()
        g_nan[n // 2] = float("nan")
        for offset, h7, kind, ema in step_cases(n):
            name = f"n{n}.o{offset}.h{h7}.{kind}.{'ema' if ema else 'raw'}"
            hy = hyper(h7, w=9 / 11 if ema else None)
            start = Arrays(n, offset, (p, m, v, e))
            gd = _based_on(g_nan if kind == "guard_nan" else g, offset)
            lo, hi = (float(x) for x in inp[f"n{n}.max_norm"][STEP_H7.index(h7)])
            clip = {"plain": None, "clip_lt1": lo, "clip_eq1": hi, "guard": lo, "guard_nan": None}[kind]
            clip = None if kind == "plain" else norm(gd, hy, clip)
            gu = guard() if kind.startswith("guard") else None
            got = start.copy()
            (got.step_ema if ema else got.step)(gd, hy, clip, gu)
            if clip is not None:
                out[name + ".clip"] = as_bits(clip)
            if gu is not None:
                out[name + ".guard"] = gu.cpu().numpy()
            if kind == "guard_nan":
                out[name + ".untouched"] = np.array([got.differing(start) == []])
            else:
                assert got.differing(start) == ["p", "m", "v"] + ["e"] * ema, name
                for k in "pmve" if ema else "pmv":
                    out[f"{name}.{k}"] = as_bits(getattr(got, k))
    off = np.concatenate([[0], np.cumsum(LOSS_SIZES)]).tolist()
    for cls in (train.RelL2Loss, train.MSELoss):
        pred = torch.from_numpy(np.asarray(inp["loss.pred"])).cuda().requires_grad_(True)
        loss = cls()(off, pred, torch.from_numpy(np.asarray(inp["loss.tgt"])).cuda())
        loss.backward()
        out[f"loss.{cls.__name__}.loss"] = as_bits(loss.reshape(1))
        out[f"loss.{cls.__name__}.dpred"] = as_bits(pred.grad)
    return out


# ------------------------------------------------------------------ recorded bits (tests/golden/train_family_bits.npz)
# The same for the loss family and the slice-table update, written by the build before RelL2Loss / MSELoss moved
# onto the Lp kernels and the two AdamW kernels onto one element update (scripts/diag_bitwise_ab.py record-family).
FAMILY_F1E_OFF = [0, 37, 37, 38, 2087]    # LOSS_SIZES' rows with an empty sample: gnot_rel_l2_loss alone takes one
FAMILY_F2_SIZES = [4096, 4097]            # one channel: the exact multiple of the split, two splits and a row
FAMILY_WEIGHTS = [1.0, 0.0, 3.0]
FAMILY_NZ = ([0.3, -1.7, 0.05], [1.9, 0.6, 3.3])      # y mean / std, no powers of two: pred * std + mean rounds
GROUPS_N, GROUPS_H7 = 257, 0.3
GROUPS_ROWS = [[0, 100, 0], [130, 127, 1]]            # elements 100 to 129 are frozen
GROUPS_GHYPER = [[1.0, 0.01], [0.5, 0.0]]
GROUPS_KINDS = ("plain", "clip_lt1", "guard", "guard_nan")
GROUPS_NAN_AT = 50                                    # guard_nan: a trainable element of the gradient


def _groups_frozen():
    live = torch.zeros(GROUPS_N, dtype=torch.bool)
    for begin, length, _ in GROUPS_ROWS:
        live[begin:begin + length] = True
    return ~live


def loss_inputs():
    """the inputs of loss_replay, drawn here once and stored with the results"""
    gen = torch.Generator().manual_seed(12)
    inp = {}
    for name, rows, C in (("f1", sum(LOSS_SIZES), LOSS_C), ("f2", sum(FAMILY_F2_SIZES), 1)):
        inp[name + ".pred"] = torch.randn(rows, C, generator=gen).numpy()
        inp[name + ".tgt"] = (torch.randn(rows, C, generator=gen) + 0.5).numpy()     # every denominator positive
    a = Arrays(GROUPS_N)
    g = torch.randn(GROUPS_N, generator=gen)
    for k, t in (("p", a.p), ("m", a.m), ("v", a.v), ("e", a.e), ("g", g)):
        inp["g." + k] = t.cpu().numpy()
    norm64 = float(g[~_groups_frozen()].double().pow(2).sum().sqrt())
    inp["g.max_norm"] = np.array([0.5 * GROUPS_H7 * norm64], dtype=np.float32)       # it clips
    return inp


def _loss_pass(fn, off, pred, tgt, grad, terms=False):
    """(loss [1], terms or None, dpred or None) of one pass of the loss module fn"""
    p = pred.clone().requires_grad_(grad)
    loss, e = fn.loss_and_terms(off, p, tgt) if terms else (fn(off, p, tgt), None)
    if grad:
        loss.backward()
    return loss.detach().reshape(1), e, p.grad


def loss_replay(inp):
    """{name: array of bits} of the blocks F1, F1e, F2 (RelL2Loss, MSELoss and LpLoss; raw and with a normalizer,
    with and without component weights) and G (gnot_adamw_step_groups behind the slice-table norm entries) on the
    inputs inp.  Asserts on the way that an LpLoss gives the same bits with and without the terms, and that
    rel2 / mse without weights give those of RelL2Loss / MSELoss."""
    from gnot_amd import Normalizer
    as_bits = lambda t: t.detach().cpu().contiguous().view(torch.int32).numpy()
    same = lambda x, y: (x is None and y is None) or torch.equal(bits(x), bits(y))
    dev = lambda k: torch.from_numpy(np.asarray(inp[k])).cuda()
    nzs = lambda C: (("raw", None), ("nz", Normalizer.from_stats(([0.0], [1.0]), ([0.0], [1.0]),
                                                                 (FAMILY_NZ[0][:C], FAMILY_NZ[1][:C]))))
    out = {}

    def classes(block, off, pred, tgt):
        """RelL2Loss and, unless a sample is empty, MSELoss: {(class name, raw / nz): (loss, None, dpred)}"""
        res = {}
        for cls in (train.RelL2Loss, train.MSELoss)[:1 if block == "f1e" else 2]:
            for tag, nz in nzs(pred.shape[1]):
                res[cls.__name__, tag] = r = _loss_pass(cls(nz), off, pred, tgt, True)
                out[f"{block}.{cls.__name__}.{tag}.loss"] = as_bits(r[0])
                out[f"{block}.{cls.__name__}.{tag}.dpred"] = as_bits(r[2])
        return res

    def family(block, off, pred, tgt, ref, weights, tags, dpred_kinds):
        for kind in L.KINDS:
            for wtag, w in weights:
                for tag, nz in nzs(pred.shape[1]):
                    if tag not in tags:
                        continue
                    grad = kind in L.DIFFERENTIABLE
                    r = _loss_pass(train.LpLoss(kind, w, nz), off, pred, tgt, grad, terms=True)
                    bare = _loss_pass(train.LpLoss(kind, w, nz), off, pred, tgt, grad)
                    name = f"{block}.lp.{kind}.{wtag}.{tag}"
                    assert same(r[0], bare[0]) and same(r[2], bare[2]), name
                    if w is None and kind in ("rel2", "mse"):
                        c = ref["RelL2Loss" if kind == "rel2" else "MSELoss", tag]
                        assert same(r[0], c[0]) and same(r[2], c[2]), name
                    out[name + ".loss"], out[name + ".terms"] = as_bits(r[0]), as_bits(r[1])
                    if kind in dpred_kinds:
                        out[name + ".dpred"] = as_bits(r[2])

    off1 = np.concatenate([[0], np.cumsum(LOSS_SIZES)]).tolist()
    pred, tgt = dev("f1.pred"), dev("f1.tgt")
    family("f1", off1, pred, tgt, classes("f1", off1, pred, tgt), (("u", None), ("w", FAMILY_WEIGHTS)),
           ("raw", "nz"), L.DIFFERENTIABLE)
    classes("f1e", FAMILY_F1E_OFF, pred, tgt)
    off2 = np.concatenate([[0], np.cumsum(FAMILY_F2_SIZES)]).tolist()
    pred, tgt = dev("f2.pred"), dev("f2.tgt")
    family("f2", off2, pred, tgt, classes("f2", off2, pred, tgt), (("u", None),), ("raw",), ("rel1", "l1"))

    # G: the slice-table update; the frozen range of the gradient holds NaN, and every array is stored as its
    # whole allocation, the elements around it and the frozen gap included
    n, frozen = GROUPS_N, _groups_frozen()
    p, m, v, e = (torch.from_numpy(np.asarray(inp["g." + k])) for k in "pmve")
    g = torch.from_numpy(np.asarray(inp["g.g"])).clone()
    g[frozen] = float("nan")
    g_nan = g.clone()
    g_nan[GROUPS_NAN_AT] = float("nan")
    max_norm = float(inp["g.max_norm"][0])
    table = Table(GROUPS_ROWS, GROUPS_GHYPER)
    for offset in (0, 1):
        for kind in GROUPS_KINDS:
            for ema in (False, True):
                name = f"g.o{offset}.{kind}.{'ema' if ema else 'raw'}"
                hy = hyper(GROUPS_H7, w=9 / 11 if ema else None)
                start = Arrays(n, offset, (p, m, v, e))
                gd = _based_on(g_nan if kind == "guard_nan" else g, offset)
                clip = None if kind == "plain" else groups_norm(gd, n, hy, table,
                                                                None if kind == "guard_nan" else max_norm)
                gu = guard() if kind.startswith("guard") else None
                got = start.copy()
                groups_step(got, gd, hy, table, clip, gu, ema)
                if clip is not None:
                    out[name + ".clip"] = as_bits(clip)
                if gu is not None:
                    out[name + ".guard"] = gu.cpu().numpy()
                if kind == "guard_nan":
                    out[name + ".untouched"] = np.array([got.differing(start) == []])
                else:
                    assert got.differing(start) == ["p", "m", "v"] + ["e"] * ema, name
                for k in "pmve" if ema else "pmv":
                    out[f"{name}.{k}b"] = as_bits(getattr(got, k + "b"))
    return out
