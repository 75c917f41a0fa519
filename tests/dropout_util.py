"""Shared pieces of the attention-dropout tests (tests/test_dropout.py on the CPU, tests/test_gpu_dropout*.py): a
vectorised numpy Philox4x32-10, the mask * scale array of a call site, and the float64 reference of
GNOT(..., attn_dropout=p) -- the stock-torch port (oracle/torch_port.py) with the return value of its `_attention`
multiplied by the site's mask * scale, wrapped at run time and restored on exit (the device of
tests/prenorm_util.py; oracle/ is not edited).  Models, shapes and inputs are prenorm_util's."""
import contextlib

import numpy as np
import torch

import golden_util as GU
import prenorm_util as PU

P_DROP = 0.25
SEED = 1234
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 of counter = (c0, c1, c2, c3) and key = (k0, k1), each an integer or an array of values
    below 2^32 (broadcast against each other); returns the four output words as uint64 arrays holding uint32
    values.  uint64 arithmetic: a 32 x 32 product fits."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) for c in counter])
    k0, k1 = [np.asarray(k, np.uint64) for k in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return c0, c1, c2, c3


def threshold(p):
    """(T, scale) as the library forms them: p rounded to float32, T = floor(p 2^32 + 0.5) in double,
    scale = float32(2^32 / (2^32 - T))"""
    p32 = float(np.float32(p))
    T = int(np.floor(p32 * 2.0 ** 32 + 0.5))
    return T, np.float32(2.0 ** 32 / (2.0 ** 32 - T))


def random_words(Ns, glo, C, seed, step, site):
    """the uint32 word of every element: [sum Ns, C] (uint64 holding uint32), rows packed sample after sample,
    sample b's row j being its point glo[b] + j"""
    nq = (C + 3) // 4
    out = []
    for b, n in enumerate(Ns):
        pts = (np.arange(n, dtype=np.uint64) + np.uint64(glo[b]))[:, None]
        q = np.arange(nq, dtype=np.uint64)[None, :]
        w = philox4x32_10((pts, np.uint64(b), (np.uint64(site) << np.uint64(8)) | q, np.uint64(step)),
                          (seed & 0xFFFFFFFF, seed >> 32))
        out.append(np.stack(w, -1).reshape(n, 4 * nq)[:, :C])
    return np.concatenate(out) if out else np.zeros((0, C), np.uint64)


def mask_scale(Ns, glo, C, seed, step, site, p):
    """float32 [sum Ns, C]: scale where the element is kept, 0 where it is dropped"""
    T, scale = threshold(p)
    keep = random_words(Ns, glo, C, seed, step, site) >= np.uint64(T)
    return np.where(keep, scale, np.float32(0)).astype(np.float32)


def model(case, seed=5, **kw):
    """GNOT(..., attn_dropout=P_DROP, dropout_seed=SEED) of a prenorm_util case on the CPU, without pre-norm, with
    the weights of prenorm_util.model(case) (kw overrides)"""
    from gnot_amd import GNOT
    torch.manual_seed(seed)
    return GNOT(*GU.model_args(PU.cfg_of(case)), **dict(dict(attn_dropout=P_DROP, dropout_seed=SEED), **kw))


@contextlib.contextmanager
def masked_port(masks):
    """Inside the context oracle.torch_port._attention returns its value times masks[k], k counting its calls: the
    port then IS the model with dropout.  masks: one float array [N, d] per call, in gnot_forward's order (site
    0, 1, .. of the first reference call, then of the next).  Only the port module's own name is replaced, and it is
    restored on exit."""
    from oracle import torch_port
    plain = torch_port._attention
    calls = [0]

    def attention(p, prefix, query, srcs, H, key_names, value_names):
        out = plain(p, prefix, query, srcs, H, key_names, value_names)
        m = masks[calls[0]]
        calls[0] += 1
        return out * torch.as_tensor(np.asarray(m, np.float64), dtype=out.dtype)[None]

    torch_port._attention = attention
    try:
        yield calls
    finally:
        torch_port._attention = plain


def site_masks(cfg, Ns, steps, p=P_DROP, seed=SEED, glo=None, order=None):
    """the masks of masked_port for one B = 1 reference call per non-empty sample (in `order`, default sample
    order): steps[b] the dropout step of sample b's forward (an int: every sample the same packed forward)"""
    d, L = cfg["d"], cfg["n_attn_layers"]
    glo = [0] * len(Ns) if glo is None else glo
    steps = [steps] * len(Ns) if np.isscalar(steps) else steps
    off = np.concatenate([[0], np.cumsum(Ns)])
    per_site = {}
    masks = []
    for b in (order if order is not None else [b for b in range(len(Ns)) if Ns[b] > 0]):
        for site in range(2 * L):
            k = (steps[b], site)
            if k not in per_site:
                per_site[k] = mask_scale(Ns, glo, d, seed, steps[b], site, p)
            masks.append(per_site[k][off[b]:off[b + 1]])
    return masks


def reference(cfg, params, xs, thetas, fns_ps, Gs, steps=0, p=P_DROP, seed=SEED):
    """golden_util.port_reference of the model with dropout: (samples, grads, e32) as check_parity_per_sample
    takes them, e32 the float32 masked port's own distance from the float64 one.  The samples are those of ONE
    packed forward at step `steps` (or steps[b] per sample)."""
    groups = [[b] for b in range(len(xs)) if len(xs[b]) > 0]
    masks = site_masks(cfg, [len(x) for x in xs], steps, p, seed)
    passes = []
    for dt in ("float64", "float32"):
        with masked_port(masks) as calls:
            passes.append(GU._port_pass(cfg, params, xs, thetas, fns_ps, Gs, groups, dt))
        assert calls[0] == len(masks)
    return GU._port_compare(cfg, xs, thetas, fns_ps, Gs, *passes)


def as_fx(ref):
    samples, grads, e32 = ref
    return dict(samples=samples, grads=grads, e32=e32, out=np.concatenate([s["out"] for s in samples]))


_FX = {}


def fixture(case):
    """(model on the CPU, inputs, fx) of a case at step 0: fx the dict check_parity_per_sample takes (samples,
    grads, e32, out).  Computed once per process, shared by the tests that need it and left unchanged."""
    if case not in _FX:
        m = model(case)
        data = PU.inputs(case)
        _FX[case] = (m, data, as_fx(reference(PU.cfg_of(case), PU.params64(m), *data, steps=0)))
    return _FX[case]
