"""The Fourier-feature embedding on the GPU (csrc/fourier.hip, gnot_plan_set_fourier, GNOT(..., x_fourier=,
fn_fourier=)):

  1. the embed kernel point by point against sin / cos of the exact product in float64, |err| <= 2^-21 (four
     ulps of 1: room for a correctly reduced single-precision routine -- numpy's float32 sin stays within 6.9e-8
     of float64 on these points, a range reduction in fp32 revolutions misses by 8.9e-5); raw columns bitwise,
     pad columns exact zeros; the worst error goes to profiles/fourier_parity.txt;
  2. the backward kernel against the float64 formula, |err| <= (2^-21 + (4 n + 3) 2^-24) S with
     S = |g_0| + sum_k f_k (|g_cos,k| + |g_sin,k|) (the trig bound plus naive fp32 summation over 4 n + 3 terms),
     with one gradient source and with two added;
  3. the engine path is the kernel plus the existing path, bitwise: model A with the embedding against the plain
     wide model B on fourier_embed of the inputs;
  4. parity against float64: the stock-torch port of the wide configuration on fourier_features of the float64
     inputs (fourier_util.reference), golden_util.check_parity_per_sample's 1e-4 rule, and dx / dtheta / dfn
     against float64 autograd through fourier_features at 1e-4 norm-wise per tensor; bf16 mode, MoE recompute, an
     empty sample;
  5. the padded calling convention; 6. point sharding over two ranks; 7. the training loop, bitwise against the
     wide model on a dataset embedded up front.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fourier_util as FU
from golden_util import check_parity, check_parity_per_sample, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


# ------------------------------------------------------------------ 1, 2: the kernels
@functools.lru_cache(maxsize=None)
def _pool():
    """float32 test values in [-4, 4]: a uniform grid, 0, -0, a denormal, +-2^k, and v = a / 2^8 for the float32
    neighbours a of every multiple of pi / 2 up to 4 * 2^8 -- at order 8 the highest frequency's argument
    f v is then a itself, up to 1024 rad"""
    grid = np.linspace(-4, 4, 1001).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40] + [s * 2.0 ** k for k in range(-12, 3) for s in (1, -1)], np.float32)
    m = np.arange(1, int(1024 / (np.pi / 2)) + 1)
    a = (m * (np.pi / 2)).astype(np.float32)
    near = np.concatenate([a, np.nextafter(a, np.float32(0)), np.nextafter(a, np.float32(2000))])
    near = near[near <= 1024] / np.float32(256)
    pool = np.concatenate([grid, special, near, -near]).astype(np.float32)
    assert np.abs(pool).max() <= 4 and np.abs(pool.astype(np.float64) * 256).max() > 1020
    return pool


def _values(rows, C, seed):
    """[rows, C] values out of the pool: a stride coprime to its size walks all of it, from a start that
    depends on the case"""
    pool = _pool()
    idx = (seed * 97 + np.arange(rows * C, dtype=np.int64) * 389) % len(pool)
    assert np.gcd(389, len(pool)) == 1
    return pool[idx].reshape(rows, C)


_WORST = {}
KERNEL_CASES = [(n, C, rows) for n in (1, 3, 8) for C in (1, 2, 3, 5) for rows in (1, 63, 257)]
# beside the grid of shapes above: the whole pool at every order (C = 3, as many rows as it takes)
POOL_CASES = [(n, 3, -1) for n in (1, 3, 8)]


def _embed_case(n, C, rows):
    if rows < 0:
        pool = _pool()
        rows = -(-len(pool) // C)
        v = np.resize(pool, rows * C).reshape(rows, C)
    else:
        v = _values(rows, C, seed=100 * n + 10 * C + rows)
    return v


@pytest.mark.parametrize("n,C,rows", KERNEL_CASES + POOL_CASES)
def test_embed_kernel_point_by_point(n, C, rows):
    from gnot_amd import fourier_embed
    v, whole_pool = _embed_case(n, C, rows), rows < 0
    rows = v.shape[0]
    W, pad = 4 * n + 3, 3
    t = torch.from_numpy(v).to(DEV)
    dense = fourier_embed(t, n)
    pitched = fourier_embed(t, n, ld=C * W + pad)
    torch.cuda.synchronize()
    assert dense.shape == (rows, C * W) and pitched.shape == (rows, C * W + pad)
    assert torch.equal(dense.view(torch.int32), pitched[:, :C * W].contiguous().view(torch.int32))
    assert torch.equal(pitched[:, C * W:].contiguous().view(torch.int32),
                       torch.zeros(rows, pad, dtype=torch.int32, device=DEV))       # exact (+0) zeros
    got = dense.cpu().numpy()
    # raw columns: the input bit for bit (the sign of -0 and the denormal included)
    assert np.array_equal(got[:, ::W].view(np.int32), v.view(np.int32))
    want = FU.formula64(v, n)                      # sin / cos of the exact product: f_k v is exact in float64
    err = np.abs(got.astype(np.float64) - want)
    worst = float(err.max())
    w = np.unravel_index(int(err.argmax()), err.shape)
    print(f"\nembed n={n} C={C} rows={rows}: worst |err| {worst:.3e} at v={v[w[0], w[1] // W]!r} column {w[1] % W}")
    key = (n, "pool" if whole_pool else "shapes")
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    assert worst <= 2.0 ** -21, (worst, v[w[0], w[1] // W], w[1] % W)


@pytest.mark.parametrize("sources", [1, 2])
@pytest.mark.parametrize("n,C,rows", KERNEL_CASES)
def test_embed_backward_kernel(n, C, rows, sources):
    from gnot_amd import fourier_embed
    from gnot_amd.fourier import fourier_embed_bwd
    v = _embed_case(n, C, rows)
    W = 4 * n + 3
    rng = np.random.default_rng(1000 * n + 10 * C + rows)
    ld, lda, ldb = C * W + 1, C * W + 2, C * W                 # three different pitches
    ga = rng.standard_normal((rows, lda)).astype(np.float32)
    gb = rng.standard_normal((rows, ldb)).astype(np.float32) if sources == 2 else None
    emb = fourier_embed(torch.from_numpy(v).to(DEV), n, ld=ld)
    dv = fourier_embed_bwd(emb, torch.from_numpy(ga).to(DEV), n, C,
                           None if gb is None else torch.from_numpy(gb).to(DEV))
    again = fourier_embed_bwd(emb, torch.from_numpy(ga).to(DEV), n, C,
                              None if gb is None else torch.from_numpy(gb).to(DEV))
    torch.cuda.synchronize()
    assert dv.shape == (rows, C) and torch.equal(dv.view(torch.int32), again.view(torch.int32))
    g = ga[:, :C * W].astype(np.float64) + (0 if gb is None else gb[:, :C * W].astype(np.float64))
    want, S = FU.formula64_bwd(v, g, n)
    err = np.abs(dv.cpu().numpy().astype(np.float64) - want)
    bound = (2.0 ** -21 + W * 2.0 ** -24) * S
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"\nembed bwd n={n} C={C} rows={rows} sources={sources}: worst |err| / bound {ratio:.3f}")
    _WORST[(n, f"bwd{sources}")] = max(_WORST.get((n, f"bwd{sources}"), 0.0), ratio)
    assert (err <= bound).all(), ratio


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    """profiles/fourier_parity.txt: the worst figures of the kernel tests above, written when the module is done
    and all of them ran"""
    yield
    if len(_WORST) < 12:               # a partial run (-k ...) leaves the file alone
        return
    fig = lambda k, f: format(_WORST[k], f)
    lines = ["Fourier embedding kernels against float64 (tests/test_gpu_fourier.py)",
             "forward: worst |err| against sin / cos of the exact product; bound 2^-21 = 4.768e-07",
             "backward: worst |err| / ((2^-21 + (4 n + 3) 2^-24) S); bound 1"]
    for n in (1, 3, 8):
        lines.append(f"n = {n}: forward, the shape grid {fig((n, 'shapes'), '.3e')}, the whole pool "
                     f"{fig((n, 'pool'), '.3e')}; backward, one source {fig((n, 'bwd1'), '.3f')}, two sources "
                     f"{fig((n, 'bwd2'), '.3f')}")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fourier_parity.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------ the model cases
def _t(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV).requires_grad_(grad)


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()


def _packed(case, xs, thetas, fns_ps):
    I = FU.CASES[case]["I"]
    x = np.concatenate(xs)
    fns = [np.concatenate([fns_ps[b][i] for b in range(len(xs))]) for i in range(I)]
    return (x, _off([len(a) for a in xs]), np.stack(thetas), fns,
            [_off([len(fns_ps[b][i]) for b in range(len(xs))]) for i in range(I)])


@functools.lru_cache(maxsize=None)
def _fx(case, Ns=tuple(FU.NS)):
    """the case's models' weights, inputs and float64 reference (computed once, shared, never modified)"""
    A, _ = FU.models(case)
    xs, thetas, fns_ps, Gs = FU.inputs(case, Ns=list(Ns))
    params = FU.params64(A)
    samples, grads, e32 = FU.reference(case, params, xs, thetas, fns_ps, Gs)
    return dict(sd=A.state_dict(), params=params, xs=xs, thetas=thetas, fns_ps=fns_ps, Gs=Gs, samples=samples,
                grads=grads, e32=e32, out=np.concatenate([s["out"] for s in samples]))


def _gpu_models(case, sd):
    A, B = FU.models(case)
    A.load_state_dict(sd)
    B.load_state_dict(sd)
    return A.to(DEV), B.to(DEV)


def _run(m, x, x_off, theta, fns, fn_offs, G, want):
    """forward + backward of a packed batch; want: x, theta and the input functions require grad"""
    xt, tt, ft = _t(x, want), _t(theta, want), [_t(f, want) for f in fns]
    m.zero_grad(set_to_none=True)
    out = m.forward_packed(xt, x_off, tt, ft, fn_offs)
    (out * _t(G)).sum().backward()
    torch.cuda.synchronize()
    res = dict(out=out.detach().clone(), pg={k: p.grad.detach().clone() for k, p in m.named_parameters()})
    if want:
        res.update(dx=xt.grad, dtheta=tt.grad, dfns=[f.grad for f in ft])
    return res


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ 3: kernel + existing path, bitwise
@pytest.mark.parametrize("case", ["d64", "d256"])
def test_engine_path_is_the_kernel_plus_the_existing_path(case):
    from gnot_amd import fourier_embed
    c, fx = FU.CASES[case], _fx(case)
    A, B = _gpu_models(case, fx["sd"])
    x, x_off, theta, fns, fn_offs = _packed(case, fx["xs"], fx["thetas"], fx["fns_ps"])
    G = np.concatenate(fx["Gs"])
    a = _run(A, x, x_off, theta, fns, fn_offs, G, want=False)
    ex = fourier_embed(_t(x), c["nx"])
    ef = [fourier_embed(_t(f), c["nf"]) if c["nf"] else _t(f) for f in fns]
    assert ex.shape == (len(x), FU.IN * FU.width(c["nx"]))
    b = _run(B, ex.cpu().numpy(), x_off, theta, [f.cpu().numpy() for f in ef], fn_offs, G, want=False)
    assert _same_bits(a["out"], b["out"])
    assert list(a["pg"]) == list(b["pg"])
    for k in a["pg"]:
        assert _same_bits(a["pg"][k], b["pg"][k]), k
    # asking for input gradients leaves output and parameter gradients alone; a second run gives the same bits
    w1 = _run(A, x, x_off, theta, fns, fn_offs, G, want=True)
    w2 = _run(A, x, x_off, theta, fns, fn_offs, G, want=True)
    for r in (w1, w2):
        assert _same_bits(a["out"], r["out"])
        assert all(_same_bits(a["pg"][k], r["pg"][k]) for k in a["pg"])
    assert w1["dx"].shape == (len(x), FU.IN) and all(g.shape == (len(f), FU.F) for g, f in zip(w1["dfns"], fns))
    assert _same_bits(w1["dx"], w2["dx"]) and _same_bits(w1["dtheta"], w2["dtheta"])
    assert all(_same_bits(p, q) for p, q in zip(w1["dfns"], w2["dfns"]))
    # dtheta does not pass through the embedding: model B's, bit for bit
    bw = _run(B, ex.cpu().numpy(), x_off, theta, [f.cpu().numpy() for f in ef], fn_offs, G, want=True)
    assert _same_bits(w1["dtheta"], bw["dtheta"])


# ------------------------------------------------------------------ 4: parity against float64
def _got(r):
    np64 = lambda t: t.detach().double().cpu().numpy()
    return dict(out=np64(r["out"]), grads={k: np64(v) for k, v in r["pg"].items()}, dx=np64(r["dx"]),
                dtheta=np64(r["dtheta"]), dfns=[np64(f) for f in r["dfns"]])


def _input_grad_errors(got, fx):
    """norm-wise relative error per tensor: dx, dtheta, every dfn, and all of them concatenated"""
    I = len(got["dfns"])
    S = fx["samples"]
    ref = [np.concatenate([s["dx"] for s in S]), np.stack([s["dtheta"] for s in S])] + \
          [np.concatenate([s["dfns"][i] for s in S]) for i in range(I)]
    mine = [got["dx"], got["dtheta"]] + got["dfns"]
    errs = [rel(g, r) for g, r in zip(mine, ref)]
    return errs, rel(np.concatenate([g.ravel() for g in mine]), np.concatenate([r.ravel() for r in ref]))


@pytest.mark.parametrize("case,prec,recompute", [("d64", "fp32", False), ("d256", "fp32", False),
                                                 ("d256", "fp32", True), ("d256", "bf16", False),
                                                 ("d64b", "fp32", False)])
def test_parity_against_float64(case, prec, recompute):
    fx = _fx(case)
    A, _ = _gpu_models(case, fx["sd"])
    A.set_precision(prec)
    A.set_moe_recompute(recompute)
    x, x_off, theta, fns, fn_offs = _packed(case, fx["xs"], fx["thetas"], fx["fns_ps"])
    got = _got(_run(A, x, x_off, theta, fns, fn_offs, np.concatenate(fx["Gs"]), want=True))
    errs, e_all = _input_grad_errors(got, fx)
    print(f"\nfourier {case} {prec} recompute={recompute}: out {rel(got['out'], fx['out']):.2e} dx {errs[0]:.2e} "
          f"dtheta {errs[1]:.2e} dfns {[f'{e:.2e}' for e in errs[2:]]} all {e_all:.2e}")
    if prec == "fp32":
        bad = check_parity_per_sample(got, fx)
        assert not bad, bad
        assert all(e <= 1e-4 for e in errs), errs
    else:
        # tests/test_gpu_input_grads.py's bf16 bars: 1e-2 norm-wise on the output, on the parameter gradients
        # concatenated, on all input gradients concatenated and on dx; 2e-2 on each other input gradient
        assert rel(got["out"], fx["out"]) <= 1e-2
        keys = sorted(fx["grads"])
        assert rel(np.concatenate([got["grads"][k].ravel() for k in keys]),
                   np.concatenate([fx["grads"][k].ravel() for k in keys])) <= 1e-2
        assert e_all <= 1e-2 and errs[0] <= 1e-2, (e_all, errs)
        assert all(e <= 2e-2 for e in errs), errs


def test_parity_with_an_empty_sample():
    case = "d64"
    fx = _fx(case, Ns=(65, 0, 1))
    A, _ = _gpu_models(case, fx["sd"])
    x, x_off, theta, fns, fn_offs = _packed(case, fx["xs"], fx["thetas"], fx["fns_ps"])
    assert x_off == [0, 65, 65, 66]
    got = _got(_run(A, x, x_off, theta, fns, fn_offs, np.concatenate(fx["Gs"]), want=True))
    for k, v in [("out", got["out"]), ("dx", got["dx"]), ("dtheta", got["dtheta"])] + \
            [(f"dfn{i}", g) for i, g in enumerate(got["dfns"])] + list(got["grads"].items()):
        assert np.isfinite(v).all(), k
    assert np.array_equal(got["dtheta"][1], np.zeros(FU.TH))                    # exact zeros for the empty sample
    for i, g in enumerate(got["dfns"]):
        assert np.array_equal(g[fn_offs[i][1]:fn_offs[i][2]], np.zeros((FU.MS[1], FU.F)))
    bad = check_parity_per_sample(got, fx)
    assert not bad, bad
    errs, _ = _input_grad_errors(got, fx)
    assert all(e <= 1e-4 for e in errs), errs


# ------------------------------------------------------------------ 5: the padded call
def test_padded_call_matches_the_port_on_embedded_padded_tensors():
    """A(x_padded, theta, fns_stacked): padding happens before the embedding, a zero pad row embeds to
    [0, 1 .., 0 ..], which is what the wide reference sees -- the port of the wide configuration on
    fourier_features of the padded tensors, pad rows included."""
    from gnot_amd import fourier_features
    from oracle import torch_port
    case = "d64b"
    c, fx = FU.CASES[case], _fx(case)
    A, _ = _gpu_models(case, fx["sd"])
    rng = np.random.default_rng(11)
    B, N, M, I = 2, 96, 40, c["I"]
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    x = r32(rng.uniform(-1, 1, (B, N, FU.IN)))
    x[1, 70:] = 0.0                                    # the zero-padded tail of the shorter sample
    th = r32(rng.random((B, FU.TH)))
    fns = r32(rng.uniform(-1, 1, (I, B, M, FU.F)))
    fns[0, 1, 25:] = 0.0
    G = r32(rng.standard_normal((B, N, FU.OUT)))
    xg, tg, fg = _t(x, True), _t(th, True), _t(fns, True)
    out = A(xg, tg, fg)
    (out * _t(G)).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == (B, N, FU.OUT) and xg.grad.shape == x.shape and fg.grad.shape == fns.shape
    sd64 = {k: torch.tensor(v) for k, v in fx["params"].items()}
    xr, tr, fr = (torch.tensor(a).requires_grad_(True) for a in (x, th, fns))
    ref = torch_port.gnot_forward(sd64, FU.wide_cfg(case), fourier_features(xr, c["nx"]), tr,
                                  [fourier_features(fr[i], c["nf"]) for i in range(I)])
    (ref * torch.tensor(G)).sum().backward()
    errs = {"out": rel(out.detach().double().cpu().numpy(), ref.detach().numpy())}
    for name, got, want in (("dx", xg.grad, xr.grad), ("dtheta", tg.grad, tr.grad), ("dfns", fg.grad, fr.grad)):
        errs[name] = rel(got.double().cpu().numpy(), want.numpy())
    print(f"\nfourier padded {case}: {errs}")
    assert all(e <= 1e-4 for e in errs.values()), errs


# ------------------------------------------------------------------ 6: point sharding
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank(rank, world, port, case, q):
    """One rank of the d = 64 case: its slice of every sample's x, the input functions whole.  Every rank
    reports its output rows, dx rows, dtheta, dfns and rank-summed parameter gradients; rank 0 checks."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gnot-replication_amd"), os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gnot_amd import parallel as par
        fx = _fx(case)
        A, _ = _gpu_models(case, fx["sd"])
        A.set_point_shard(par.PointShardComm(stage_via_host=True))
        Ns = [len(a) for a in fx["xs"]]
        loc_off, ranges = par.shard_offsets(Ns, rank, world)
        _, _, theta, fns, fn_offs = _packed(case, fx["xs"], fx["thetas"], fx["fns_ps"])
        x = _t(np.concatenate([fx["xs"][b][lo:hi] for b, (lo, hi) in enumerate(ranges)]).reshape(-1, FU.IN), True)
        th, ft = _t(theta, True), [_t(f, True) for f in fns]
        G = _t(np.concatenate([fx["Gs"][b][lo:hi] for b, (lo, hi) in enumerate(ranges)]).reshape(-1, FU.OUT))
        out = A.forward_packed(x, loc_off, th, ft, fn_offs, n_global=Ns)
        (out * G).sum().backward()
        h = A.engine().grad_flat.cpu()
        dist.all_reduce(h)                             # parameter gradients: sum over ranks
        A.engine().grad_flat.copy_(h.to(DEV))
        torch.cuda.synchronize()
        np64 = lambda t: t.detach().double().cpu().numpy()
        mine = dict(ranges=ranges, out=np64(out), dx=np64(x.grad), dtheta=np64(th.grad), dfns=[np64(f.grad) for f in ft],
                    grads={k: np64(p.grad) for k, p in A.named_parameters()})
        parts = [None] * world
        dist.all_gather_object(parts, mine)
        if rank == 0:
            errs = []
            S = fx["samples"]
            full = dict(out=[np.full_like(s["out"], np.nan) for s in S], dx=[np.full_like(s["dx"], np.nan) for s in S])
            for p in parts:
                k = 0
                for b, (lo, hi) in enumerate(p["ranges"]):
                    full["out"][b][lo:hi] = p["out"][k:k + hi - lo]
                    full["dx"][b][lo:hi] = p["dx"][k:k + hi - lo]
                    k += hi - lo
            errs += check_parity(np.concatenate(full["out"]), parts[0]["grads"], fx)     # tests/test_gpu_shard.py's rule
            e = rel(np.concatenate(full["dx"]), np.concatenate([s["dx"] for s in S]))
            if not e <= 1e-4:
                errs.append(f"dx {e:.3e}")
            for r, p in enumerate(parts):              # every rank holds the rank sums, summed once
                for k in parts[0]["grads"]:
                    if not np.array_equal(p["grads"][k], parts[0]["grads"][k]):
                        errs.append(f"rank {r} holds another {k} gradient than rank 0")
                e = rel(p["dtheta"], np.stack([s["dtheta"] for s in S]))
                if not e <= 1e-4:
                    errs.append(f"rank {r} dtheta {e:.3e}")
                for i in range(len(p["dfns"])):
                    e = rel(p["dfns"][i], np.concatenate([s["dfns"][i] for s in S]))
                    if not e <= 1e-4:
                        errs.append(f"rank {r} dfn{i} {e:.3e}")
                    if not np.array_equal(p["dfns"][i], parts[0]["dfns"][i]):
                        errs.append(f"rank {r} holds another dfn{i} than rank 0")
            q.put(errs)
    except Exception as e:  # report instead of hanging the other rank's collectives
        if rank == 0:
            q.put([f"rank0 exception: {e!r}"])
        raise
    finally:
        dist.destroy_process_group()


def test_point_sharded_over_two_ranks():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, "d64", q)) for r in range(world)]
    for p in procs:
        p.start()
    errs = q.get(timeout=200)
    for p in procs:
        p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert not errs, errs


# ------------------------------------------------------------------ 7: the training loop
def _train_sets():
    from gnot_amd import data
    rng = np.random.default_rng(17)
    mk = lambda k: [data.synthetic_sample(rng, int(rng.integers(40, 131)), fn_points=(int(rng.integers(10, 30)),) * 2)
                    for _ in range(k)]
    return mk(6), mk(2)


def test_training_loop_equals_the_wide_model_on_an_embedded_dataset(tmp_path):
    from gnot_amd import Normalizer, data, fourier_embed, train
    import train_step_util as U
    case = "d64"
    c, fx = FU.CASES[case], _fx(case)
    tr, te = _train_sets()
    runs = []
    for embedded_up_front in (False, True):
        A, B = _gpu_models(case, fx["sd"])
        sets = [data.DeviceDataset(s, DEV) for s in (tr, te)]
        assert all(40 <= b - a <= 130 for a, b in zip(sets[0].x_off, sets[0].x_off[1:])) and len(sets[0]) == 6
        if embedded_up_front:
            for ds in sets:
                ds.x_all = fourier_embed(ds.x_all, c["nx"])
                ds.fn_all = [fourier_embed(f, c["nf"]) for f in ds.fn_all]
        model = B if embedded_up_front else A
        hist = train.fit(model, data.DeviceLoader(sets[0], 2), data.DeviceLoader(sets[1], 2), epochs=2,
                         log=lambda msg: None)
        runs.append((hist, U.flat_params(model).clone()))
    (h0, p0), (h1, p1) = runs
    assert len(h0[0]) == 2 and len(h0[1]) == 2 and all(np.isfinite(h0[0] + h0[1]))
    assert h0 == h1                                                # per-epoch train losses and test metrics
    assert torch.equal(U.bits(p0), U.bits(p1))                     # the final parameters
    assert not torch.equal(U.bits(p0), U.bits(U.flat_params(_gpu_models(case, fx["sd"])[0])))   # it did train

    # statistics of the embedded x cannot be folded into the checkpoint: refused before the first step
    A, _ = _gpu_models(case, fx["sd"])
    before = U.flat_params(A).clone()
    ident = lambda C: ([0.0] * C, [1.0] * C)
    nz = Normalizer.from_stats(([0.5, 0.5], [0.3, 0.3]), ident(1), ident(1), [ident(3), ident(3)], device=DEV)
    ds = data.DeviceDataset(tr, DEV)
    with pytest.raises(ValueError, match=r"statistics for x \(x_fourier=3\)"):
        train.fit(A, data.DeviceLoader(ds, 2, normalizer=nz), data.DeviceLoader(ds, 2, normalizer=nz), epochs=1,
                  normalizer=nz, checkpoint=str(tmp_path / "ck.pth"), log=lambda msg: None)
    assert torch.equal(U.bits(before), U.bits(U.flat_params(A))) and not (tmp_path / "ck.pth").exists()
