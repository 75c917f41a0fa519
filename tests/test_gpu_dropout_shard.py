"""GNOT(..., attn_dropout=0.25) point-sharded over 2 ranks (gloo, both on cuda:0, spawned as
tests/test_gpu_prenorm_shard.py does): every rank counts the same steps and keys its rows on the global (sample,
point), so the sharded run drops exactly the elements of the unsharded one.  Output rows, parameter gradients
summed over the ranks, dx, and dtheta / dfns after gnot_input_grads' rank sums against the masked float64
reference of tests/dropout_util.py under the per-sample parity rule; rank 1's dropped rows themselves."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "d64s"            # d = 64, 4 heads, one input function, one block


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gnot-replication_amd"), os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import dropout_util as DU
        import golden_util as GU
        import prenorm_util as PU
        from gnot_amd import parallel as par
        m, (xs, thetas, fns_ps, Gs), fx = DU.fixture(CASE)
        Ns = [len(a) for a in xs]
        x_off = np.concatenate([[0], np.cumsum(Ns)])
        dev = torch.device("cuda", 0)
        m = m.to(dev)
        m.set_point_shard(par.PointShardComm(stage_via_host=True))
        loc_off, ranges = par.shard_offsets(Ns, rank, world)
        rows = np.concatenate([np.arange(x_off[b] + lo, x_off[b] + hi) for b, (lo, hi) in enumerate(ranges)]).astype(np.int64)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
        x = t(np.concatenate(xs)[rows]).requires_grad_(True)
        theta = t(np.stack(thetas)).requires_grad_(True)
        fn = t(np.concatenate([f[0] for f in fns_ps])).requires_grad_(True)
        fn_off = np.concatenate([[0], np.cumsum([len(f[0]) for f in fns_ps])]).tolist()
        out = m.forward_packed(x, loc_off, theta, [fn], [fn_off], n_global=Ns)
        (out * t(np.concatenate(Gs)[rows])).sum().backward()       # gnot_input_grads sums dtheta / dfns over the ranks
        h = m.engine().grad_flat.cpu()
        dist.all_reduce(h)                                        # parameter gradients: sum over ranks
        m.engine().grad_flat.copy_(h.to(dev))
        torch.cuda.synchronize()
        f64 = lambda v: v.detach().double().cpu().numpy()
        # this rank's dropped rows: zero exactly at the global mask's positions
        a = m.engine().debug_tensor("b0.a", len(rows), 64).cpu().numpy()
        zeros_ok = bool(np.array_equal(a == 0, DU.mask_scale(Ns, [0] * len(Ns), 64, DU.SEED, 0, 0, DU.P_DROP)[rows] == 0))
        parts = [None] * world
        dist.all_gather_object(parts, (rows, f64(out), f64(x.grad), f64(theta.grad), f64(fn.grad), zeros_ok))
        if rank == 0:
            P = int(x_off[-1])
            got = dict(out=np.zeros((P, PU.OUT)), dx=np.zeros((P, PU.IN)), dtheta=parts[0][3], dfns=[parts[0][4]],
                       grads={k: f64(p.grad) for k, p in m.named_parameters()})
            errs = []
            for r, (r_rows, o, dx, dth, dfn, ok) in enumerate(parts):
                got["out"][r_rows], got["dx"][r_rows] = o, dx
                # the rank sums are the same on every rank
                assert np.array_equal(dth, got["dtheta"]) and np.array_equal(dfn, got["dfns"][0])
                if not ok:
                    errs.append(f"rank {r}: the zeros of b0.a are not at the global mask's positions")
            q.put(errs + GU.check_parity_per_sample(got, fx))
    except Exception as e:  # report instead of hanging the other rank's collectives
        if rank == 0:
            q.put([f"rank0 exception: {e!r}"])
        raise
    finally:
        dist.destroy_process_group()


def test_point_sharded_dropout_matches_the_reference():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    errs = q.get(timeout=100)
    for p in procs:
        p.join(timeout=30)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert not errs, errs
