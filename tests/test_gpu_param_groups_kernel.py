"""The slice-table entries of the training step on the GPU (gnot_adamw_step_groups, gnot_grad_norm_groups,
gnot_grad_clip_groups): FlatAdamW(groups=) against torch.optim.AdamW's parameter groups, frozen ranges that are
neither read nor written, one covering group against the four plain entries bit for bit, and the norm of the
trainable gradient against float64.

The arena holds tensors of 1, 3, 255, 8191, 8192 and 8193 elements (one element, less than a 16-byte load, less
than a workgroup's stride, one short of a slice, a slice, a slice and one element); the third and the last are
frozen; three groups.  Every array's base is 0 to 3 floats behind a 16-byte boundary."""
import pytest
import torch

import train_step_util as U
from gnot_amd import train
from train_step_util import Table, groups_norm, groups_step

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 255, 8191, 8192, 8193]
GROUP_OF = [0, 1, None, 2, 0, None]                   # the third and the last tensor are frozen
GHYPER = [[1.0, 1e-2], [0.1, 0.0], [3.0, 0.1]]        # {lr_scale, weight_decay} per group
N = sum(SIZES)
BOUNDS = [sum(SIZES[:k]) for k in range(len(SIZES) + 1)]
ROWS = train.slice_table(SIZES, GROUP_OF)
FROZEN = torch.zeros(N, dtype=torch.bool)
for _k, _g in enumerate(GROUP_OF):
    if _g is None:
        FROZEN[BOUNDS[_k]:BOUNDS[_k + 1]] = True
OFFSETS = [0, 1, 2, 3]


# ------------------------------------------------------------------ against torch's parameter groups
@pytest.mark.parametrize("max_norm", [None, 1.0])
@pytest.mark.parametrize("offset", [0, 3])
def test_flat_adamw_groups_match_torch_param_groups_with_onecycle(offset, max_norm):
    """Ten steps of FlatAdamW(groups=) under OneCycle against torch.optim.AdamW(param_groups, foreach=False) with
    per-group lr = s lr under OneCycleLR (per-group max_lr), the bound of
    test_flat_adamw_matches_torch_adamw_with_onecycle: 1e-6 max(1, |p|max) per tensor.  With max_norm the clip is
    torch.nn.utils.clip_grad_norm_ over the trainable tensors."""
    gen = torch.Generator().manual_seed(7)
    init = torch.randn(N, generator=gen)
    flat, buf = U.based(init, offset)
    names = [f"t{k}.weight" for k in range(len(SIZES))]
    groups = [{"tensors": [names[k] for k in range(len(SIZES)) if GROUP_OF[k] == j], "lr_scale": GHYPER[j][0],
               "weight_decay": GHYPER[j][1], "frozen": False} for j in range(3)]
    groups.append({"tensors": [names[k] for k in range(len(SIZES)) if GROUP_OF[k] is None], "lr_scale": 0.0,
                   "weight_decay": 0.0, "frozen": True})
    opt = train.FlatAdamW(flat, lr=1e-3, schedule=train.OneCycle(1e-3, 3, 4), groups=groups,
                          layout=list(zip(names, SIZES)), max_grad_norm=max_norm)
    ref = [torch.nn.Parameter(init[BOUNDS[k]:BOUNDS[k + 1]].clone().cuda()) for k in range(len(SIZES))]
    live = [p for k, p in enumerate(ref) if GROUP_OF[k] is not None]
    topt = torch.optim.AdamW([{"params": [ref[k] for k in range(len(SIZES)) if GROUP_OF[k] == j],
                               "lr": GHYPER[j][0] * 1e-3, "weight_decay": GHYPER[j][1]} for j in range(3)],
                             foreach=False)
    tsch = torch.optim.lr_scheduler.OneCycleLR(topt, max_lr=[s * 1e-3 for s, _ in GHYPER], steps_per_epoch=4, epochs=3)
    for step in range(10):
        scale = 1e-3 if step % 2 == 0 else 1.0            # with max_norm: no clip on the even steps, a clip on the odd
        gr = torch.randn(N, generator=gen) * scale
        gdev = U._based_on(torch.where(FROZEN, torch.full_like(gr, float("nan")), gr), offset)
        for k, p in enumerate(ref):
            p.grad = gr[BOUNDS[k]:BOUNDS[k + 1]].clone().cuda()
        if max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(live, max_norm))
            assert norm < 0.5 if step % 2 == 0 else norm > 2.0, (step, norm)
        topt.step()
        tsch.step()
        opt.step(gdev)
        opt.schedule.step()
        if max_norm is not None:
            assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm, (step, float(opt.grad_norm), norm)
    torch.cuda.synchronize()
    assert U.intact(flat, buf)
    for k, p in enumerate(ref):
        got = flat[BOUNDS[k]:BOUNDS[k + 1]]
        if GROUP_OF[k] is None:
            assert torch.equal(U.bits(got), U.bits(init[BOUNDS[k]:BOUNDS[k + 1]].cuda())), k      # never touched
            continue
        err = (got - p.detach()).abs().max().item()
        print(f"tensor {k} ({SIZES[k]} elements, group {GROUP_OF[k]}): max abs err {err:.3e}")
        assert err <= 1e-6 * max(1.0, p.detach().abs().max().item()), (k, err)
    assert bool(torch.isfinite(flat).all())          # the NaN of the frozen gradient ranges went nowhere


# ------------------------------------------------------------------ frozen ranges
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("kind", ["plain", "clip", "guard"])
@pytest.mark.parametrize("ema", [False, True])
def test_frozen_ranges_are_neither_read_nor_written(offset, kind, ema):
    """param / exp_avg / exp_avg_sq / ema keep their bits on the frozen ranges (each array holds its own
    sentinel there), the frozen ranges of the gradient hold NaN, and every result is finite."""
    table = Table(ROWS, GHYPER)
    start = U.Arrays(N, offset)
    for t, sentinel in ((start.p, 11.0), (start.m, 12.0), (start.v, 13.0), (start.e, 14.0)):
        t[FROZEN.cuda()] = sentinel
    gen = torch.Generator().manual_seed(offset)
    gr = torch.randn(N, generator=gen)
    g = U._based_on(torch.where(FROZEN, torch.full_like(gr, float("nan")), gr), offset)
    hy = U.hyper(0.5, w=9 / 11 if ema else None)
    clip = guard = None
    if kind != "plain":
        clip = groups_norm(g, N, hy, table, 1.0)
        assert bool(torch.isfinite(clip).all()) and float(clip[1]) < 1.0
    if kind == "guard":
        guard = U.guard()
    got = start.copy()
    groups_step(got, g, hy, table, clip, guard, ema)
    torch.cuda.synchronize()
    if guard is not None:
        assert guard.tolist() == [0, 0, 0]
    fz = FROZEN.cuda()
    for k in U.Arrays.NAMES:
        a, b = getattr(got, k), getattr(start, k)
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(U.bits(a[fz]), U.bits(b[fz])), k                # the sentinels' bits
        changed = (U.bits(a) != U.bits(b)) & ~fz
        if k == "e" and not ema:
            assert not bool(changed.any())
        else:
            assert int(changed.sum()) > 0.99 * int((~fz).sum()), k         # the trainable ranges were updated


# ------------------------------------------------------------------ one covering group == the plain entries
COVER = train.slice_table(SIZES, [0] * len(SIZES))


# hyper[7] = 0.3 makes grad * hyper[7] inexact; gnot_adamw_step alone fuses that product into exp_avg, so the
# contract with it holds for powers of two (gnot_hip.h) and that one combination is not a case
COVER_CASES = [(h7, kind, ema) for h7 in (1.0, 0.5, 0.3)
               for kind in ("plain", "clip_lt1", "clip_eq1", "guard", "guard_nan") for ema in (False, True)
               if not (h7 == 0.3 and kind == "plain" and not ema)]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("h7,kind,ema", COVER_CASES)
def test_one_covering_group_is_the_plain_entry_bit_for_bit(offset, h7, kind, ema):
    """One group {1, hyper[4]} whose slices cover [0, n): gnot_adamw_step (hyper[7] a power of two),
    gnot_adamw_step_clipped, _guarded and _ema give the same bits, a guarded skip that changes nothing but
    guard included."""
    hy = U.hyper(h7, w=9 / 11 if ema else None)
    table = Table(COVER, [[1.0, float(hy[4])]])
    start = U.Arrays(N, offset)
    gr = torch.randn(N, generator=torch.Generator().manual_seed(N + offset))
    if kind == "guard_nan":
        gr[N // 2] = float("nan")
    g = U._based_on(gr, offset)
    norm64 = h7 * float(torch.nan_to_num(gr).double().pow(2).sum().sqrt())
    max_norm = {"plain": None, "clip_lt1": 0.5 * norm64, "clip_eq1": 2.0 * norm64, "guard": 0.5 * norm64,
                "guard_nan": None}[kind]
    clip = None if kind == "plain" else U.norm(g, hy, max_norm)          # the plain norm entry: one clip for both
    want, got = start.copy(), start.copy()
    gu_want = U.guard() if kind.startswith("guard") else None
    gu_got = U.guard() if kind.startswith("guard") else None
    (want.step_ema if ema else want.step)(g, hy, clip, gu_want)
    groups_step(got, g, hy, table, clip, gu_got, ema)
    torch.cuda.synchronize()
    assert got.differing(want) == []
    if kind == "guard_nan":
        assert got.differing(start) == [] and gu_got.tolist() == [1, 1, 0]
    else:
        assert got.differing(start) == ["p", "m", "v"] + ["e"] * ema
    if gu_got is not None:
        assert gu_got.tolist() == gu_want.tolist()


# ------------------------------------------------------------------ the norm of the trainable gradient
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("h7", [1.0, 0.5])
def test_norm_is_over_the_trainable_elements(offset, h7):
    """Against the float64 sum over the trainable elements at the existing clip test's bound (1e-5 relative, the
    coefficient likewise); NaN in the frozen ranges is never read; two runs give identical bits."""
    table = Table(ROWS, GHYPER)
    gr = torch.randn(N, generator=torch.Generator().manual_seed(offset + 17))
    g = U._based_on(torch.where(FROZEN, torch.full_like(gr, float("nan")), gr), offset)
    hy = U.hyper(h7)
    norm = abs(h7) * float(gr[~FROZEN].double().pow(2).sum().sqrt())
    c = groups_norm(g, N, hy, table).cpu()
    print(f"offset {offset} h7 {h7}: norm rel err {abs(float(c[0]) - norm) / norm:.2e}")
    assert abs(float(c[0]) - norm) <= 1e-5 * norm and float(c[1]) == 1.0
    assert torch.equal(U.bits(c), U.bits(groups_norm(g, N, hy, table).cpu()))
    for max_norm, clipping in ((2.0 * norm, False), (0.5 * norm, True)):
        c2 = groups_norm(g, N, hy, table, max_norm).cpu()
        coef = min(1.0, max_norm / (norm + 1e-6))
        assert torch.equal(U.bits(c2[0]), U.bits(c[0]))                   # the norm entry's bits
        assert abs(float(c2[1]) - coef) <= 1e-5 * coef
        assert clipping == (float(c2[1]) < 1.0)
        if not clipping:
            assert float(c2[1]) == 1.0
        assert torch.equal(U.bits(c2), U.bits(groups_norm(g, N, hy, table, max_norm).cpu()))


def test_norm_over_a_covering_table_agrees_with_the_plain_entry():
    """The same elements, other slice boundaries: equal to rounding, not bit for bit (gnot_hip.h)."""
    table = Table(COVER, [[1.0, 1e-2]])
    g = U.grad(N, 1)
    hy = U.hyper(1.0)
    a, b = float(groups_norm(g, N, hy, table)[0]), float(U.norm(g, hy)[0])
    assert abs(a - b) <= 1e-5 * b


# ------------------------------------------------------------------ capture
def test_groups_launch_replays_with_the_norm_of_each_replay():
    """One torch.cuda.graph over launch() with groups, a clip and the guard: norm stage 1 -> stage 2 -> update, a
    linear chain whose table and constants are read from device memory.  A replay on a large gradient clips, one
    on a small gradient does not, one on a NaN in a trainable range skips; each equals an eager optimizer's step
    bit for bit, and the frozen ranges keep their bits throughout."""
    names = [f"t{k}.weight" for k in range(len(SIZES))]
    groups = [{"tensors": [names[k] for k in range(len(SIZES)) if GROUP_OF[k] == j], "lr_scale": GHYPER[j][0],
               "weight_decay": GHYPER[j][1], "frozen": False} for j in range(3)]
    groups.append({"tensors": [names[k] for k in range(len(SIZES)) if GROUP_OF[k] is None], "lr_scale": 0.0,
                   "weight_decay": 0.0, "frozen": True})
    gen = torch.Generator().manual_seed(5)
    flat0 = torch.randn(N, generator=gen).cuda()
    mk = lambda: train.FlatAdamW(flat0.clone(), groups=groups, layout=list(zip(names, SIZES)), max_grad_norm=1.0,
                                 skip_nonfinite=True, ema_decay=0.9)
    opt_g, opt_e = mk(), mk()
    g_static = torch.zeros(N, device="cuda")
    g0 = torch.randn(N, generator=gen).cuda() * 1e-2
    g_static.copy_(g0)
    opt_g.step(g_static)                 # one eager step on both first (loads the kernels)
    opt_e.step(g0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.launch(g_static)
    fz = FROZEN.cuda()
    for scale, bad, clipped, skipped in ((1.0, False, True, 0), (1e-4, False, False, 0), (1.0, True, None, 1)):
        gk = torch.randn(N, generator=gen).cuda() * scale
        gk[fz] = float("nan")            # never read
        if bad:
            gk[BOUNDS[3] + 5] = float("nan")
        g_static.copy_(gk)
        opt_g.prepare()
        graph.replay()
        opt_e.step(gk)
        torch.cuda.synchronize()
        assert int(opt_g.last_skipped) == skipped == int(opt_e.last_skipped)
        if clipped is not None:
            assert (float(opt_g.grad_norm) > 1.0) == clipped
        assert torch.equal(U.bits(opt_g.grad_norm), U.bits(opt_e.grad_norm))
        for x, y in ((opt_g.flat, opt_e.flat), (opt_g.m, opt_e.m), (opt_g.v, opt_e.v), (opt_g.ema.ema, opt_e.ema.ema)):
            assert torch.equal(U.bits(x), U.bits(y))
        assert torch.equal(U.bits(opt_g.flat[fz]), U.bits(flat0[fz])) and not bool(opt_g.m[fz].any())
        assert torch.equal(U.bits(opt_g.ema.ema[fz]), U.bits(flat0[fz]))
    assert bool(torch.isfinite(opt_g.flat).all())
