"""Frozen tensors and AdamW parameter groups on the CPU: the pattern resolution of train.param_groups, the slice
table builder, the refusals of the three slice-table entries (they return before any launch, so dummy device
pointers are enough), FlatAdamW's host checks, the state-file entry and the command line of scripts/train_ns2d.py."""
import ctypes
import importlib.util
import os

import pytest
import torch

from gnot_amd import GNOT, _lib, train

DUMMY = 0x1000      # a non-null "device pointer": the checks must never get as far as using it
SMALL2 = (2, 1, 3, 1, 2, 32, 2, 32, 32, 2, 4, 1)      # two blocks, two experts, one input function


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GNOT(*SMALL2)


# ------------------------------------------------------------------ layout and pattern resolution
def test_arena_layout_is_the_linears_in_order(model):
    layout = train.arena_layout(model)
    lins = model.linears()
    assert len(layout) == 2 * len(lins)
    sd = model.state_dict()
    for k, (name, numel) in enumerate(layout):
        p = lins[k // 2].weight if k % 2 == 0 else lins[k // 2].bias
        assert sd[name].data_ptr() == p.data_ptr() and numel == p.numel()
        assert name.endswith(".weight" if k % 2 == 0 else ".bias")
    assert sum(n for _, n in layout) == sum(p.numel() for p in model.parameters())


def test_no_arguments_give_one_group_over_everything(model):
    (g,) = train.param_groups(model)
    assert g["tensors"] == [n for n, _ in train.arena_layout(model)]
    assert (g["lr_scale"], g["weight_decay"], g["frozen"]) == (1.0, 1e-2, False)


def test_patterns_resolve_to_groups(model):
    names = [n for n, _ in train.arena_layout(model)]
    groups = train.param_groups(model, freeze=["x.*", "gating.*", "input_func_mlps.*", "blocks.0.*"],
                                no_decay=["*.bias"], lr_scale={"blocks.*": 0.1})
    assert sorted(n for g in groups for n in g["tensors"]) == sorted(names)       # a partition of the arena
    by_key = {(g["frozen"], g["lr_scale"], g["weight_decay"]): g["tensors"] for g in groups}
    assert len(by_key) == len(groups) == 5
    low = lambda n: n.startswith(("x.", "gating.", "input_func_mlps.", "blocks.0."))
    assert by_key[(True, 0.0, 0.0)] == [n for n in names if low(n)]
    assert by_key[(False, 0.1, 1e-2)] == [n for n in names if n.startswith("blocks.1.") and n.endswith(".weight")]
    assert by_key[(False, 0.1, 0.0)] == [n for n in names if n.startswith("blocks.1.") and n.endswith(".bias")]
    assert by_key[(False, 1.0, 1e-2)] == [n for n in names if n.startswith("out.") and n.endswith(".weight")]
    assert by_key[(False, 1.0, 0.0)] == [n for n in names if n.startswith("out.") and n.endswith(".bias")]
    # the model is not changed
    assert all(p.requires_grad for p in model.parameters())


def test_first_matching_lr_scale_wins(model):
    groups = train.param_groups(model, lr_scale={"blocks.1.*": 3.0, "blocks.*": 0.1, "*": 0.5})
    scale = {n: g["lr_scale"] for g in groups for n in g["tensors"]}
    assert scale["blocks.1.self_attention.query.weight"] == 3.0
    assert scale["blocks.0.self_attention.query.weight"] == 0.1
    assert scale["out.layers.0.bias"] == 0.5


def test_weight_decay_argument_and_case_sensitivity(model):
    groups = train.param_groups(model, no_decay=["*.bias"], weight_decay=0.1)
    assert sorted({g["weight_decay"] for g in groups}) == [0.0, 0.1]
    with pytest.raises(ValueError, match="matches no parameter"):
        train.param_groups(model, freeze=["OUT.*"])


@pytest.mark.parametrize("kwargs,match", [
    (dict(freeze=["decoder.*"]), "freeze pattern 'decoder.\\*' matches no parameter"),
    (dict(no_decay=["*.gamma"]), "no_decay pattern"),
    (dict(lr_scale={"blocks.7.*": 0.1}), "lr_scale pattern"),
    (dict(lr_scale={"out.*": 0.0}), "positive and finite"),
    (dict(lr_scale={"out.*": -1.0}), "positive and finite"),
    (dict(lr_scale={"out.*": float("inf")}), "positive and finite"),
    (dict(lr_scale={"out.*": float("nan")}), "positive and finite"),
    (dict(freeze="out.*"), "not one string"),
    (dict(weight_decay=-1.0), "weight_decay"),
])
def test_param_groups_refuses(model, kwargs, match):
    with pytest.raises(ValueError, match=match):
        train.param_groups(model, **kwargs)


# ------------------------------------------------------------------ the slice table
SIZES = [1, 3, 8191, 8192, 8193]


def test_slice_table_on_the_edge_sizes():
    rows = train.slice_table(SIZES, [0, 1, 2, 0, 1])
    assert rows == [[0, 1, 0], [1, 3, 1], [4, 8191, 2], [8195, 8192, 0], [16387, 8192, 1], [24579, 1, 1]]
    assert train.SLICE == 8192


@pytest.mark.parametrize("frozen", [(), (0,), (2,), (4,), (1, 3), (0, 1, 2, 3, 4)])
def test_slice_table_covers_the_trainable_tensors_exactly(frozen):
    group_of = [None if k in frozen else k % 3 for k in range(len(SIZES))]
    rows = train.slice_table(SIZES, group_of)
    covered = torch.zeros(sum(SIZES), dtype=torch.int64)
    group = torch.full((sum(SIZES),), -1, dtype=torch.int64)
    end = 0
    for begin, length, g in rows:
        assert begin >= end and 1 <= length <= 8192        # sorted, disjoint, bounded
        covered[begin:begin + length] += 1
        group[begin:begin + length] = g
        end = begin + length
    o = 0
    for k, n in enumerate(SIZES):
        want = 0 if k in frozen else 1
        assert bool((covered[o:o + n] == want).all()), k
        assert bool((group[o:o + n] == (-1 if k in frozen else k % 3)).all()), k
        o += n
    # no row crosses a tensor boundary, and only a tensor's last row is short
    bounds = set(torch.tensor([0] + SIZES).cumsum(0).tolist())
    for begin, length, _ in rows:
        inside = [b for b in bounds if begin < b < begin + length]
        assert not inside
        assert length == 8192 or begin + length in bounds


# ------------------------------------------------------------------ the C entries
def test_new_symbols_are_exported_and_declared():
    lib = _lib.load()
    for name, nargs in (("gnot_adamw_step_groups", 15), ("gnot_grad_norm_groups", 9), ("gnot_grad_clip_groups", 10)):
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs


def _table(rows):
    return (ctypes.c_int64 * (3 * len(rows)))(*[v for r in rows for v in r]), len(rows)


def _step(rows, n=100, G=2, ema=None, clip=DUMMY, guard=None, host=True, ptrs=None):
    t, k = _table(rows)
    p = ptrs or [DUMMY] * 7      # param, grad, m, v, hyper, ghyper, slices_dev
    return _lib.load().gnot_adamw_step_groups(p[0], p[1], p[2], p[3], ema, n, p[4], p[5], G, p[6], t if host else None,
                                              k, clip, guard, None)


BAD_TABLES = [
    ([], "nslices"),
    ([[0, 0, 0]], "length"),
    ([[0, 8193, 0]], "length"),
    ([[-1, 4, 0]], "sorted"),
    ([[10, 4, 0], [12, 4, 0]], "sorted"),          # overlapping
    ([[10, 4, 0], [0, 4, 0]], "sorted"),           # not sorted
    ([[98, 3, 0]], "inside"),                      # past n = 100
    ([[100, 1, 0]], "inside"),
    ([[0, 4, 2]], "group"),                        # G = 2
    ([[0, 4, -1]], "group"),
]


@pytest.mark.parametrize("rows,word", BAD_TABLES)
def test_step_groups_refuses_a_bad_table(rows, word):
    assert _step(rows, n=100 if len(rows) != 1 or rows[0][1] != 8193 else 10000) == -1       # GNOT_E_INVALID
    assert word in _lib.load().gnot_last_error().decode()


@pytest.mark.parametrize("rows,word", [c for c in BAD_TABLES if c[1] != "group"])
def test_norm_groups_refuse_a_bad_table(rows, word):
    lib = _lib.load()
    n = 100 if len(rows) != 1 or rows[0][1] != 8193 else 10000
    t, k = _table(rows)
    assert lib.gnot_grad_norm_groups(DUMMY, n, DUMMY, DUMMY, t, k, DUMMY, DUMMY, None) == -1
    assert word in lib.gnot_last_error().decode()
    assert lib.gnot_grad_clip_groups(DUMMY, n, DUMMY, 1.0, DUMMY, t, k, DUMMY, DUMMY, None) == -1
    assert word in lib.gnot_last_error().decode()


def test_entries_refuse_null_pointers_and_bad_scalars():
    lib = _lib.load()
    good = [[0, 4, 0], [4, 96, 1]]
    for k in range(7):
        ptrs = [DUMMY] * 7
        ptrs[k] = None
        assert _step(good, ptrs=ptrs) == -1
    assert _step(good, host=False) == -1
    assert _step(good, n=0) == -1
    assert _step(good, G=0) == -1
    assert _step(good, clip=None, guard=DUMMY) == -1           # a guard needs a clip
    assert "guard needs a clip" in lib.gnot_last_error().decode()
    assert _step(good, ema=DUMMY) == -1                        # ema must not alias param
    t, k = _table(good)
    for j in range(5):
        ptrs = [DUMMY] * 5      # grad, hyper, slices_dev, work, clip
        ptrs[j] = None
        assert lib.gnot_grad_norm_groups(ptrs[0], 100, ptrs[1], ptrs[2], t, k, ptrs[3], ptrs[4], None) == -1
        assert lib.gnot_grad_clip_groups(ptrs[0], 100, ptrs[1], 1.0, ptrs[2], t, k, ptrs[3], ptrs[4], None) == -1
    assert lib.gnot_grad_norm_groups(DUMMY, 100, DUMMY, DUMMY, None, k, DUMMY, DUMMY, None) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.gnot_grad_clip_groups(DUMMY, 100, DUMMY, bad, DUMMY, t, k, DUMMY, DUMMY, None) == -1
        assert "max_norm" in lib.gnot_last_error().decode()


# ------------------------------------------------------------------ FlatAdamW's host checks
def _groups(**over):
    g = [{"tensors": ["a.weight"], "lr_scale": 1.0, "weight_decay": 1e-2, "frozen": False},
         {"tensors": ["a.bias"], "lr_scale": 0.0, "weight_decay": 0.0, "frozen": True}]
    g[0].update(over)
    return g


LAYOUT = [("a.weight", 12), ("a.bias", 4)]


@pytest.mark.parametrize("groups,layout,match", [
    (_groups(), None, "need the layout"),
    (_groups(), [("a.weight", 12), ("a.bias", 5)], "elements"),
    (_groups(tensors=["a.weight", "a.bias"]), LAYOUT, "more than one group"),
    (_groups(tensors=["b.weight"]), LAYOUT, "different tensors"),
    (_groups(lr_scale=0.0), LAYOUT, "lr_scale"),
    (_groups(weight_decay=-0.1), LAYOUT, "weight_decay"),
    (_groups(frozen=True), LAYOUT, "every tensor is frozen"),
])
def test_flat_adamw_refuses_bad_groups_on_the_host(groups, layout, match):
    flat = torch.zeros(16)          # a host tensor: every refusal comes before anything touches a device
    with pytest.raises(ValueError, match=match):
        train.FlatAdamW(flat, groups=groups, layout=layout)
    with pytest.raises(ValueError, match="layout without groups"):
        train.FlatAdamW(flat, layout=LAYOUT)


# ------------------------------------------------------------------ the state file and fit's host checks
class _Opt:
    def state_dict(self):
        return {"t": 3}


class _Sched(_Opt):
    pass


def test_state_file_carries_the_param_groups_entry(tmp_path, model):
    path = str(tmp_path / "state.pt")
    entry = dict(freeze=["x.*"], no_decay=["*.bias"], lr_scale={"blocks.*": 0.1})
    train.save_training_state(path, model, _Opt(), _Sched(), 1, 0.5, [1.0], [2.0], {"epochs": 2}, param_groups=entry)
    state = train.load_training_state(path)                  # weights_only=True
    assert state["param_groups"] == entry
    train.save_training_state(path, model, _Opt(), _Sched(), 1, 0.5, [1.0], [2.0], {"epochs": 2})
    assert "param_groups" not in train.load_training_state(path)


def test_fit_refuses_patterns_before_any_gpu_work(model):
    with pytest.raises(ValueError, match="matches no parameter"):
        train.fit(model, [], freeze=["nothing.*"])
    with pytest.raises(ValueError, match="nothing to train"):
        train.fit(model, [], freeze=["*"])
    assert all(p.requires_grad for p in model.parameters())


# ------------------------------------------------------------------ the command line
def test_train_script_parses_the_fine_tuning_flags():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_ns2d", os.path.join(root, "scripts", "train_ns2d.py"))
    train_ns2d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train_ns2d)
    args = train_ns2d.parse_args(["--synthetic", "8", "--init", "best.pth", "--freeze", "x.*,gating.*", "--no-decay",
                                  "*.bias", "--lr-scale", "blocks.*=0.1,out.*=2"])
    assert args.init == "best.pth" and args.freeze == ["x.*", "gating.*"] and args.no_decay == ["*.bias"]
    assert args.lr_scale == {"blocks.*": 0.1, "out.*": 2.0}
    args = train_ns2d.parse_args(["--synthetic", "8"])
    assert args.init is None and args.freeze is None and args.no_decay is None and args.lr_scale is None
    for bad in ("x", "x=0", "x=abc", "=3", "x=inf"):
        with pytest.raises(SystemExit):
            train_ns2d.parse_args(["--lr-scale", bad])


# ------------------------------------------------------------------ the plan's trainable mask (host only)
def _backward_plan(model, trainable, input_grads=False):
    """gnot_debug_backward_plan of a training plan of `model` whose Linears matching none of the fnmatch patterns
    `trainable` are frozen (None: no mask at all), for two samples of 37 and 91 points"""
    import fnmatch
    lib = _lib.load()
    cfg = _lib.GnotConfig(**model._plan_cfg)
    plan = ctypes.c_void_p()
    _lib.check(lib.gnot_plan_create(ctypes.byref(cfg), ctypes.byref(plan)))
    try:
        if trainable is not None:
            names = [n for n, _ in train.arena_layout(model)][::2]              # the weights: one per Linear
            mask = (ctypes.c_uint8 * len(names))(*[int(any(fnmatch.fnmatchcase(n, p) for p in trainable))
                                                  for n in names])
            assert len(names) == lib.gnot_plan_num_linears(plan)
            _lib.check(lib.gnot_plan_set_trainable(plan, mask))
        _lib.check(lib.gnot_plan_set_input_grads(plan, int(input_grads)))
        jobs, stage = ctypes.c_int(), ctypes.c_int()
        assert lib.gnot_debug_backward_plan(plan, ctypes.byref(jobs), ctypes.byref(stage)) == -3     # set_batch first
        xo = (ctypes.c_int64 * 3)(0, 37, 128)
        fo = (ctypes.c_int64 * 3)(0, 13, 42)
        _lib.check(lib.gnot_plan_set_batch(plan, 2, xo, fo, 1))
        need = lib.gnot_plan_workspace_bytes(plan)
        got = _lib.backward_plan(plan)
        return got + (need,)
    finally:
        lib.gnot_plan_destroy(plan)


def test_backward_plan_of_the_frozen_sets(model):
    L = 2
    all_jobs, stage, need = _backward_plan(model, None)
    assert all_jobs == len(model.linears()) and stage == -1          # heads of 8: one job per Linear
    assert _backward_plan(model, ["*"]) == (all_jobs, -1, need)      # an all-ones mask is the default
    assert _backward_plan(model, ["out.*"])[:2] == (3, L)            # the decoder alone: its three Linears
    jobs, stage, _ = _backward_plan(model, ["blocks.1.*"])
    assert stage == 1 and jobs == len(model.blocks[1].linears())
    jobs, stage, _ = _backward_plan(model, ["gating.*"])
    assert stage == -1 and jobs == 3
    assert _backward_plan(model, [])[:2] == (0, L + 1)               # all frozen: nothing to do
    assert _backward_plan(model, [], input_grads=True)[:2] == (0, -1)
    # the saved activations stay; only the split-K slab and the job tables shrink with the jobs
    for pats in (["out.*"], ["blocks.0.ffn1.0.*"], []):
        assert _backward_plan(model, pats)[2] <= need


def test_set_trainable_and_debug_entry_refuse_null():
    lib = _lib.load()
    assert lib.gnot_plan_set_trainable(None, None) == -1
    assert lib.gnot_debug_backward_plan(None, None, None) == -1
    for name in ("gnot_plan_set_trainable", "gnot_debug_backward_plan"):
        assert name in _lib.EXPORTS
