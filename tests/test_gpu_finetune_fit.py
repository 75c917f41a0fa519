"""Fine-tuning through train.fit(freeze=, no_decay=, lr_scale=) on the GPU, against a stock-torch replica (the
torch_port forward + autograd, torch.optim.AdamW with parameter groups, OneCycleLR with per-group max_lr stepped
per epoch): losses, metrics and weights at the bounds of test_fit_evaluate_checkpoint_match_torch_reference, frozen
parameters bit-identical to their initial values (also with the weight average, clipping and the non-finite guard
on), a killed and resumed run against the uninterrupted one bit for bit, the refusals of resume by name, and the
training script started from a checkpoint."""
import fnmatch
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import train_step_util as U
from gnot_amd import GNOT, train

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = (2, 1, 3, 1, 2, 32, 2, 32, 32, 2, 4, 1)        # train_step_util.SMALL with two blocks
TCFG = dict(n_mlp_num_layers=2, n_expert=2, n_head=4, n_attn_layers=2, n_input_functions=1)
ARGS = dict(freeze=["x.*", "gating.*", "input_func_mlps.*", "blocks.0.*"], no_decay=["*.bias"],
            lr_scale={"blocks.*": 0.1})
EPOCHS = 2
bits = U.bits


def _model(seed=0):
    torch.manual_seed(seed)
    return GNOT(*CFG).cuda()


def _is_frozen(name):
    return any(fnmatch.fnmatchcase(name, p) for p in ARGS["freeze"])


def _replica_out(torch_port, p, b, dev):
    """reference forward of one packed batch: one unpadded B=1 call per sample"""
    outs = []
    for i in range(len(b["x_off"]) - 1):
        s, e = b["x_off"][i], b["x_off"][i + 1]
        fo = b["fn_offs"][0]
        outs.append(torch_port.gnot_forward(p, TCFG, b["x"][s:e][None].to(dev), b["theta"][i:i + 1].to(dev),
                                            [b["fns"][0][fo[i]:fo[i + 1]][None].to(dev)])[0])
    return torch.cat(outs), b["x_off"]


def _rel_l2(out, y, off):
    tot = [(((out[s:e] - y[s:e]) ** 2).sum(0) / (y[s:e] ** 2).sum(0)).sqrt() for s, e in zip(off[:-1], off[1:])]
    return torch.stack(tot).mean()


def _replica(init, train_loader, test_loader, dev):
    """torch's own parameter groups, resolved here from the names and not through train.param_groups: frozen
    tensors are left out of the optimizer and do not require grad, biases take no decay, blocks.* a tenth of the
    rate at every step of the schedule"""
    sys.path.insert(0, ROOT)
    from oracle import torch_port
    p = {k: v.clone().requires_grad_(not _is_frozen(k)) for k, v in init.items()}
    keyed = {}
    for k, v in p.items():
        if not _is_frozen(k):
            keyed.setdefault((0.1 if k.startswith("blocks.") else 1.0, 0.0 if k.endswith(".bias") else 1e-2), []).append(v)
    assert len(keyed) == 4
    opt = torch.optim.AdamW([{"params": v, "lr": s * 1e-3, "weight_decay": wd} for (s, wd), v in keyed.items()],
                            foreach=False)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[s * 1e-3 for s, _ in keyed], steps_per_epoch=len(train_loader),
                                                epochs=EPOCHS)
    hist_train, hist_test = [], []
    for _ in range(EPOCHS):
        losses = []
        for b in train_loader:
            opt.zero_grad()
            out, off = _replica_out(torch_port, p, b, dev)
            loss = _rel_l2(out, b["y"].to(dev), off)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        sched.step()
        hist_train.append(np.mean(losses))
        with torch.no_grad():
            vals = []
            for b in test_loader:
                out, off = _replica_out(torch_port, p, b, dev)
                vals.append(float(_rel_l2(out, b["y"].to(dev), off)))
        hist_test.append(np.mean(vals))
    return hist_train, hist_test, {k: v.detach().clone() for k, v in p.items()}


def _moves(name):
    """a tensor the run must have changed: a trainable weight (its decay alone moves it; a bias whose gradient is
    at rounding level -- the keys' in front of a softmax -- may stay where it is under a clip)"""
    return not _is_frozen(name) and name.endswith(".weight")


def _assert_frozen_kept(model, init):
    """frozen parameters keep their bits, the trainable weights moved, and the caller's requires_grad flags (all
    True on a fresh model) are back"""
    for k, v in model.named_parameters():
        same = torch.equal(bits(v.detach()), bits(init[k]))
        assert same or not _is_frozen(k), k
        assert not (same and _moves(k)), k
        assert v.requires_grad, k


def test_fine_tuning_fit_matches_torch_param_groups(tmp_path):
    dev = torch.device("cuda")
    tr, te = U.batches()
    model = _model()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ref_train, ref_test, ref_final = _replica(init, tr, te, dev)
    path = os.path.join(tmp_path, "s.pt")
    got_train, got_test = train.fit(model, tr, te, epochs=EPOCHS, log=lambda msg: None, state_path=path, **ARGS)
    print("train", got_train, ref_train, "test", got_test, ref_test)
    assert np.allclose(got_train, ref_train, rtol=1e-4, atol=0), (got_train, ref_train)
    assert np.allclose(got_test, ref_test, rtol=1e-4, atol=0), (got_test, ref_test)
    sd = model.state_dict()
    assert list(sd.keys()) == list(init.keys())
    for k in sd:
        r = ref_final[k]
        assert float((sd[k] - r).norm() / r.norm().clamp_min(1e-12)) < 1e-3, k
    _assert_frozen_kept(model, init)
    # the state file: the three arguments in an entry of their own, the resolved groups in the optimizer's state,
    # and no moment of a frozen tensor ever written
    state = train.load_training_state(path)
    assert state["param_groups"] == dict(ARGS, lr_scale=dict(ARGS["lr_scale"]))
    assert "param_groups" not in state["args"]
    assert state["optimizer"]["groups"] == train.param_groups(_model(), **ARGS)
    o = 0
    for name, n in train.arena_layout(model):
        for k in ("exp_avg", "exp_avg_sq"):
            zeros = bool((state["optimizer"][k][o:o + n] == 0).all())
            assert zeros or not _is_frozen(name), (name, k)
            assert not (zeros and _moves(name)), (name, k)
        o += n


def test_frozen_parameters_keep_their_bits_with_every_option_on(tmp_path):
    """ema_decay, max_grad_norm and skip_nonfinite together, one batch with a NaN target (a skipped step per epoch);
    the average of a frozen weight stays equal to the weight (both read from the state file)"""
    tr, te = U.batches()
    tr = [dict(b) for b in tr]
    tr[1]["y"] = tr[1]["y"].clone()
    tr[1]["y"][5] = float("nan")
    model = _model()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    path = os.path.join(tmp_path, "s.pt")
    hist = train.fit(model, tr, te, epochs=EPOCHS, log=lambda msg: None, ema_decay=0.9, state_path=path,
                     max_grad_norm=0.05 * U.first_grad_norm(), skip_nonfinite=True, **ARGS)
    state = train.load_training_state(path)
    assert state["optimizer"]["skipped"] == EPOCHS and all(np.isfinite(hist[0])) and all(np.isfinite(hist[1]))
    _assert_frozen_kept(model, init)
    ema, o = state["optimizer"]["ema"]["ema"], 0
    for name, n in train.arena_layout(model):
        same = torch.equal(bits(ema[o:o + n]), bits(state["model"][name].reshape(-1)))
        assert same or not _is_frozen(name), name
        assert not (same and _moves(name)), name
        o += n


def test_caller_flags_come_back_and_the_engine_skips_the_frozen_stages():
    """fit freezes through requires_grad, so the engine plans the shortened backward while it runs (seen from the
    log callback) and the caller's own flags -- one set to False by hand here -- are back afterwards"""
    tr, te = U.batches()
    model = _model()
    by_hand = model.out.linears()[0].bias
    by_hand.requires_grad_(False)
    seen = []
    train.fit(model, tr, te, epochs=1, log=lambda msg: seen.append(model.engine().backward_plan()) if "Loss" in msg else None, **ARGS)
    live = len(model.blocks[1].linears()) + len(model.out.linears())
    assert seen and all(plan == (live, 1) for plan in seen), seen
    assert not by_hand.requires_grad
    assert all(p.requires_grad for p in model.parameters() if p is not by_hand)


def test_frozen_first_layers_with_the_normalizer_fold_as_before(tmp_path):
    """fit(normalizer=, freeze=) with the first Linears -- the ones Normalizer.fold rewrites in the checkpoint --
    frozen: the raw weights keep their bits, and the folded checkpoint predicts physical outputs from raw inputs
    at the run's metric (the bound of test_folded_checkpoint_predicts_physical_outputs_from_raw_inputs)"""
    from gnot_amd import data
    rng = np.random.default_rng(5)
    mk = lambda k: [data.synthetic_sample(rng, int(rng.integers(40, 120)), fn_points=(int(rng.integers(10, 30)),))
                    for _ in range(k)]
    dtr, dte = data.DeviceDataset(mk(8), "cuda"), data.DeviceDataset(mk(4), "cuda")
    nz = data.Normalizer.fit(dtr)
    model = _model()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    best = os.path.join(tmp_path, "best.pth")
    hist = train.fit(model, data.DeviceLoader(dtr, 2, normalizer=nz), data.DeviceLoader(dte, 2, normalizer=nz),
                     epochs=EPOCHS, normalizer=nz, checkpoint=best, log=lambda msg: None, **ARGS)
    _assert_frozen_kept(model, init)
    fresh = _model(seed=5)
    fresh.load_state_dict(torch.load(best, map_location="cpu", weights_only=True))
    got = train.evaluate(fresh, data.DeviceLoader(dte, 2), train.RelL2Loss())          # raw inputs, plain metric
    want = min(hist[1])
    print(f"folded checkpoint: metric {got!r} on raw inputs, {want!r} in the run")
    assert abs(got - want) <= 1e-4 * want


def test_killed_and_resumed_fine_tuning_is_the_uninterrupted_run_bitwise(tmp_path):
    tr, te = U.batches()
    p, q = os.path.join(tmp_path, "p.pt"), os.path.join(tmp_path, "q.pt")
    ref = _model()
    ref_hist = train.fit(ref, tr, te, epochs=EPOCHS, state_path=p, log=lambda msg: None, **ARGS)
    lines = []

    def log(msg):
        lines.append(msg)
        if sum("Test Metric" in l for l in lines) == 2:       # in epoch 1, after epoch 0's state was written
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(_model(), tr, te, epochs=EPOCHS, state_path=q, log=log, **ARGS)
    assert train.load_training_state(q)["next_epoch"] == 1
    got = _model(seed=123)                                   # a fresh module with other weights
    got_hist = train.fit(got, tr, te, epochs=EPOCHS, state_path=q, resume=True, log=lambda msg: None, **ARGS)
    assert got_hist == ref_hist
    assert torch.equal(bits(U.flat_params(got)), bits(U.flat_params(ref)))
    a, b = train.load_training_state(p), train.load_training_state(q)
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(bits(a["optimizer"][k]), bits(b["optimizer"][k])), k
    assert a["optimizer"]["groups"] == b["optimizer"]["groups"] and a["param_groups"] == b["param_groups"]

    # another freeze, lr_scale or no_decay is another run: refused by name, an absent entry included
    kw = dict(epochs=EPOCHS, state_path=p, resume=True, log=lambda msg: None)
    with pytest.raises(ValueError, match="freeze="):
        train.fit(_model(), tr, te, **dict(kw, **dict(ARGS, freeze=["x.*"])))
    with pytest.raises(ValueError, match="lr_scale="):
        train.fit(_model(), tr, te, **dict(kw, **dict(ARGS, lr_scale={"blocks.*": 0.2})))
    with pytest.raises(ValueError, match="no_decay="):
        train.fit(_model(), tr, te, **dict(kw, **dict(ARGS, no_decay=None)))
    with pytest.raises(ValueError, match="freeze="):
        train.fit(_model(), tr, te, **kw)                     # this call has no groups, the file has
    plain = os.path.join(tmp_path, "plain.pt")
    train.fit(_model(), tr, te, epochs=EPOCHS, state_path=plain, log=lambda msg: None)
    assert "param_groups" not in train.load_training_state(plain)
    with pytest.raises(ValueError, match="freeze="):
        train.fit(_model(), tr, te, **dict(kw, state_path=plain, **ARGS))       # the file has none, this call has


def test_training_script_fine_tunes_from_a_checkpoint(tmp_path, monkeypatch, capsys):
    """scripts/train_ns2d.py --synthetic 8 --init ... --freeze ...: one epoch from a stored model; the checkpoint
    it writes holds the frozen tensors' stored bits and other values everywhere else"""
    spec = importlib.util.spec_from_file_location("train_ns2d", os.path.join(ROOT, "scripts", "train_ns2d.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    torch.manual_seed(4)
    start = GNOT(*CFG)
    init, out = os.path.join(tmp_path, "init.pth"), os.path.join(tmp_path, "tuned.pth")
    train.save_checkpoint(start, init)
    monkeypatch.setattr(sys, "argv", [
        "train_ns2d.py", "--synthetic", "8", "--epochs", "1", "--packed", "--n_attn_layers", "2", "--n_attn_hidden_dim",
        "32", "--n_mlp_num_layers", "2", "--n_mlp_hidden_dim", "32", "--n_input_hidden_dim", "32", "--n_expert", "2",
        "--n_head", "4", "--init", init, "--checkpoint", out, "--freeze", ",".join(ARGS["freeze"]), "--no-decay",
        "*.bias", "--lr-scale", "blocks.*=0.1"])
    script.main()
    assert "Best Test Metric" in capsys.readouterr().out
    tuned = torch.load(out, map_location="cpu", weights_only=True)
    sd = start.state_dict()
    assert list(tuned.keys()) == list(sd.keys())
    for k in sd:
        same = torch.equal(bits(tuned[k]), bits(sd[k]))
        assert same or not _is_frozen(k), k
        assert not (same and _moves(k)), k
