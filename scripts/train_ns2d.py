#!/usr/bin/env python3
"""Train GNOT on NS2d-format data with the MI355X core: the reference's main.py (argparse flags of
main.py:15-23, batch 4, AdamW lr 1e-3, OneCycleLR stepped per epoch, RelL2 metric, best checkpoint)
with plain tensors instead of dgl graphs.  Batches are zero-padded exactly like main.py:60-89 by
default (the pad rows enter the attention sums, as in the reference); --packed uses packed offsets.
--device-data keeps the datasets in device memory and gathers the packed batches there; --points-per-mesh K
trains on K randomly chosen points of every mesh per step.  --normalize trains on unit-Gaussian inputs and
targets (statistics of the training set, computed on the device) and writes a checkpoint that takes raw inputs.
--x-fourier N / --fn-fourier N embed the coordinates / the input functions in multi-scale Fourier features of
order N inside the model (the original GNOT code's horiz_fourier_dim), behind the normalisation.
--pre-norm normalises the attention inputs (a parameter-free LayerNorm, the original GNOT code's ln1 .. ln5).
--loss rel_l1 / l1 and --component-weights W0,W1,... train on the original GNOT code's other named losses and on
weighted output components (train.LpLoss); --log-components logs the test metric per output component every epoch
and prints the five worst test samples at the end (train.evaluate_table).
--init CHECKPOINT starts from a trained model's weights (fine-tuning); --freeze P1,P2 keeps the parameters matching
those fnmatch patterns (state_dict names: "blocks.0.*", "x.*") as they are, --no-decay P1,P2 takes them out of
the weight decay ("*.bias") and --lr-scale PATTERN=S[,...] trains them at S times the schedule's rate.

    python scripts/train_ns2d.py --train train.pkl --test test.pkl [--epochs 100 ...]
    python scripts/train_ns2d.py --synthetic 64 --epochs 2          # generated meshes, same format
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnot-replication_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gnot_amd import GNOT, data, train  # noqa: E402


LOSS_KINDS = {"rel_l2": "rel2", "mse": "mse", "rel_l1": "rel1", "l1": "l1"}       # --loss -> train.LpLoss's kind


def parse_args(argv=None):
    """The command line (argv: a list, default sys.argv[1:]) as a namespace; host only.  `normalize` becomes the
    set of arrays to normalise (or None) and `component_weights` a list of floats (or None)."""
    ap = argparse.ArgumentParser(description="GNOT (MI355X)")
    ap.add_argument("--gpu_id", type=int, default=0)
    ap.add_argument("--n_attn_layers", type=int, default=4)
    ap.add_argument("--n_attn_hidden_dim", type=int, default=256)
    ap.add_argument("--n_mlp_num_layers", type=int, default=4)
    ap.add_argument("--n_mlp_hidden_dim", type=int, default=256)
    ap.add_argument("--n_input_hidden_dim", type=int, default=256)
    ap.add_argument("--n_expert", type=int, default=3)
    ap.add_argument("--n_head", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--train")
    ap.add_argument("--test")
    ap.add_argument("--synthetic", type=int, default=0, help="generate this many training meshes instead")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--per-batch-schedule", action="store_true", help="step OneCycleLR per batch (main.py steps it per epoch)")
    ap.add_argument("--checkpoint", default="best_model.pth")
    ap.add_argument("--packed", action="store_true",
                    help="packed batches (per-sample exact); default: main.py's zero-padded batches")
    ap.add_argument("--loss", choices=list(LOSS_KINDS), default="rel_l2",
                    help="training loss: RelL2Loss (main.py:98), MSELoss (main.py:97), or the original GNOT code's "
                         "relative L1 / L1 (train.LpLoss); the test metric stays RelL2")
    ap.add_argument("--component-weights", default=None, metavar="W0,W1,...",
                    help="one non-negative weight per output component in the training loss (normalised to sum 1; "
                         "0 takes a component out of the loss).  Default: every component weighs the same")
    ap.add_argument("--log-components", action="store_true",
                    help="log the test metric per output component every epoch (mean over the test samples) and "
                         "print the five worst test samples, with their per-component RelL2, after training")
    ap.add_argument("--grad-clip", type=float, default=None, metavar="FLOAT",
                    help="clip the global gradient norm to this value before every AdamW step (default: off)")
    ap.add_argument("--accum-steps", type=int, default=1, metavar="N",
                    help="accumulate gradients over N consecutive batches per optimizer step (an effective batch of "
                         "N x --batch meshes when that many do not fit one plan; default 1: a step per batch)")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="leave the parameters and moments alone on a step whose gradient norm is NaN or infinite "
                         "(tested on the device; default: off, one bad gradient ends the run)")
    ap.add_argument("--state", default=None, metavar="PATH",
                    help="write the whole training state here after every epoch (default: off)")
    ap.add_argument("--resume", action="store_true",
                    help="continue the run stored in --state if that file exists, else start from scratch")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="FLOAT",
                    help="keep an exponential moving average of the weights with this decay (e.g. 0.999) and "
                         "evaluate and checkpoint it instead of the raw weights (default: off)")
    ap.add_argument("--no-ema-warmup", action="store_true",
                    help="use --ema-decay from the first step on (default: min(decay, (1 + t) / (10 + t)) at step t)")
    ap.add_argument("--device-data", action="store_true",
                    help="keep both datasets in device memory and assemble the (packed) batches there "
                         "(data.DeviceLoader; implies --packed)")
    ap.add_argument("--points-per-mesh", type=int, default=None, metavar="K",
                    help="train on a fresh uniform subsample of K points of every mesh per step (meshes of fewer "
                         "points whole); input functions stay whole and the test set is evaluated at full "
                         "resolution (implies --device-data)")
    ap.add_argument("--normalize", nargs="?", const="x,theta,fns,y", default=None, metavar="ARRAYS",
                    help="normalise per channel to zero mean and unit variance with the training set's statistics: "
                         "all four arrays, or a comma-separated subset of x,theta,fns,y.  Loss and metric stay in "
                         "physical units and the checkpoint has the statistics folded in (implies --device-data)")
    ap.add_argument("--point-weights", action="store_true",
                    help="read a fifth entry W [N] of every sample, one weight >= 0 per query point (quadrature "
                         "weights, a 0/1 mask): the loss, the test metric and, with --normalize, the target statistics "
                         "weigh the points with it, and rows of weight zero are never read (their targets may be "
                         "NaN).  For --device-data and the host loaders alike (implies --packed; default: off)")
    ap.add_argument("--x-fourier", type=int, default=0, metavar="N",
                    help="embed every coordinate v as [v, cos(2^k v), sin(2^k v)], k = -N .. N, inside the model "
                         "(4 N + 3 columns per channel, N up to 8; default 0: raw coordinates)")
    ap.add_argument("--fn-fourier", type=int, default=0, metavar="N",
                    help="the same embedding for every input function's channels (default 0)")
    ap.add_argument("--pre-norm", action="store_true",
                    help="LayerNorm (no gamma / beta, eps 1e-5) on the inputs of every attention call; the "
                         "checkpoint then has one more key, pre_norm_eps, and loads only into GNOT(pre_norm=True)")
    ap.add_argument("--attn-dropout", type=float, default=0.0, metavar="P",
                    help="dropout with probability P in [0, 1) on the output of every attention call, in the training "
                         "forwards only (default 0: off); the state file carries its step counter")
    ap.add_argument("--dropout-seed", type=int, default=0, metavar="S",
                    help="the seed of the dropout masks (default 0); a run resumes only under the seed that wrote it")
    ap.add_argument("--init", default=None, metavar="CHECKPOINT",
                    help="load this state_dict checkpoint (train.load_checkpoint) before training: fine-tuning a "
                         "trained model.  Unlike --resume it starts a new run: step 0 of a fresh schedule")
    ap.add_argument("--freeze", default=None, metavar="P1,P2",
                    help="fnmatch patterns over the state_dict names (\"blocks.0.*\", \"x.*\"): the matching "
                         "parameters are not trained -- no update and no weight decay")
    ap.add_argument("--no-decay", default=None, metavar="P1,P2",
                    help="patterns of the parameters that take no weight decay (\"*.bias\")")
    ap.add_argument("--lr-scale", default=None, metavar="PATTERN=S[,...]",
                    help="train the parameters matching PATTERN at S times the schedule's learning rate, S > 0; the "
                         "first matching pattern counts (\"blocks.*=0.1\")")
    args = ap.parse_args(argv)
    for name in ("freeze", "no_decay"):
        v = getattr(args, name)
        if v is not None:
            setattr(args, name, [p for p in v.split(",") if p])
            if not getattr(args, name):
                ap.error(f"--{name.replace('_', '-')} takes comma-separated patterns")
    if args.lr_scale is not None:
        scales = {}
        for item in filter(None, args.lr_scale.split(",")):
            pat, sep, val = item.rpartition("=")
            try:
                scales[pat] = float(val)
            except ValueError:
                sep = ""
            if not sep or not pat or not (scales[pat] > 0 and scales[pat] < float("inf")):
                ap.error("--lr-scale takes PATTERN=S[,PATTERN=S...] with positive finite S")
        if not scales:
            ap.error("--lr-scale takes PATTERN=S[,PATTERN=S...] with positive finite S")
        args.lr_scale = scales
    if not (0.0 <= args.attn_dropout < 1.0):
        ap.error("--attn-dropout takes a probability in [0, 1)")
    if not (0 <= args.dropout_seed < 1 << 64):
        ap.error("--dropout-seed takes an integer in [0, 2^64)")
    if args.component_weights is not None:
        try:
            args.component_weights = [float(v) for v in args.component_weights.split(",")]
            train.LpLoss(LOSS_KINDS[args.loss], args.component_weights)      # the host checks of the weights
        except ValueError as e:
            ap.error(f"--component-weights takes comma-separated non-negative numbers with a positive sum ({e})")
    norm = None if args.normalize is None else set(filter(None, args.normalize.split(",")))
    if norm is not None and (not norm or norm - {"x", "theta", "fns", "y"}):
        ap.error("--normalize takes a comma-separated subset of x,theta,fns,y")
    for flag, order, block in (("--x-fourier", args.x_fourier, "x"), ("--fn-fourier", args.fn_fourier, "fns")):
        if order and norm is not None and block in norm and args.checkpoint:
            ap.error(f"{flag} with --normalize {block}: the embedding is not affine, so the statistics of {block} "
                     f"cannot be folded into the checkpoint; normalise {block} in the dataset itself or drop it "
                     "from --normalize")
    args.device_data = args.device_data or args.points_per_mesh is not None or norm is not None
    args.normalize = norm
    if args.point_weights:
        if args.synthetic:
            ap.error("--point-weights reads the samples' fifth entry; --synthetic meshes have none")
        args.packed = True       # padded batches take no weights
    return args


def training_loss(args, normalizer=None):
    """The loss of --loss / --component-weights: RelL2Loss or MSELoss as before, an LpLoss for the new kinds and
    for any weights"""
    if args.component_weights is None and args.loss in ("rel_l2", "mse"):
        return train.MSELoss(normalizer) if args.loss == "mse" else train.RelL2Loss(normalizer)
    return train.LpLoss(LOSS_KINDS[args.loss], args.component_weights, normalizer)


def main():
    args = parse_args()
    norm = args.normalize
    if args.synthetic:
        rng = np.random.default_rng(0)
        tr = data.NS2dData([data.synthetic_sample(rng, int(rng.integers(1000, 4000))) for _ in range(args.synthetic)])
        te = data.NS2dData([data.synthetic_sample(rng, int(rng.integers(1000, 4000))) for _ in range(max(4, args.synthetic // 8))])
    else:
        tr, te = data.NS2dData(args.train, args.point_weights), data.NS2dData(args.test, args.point_weights)
    x0, y0, th0, f0 = tr[0][:4]
    dev = torch.device("cuda", args.gpu_id)
    model = GNOT(x0.shape[1], len(np.atleast_1d(th0)), f0[0].shape[1], y0.shape[1], args.n_attn_layers,
                 args.n_attn_hidden_dim, args.n_mlp_num_layers, args.n_mlp_hidden_dim, args.n_input_hidden_dim,
                 args.n_expert, args.n_head, len(f0), x_fourier=args.x_fourier, fn_fourier=args.fn_fourier,
                 pre_norm=args.pre_norm, attn_dropout=args.attn_dropout, dropout_seed=args.dropout_seed).to(dev)
    if args.init:
        train.load_checkpoint(model, args.init)
    dl = lambda ds, sh: torch.utils.data.DataLoader(ds, batch_size=args.batch, shuffle=sh,
                                                    collate_fn=data.collate_packed if args.packed
                                                    else data.collate_padded)
    nz = None
    if args.device_data:       # the test set stays at full resolution
        dtr = data.DeviceDataset(tr, dev, args.point_weights)
        if norm is not None:   # the training set's statistics serve both loaders
            nz = data.Normalizer.fit(dtr, **{k: k in norm for k in ("x", "theta", "fns", "y")})
        loaders = (data.DeviceLoader(dtr, args.batch, shuffle=True, points_per_mesh=args.points_per_mesh,
                                     normalizer=nz),
                   data.DeviceLoader(data.DeviceDataset(te, dev, args.point_weights), args.batch, normalizer=nz))
    else:
        loaders = dl(tr, True), dl(te, False)
    _, test = train.fit(model, *loaders, epochs=args.epochs,
                        per_epoch_schedule=not args.per_batch_schedule, checkpoint=args.checkpoint,
                        loss_fn=training_loss(args, nz), log_components=args.log_components,
                        max_grad_norm=args.grad_clip, accum_steps=args.accum_steps,
                        skip_nonfinite=args.skip_nonfinite, state_path=args.state, resume=args.resume,
                        ema_decay=args.ema_decay, ema_warmup=not args.no_ema_warmup, normalizer=nz,
                        freeze=args.freeze, no_decay=args.no_decay, lr_scale=args.lr_scale)
    print(f"\nBest Test Metric: {min(test)}")
    if args.log_components:      # of the final weights (the raw ones, also with --ema-decay)
        table = train.evaluate_table(model, loaders[1], "rel2", nz)
        worst = table.mean(1).argsort(descending=True)[:5].tolist()
        print("Worst test samples (index, RelL2 per component):")
        for i in worst:
            print(f"  {i}: {table[i].tolist()}")


if __name__ == "__main__":
    main()
