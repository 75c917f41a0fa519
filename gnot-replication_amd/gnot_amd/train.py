"""The training step around the GNOT path on the GPU.

* `RelL2Loss` -- reference loss.py:14-23 (`RelL2Loss()(g, pred, tgt)`, dgl SumPooling over the
  batched graph) restated over packed offsets: `RelL2Loss()(x_off, pred, tgt)`.  One native pass
  (libgnot_hip.so gnot_rel_l2_loss) computes the per-sample segment sums, the loss and d loss/d pred.
* `OneCycle` -- torch's OneCycleLR (main.py:52: max_lr=1e-3, steps_per_epoch, epochs; cosine,
  two phases, cycle_momentum -> AdamW's beta1) as host arithmetic.  Calling `step()` once per
  EPOCH reproduces the reference's call pattern (main.py:106) although the schedule is sized per
  batch, so the LR stays near max_lr / 25; calling it per batch is the intended OneCycle.
* `FlatAdamW` -- torch.optim.AdamW (main.py:51, default betas/eps/weight_decay) over ONE flat fp32
  arena: the model's parameters are re-homed into a single buffer laid out exactly like the engine's
  gradient arena, so the whole update is one kernel (gnot_adamw_step) reading the step's flat
  gradient buffer directly.  The hyper-parameters live in a small device array that `prepare()`
  refreshes from the host schedule, so `launch()` can be captured in a hipGraph.  `max_grad_norm`
  adds torch.nn.utils.clip_grad_norm_ in front of the update, computed on the device
  (gnot_grad_clip + gnot_adamw_step_clipped), still without a host synchronisation.  `skip_nonfinite`
  puts a device-side test of that norm in front of the update (gnot_adamw_step_guarded): a NaN or
  infinite gradient leaves parameters and moments untouched.
* `save_training_state` / `load_training_state` and `fit(state_path=..., resume=True)` -- the whole
  training state (weights, moments, step count, schedule position, histories, host random state) once
  per epoch, so a killed run continues bit for bit.
* `MSELoss` -- reference loss.py:4-12 (dgl AvgPooling: per-sample mean over points, then the mean over
  samples x channels), the reference's second loss, through gnot_mse_loss.
* `WeightEMA` and `FlatAdamW(ema_decay=...)` / `fit(ema_decay=...)` -- an exponential moving average of the
  parameters, updated inside the AdamW kernel (gnot_adamw_step_ema) and evaluated and checkpointed in place
  of the raw weights (`WeightEMA.swapped()`).
* `RelL2Loss(normalizer=)` / `MSELoss(normalizer=)` / `fit(normalizer=)` -- training on unit-Gaussian inputs and
  targets (data.Normalizer): the losses de-normalise the prediction inside their kernels
  (gnot_rel_l2_loss_affine / gnot_mse_loss_affine), the statistics travel in the state file, and the best
  checkpoint is written with them folded into its first and last Linears.
* `LpLoss(kind, component_weights, normalizer)` -- the original GNOT code's named losses (rel2, rel1, relinf, mse,
  l1, linf) with per-component weights through gnot_lp_loss, its `terms()` per (sample, channel),
  `evaluate_table` (the per-sample error table of a test set) and `fit(log_components=True)`.  Every loss entry
  runs the one kernel family of gnot_lp_loss: gnot_rel_l2_loss and gnot_mse_loss (and their _affine forms) are
  its kinds rel2 and mse without weights and terms, so `LpLoss("rel2")` / `LpLoss("mse")` launch what
  `RelL2Loss()` / `MSELoss()` launch, with the terms or without.
* `param_groups` / `FlatAdamW(groups=, layout=)` / `fit(freeze=, no_decay=, lr_scale=)` -- fine-tuning: fnmatch
  patterns over the state_dict names resolve to frozen tensors and AdamW parameter groups, and the norm and the
  update run over a slice table of the trainable tensors (gnot_grad_norm_groups / gnot_grad_clip_groups,
  gnot_adamw_step_groups), so a frozen tensor is neither read nor written.
"""
import contextlib
import ctypes
import fnmatch
import inspect
import math
import os

import torch

from . import _lib


# ------------------------------------------------------------------ loss (loss.py:14-23)
class _NativeLoss(torch.autograd.Function):
    """loss and d loss / d pred in one pass of the native entry `entry` (gnot_rel_l2_loss or gnot_mse_loss);
    stats: the targets' stats block on pred's device, and `entry` is then the _affine entry that takes it"""

    @staticmethod
    def forward(ctx, pred, tgt, off_dev, off_host, work, entry, stats=None):
        B = len(off_host) - 1
        C = pred.shape[1]
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        dpred = torch.empty_like(pred) if pred.requires_grad else None
        oh = (ctypes.c_int64 * (B + 1))(*off_host)
        s = ctypes.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
        tail = (work.data_ptr(), loss.data_ptr(), dpred.data_ptr() if dpred is not None else None, s)
        if stats is not None:
            tail = (stats.data_ptr(),) + tail
        _lib.check(getattr(_lib.load(), entry)(pred.data_ptr(), tgt.data_ptr(), off_dev.data_ptr(), oh, B, C, *tail))
        ctx.save_for_backward(dpred) if dpred is not None else None
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None, None, None, None


class RelL2Loss(torch.nn.Module):
    """mean over (sample, channel) of sqrt(sum_n (p - t)^2 / sum_n t^2) (reference loss.py:14-23).
    The dgl graph argument of the reference becomes the packed offsets x_off [B+1] (host list).
    normalizer (a data.Normalizer): `predictions` is read as a NORMALISED prediction and compared with the raw
    targets in physical units -- the loss of predictions * std_y + mean_y, in one pass of the _affine entry
    (no de-normalised copy of the prediction, the gradient scaled by std_y in the same kernel).  None
    (default): the plain entry.  The point-sharded losses of parallel.py take no normalizer."""

    _entry, _work_floats, _kind = "gnot_rel_l2_loss", "gnot_rel_l2_work_floats", "rel2"

    def __init__(self, normalizer=None):
        super().__init__()
        self._cache = {}
        self.normalizer = normalizer
        self._stats = None         # the normalizer's y block on the predictions' device

    def _geometry(self, x_off, predictions, weighted=False):
        """(device offsets, work buffer, host offsets) of the packed geometry x_off, cached for the last one;
        weighted: the work buffer of the weighted entry (gnot_lp_loss_weighted_work_floats)"""
        key = (tuple(int(v) for v in x_off), predictions.shape[1], predictions.device) + ((True,) if weighted else ())
        if key not in self._cache:
            B = len(key[0]) - 1
            oh = (ctypes.c_int64 * (B + 1))(*key[0])
            n = getattr(_lib.load(), "gnot_lp_loss_weighted_work_floats" if weighted else self._work_floats)(
                oh, B, key[1])
            # pinned source + non_blocking: a new geometry must not stall the host on the stream
            # (a pageable copy would); the pinned tensor lives in the cache entry past the copy
            pinned = torch.tensor(key[0], dtype=torch.int64).pin_memory()
            self._cache = {key: (pinned.to(predictions.device, non_blocking=True),
                                 torch.empty(n, dtype=torch.float32, device=predictions.device), pinned)}
        off_dev, work, _ = self._cache[key]
        return off_dev, work, key[0]

    def _y_stats(self, predictions):
        """the normalizer's y block on the predictions' device (None without a normalizer)"""
        if self.normalizer is None:
            return None
        if self._stats is None or self._stats.device != predictions.device:
            self._stats = self.normalizer.y.to(predictions.device).contiguous()
        if self._stats.shape[1] != predictions.shape[1]:
            raise ValueError(f"{type(self).__name__}: the normalizer's y statistics hold {self._stats.shape[1]} "
                             f"channels, the prediction {predictions.shape[1]}")
        return self._stats

    def _point_weights(self, point_weights, predictions):
        """`point_weights` as the contiguous fp32 [rows] tensor the weighted entry reads (a constant: detached), or
        ValueError -- host checks only, before any GPU work"""
        who = f"{type(self).__name__}: point_weights"
        rows = predictions.shape[0]
        if not torch.is_tensor(point_weights) or not point_weights.is_floating_point():
            raise ValueError(f"{who} must be a float tensor [rows] or [rows, 1]")
        if tuple(point_weights.shape) not in ((rows,), (rows, 1)):
            raise ValueError(f"{who} have shape {tuple(point_weights.shape)}, the prediction has {rows} rows "
                             f"(expected [{rows}] or [{rows}, 1])")
        if point_weights.device != predictions.device:
            raise ValueError(f"{who} are on {point_weights.device}, the prediction on {predictions.device}")
        return point_weights.detach().reshape(-1).contiguous().float()

    def forward(self, x_off, predictions, targets, point_weights=None):
        """point_weights: one weight w_n >= 0 per query point, a float tensor [rows] or [rows, 1] on the
        predictions' device (another shape or device: ValueError before any GPU work) -- a quadrature weight, a
        mask: sum_n becomes sum_n w_n, a mean over points divides by sum w, and a row of weight zero is not read
        (gnot_lp_loss_weighted; a NaN target under a mask is harmless).  A constant: no gradient flows to it.
        None (default): the unweighted call, exactly."""
        if point_weights is not None:
            point_weights = self._point_weights(point_weights, predictions)
        if not predictions.is_cuda:
            raise RuntimeError(f"gnot_amd.{type(self).__name__} runs on a ROCm GPU only (libgnot_hip.so)")
        if point_weights is not None:
            off_dev, work, off_host = self._geometry(x_off, predictions, weighted=True)
            return _NativeLpLoss.apply(predictions.contiguous().float(), targets.contiguous().float(), off_dev, off_host,
                                       work, self._kind, None, self._y_stats(predictions), None, point_weights)
        off_dev, work, off_host = self._geometry(x_off, predictions)
        stats = self._y_stats(predictions)
        if stats is None:
            return _NativeLoss.apply(predictions.contiguous().float(), targets.contiguous().float(), off_dev, off_host,
                                     work, self._entry)
        return _NativeLoss.apply(predictions.contiguous().float(), targets.contiguous().float(), off_dev, off_host, work,
                                 self._entry + "_affine", stats)


class MSELoss(RelL2Loss):
    """mean over (sample, channel) of the per-sample mean over points of (p - t)^2 (reference loss.py:4-12,
    dgl AvgPooling): `MSELoss()(x_off, pred, tgt)`, one native pass (gnot_mse_loss) for the segment means,
    the loss and d loss/d pred.  Not torch.nn.MSELoss: every sample weighs the same whatever its size.
    A sample without points is refused (its mean is undefined)."""

    _entry, _work_floats, _kind = "gnot_mse_loss", "gnot_mse_work_floats", "mse"


class _NativeLpLoss(torch.autograd.Function):
    """gnot_lp_loss: the loss, d loss / d pred where pred needs it, and the unweighted terms into `terms`
    ([B, C], or None) in the same pass.  point_w (fp32 [rows] on pred's device, or None): the same through
    gnot_lp_loss_weighted, `work` sized for it."""

    @staticmethod
    def forward(ctx, pred, tgt, off_dev, off_host, work, kind, weights, stats, terms, point_w=None):
        B = len(off_host) - 1
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        dpred = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        oh = (ctypes.c_int64 * (B + 1))(*off_host)
        s = ctypes.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
        ptr = lambda t: None if t is None else t.data_ptr()
        tail = (off_dev.data_ptr(), oh, B, pred.shape[1], _lib.LP_KINDS[kind], ptr(weights), ptr(stats),
                work.data_ptr(), loss.data_ptr(), ptr(terms), ptr(dpred), s)
        if point_w is None:
            _lib.check(_lib.load().gnot_lp_loss(pred.data_ptr(), tgt.data_ptr(), *tail))
        else:
            _lib.check(_lib.load().gnot_lp_loss_weighted(pred.data_ptr(), tgt.data_ptr(), point_w.data_ptr(), *tail))
        ctx.save_for_backward(dpred) if dpred is not None else None
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return (dpred * g,) + (None,) * 9


class LpLoss(RelL2Loss):
    """The loss family of the original GNOT recipe, `LpLoss(kind)(x_off, pred, tgt)` in RelL2Loss's call
    convention, one native pass (gnot_lp_loss).  With d = pred - tgt over the N_b points of sample b, the term
    of (sample b, channel c) is
        rel2  sqrt(sum d^2 / sum t^2)    rel1  sum |d| / sum |t|    relinf  max |d| / max |t|
        mse   sum d^2 / N_b              l1    sum |d| / N_b        linf    max |d|
    and the loss (1/B) sum_b sum_c w_c e[b, c] / sum_c w_c.
    component_weights: C non-negative numbers with a positive sum, one per output channel (ValueError for a
    negative or non-finite one, a zero sum, or -- at the call -- another length than the prediction's
    channels); a channel of weight zero gets a gradient of exact zeros.  None (default): every channel 1 / C,
    and `rel2` / `mse` are then RelL2Loss / MSELoss bit for bit, loss and gradient.
    relinf and linf are metrics: a prediction that requires grad is a ValueError.  A sample without points is
    refused for every kind.  normalizer: as in RelL2Loss.
    `terms(x_off, pred, tgt)` is the [B, C] table of the unweighted e[b, c] (a device tensor, no_grad);
    `trajectory_name()` names kind and weights for fit's state file."""

    _work_floats = "gnot_lp_loss_work_floats"

    def __init__(self, kind="rel2", component_weights=None, normalizer=None):
        if kind not in _lib.LP_KINDS:
            raise ValueError(f"LpLoss: unknown kind {kind!r} (one of {', '.join(_lib.LP_KINDS)})")
        if component_weights is not None:
            component_weights = [float(v) for v in component_weights]
            if not component_weights:
                raise ValueError("LpLoss: component_weights is empty")
            if not all(math.isfinite(v) for v in component_weights):
                raise ValueError("LpLoss: component_weights must be finite")
            if min(component_weights) < 0:
                raise ValueError("LpLoss: component_weights must not be negative")
            total = float(torch.tensor(component_weights, dtype=torch.float32).sum())
            if not (total > 0 and math.isfinite(total)):
                raise ValueError("LpLoss: component_weights need a positive (fp32-finite) sum")
        super().__init__(normalizer)
        self.kind, self.component_weights = kind, component_weights
        self._w = None             # the weights on the predictions' device

    def trajectory_name(self):
        w = "" if self.component_weights is None else f", w={self.component_weights}"
        return f"LpLoss({self.kind}{w})"

    def _run(self, x_off, predictions, targets, want_terms, point_weights=None):
        """(loss, terms or None); every refusal the host can make comes before any GPU work"""
        C = predictions.shape[1]
        if point_weights is not None:
            point_weights = self._point_weights(point_weights, predictions)
        if self.kind in ("relinf", "linf") and predictions.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"LpLoss({self.kind}) is a metric only: it has no gradient, and this prediction requires "
                             "one (call it under torch.no_grad() or on a detached prediction)")
        if self.component_weights is not None and len(self.component_weights) != C:
            raise ValueError(f"LpLoss: {len(self.component_weights)} component_weights, the prediction has {C} channels")
        if not predictions.is_cuda:
            raise RuntimeError("gnot_amd.LpLoss runs on a ROCm GPU only (libgnot_hip.so)")
        off_dev, work, off_host = self._geometry(x_off, predictions, weighted=point_weights is not None)
        stats = self._y_stats(predictions)
        if self.component_weights is not None and (self._w is None or self._w.device != predictions.device):
            self._w = torch.tensor(self.component_weights, dtype=torch.float32, device=predictions.device)
        terms = torch.empty(len(off_host) - 1, C, dtype=torch.float32, device=predictions.device) if want_terms else None
        loss = _NativeLpLoss.apply(predictions.contiguous().float(), targets.contiguous().float(), off_dev, off_host,
                                   work, self.kind, self._w, stats, terms, point_weights)
        return loss, terms

    def forward(self, x_off, predictions, targets, point_weights=None):
        """point_weights: as in RelL2Loss.forward -- the terms above with sum_n w_n in place of sum_n, sum w in
        place of N_b and the maxima over the rows with w_n > 0 (gnot_lp_loss_weighted)"""
        return self._run(x_off, predictions, targets, False, point_weights)[0]

    def loss_and_terms(self, x_off, predictions, targets, point_weights=None):
        """(loss, terms [B, C]) of one pass; the loss is forward()'s, bit for bit, and differentiable like it"""
        return self._run(x_off, predictions, targets, True, point_weights)

    def terms(self, x_off, predictions, targets, point_weights=None):
        """the e[b, c] as a [B, C] device tensor (no_grad; they do not depend on the component weights)"""
        with torch.no_grad():
            return self._run(x_off, predictions, targets, True, point_weights)[1]


# ------------------------------------------------------------------ OneCycleLR (main.py:52)
class OneCycle:
    """torch.optim.lr_scheduler.OneCycleLR(max_lr, total_steps = epochs * steps_per_epoch) defaults:
    pct_start 0.3, cosine annealing, div_factor 25, final_div_factor 1e4, cycle_momentum with
    base/max momentum 0.85/0.95 applied to AdamW's beta1."""

    def __init__(self, max_lr, epochs, steps_per_epoch, pct_start=0.3, div_factor=25.0, final_div_factor=1e4,
                 base_momentum=0.85, max_momentum=0.95):
        self._ctor = dict(max_lr=max_lr, epochs=epochs, steps_per_epoch=steps_per_epoch, pct_start=pct_start,
                          div_factor=div_factor, final_div_factor=final_div_factor, base_momentum=base_momentum,
                          max_momentum=max_momentum)
        self.total = epochs * steps_per_epoch
        self.max_lr = max_lr
        self.initial_lr = max_lr / div_factor
        self.min_lr = self.initial_lr / final_div_factor
        self.phases = [(float(pct_start * self.total) - 1, self.initial_lr, max_lr, max_momentum, base_momentum),
                       (self.total - 1, max_lr, self.min_lr, base_momentum, max_momentum)]
        self.last = 0          # OneCycleLR.__init__ performs the first step(): last_epoch = 0

    @staticmethod
    def _cos(start, end, pct):
        return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)

    def values(self, step=None):
        """(lr, beta1) at scheduler step `step` (default: the current one)."""
        s = self.last if step is None else step
        start = 0.0
        for i, (end, lr0, lr1, m0, m1) in enumerate(self.phases):
            if s <= end or i == len(self.phases) - 1:
                pct = (s - start) / (end - start)
                return self._cos(lr0, lr1, pct), self._cos(m0, m1, pct)
            start = end
        raise AssertionError

    def step(self):
        self.last += 1

    def state_dict(self):
        """`last` and the constructor values (plain Python numbers)."""
        return dict(self._ctor, last=self.last, total=self.total)

    def load_state_dict(self, state):
        """Continue at the stored position.  A schedule of a different length or peak is another trajectory
        and is refused; the shape arguments (pct_start, the factors, the momenta) are taken from the file."""
        for k in ("total", "max_lr"):
            if state[k] != getattr(self, k):
                raise ValueError(f"OneCycle.load_state_dict: {k} is {state[k]!r} in the stored state, "
                                 f"{getattr(self, k)!r} here")
        self.__init__(**{k: state[k] for k in self._ctor})
        self.last = int(state["last"])


# ------------------------------------------------------------------ AdamW (main.py:51)
def flatten_parameters(model):
    """Re-home every Linear's weight/bias into ONE device buffer laid out like the engine's gradient
    arena (W0, b0, W1, b1, ... in canonical order).  Parameters keep their identity (only .data
    moves), so existing optimizers and state_dict() are unaffected.  Returns the flat buffer."""
    lins = model.linears()
    dev = lins[0].weight.device
    total = sum(l.weight.numel() + l.bias.numel() for l in lins)
    flat = torch.empty(total, dtype=torch.float32, device=dev)
    o = 0
    with torch.no_grad():
        for l in lins:
            for p in (l.weight, l.bias):
                n = p.numel()
                flat[o:o + n].copy_(p.reshape(-1))
                p.data = flat[o:o + n].view(p.shape)
                o += n
    model._engine = None        # parameter pointers moved: rebind
    return flat


# ------------------------------------------------------------------ frozen tensors and AdamW parameter groups
SLICE = 8192        # elements per row of a slice table: kClipSlice of csrc/train.hip, the bound gnot_hip.h states


def arena_layout(model):
    """[(state_dict name, numel)] of the 2 L tensors of the flat arena in its order (W0, b0, W1, b1, ...: the
    engine's gradient arena, flatten_parameters' buffer).  Host only."""
    names = {id(p): n for n, p in model.named_parameters()}
    return [(names[id(p)], p.numel()) for l in model.linears() for p in (l.weight, l.bias)]


def _matching(patterns, names, what):
    """the names any of the fnmatch patterns matches; a pattern that matches none of them is a ValueError"""
    hit = set()
    for pat in patterns:
        if not isinstance(pat, str):
            raise ValueError(f"param_groups: {what} takes fnmatch patterns (strings), got {pat!r}")
        found = [n for n in names if fnmatch.fnmatchcase(n, pat)]
        if not found:
            raise ValueError(f"param_groups: the {what} pattern {pat!r} matches no parameter (names look like "
                             f"{names[0]!r}, {names[-1]!r})")
        hit.update(found)
    return hit


def param_groups(model, freeze=(), no_decay=(), lr_scale=None, weight_decay=1e-2):
    """The AdamW parameter groups of a fine-tuning run over the 2 L arena tensors (arena_layout), for
    FlatAdamW(groups=).  freeze / no_decay: lists of fnmatch patterns (case-sensitive) over the state_dict names
    -- "blocks.0.*", "*.bias", "out.*".  A frozen tensor is never read or written by the optimizer: no update,
    no weight decay, no moments, and its gradient stays out of the norm.  A no_decay tensor has weight_decay 0,
    every other trainable one `weight_decay`.  lr_scale: {pattern: s}, the first matching pattern (in the dict's
    order) gives a tensor's learning rate lr * s at every step of the schedule, s > 0 and finite; no match: 1.
    A pattern of any of the three that matches no name is a ValueError, as is a string in place of a list.
    Returns a list of {"tensors": [names in arena order], "lr_scale", "weight_decay", "frozen"}: the frozen
    tensors (if any) in one entry with lr_scale 0.0 and weight_decay 0.0, the trainable ones grouped by their
    (lr_scale, weight_decay) in order of first appearance.  Host only; the model is not changed."""
    for what, v in (("freeze", freeze), ("no_decay", no_decay)):
        if isinstance(v, str):
            raise ValueError(f"param_groups: {what} is a list of patterns, not one string")
    weight_decay = float(weight_decay)
    if not (weight_decay >= 0 and math.isfinite(weight_decay)):
        raise ValueError("param_groups: weight_decay must be finite and not negative")
    names = [n for n, _ in arena_layout(model)]
    frozen = _matching(freeze, names, "freeze")
    plain = _matching(no_decay, names, "no_decay")
    scales = []
    for pat, s in (lr_scale or {}).items():
        s = float(s)
        if not (s > 0 and math.isfinite(s)):
            raise ValueError(f"param_groups: lr_scale[{pat!r}] = {s!r} must be positive and finite")
        scales.append((_matching([pat], names, "lr_scale"), s))
    groups, index = [], {}
    for n in names:
        if n in frozen:
            key = (True, 0.0, 0.0)
        else:
            key = (False, next((s for hit, s in scales if n in hit), 1.0), 0.0 if n in plain else weight_decay)
        if key not in index:
            index[key] = len(groups)
            groups.append({"tensors": [], "lr_scale": key[1], "weight_decay": key[2], "frozen": key[0]})
        groups[index[key]]["tensors"].append(n)
    return groups


def slice_table(numels, group_of):
    """The slice table of gnot_adamw_step_groups / gnot_grad_norm_groups for an arena of consecutive tensors of
    numels[i] elements: every tensor whose group_of[i] is not None cut into rows [begin, len, group_of[i]] of at
    most SLICE elements (all but a tensor's last row full), in arena order; a tensor with None has no row.  Rows
    start at tensor boundaries, so the table depends on the layout and the groups alone."""
    rows, begin = [], 0
    for n, g in zip(numels, group_of):
        if g is not None:
            rows += [[begin + o, min(SLICE, n - o), int(g)] for o in range(0, n, SLICE)]
        begin += n
    return rows


class WeightEMA:
    """An exponential moving average of a flat parameter arena: ema += w_t (flat - ema) after optimizer step t,
    w_t = 1 - decay_t.  `ema` starts as a copy of `flat`.
    warmup: decay_t = min(decay, (1 + t) / (10 + t)), so the first steps -- far from anything worth
    averaging -- fade quickly; False: decay_t = decay throughout.
    `FlatAdamW(ema_decay=...)` owns one and updates it inside its update kernel; `update(t)` is the same
    arithmetic as a pass of its own (gnot_ema_update) behind any other optimizer.  `swapped()` makes the
    average the module's parameters for an evaluation or a checkpoint."""

    def __init__(self, flat, decay, warmup=True):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError("WeightEMA: decay must lie strictly between 0 and 1")
        self.flat, self.decay, self.warmup = flat, decay, bool(warmup)
        self.ema = flat.detach().clone()
        self._w = torch.zeros(1, dtype=torch.float32, device=flat.device)

    def weight(self, t):
        """w_t = 1 - decay_t of optimizer step t (1, 2, ...): host double arithmetic, rounded to fp32."""
        d = min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay
        return torch.tensor(1.0 - d, dtype=torch.float32).item()

    def update(self, t):
        """ema += w_t (flat - ema) on the current stream (one fill, one kernel, no synchronisation)."""
        self._w.fill_(self.weight(t))
        s = ctypes.c_void_p(torch.cuda.current_stream(self.flat.device).cuda_stream)
        _lib.check(_lib.load().gnot_ema_update(self.ema.data_ptr(), self.flat.data_ptr(), self.flat.numel(),
                                               self._w.data_ptr(), s))

    def _exchange(self):
        with torch.no_grad():
            tmp = self.flat.clone()
            self.flat.copy_(self.ema)
            self.ema.copy_(tmp)

    @contextlib.contextmanager
    def swapped(self):
        """Inside the block `flat` -- the module's parameters -- holds the average and `ema` the raw weights;
        the contents are exchanged in place (the engine re-packs its weight images from the same pointers at
        every forward: no rebind) and exchanged back on exit, also after an exception."""
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()

    def state_dict(self):
        return {"ema": self.ema.detach().clone(), "decay": self.decay, "warmup": self.warmup,
                "numel": self.flat.numel()}

    def load_state_dict(self, state):
        """Continue the stored average.  Another size or decay is another average and is refused; the warm-up
        flag is taken from the file."""
        if int(state["numel"]) != self.flat.numel() or state["ema"].numel() != self.flat.numel():
            raise ValueError(f"WeightEMA.load_state_dict: the stored average has numel {int(state['numel'])}, "
                             f"this arena {self.flat.numel()}")
        if float(state["decay"]) != self.decay:
            raise ValueError(f"WeightEMA.load_state_dict: decay is {state['decay']!r} in the stored state, "
                             f"{self.decay!r} here")
        self.warmup = bool(state["warmup"])
        self.ema.copy_(state["ema"].reshape(-1))


class FlatAdamW:
    """torch.optim.AdamW(params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2) on a flat arena.
    grad: the flat gradient buffer of the step (Engine.grad_flat, same layout as `flat`).

    max_grad_norm: torch.nn.utils.clip_grad_norm_(params, max_grad_norm) (L2, error_if_nonfinite=False)
    in front of every step, on the device: `launch()` issues gnot_grad_clip (the global norm of the whole
    arena and the coefficient min(1, max / (norm + 1e-6))) and gnot_adamw_step_clipped, which scales each
    gradient element as it reads it.  Unlike torch, which scales `.grad` in place, the gradient buffer is
    NOT modified: `grad_flat` stays unclipped after the step.  `grad_norm` is a 0-d device tensor (a view
    of the norm the last launch computed, before clipping); reading it is the caller's synchronisation.
    With several ranks every rank holds the same summed gradient after the backward, so every rank
    computes the same norm: no collective.  None (default): the plain gnot_adamw_step, nothing else.

    skip_nonfinite: a step whose gradient norm is NaN or infinite changes no parameter and no moment.  The
    test runs on the device inside the update kernel (gnot_adamw_step_guarded, behind gnot_grad_clip with
    max_grad_norm and gnot_grad_norm without), so `launch()` still never synchronises and stays capturable:
    every replay decides on its own gradient.  `skipped_steps` (skips since construction) and `last_skipped`
    (1 if the last launch skipped) are 0-d int32 device views; reading them is the caller's
    synchronisation, like `grad_norm`.  A skipped step still consumes its step number `t` and its schedule
    slot -- `prepare()` runs before the device knows the outcome -- unlike torch's GradScaler, which does
    not call optimizer.step() on a skip.  A finite gradient whose sum of squares overflows fp32 is skipped
    too.  With ranks or accumulated micro-batches every rank tests the same summed arena: one decision.
    False (default): the paths above, unchanged.

    ema_decay: keep an exponential moving average of the parameters, `opt.ema` (a WeightEMA; ema_warmup is
    its warm-up flag).  The update kernel of whichever path above is replaced by gnot_adamw_step_ema, which
    computes the same parameters and moments bit for bit and moves the average in the same pass; the weight
    w_t of step t is a ninth hyper-parameter `prepare()` writes, so `launch()` stays capturable.  A step the
    guard skips leaves the average alone.  None (default): no average, the kernels and the 8-float hyper
    above.

    groups, layout: fine-tuning -- frozen tensors and torch.optim.AdamW's parameter groups.  groups: the list
    param_groups(model, freeze, no_decay, lr_scale) returns; layout: arena_layout(model), the names and sizes
    the entries' "tensors" refer to (every tensor of the layout in exactly one entry; at least one not
    frozen).  The norm and the update then run over a slice table of the trainable tensors
    (gnot_grad_norm_groups / gnot_grad_clip_groups and gnot_adamw_step_groups, one launch each as above): a
    tensor of entry k steps with lr * lr_scale_k -- of the schedule's lr at every step -- and weight_decay_k,
    the constructor's weight_decay is not used, and a frozen tensor is neither read nor written: its
    parameters, moments (zeros) and average (the weight itself) keep their bits, and a NaN in its gradient
    changes nothing.  `grad_norm` is the norm of the trainable gradient, which is also what max_grad_norm
    clips by and skip_nonfinite tests.  max_grad_norm, skip_nonfinite and ema_decay combine as above and
    `launch()` stays capturable.  One group of lr_scale 1 over every tensor computes the update above bit for
    bit (with a power-of-two gradient scale; the norm's bits differ, its slices start at tensor boundaries).
    state_dict() names the groups and load_state_dict refuses a state written under other ones.  None
    (default): the entries above, nothing else."""

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, schedule=None,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=True, groups=None, layout=None):
        self.groups = None
        nparts = None
        if groups is not None:
            nparts = self._init_groups(flat, groups, layout)
        elif layout is not None:
            raise ValueError("FlatAdamW: a layout without groups")
        self.ema = None if ema_decay is None else WeightEMA(flat, ema_decay, ema_warmup)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.grad_norm = self.skipped_steps = self.last_skipped = None
        if self.max_grad_norm is not None and not (self.max_grad_norm > 0 and math.isfinite(self.max_grad_norm)):
            raise ValueError("max_grad_norm must be positive and finite")
        if self.max_grad_norm is not None or self.skip_nonfinite:
            self._clip = torch.zeros(2, dtype=torch.float32, device=flat.device)       # {norm, coefficient}
            self._clip_work = torch.empty(_lib.load().gnot_grad_clip_work_floats(flat.numel()) if nparts is None
                                          else nparts, dtype=torch.float32, device=flat.device)
            self.grad_norm = self._clip[0]
        if self.skip_nonfinite:
            self._guard = torch.zeros(2, dtype=torch.int32, device=flat.device)        # {skipped, skipped now}
            self.skipped_steps, self.last_skipped = self._guard[0], self._guard[1]
        self.flat = flat
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.schedule = schedule
        self.t = 0
        nh = 8 if self.ema is None else 9          # hyper[8]: the EMA weight of the step
        self.hyper = torch.zeros(nh, dtype=torch.float32, device=flat.device)
        # pinned staging ring: the host may run steps ahead of the GPU; a slot is rewritten only
        # after the copy that last read it has executed (its event)
        self._ring = [torch.zeros(nh, dtype=torch.float32).pin_memory() for _ in range(4)]
        self._ev = [None] * 4

    def _init_groups(self, flat, groups, layout):
        """Check `groups` against `layout`, keep a plain copy in self.groups and upload the slice table and the
        group constants; returns the number of slices.  Host checks first, then two small copies."""
        if layout is None:
            raise ValueError("FlatAdamW: groups need the layout they name (arena_layout(model))")
        layout = [(str(n), int(k)) for n, k in layout]
        if sum(k for _, k in layout) != flat.numel():
            raise ValueError(f"FlatAdamW: the layout holds {sum(k for _, k in layout)} elements, the arena "
                             f"{flat.numel()}")
        spec, owner, ghyper = [], {}, []
        for g in groups:
            e = {"tensors": [str(n) for n in g["tensors"]], "lr_scale": float(g["lr_scale"]),
                 "weight_decay": float(g["weight_decay"]), "frozen": bool(g["frozen"])}
            if not e["frozen"]:
                if not (e["lr_scale"] > 0 and math.isfinite(e["lr_scale"])):
                    raise ValueError(f"FlatAdamW: lr_scale {e['lr_scale']!r} of a group must be positive and finite")
                if not (e["weight_decay"] >= 0 and math.isfinite(e["weight_decay"])):
                    raise ValueError(f"FlatAdamW: weight_decay {e['weight_decay']!r} of a group must be finite and "
                                     "not negative")
            for n in e["tensors"]:
                if n in owner:
                    raise ValueError(f"FlatAdamW: {n!r} is in more than one group")
                owner[n] = None if e["frozen"] else len(ghyper)
            if not e["frozen"]:
                ghyper.append([e["lr_scale"], e["weight_decay"]])
            spec.append(e)
        names = [n for n, _ in layout]
        if set(owner) != set(names) or len(set(names)) != len(names):
            odd = sorted(set(owner) ^ set(names))
            raise ValueError(f"FlatAdamW: the groups and the layout name different tensors ({odd[:4]})")
        rows = slice_table([k for _, k in layout], [owner[n] for n in names])
        if not rows:
            raise ValueError("FlatAdamW: every tensor is frozen, there is nothing to optimise")
        self.groups = spec
        self._ngroups = len(ghyper)
        self._slices_host = (ctypes.c_int64 * (3 * len(rows)))(*[v for r in rows for v in r])
        self._slices = torch.tensor(rows, dtype=torch.int64).to(flat.device)
        self._ghyper = torch.tensor(ghyper, dtype=torch.float32).to(flat.device)
        return len(rows)

    def prepare(self):
        """Advance the step count and write this step's hyper-parameters to the device array."""
        self.t += 1
        lr, b1 = (self.lr, self.betas[0]) if self.schedule is None else self.schedule.values()
        b2 = self.betas[1]
        k = self.t % len(self._ring)
        if self._ev[k] is not None:
            self._ev[k].synchronize()
        h = self._ring[k]
        for i, val in enumerate((lr, b1, b2, self.eps, self.wd, 1 - b1 ** self.t, 1 - b2 ** self.t, 1.0)):
            h[i] = val
        if self.ema is not None:
            h[8] = self.ema.weight(self.t)
        self.hyper.copy_(h, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ev[k] = ev

    def launch(self, grad):
        """The update kernel only -- with max_grad_norm, the two norm kernels and the clipped update; with
        skip_nonfinite, the two norm kernels and the guarded update (graph-capturable every way).  With
        ema_decay the update is gnot_adamw_step_ema in each case, behind the same norm kernels."""
        if grad.numel() != self.flat.numel():
            raise ValueError("gradient buffer does not match the parameter arena")
        s = ctypes.c_void_p(torch.cuda.current_stream(self.flat.device).cuda_stream)
        lib, n, hyper = _lib.load(), self.flat.numel(), self.hyper.data_ptr()
        clip = guard = None
        if self.groups is not None:
            return self._launch_groups(grad, lib, n, hyper, s)
        # at most one norm step ...
        if self.grad_norm is not None:
            clip = self._clip.data_ptr()
            if self.max_grad_norm is not None:
                _lib.check(lib.gnot_grad_clip(grad.data_ptr(), n, hyper, self.max_grad_norm,
                                              self._clip_work.data_ptr(), clip, s))
            else:
                _lib.check(lib.gnot_grad_norm(grad.data_ptr(), n, hyper, self._clip_work.data_ptr(), clip, s))
        if self.skip_nonfinite:
            guard = self._guard.data_ptr()
        # ... then one update, through the entry of the options that are on
        arrays = (self.flat.data_ptr(), grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr())
        if self.ema is not None:
            rc = lib.gnot_adamw_step_ema(*arrays, self.ema.ema.data_ptr(), n, hyper, clip, guard, s)
        elif guard is not None:
            rc = lib.gnot_adamw_step_guarded(*arrays, n, hyper, clip, guard, s)
        elif clip is not None:
            rc = lib.gnot_adamw_step_clipped(*arrays, n, hyper, clip, s)
        else:
            rc = lib.gnot_adamw_step(*arrays, n, hyper, s)
        _lib.check(rc)

    def _launch_groups(self, grad, lib, n, hyper, s):
        """launch() with groups: the same sequence through the slice-table entries"""
        clip = guard = None
        table = (self._slices.data_ptr(), self._slices_host, self._slices.shape[0])
        if self.grad_norm is not None:
            clip = self._clip.data_ptr()
            if self.max_grad_norm is not None:
                _lib.check(lib.gnot_grad_clip_groups(grad.data_ptr(), n, hyper, self.max_grad_norm, *table,
                                                     self._clip_work.data_ptr(), clip, s))
            else:
                _lib.check(lib.gnot_grad_norm_groups(grad.data_ptr(), n, hyper, *table, self._clip_work.data_ptr(),
                                                     clip, s))
        if self.skip_nonfinite:
            guard = self._guard.data_ptr()
        _lib.check(lib.gnot_adamw_step_groups(
            self.flat.data_ptr(), grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
            None if self.ema is None else self.ema.ema.data_ptr(), n, hyper, self._ghyper.data_ptr(), self._ngroups,
            *table, clip, guard, s))

    def step(self, grad):
        self.prepare()
        self.launch(grad)

    def state_dict(self):
        """Copies of exp_avg / exp_avg_sq, the step count, the skipped count (a device read when
        skip_nonfinite is on), the scalar hyper-parameters and, with ema_decay, the average ("ema": WeightEMA's
        state).  The parameters themselves are the model's."""
        state = {"exp_avg": self.m.detach().clone(), "exp_avg_sq": self.v.detach().clone(), "t": self.t,
                 "skipped": int(self.skipped_steps) if self.skip_nonfinite else 0, "numel": self.flat.numel(),
                 "lr": self.lr, "beta1": self.betas[0], "beta2": self.betas[1], "eps": self.eps,
                 "weight_decay": self.wd, "max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite}
        if self.ema is not None:
            state["ema"] = self.ema.state_dict()       # only with ema_decay: the keys above are the rest
        if self.groups is not None:
            state["groups"] = [dict(g, tensors=list(g["tensors"])) for g in self.groups]      # only with groups
        return state

    def load_state_dict(self, state):
        """Continue from state_dict()'s values: moments, step count, skipped count, lr / betas / eps /
        weight_decay.  An arena of another size is refused.  max_grad_norm and skip_nonfinite stay the
        constructor's (they decide which kernels launch() issues)."""
        if int(state["numel"]) != self.flat.numel() or state["exp_avg"].numel() != self.flat.numel() \
                or state["exp_avg_sq"].numel() != self.flat.numel():
            raise ValueError(f"FlatAdamW.load_state_dict: the stored state has numel {int(state['numel'])}, "
                             f"this arena {self.flat.numel()}")
        if (self.ema is not None) != (state.get("ema") is not None):
            raise ValueError("FlatAdamW.load_state_dict: the stored state "
                             + ("holds no weight average (ema_decay is set here)" if self.ema is not None
                                else "holds a weight average (ema_decay is not set here)"))
        if state.get("groups") != self.groups:
            raise ValueError("FlatAdamW.load_state_dict: the stored state was written under "
                             + ("no parameter groups" if state.get("groups") is None else "other parameter groups")
                             + (", this optimizer has none" if self.groups is None else " than this optimizer's"))
        if self.ema is not None:
            self.ema.load_state_dict(state["ema"])
        self.m.copy_(state["exp_avg"].reshape(-1))
        self.v.copy_(state["exp_avg_sq"].reshape(-1))
        self.t = int(state["t"])
        self.lr, self.betas, self.eps, self.wd = state["lr"], (state["beta1"], state["beta2"]), state["eps"], \
            state["weight_decay"]
        if self.skip_nonfinite:
            self._guard.copy_(torch.tensor([int(state["skipped"]), 0], dtype=torch.int32))


# ------------------------------------------------------------------ driver (main.py:55-153)
def save_checkpoint(model, path, normalizer=None):
    """torch.save(model.state_dict()) exactly as main.py:151 (reference-compatible keys/shapes).
    normalizer: the model was trained on normalised data; the statistics are folded into its first and last
    Linears (Normalizer.fold), so the file predicts physical outputs from raw inputs -- in gnot_amd.GNOT and in
    the reference module alike -- and holds the reference's keys and nothing else (a GNOT(pre_norm=True) adds its
    one buffer, pre_norm_eps, which only a model with the option loads).  Statistics of a block the
    model embeds in Fourier features cannot be folded: ValueError unless that block is the identity (_foldable)."""
    sd = model.state_dict()
    torch.save(sd if normalizer is None else _foldable(model, normalizer).fold(sd, model._cfg["n_mlp_num_layers"]),
               path)


def _is_identity(block):
    """a stats block of mean 0, rstd 1: encode returns its argument"""
    b = block.detach().cpu()
    return bool((b[0] == 0).all() and (b[2] == 1).all())


def _foldable(model, normalizer):
    """The normalizer whose fold fits `model`'s first Linears.  The Fourier embedding (GNOT's x_fourier /
    fn_fourier) is not affine, so the statistics of an embedded block cannot move into the Linear behind it:
    ValueError if the normalizer holds other than identity statistics for such a block; an identity block of
    an embedded input is widened to the embedded width (it folds to nothing), and theta, y and every block
    that is not embedded fold as always.  Host only."""
    nx, nf = getattr(model, "x_fourier", 0), getattr(model, "fn_fourier", 0)
    if normalizer is None or not (nx or nf):
        return normalizer
    from .data import Normalizer
    from .fourier import width
    bad = [name for name, b in normalizer.blocks().items()
           if ((name == "x" and nx) or (name.startswith("fns.") and nf)) and not _is_identity(b)]
    if bad:
        what = {"x": f"x (x_fourier={nx})"}
        names = ", ".join(what.get(n, f"{n} (fn_fourier={nf})") for n in bad)
        raise ValueError(f"the normalizer holds statistics for {names}, which the model embeds in Fourier features: "
                         "the embedding is not affine, so they cannot be folded into the checkpoint's first Linear.  "
                         "Normalise that block in the dataset itself, or drop it from --normalize (an identity "
                         "block); the state file (state_path / resume) is not affected")
    wide = lambda b, n: Normalizer.identity(b.shape[1] * width(n), b.device) if n else b
    return Normalizer(wide(normalizer.x, nx), normalizer.theta, normalizer.y, [wide(f, nf) for f in normalizer.fns])


def load_checkpoint(model, path):
    """Load a reference (or gnot_amd) state_dict checkpoint; tensors only (weights_only=True)."""
    model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    return model


# the arguments of fit that decide the trajectory: a stored state continues only the run that wrote it
# (compared in this order; steps_per_epoch = ceil(len(train_loader) / accum_steps) last, so a changed
# accum_steps is named as such)
TRAJECTORY_ARGS = ("epochs", "lr", "accum_steps", "per_epoch_schedule", "max_grad_norm", "loss", "skip_nonfinite",
                   "steps_per_epoch")


def _cpu(obj):
    """tensors of a (nested) state moved to the host as copies, everything else as it is"""
    if torch.is_tensor(obj):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_cpu(v) for v in obj]
    return obj


def rng_state(train_loader=None):
    """The host random state a shuffling loader draws from: torch's CPU generator (a DataLoader without a
    generator seeds every epoch's permutation from it) and the loader's own `generator`, if it has one."""
    gen = getattr(train_loader, "generator", None)
    return {"torch": torch.get_rng_state(), "loader": gen.get_state() if gen is not None else None}


def restore_rng_state(state, train_loader=None):
    """Put back what rng_state() returned (the loader state only if this loader has a generator too)."""
    torch.set_rng_state(state["torch"])
    gen = getattr(train_loader, "generator", None)
    if gen is not None and state.get("loader") is not None:
        gen.set_state(state["loader"])


def save_training_state(path, model, opt, sched, next_epoch, best, hist_train, hist_test, args, train_loader=None,
                        ema_args=None, normalizer=None, dropout=None, param_groups=None):
    """Everything fit needs to continue a run bit for bit, in one torch.save of tensors (on the host) and plain
    Python values, readable with weights_only=True: the model state_dict (reference keys), the optimizer's
    and the schedule's state_dict(), the next epoch, the best metric, both histories, the host random state
    (rng_state) and the trajectory arguments `args` (TRAJECTORY_ARGS); with a weight average also `ema_args`
    (fit's ema_decay / ema_warmup; the average itself travels in the optimizer's state, the model entry holds
    the raw weights); with a normalizer its statistics ("normalizer": Normalizer.state_dict(); the model
    entry holds the unfolded weights, which take normalised inputs); with attention dropout its {p, seed, step}
    ("dropout": GNOT.dropout_state(), the step counter the next training forward takes); with frozen tensors or
    parameter groups fit's three arguments ("param_groups": {freeze, no_decay, lr_scale}; the groups they resolve
    to travel in the optimizer's state).  Written under a
    temporary name in the same directory and moved into place with os.replace: a kill in mid-write leaves the
    previous file."""
    state = {"model": _cpu(model.state_dict()), "optimizer": _cpu(opt.state_dict()), "schedule": sched.state_dict(),
             "next_epoch": int(next_epoch), "best": float(best), "hist_train": [float(v) for v in hist_train],
             "hist_test": [float(v) for v in hist_test], "rng": rng_state(train_loader), "args": dict(args)}
    if ema_args is not None:
        state["ema_args"] = dict(ema_args)
    if normalizer is not None:
        state["normalizer"] = normalizer.state_dict()
    if dropout is not None:
        state["dropout"] = dict(dropout)
    if param_groups is not None:
        state["param_groups"] = dict(param_groups)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load_training_state(path):
    """The dict save_training_state wrote; tensors on the host (weights_only=True, like load_checkpoint)."""
    return torch.load(path, map_location="cpu", weights_only=True)


def _to(batch, dev):
    return (batch["x"].to(dev), batch["x_off"], batch["theta"].to(dev), [f.to(dev) for f in batch["fns"]],
            batch["fn_offs"], batch["y"].to(dev))


def _forward_batch(model, batch, dev, encoder=None):
    """(prediction [sum N, out], packed offsets, target) of one batch.  Packed batches (collate_packed)
    go through forward_packed; padded batches (collate_padded) through the reference calling
    convention `model(x, theta, input_functions)` (main.py:84) and are un-padded with the real point
    counts (main.py:87-89) -- the pad rows still enter the attention sums, exactly as in main.py.
    encoder: a data.Normalizer whose encode_batch the (packed) batch still needs, applied on the device."""
    if encoder is not None:
        if "counts" in batch:
            raise ValueError("normalisation takes packed batches (collate_packed) only")
        x, x_off, theta, fns, fn_offs, y = _to(batch, dev)
        enc = encoder.encode_batch(dict(x=x, theta=theta, fns=fns))
        return model.forward_packed(enc["x"], x_off, enc["theta"], enc["fns"], fn_offs), x_off, y
    if "counts" in batch:
        x = batch["x"].to(dev)
        fns = batch["fns"].to(dev) if batch["fns"] is not None else None
        out = model(x, batch["theta"].to(dev), fns)
        counts = batch["counts"]
        pred = torch.cat([out[b, :n] for b, n in enumerate(counts)])
        off = [0]
        for n in counts:
            off.append(off[-1] + n)
        return pred, off, batch["y"].to(dev)
    x, x_off, theta, fns, fn_offs, y = _to(batch, dev)
    return model.forward_packed(x, x_off, theta, fns, fn_offs), x_off, y


def _point_weight_args(batch, dev, fn):
    """{"point_weights": w on the device} for a batch that carries per-point weights (the key `w`: collate_packed
    on 5-tuple items, a DeviceLoader over a dataset with weights), {} for every other batch -- the keyword of the
    call `fn` (a loss's forward / loss_and_terms / terms) that follows.  A callable without that keyword is a
    TypeError that says so: weighted data must not train on an unweighted loss in silence."""
    if "w" not in batch:
        return {}
    target = fn.forward if isinstance(fn, torch.nn.Module) else fn
    params = inspect.signature(target).parameters
    if "point_weights" not in params and not any(p.kind is p.VAR_KEYWORD for p in params.values()):
        name = type(fn).__name__ if isinstance(fn, torch.nn.Module) else getattr(fn, "__qualname__", repr(fn))
        raise TypeError(f"the batch carries point weights (its key 'w'), but {name} takes no point_weights keyword: "
                        "use RelL2Loss / MSELoss / LpLoss, give the loss the keyword, or load the data without weights")
    return {"point_weights": batch["w"].to(dev)}


@contextlib.contextmanager
def _eval_mode(model):
    """the model in eval mode (no attention dropout, as nn.Dropout), its `training` flag restored on exit"""
    was = model.training
    model.eval()
    try:
        yield model
    finally:
        model.train(was)


def _dropout_state(model):
    """GNOT.dropout_state() of a model that drops (attn_dropout > 0), else None"""
    return model.dropout_state() if getattr(model, "attn_dropout", 0.0) else None


def _read_back(losses):
    """the 0-d device losses of many steps as Python floats (each exactly float(loss)): one device read"""
    return torch.stack(losses).tolist() if losses else []


def _check_normalizer(held, normalizer, who):
    """ValueError unless `held` (what a loss or a loader holds) and `normalizer` (what the call was given) are
    both None or carry the same statistics bit for bit.  Host comparisons only."""
    if held is None and normalizer is None:
        return
    if held is None or normalizer is None:
        raise ValueError(f"{who} holds {'no' if held is None else 'a'} normalizer, this call has "
                         f"{'none' if normalizer is None else 'one'}")
    bad = normalizer.mismatch(held)
    if bad is not None:
        raise ValueError(f"{who} holds a normalizer with other statistics than this call's (entry {bad!r})")


_NO_ATTR = object()


def _batch_encoder(loader, normalizer, who):
    """The normalizer whose encode_batch `loader`'s batches still need: None for a loader that has a
    `.normalizer` attribute (data.DeviceLoader normalises as it gathers) -- it must then hold the call's
    statistics, else ValueError -- and `normalizer` itself for every other loader."""
    held = getattr(loader, "normalizer", _NO_ATTR)
    if held is _NO_ATTR:
        return normalizer
    _check_normalizer(held, normalizer, who)
    return None


def evaluate(model, loader, loss_fn=None, normalizer=None):
    """main.py:108-147: mean RelL2 over the test batches, no_grad (no activations kept), the model in eval mode
    (no attention dropout; its `training` flag is restored afterwards).  Batches from
    collate_padded reproduce main.py's padded evaluation; collate_packed batches the unpadded one.
    The batch losses stay on the device and are read once, behind the last batch.
    normalizer: the model takes normalised inputs and returns normalised predictions (fit's normalizer); the
    metric is in physical units.  loss_fn, if given, must hold the same normalizer, and so must a
    data.DeviceLoader; batches of any other loader are encoded on the device (Normalizer.encode_batch)."""
    loss_fn = loss_fn or RelL2Loss(normalizer)
    _check_normalizer(getattr(loss_fn, "normalizer", None), normalizer, "evaluate: loss_fn")
    return _evaluate(model, loader, loss_fn, _batch_encoder(loader, normalizer, "evaluate: the loader"))


def _evaluate(model, loader, loss_fn, encoder, tables=None):
    """evaluate behind its checks; encoder: _batch_encoder's answer for this loader.  tables (a list; loss_fn is
    then an LpLoss): every batch's [B, C] terms are appended to it, device tensors from the same pass as its loss"""
    dev = next(model.parameters()).device
    vals = []
    with torch.no_grad(), _eval_mode(model):
        for batch in loader:
            pred, off, y = _forward_batch(model, batch, dev, encoder)
            if tables is None:
                vals.append(loss_fn(off, pred, y, **_point_weight_args(batch, dev, loss_fn)))
            else:
                loss, terms = loss_fn.loss_and_terms(off, pred, y,
                                                     **_point_weight_args(batch, dev, loss_fn.loss_and_terms))
                vals.append(loss)
                tables.append(terms)
    vals = _read_back(vals)
    return sum(vals) / max(len(vals), 1)


def evaluate_table(model, loader, kind="rel2", normalizer=None):
    """The per-sample error table of a test set: a host tensor [S, C], row s the terms e[s, c] of LpLoss(kind)
    for the s-th sample in loader order (batch after batch, samples in batch order), one column per output
    channel -- which meshes and which fields are the bad ones.  no_grad; every batch's terms stay on the device
    and the table is read once, behind the last batch.  normalizer: as in evaluate (the same checks; the errors
    are in physical units)."""
    loss_fn = LpLoss(kind, normalizer=normalizer)
    encoder = _batch_encoder(loader, normalizer, "evaluate_table: the loader")
    dev = next(model.parameters()).device
    tables = []
    with torch.no_grad(), _eval_mode(model):
        for batch in loader:
            pred, off, y = _forward_batch(model, batch, dev, encoder)
            tables.append(loss_fn.terms(off, pred, y, **_point_weight_args(batch, dev, loss_fn.terms)))
    return torch.cat(tables).cpu() if tables else torch.empty(0, 0)


def accum_groups(sizes, accum_steps):
    """Gradient accumulation over micro-batches: `sizes` (samples of every loader batch of an epoch, in
    order) in groups of `accum_steps` consecutive batches -- the tail group may be shorter -- and every
    micro-batch's weight B_i / sum B of its group.  Both native losses are means over samples, so
    sum_i (B_i / sum B) loss_i is the loss of the concatenated batch.  One optimizer step per group:
    len(groups) = ceil(len(sizes) / accum_steps) steps per epoch.  Returns (groups, weights)."""
    k = int(accum_steps)
    if k < 1:
        raise ValueError("accum_steps must be >= 1")
    groups = [list(sizes[i:i + k]) for i in range(0, len(sizes), k)]
    weights = [[b / sum(g) for b in g] for g in groups]
    return groups, weights


def _batch_samples(batch):
    return len(batch["counts"]) if "counts" in batch else len(batch["x_off"]) - 1


def _grouped(loader, k):
    """the loader's batches in lists of k consecutive ones (the last may be shorter)"""
    group = []
    for batch in loader:
        group.append(batch)
        if len(group) == k:
            yield group
            group = []
    if group:
        yield group


def _accum_step(model, eng, opt, loss_fn, group, dev, encoder=None):
    """One optimizer step on a group of micro-batches (fit's accum_steps): returns the micro-batches' losses
    (0-d device tensors, nothing read back) and their weights B_i / sum B; the step's loss is
    sum_i (B_i / sum B) loss_i."""
    _, (weights,) = accum_groups([_batch_samples(b) for b in group], len(group))
    vals = []
    for i, (batch, w) in enumerate(zip(group, weights)):
        pred, off, y = _forward_batch(model, batch, dev, encoder)
        loss = loss_fn(off, pred, y, **_point_weight_args(batch, dev, loss_fn))
        # the first micro-batch overwrites the arena (no clear), the others add; only the last one reduces
        with model.backward_options(accumulate=i > 0, reduce=i == len(group) - 1):
            (loss * w).backward()
        vals.append(loss.detach())
    opt.step(eng.grad_flat)          # the clip (max_grad_norm) and AdamW read the accumulated arena once
    return vals, weights


def fit(model, train_loader, test_loader=None, epochs=100, lr=1e-3, per_epoch_schedule=True, checkpoint=None,
        log=print, loss_fn=None, max_grad_norm=None, accum_steps=1, skip_nonfinite=False, state_path=None,
        resume=False, ema_decay=None, ema_warmup=True, normalizer=None, log_components=False, freeze=None,
        no_decay=None, lr_scale=None):
    """The reference training loop (main.py:50-153): AdamW(lr) + OneCycleLR(max_lr=lr, steps_per_epoch,
    epochs), RelL2 loss, per-epoch test metric and best checkpoint.  With per_epoch_schedule=True the
    schedule is stepped once per epoch, as main.py:106 does.  The loaders decide the batch form:
    collate_padded batches run main.py's zero-padded semantics (pad rows in the attention sums),
    collate_packed batches the packed (per-sample exact) one.
    loss_fn: the training loss, `RelL2Loss()` (default), `MSELoss()` (main.py:97-98) or an `LpLoss(kind,
    component_weights)`; the test metric is RelL2 either way (main.py:143).  A loss with a `trajectory_name()`
    (LpLoss: kind and weights) is stored under it in the state file, every other one under its class name, so a
    run resumes only under the loss that wrote it.  max_grad_norm: global-norm gradient clipping in front of every AdamW
    step (FlatAdamW's max_grad_norm; None = off, the reference's loop).
    accum_steps: every accum_steps consecutive loader batches (micro-batches; the epoch's tail group may be
    shorter) form ONE optimizer step on the gradient of their concatenation (accum_groups): micro-batch i
    runs (loss_i * B_i / sum B).backward(), the first overwriting and the others adding onto a gradient
    arena owned by fit (GNOT.set_grad_arena), only the last one reducing over ranks; AdamW and the clip read
    the arena once per group, and the schedule counts optimizer steps.  The logged loss of a step is
    sum_i (B_i / sum B) loss_i.  A batch of main.py:41's four large meshes that does not fit one plan
    runs as accum_steps = 4 loader batches of one.  1 (default): one step per loader batch, no arena.
    skip_nonfinite: FlatAdamW's device-side guard -- a step (with accum_steps, a whole group) whose gradient
    norm is NaN or infinite leaves the parameters and moments alone.  An epoch's train loss is then the mean
    over its finite step losses, and an epoch that skipped steps logs their number (one device read per
    epoch).  False (default): one NaN gradient makes every parameter NaN, as in the reference's loop.
    state_path: after every epoch (after its evaluation and checkpoint) the whole training state is written
    there (save_training_state).  resume: if state_path exists, continue the run it holds -- weights,
    moments, step count, schedule position, histories, best metric, host random state -- at its next epoch,
    bit for bit the uninterrupted run; if it does not exist, start from scratch, so one command line serves
    the first launch and every restart.  A file written under other trajectory arguments (TRAJECTORY_ARGS)
    is refused.
    ema_decay: FlatAdamW's weight average (ema_warmup: WeightEMA's warm-up).  The per-epoch test metric and
    the best checkpoint are computed on the averaged weights (`opt.ema.swapped()`); training itself -- the
    train losses, the raw weights, the moments -- is bit for bit the run without it, and the average moves
    once per optimizer step (with accum_steps, per group; with ranks every rank averages the same
    parameters: no collective).  The state file keeps the raw weights, carries the average inside the
    optimizer state and names the two arguments in its own entry, "ema_args"; resume refuses a file whose
    entry differs from this call's, an absent one included.  None (default): raw weights throughout.
    normalizer (a data.Normalizer): train on unit-Gaussian inputs and targets.  The model sees normalised x,
    theta and input functions and its output is read as a normalised prediction; both losses -- the training
    loss and the RelL2 test metric -- compare it with the raw targets in physical units (RelL2Loss /
    MSELoss(normalizer=)).  A loss_fn passed in must hold the same normalizer.  A data.DeviceLoader (train or
    test) must hold one with equal statistics and normalises as it gathers; the batches of every other loader
    are encoded on the device (Normalizer.encode_batch, the same bits).  Anything else is a ValueError, raised
    before any GPU work.  The best checkpoint is written folded (Normalizer.fold; with ema_decay the averaged
    weights are the ones folded), so it predicts physical outputs from raw inputs with the reference's keys.
    The state file keeps the unfolded weights and the statistics in an entry of its own, "normalizer"; resume
    refuses a file whose statistics differ, one that has the entry when this call has no normalizer, and one
    that lacks it when this call has one.  Padded batches and the point-sharded losses are out of scope.
    A block the model embeds in Fourier features (GNOT's x_fourier / fn_fourier) cannot be folded -- the
    embedding is not affine: with a checkpoint, non-identity statistics for such a block are a ValueError before
    any GPU work (normalise that block in the dataset, or leave it out of the statistics); the state file takes
    any combination.
    None (default): raw data, every call what it was.
    A model with attention dropout (GNOT(attn_dropout=p)) drops in the training forwards only: the test pass runs
    in eval mode and restores the flag.  The state file names {p, seed, step} in an entry of its own, "dropout";
    resume restores the step counter and refuses a file whose p or seed differ, one that has the entry when the
    model does not drop, and one that lacks it when the model does.
    log_components: with a test loader, every epoch also logs "Epoch k, Test Metric per component: [...]", one
    value per output channel: the MEAN OVER ALL TEST SAMPLES of the per-sample RelL2 terms (the column means of
    evaluate_table's rel2 table), taken from the same forwards as the scalar metric -- the metric pass writes its
    terms beside its loss (LpLoss.loss_and_terms), bit for bit the same loss.  The scalar metric stays main.py's
    mean over BATCHES of the batch means; when the last batch is short the mean of the logged components is
    therefore not the scalar metric.  The return value is unchanged.  False (default): nothing else happens.
    freeze, no_decay, lr_scale: fine-tuning a trained model (load_checkpoint first) -- param_groups' arguments:
    lists of fnmatch patterns over the state_dict names and a {pattern: s} dict.  With any of them given, fit
    sets the requires_grad of every Linear's weight and bias for the duration of the call (False on the `freeze`
    matches, True on the rest; the caller's flags are put back on return, like the engine's other settings), so
    the engine plans no weight-gradient job for a Linear whose weight and bias are both frozen and its backward
    stops at the lowest stage that still trains (GNOT.trainable_mask), and the optimizer runs per group
    (FlatAdamW(groups=)): a frozen tensor keeps its bits --
    no update, no weight decay, and with ema_decay its average stays equal to the weight --, a no_decay tensor
    has weight_decay 0, a tensor matching lr_scale follows the schedule at s times its rate, and max_grad_norm
    / skip_nonfinite see the norm of the trainable gradient only.  A pattern that matches nothing is a
    ValueError before any GPU work.  The state file names the three arguments in an entry of its
    own, "param_groups"; resume refuses a file whose entry differs from this call's in any of them, an absent
    one included.  All None (default): one group, the plain kernels, every call what it was.
    No step reads its loss back: every step's 0-d loss (with accum_steps, every micro-batch's) stays on the
    device and the epoch reads them all at its end, then does the host arithmetic above on those fp32 values;
    with a loader whose batches are on the device already (data.DeviceLoader) the host runs ahead of the GPU
    through a whole epoch.
    Returns (train losses per epoch, test metrics per epoch), the resumed epochs included."""
    accum_steps = int(accum_steps)
    if accum_steps < 1:
        raise ValueError("accum_steps must be >= 1")
    if resume and not state_path:
        raise ValueError("resume needs a state_path")
    if checkpoint:
        _foldable(model, normalizer)     # statistics of a Fourier-embedded block cannot be folded: refuse now
    loss_fn = loss_fn or RelL2Loss(normalizer)
    _check_normalizer(getattr(loss_fn, "normalizer", None), normalizer, "fit: loss_fn")
    enc_train = _batch_encoder(train_loader, normalizer, "fit: train_loader")
    enc_test = None if test_loader is None else _batch_encoder(test_loader, normalizer, "fit: test_loader")
    steps_per_epoch = -(-len(train_loader) // accum_steps)
    args = dict(epochs=int(epochs), lr=float(lr), steps_per_epoch=steps_per_epoch, accum_steps=accum_steps,
                per_epoch_schedule=bool(per_epoch_schedule),
                max_grad_norm=None if max_grad_norm is None else float(max_grad_norm),
                loss=loss_fn.trajectory_name() if hasattr(loss_fn, "trajectory_name") else type(loss_fn).__name__,
                skip_nonfinite=bool(skip_nonfinite))
    # beside args, not in it: TRAJECTORY_ARGS is the raw trajectory, which the average does not touch
    ema_args = None if ema_decay is None else dict(ema_decay=float(ema_decay), ema_warmup=bool(ema_warmup))
    group_args = groups = None
    if freeze is not None or no_decay is not None or lr_scale is not None:
        groups = param_groups(model, freeze or (), no_decay or (), lr_scale)      # refuses before any GPU work
        if all(g["frozen"] for g in groups):
            raise ValueError("fit: freeze matches every parameter, there is nothing to train")
        group_args = dict(freeze=[str(v) for v in freeze or ()], no_decay=[str(v) for v in no_decay or ()],
                          lr_scale={str(k): float(v) for k, v in (lr_scale or {}).items()})
    state = None
    if resume and os.path.exists(state_path):
        state = load_training_state(state_path)
        for k in TRAJECTORY_ARGS:
            if state["args"].get(k) != args[k]:
                raise ValueError(f"fit(resume=True): {state_path} was written with {k}={state['args'].get(k)!r}, "
                                 f"this call has {k}={args[k]!r}")
        stored = state.get("ema_args") or {}
        for k in ("ema_decay", "ema_warmup"):
            if stored.get(k) != (ema_args or {}).get(k):
                raise ValueError(f"fit(resume=True): {state_path} was written with {k}={stored.get(k)!r}, "
                                 f"this call has {k}={(ema_args or {}).get(k)!r}")
        stored = state.get("param_groups") or {}
        for k in ("freeze", "no_decay", "lr_scale"):
            if stored.get(k) != (group_args or {}).get(k):
                raise ValueError(f"fit(resume=True): {state_path} was written with {k}={stored.get(k)!r}, "
                                 f"this call has {k}={(group_args or {}).get(k)!r}")
        stored, mine = state.get("dropout"), _dropout_state(model)
        for k in ("p", "seed"):
            if (stored or {}).get(k) != (mine or {}).get(k):
                raise ValueError(f"fit(resume=True): {state_path} was written with dropout {k}={(stored or {}).get(k)!r}, "
                                 f"this call's model has {k}={(mine or {}).get(k)!r}")
        stored = state.get("normalizer")
        if (stored is None) != (normalizer is None):
            raise ValueError(f"fit(resume=True): {state_path} "
                             + ("has no normalizer entry, this call has a normalizer" if stored is None
                                else "has a normalizer entry, this call has no normalizer"))
        if normalizer is not None and normalizer.mismatch(stored) is not None:
            raise ValueError(f"fit(resume=True): {state_path} was written with other statistics in its normalizer "
                             f"entry ({normalizer.mismatch(stored)!r} differs from this call's)")
        model.load_state_dict(state["model"])       # before the parameters move into the flat arena
    layout, flags = None, None
    if groups is not None:
        layout = arena_layout(model)
        frozen = {n for g in groups if g["frozen"] for n in g["tensors"]}
        names = {id(p): n for n, p in model.named_parameters()}
        flags = [(p, p.requires_grad) for l in model.linears() for p in (l.weight, l.bias)]
        for p, _ in flags:
            p.requires_grad_(names[id(p)] not in frozen)
    flat = flatten_parameters(model)
    sched = OneCycle(lr, epochs, steps_per_epoch)
    opt = FlatAdamW(flat, lr=lr, schedule=sched, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                    ema_decay=ema_decay, ema_warmup=ema_warmup, groups=groups, layout=layout)
    dev = flat.device
    prev_arena = model._grad_arena
    if accum_steps > 1:
        model.set_grad_arena(torch.empty(flat.numel(), dtype=torch.float32, device=dev))
    eng = model.engine()
    prev = eng.param_grads
    eng.param_grads = False          # FlatAdamW reads the gradient arena; no .grad copies
    log_components = bool(log_components) and test_loader is not None
    if log_components:
        metric = LpLoss("rel2", normalizer=normalizer)      # RelL2Loss's bits, and the terms in the same pass
    else:
        metric = loss_fn if type(loss_fn) is RelL2Loss else RelL2Loss(normalizer)
    best, hist_train, hist_test, first, skipped = float("inf"), [], [], 0, 0
    if state is not None:
        opt.load_state_dict(state["optimizer"])
        sched.load_state_dict(state["schedule"])
        best, hist_train, hist_test = state["best"], list(state["hist_train"]), list(state["hist_test"])
        first, skipped = state["next_epoch"], int(state["optimizer"]["skipped"])
        restore_rng_state(state["rng"], train_loader)
        if state.get("dropout") is not None:
            model.load_dropout_state(state["dropout"])
    try:
        for epoch in range(first, epochs):
            losses = []
            if accum_steps == 1:
                for batch in train_loader:
                    pred, off, y = _forward_batch(model, batch, dev, enc_train)
                    loss = loss_fn(off, pred, y, **_point_weight_args(batch, dev, loss_fn))
                    loss.backward()
                    opt.step(eng.grad_flat)
                    if not per_epoch_schedule:
                        sched.step()
                    losses.append(loss.detach())
                losses = _read_back(losses)
            else:
                steps = []
                for group in _grouped(train_loader, accum_steps):
                    steps.append(_accum_step(model, eng, opt, loss_fn, group, dev, enc_train))
                    if not per_epoch_schedule:
                        sched.step()
                vals = iter(_read_back([l for ls, _ in steps for l in ls]))
                losses = [sum(next(vals) * w for w in weights) for _, weights in steps]
            if per_epoch_schedule:
                sched.step()
            if skip_nonfinite:
                losses = [l for l in losses if math.isfinite(l)]
            hist_train.append(sum(losses) / max(len(losses), 1))
            log(f"Epoch {epoch}, Loss: {hist_train[-1]}")
            if skip_nonfinite:
                total = int(opt.skipped_steps)
                if total > skipped:
                    log(f"Epoch {epoch}, Skipped steps: {total - skipped} (non-finite gradient norm)")
                skipped = total
            if test_loader is not None:
                # with ema_decay the metric and the checkpoint see the averaged weights
                with opt.ema.swapped() if opt.ema is not None else contextlib.nullcontext():
                    tables = [] if log_components else None
                    res = _evaluate(model, test_loader, metric, enc_test, tables)
                    hist_test.append(res)
                    log(f"Epoch {epoch}, Test Metric: {res}")
                    if tables:
                        log(f"Epoch {epoch}, Test Metric per component: "
                            f"{torch.cat(tables).cpu().double().mean(0).tolist()}")
                    if res < best and checkpoint:
                        best = res
                        save_checkpoint(model, checkpoint, normalizer)
            if state_path:       # outside the swap: the raw weights, the average inside the optimizer state
                save_training_state(state_path, model, opt, sched, epoch + 1, best, hist_train, hist_test, args,
                                    train_loader, ema_args, normalizer, _dropout_state(model), group_args)
    finally:
        eng.param_grads = prev       # ordinary autograd use after fit() gets .grad again
        for p, was in flags or ():   # ... and the caller's requires_grad flags
            p.requires_grad_(was)
        if accum_steps > 1:
            model.set_grad_arena(prev_arena)
    return hist_train, hist_test
