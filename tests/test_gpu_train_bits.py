"""The bits of the native training step, recorded from the build before the update kernels became one kernel
(tests/golden/train_step_bits.npz: inputs "in.*" and results "out.*", written on an MI355X by
`scripts/diag_bitwise_ab.py record`).  Since then "guarded equals clipped equals plain" compares a kernel with
itself; this replays the stored inputs through every entry -- gnot_adamw_step, _clipped, _guarded and _ema
(plain, a coefficient below 1 and of exactly 1, a finite and a NaN norm; hyper[7] of 1, 0.5 and 0.3; n = 1,
257 and, for a few cases, 8195; the gradient base on a 16-byte boundary and a float off), gnot_grad_clip /
gnot_grad_norm, gnot_rel_l2_loss and gnot_mse_loss (samples of 37, 1 and 2049 rows, 3 channels) -- and requires
the stored bits of param / exp_avg / exp_avg_sq / ema / guard, the clip pair, the loss and d loss / d pred.

The loss family and the slice-table update have a file of their own, tests/golden/train_family_bits.npz, recorded
from the build before RelL2Loss / MSELoss moved onto the Lp kernels and the two AdamW kernels onto one element
update (`scripts/diag_bitwise_ab.py record-family`, with the library of the commit "Add frozen Linears and AdamW
parameter groups for fine-tuning").  Until then `LpLoss("rel2")` against `RelL2Loss()` compared two sets of
kernels; now it compares a kernel with itself, and this file holds what the old set computed."""
import os

import numpy as np
import pytest

import train_step_util as U

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step_bits.npz")
FAMILY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_family_bits.npz")


def test_every_entry_reproduces_the_recorded_bits():
    stored = np.load(GOLDEN)
    inp = {k[3:]: stored[k] for k in stored.files if k.startswith("in.")}
    want = {k[4:]: stored[k] for k in stored.files if k.startswith("out.")}
    assert inp["ns"].tolist() == [1, 257, 8195]
    got = U.step_replay(inp)
    assert sorted(got) == sorted(want)
    # the file holds what the docstring says: every kind at every hyper[7], both losses
    for n, cases in ((1, 60), (257, 60), (8195, 3)):
        assert sum(k.startswith(f"n{n}.") and k.endswith((".p", ".untouched")) for k in want) == cases
    assert all(bool(want[k][0]) for k in want if k.endswith(".untouched"))
    assert all(want[k].tolist() == [1, 1, 0] for k in want if k.endswith("guard_nan.raw.guard"))
    # ... and tells the two forms of g - exp_avg apart: at a hyper[7] of 0.3 the plain entry's exp_avg is not the
    # one of a coefficient of 1 (at 1 and 0.5 it is); with the average the plain entry has the rounded form
    for h7, apart in ((1.0, False), (0.5, False), (0.3, True)):
        m = lambda kind: want[f"n257.o0.h{h7}.{kind}.m"]
        assert (not np.array_equal(m("plain.raw"), m("clip_eq1.raw"))) == apart
        assert np.array_equal(m("plain.ema"), m("clip_eq1.raw"))
    differing = [k for k in want if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    assert differing == [], f"{len(differing)} of {len(want)} arrays differ"


def test_the_loss_family_and_the_groups_update_reproduce_the_recorded_bits():
    """F1: samples of 37, 1 and 2049 rows, 3 channels -- RelL2Loss and MSELoss raw and with a normalizer, every
    LpLoss kind with and without the weights [1, 0, 3], raw and with the normalizer.  F1e: the same rows with an
    empty sample, RelL2Loss alone (its loss is a NaN, stored with its bits).  F2: samples of 4096 and 4097 rows,
    one channel -- both classes, every LpLoss kind unweighted and raw.  G: gnot_adamw_step_groups at n = 257 over
    the rows {0, 100, 0}, {130, 127, 1} behind gnot_grad_clip_groups / gnot_grad_norm_groups, hyper[7] = 0.3, the
    gradient base on a 16-byte boundary and a float off, plain / clipped / guarded / guarded with a NaN norm, with
    and without the average; every array as its whole allocation."""
    stored = np.load(FAMILY)
    inp = {k[3:]: stored[k] for k in stored.files if k.startswith("in.")}
    want = {k[4:]: stored[k] for k in stored.files if k.startswith("out.")}
    assert inp["f1.pred"].shape == (sum(U.LOSS_SIZES), U.LOSS_C) and inp["f2.pred"].shape == (sum(U.FAMILY_F2_SIZES), 1)
    assert inp["g.p"].shape == (U.GROUPS_N,)
    got = U.loss_replay(inp)
    assert sorted(got) == sorted(want)
    count = lambda prefix, suffix="": sum(k.startswith(prefix) and k.endswith(suffix) for k in want)
    # F1: 2 classes x raw / nz x (loss, dpred); 6 kinds x 2 weightings x raw / nz x (loss, terms), and dpred for
    # the 4 differentiable kinds
    assert (count("f1.RelL2Loss.") + count("f1.MSELoss."), count("f1.lp."), count("f1.lp.", ".dpred")) == (8, 64, 16)
    assert count("f1.lp.", ".terms") == 24 and all(want[k].shape == (3, 3) for k in want
                                                    if k.startswith("f1.lp.") and k.endswith(".terms"))
    # F1e: RelL2Loss alone, raw / nz x (loss, dpred), the loss a NaN
    assert count("f1e.") == count("f1e.RelL2Loss.") == 4
    assert all(np.isnan(want[f"f1e.RelL2Loss.{t}.loss"].view(np.float32)).all() for t in ("raw", "nz"))
    # F2: the classes as in F1; 6 kinds x (loss, terms), and dpred for rel1 and l1
    assert (count("f2.RelL2Loss.") + count("f2.MSELoss."), count("f2.lp."), count("f2.lp.", ".dpred")) == (8, 14, 2)
    assert "f2.lp.rel1.u.raw.dpred" in want and "f2.lp.l1.u.raw.dpred" in want
    # G: 2 bases x 4 kinds x (3 arrays without the average + 4 with it); clip for 3 kinds, guard for 2, both x 4
    assert count("g.") == 80 and count("g.", "b") == 56
    assert (count("g.", ".clip"), count("g.", ".guard"), count("g.", ".untouched")) == (12, 8, 4)
    assert all(bool(want[k][0]) for k in want if k.endswith(".untouched"))
    assert all(want[k].tolist() == [1, 1, 0] for k in want if "guard_nan" in k and k.endswith(".guard"))
    assert all(want[k].view(np.float32)[1] < 1 for k in want if "clip_lt1" in k and k.endswith(".clip"))
    # ... the allocations hold the elements around the arrays and the frozen gap: after an update the gap has the
    # input's bits, the trainable elements have not
    pb = want["g.o0.plain.raw.pb"].view(np.float32)
    assert pb.shape == (U.GROUPS_N + 3,) and (pb[U.GROUPS_N:] == U.PAD).all()
    assert np.array_equal(pb[100:130], inp["g.p"][100:130]) and (pb[:100] != inp["g.p"][:100]).all()
    differing = [k for k in want if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    assert differing == [], f"{len(differing)} of {len(want)} arrays differ: {differing[:8]}"
