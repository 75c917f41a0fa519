"""The bits of the native training step, recorded from the build before the update kernels became one kernel
(tests/golden/train_step_bits.npz: inputs "in.*" and results "out.*", written on an MI355X by
`scripts/diag_bitwise_ab.py record`).  Since then "guarded equals clipped equals plain" compares a kernel with
itself; this replays the stored inputs through every entry -- gnot_adamw_step, _clipped, _guarded and _ema
(plain, a coefficient below 1 and of exactly 1, a finite and a NaN norm; hyper[7] of 1, 0.5 and 0.3; n = 1,
257 and, for a few cases, 8195; the gradient base on a 16-byte boundary and a float off), gnot_grad_clip /
gnot_grad_norm, gnot_rel_l2_loss and gnot_mse_loss (samples of 37, 1 and 2049 rows, 3 channels) -- and requires
the stored bits of param / exp_avg / exp_avg_sq / ema / guard, the clip pair, the loss and d loss / d pred."""
import os

import numpy as np
import pytest

import train_step_util as U

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step_bits.npz")


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
