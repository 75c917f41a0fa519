"""The bits of every shape an attention call takes, recorded on an MI355X from the build before the engine's plan
described each call once (tests/golden/attn_call_bits.npz, written by `scripts/diag_bitwise_ab.py record-attn` with
the library of the commit "Fold the RelL2 and MSE loss kernels into the Lp family").  Until then a bitwise A/B of two
builds lived in a log only; this replays the cases of tests/attn_call_util.py -- d = 32 with two and without input
functions, each plain, with pre-norm, with attention dropout (p = 0.25, a fixed seed and step) and with x, theta and
the input functions requiring grad; two input functions with the encoders and block 0 frozen; padded heads (d = 30,
2 heads); d = 256 -- on the packed batch Ns = [65, 0, 1, 0, 128], Ms = [17, 5, 1, 0, 64] and requires the stored
output (194 rows) element for element, the stored SHA-256 of the parameter gradients and of every input gradient,
the stored kernel forms and the stored backward plan.

The inputs and weights are regenerated from numpy.random.RandomState: a failure of the first check means the
generator drifted, not the engine."""
import os

import numpy as np
import pytest

import attn_call_util as A

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_call_bits.npz")


@pytest.fixture(scope="module")
def stored():
    return np.load(GOLDEN)


def test_the_fixture_holds_every_case(stored):
    keys = {"in_sha", "out", "grad", "forms", "plan"}
    for name in A.FIXTURE_CASES:
        mine = {k.split(".", 1)[1] for k in stored.files if k.startswith(name + ".")}
        extra = {"dx", "dtheta"} | {f"dfn{i}" for i in range(A.CASES[name][3])} if name.endswith("_igrad") else set()
        assert mine == keys | extra, name
        assert stored[name + ".out"].shape == (A.ROWS, A.OUT) and stored[name + ".out"].dtype == np.float32
    assert len(stored.files) == sum(len(keys) + (2 + A.CASES[n][3] if n.endswith("_igrad") else 0) for n in A.FIXTURE_CASES)
    assert os.path.getsize(GOLDEN) <= 1 << 20


@pytest.mark.parametrize("name", A.FIXTURE_CASES)
def test_the_call_reproduces_the_recorded_bits(stored, name):
    want = {k.split(".", 1)[1]: stored[k] for k in stored.files if k.startswith(name + ".")}
    assert A.generate(name)[-1] == str(want["in_sha"]), "the generator drifted (inputs / weights), not the engine"
    import torch
    got = A.run(name, torch.device("cuda"))
    assert got["forms"] == str(want["forms"])
    assert got["plan"].tolist() == want["plan"].tolist()
    if name == "d32_i2_frozen":
        # the backward stops at block 1 and has fewer weight-gradient jobs than the same model unfrozen
        assert want["plan"][1] == 1 and want["plan"][0] < stored["d32_i2.plan"][0]
    assert got["out"].dtype == want["out"].dtype and got["out"].shape == want["out"].shape
    assert np.array_equal(got["out"].view(np.uint32), want["out"].view(np.uint32)), \
        f"{(got['out'] != want['out']).sum()} of {want['out'].size} output elements differ"
    for k in sorted(set(want) - {"in_sha", "out", "forms", "plan"}):
        assert A.digest(got[k]) == str(want[k]), f"the digest of {k} differs"
