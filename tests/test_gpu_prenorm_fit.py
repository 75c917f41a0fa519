"""train.fit on a GNOT(..., pre_norm=True): the state file and the checkpoint carry the option's buffer, a run
stopped after its first epoch and resumed is the uninterrupted run bit for bit, and the checkpoint loads only
into a model with the option."""
import os

import numpy as np
import pytest
import torch

import train_step_util as U

pytestmark = pytest.mark.gpu

ARGS = (2, 1, 3, 1, 1, 64, 2, 64, 64, 2, 4, 1)       # train_step_util.SMALL at d = 64
EPOCHS = 2


def _model(seed=0, pre_norm=True):
    from gnot_amd import GNOT
    torch.manual_seed(seed)
    return GNOT(*ARGS, pre_norm=pre_norm).cuda()


@pytest.fixture(scope="module")
def loaders():
    """6 synthetic meshes of 150 to 300 points: two train batches and one test batch of two"""
    from gnot_amd import data
    rng = np.random.default_rng(5)
    mk_s = lambda k: [data.synthetic_sample(rng, int(rng.integers(150, 300)), fn_points=(int(rng.integers(10, 30)),))
                      for _ in range(k)]
    mk = lambda s: list(torch.utils.data.DataLoader(data.NS2dData(s), batch_size=2, shuffle=False,
                                                    collate_fn=data.collate_packed))
    return mk(mk_s(4)), mk(mk_s(2))


def test_resumed_pre_norm_fit_is_the_uninterrupted_fit_bitwise(loaders, tmp_path):
    from gnot_amd import train
    tr, te = loaders
    p, q, ck = (os.path.join(tmp_path, n) for n in ("p.pt", "q.pt", "best.pth"))
    ref = _model()
    ref_hist = train.fit(ref, tr, te, epochs=EPOCHS, state_path=p, checkpoint=ck, log=lambda msg: None)
    ref_flat = U.flat_params(ref).clone()
    assert all(np.isfinite(v) for h in ref_hist for v in h) and len(ref_hist[0]) == EPOCHS

    def log(msg):
        if msg.startswith("Epoch 1, Loss"):               # epoch 0's state is on disk, epoch 1's is not
            raise U.Stop

    with pytest.raises(U.Stop):
        train.fit(_model(), tr, te, epochs=EPOCHS, state_path=q, log=log)
    state = train.load_training_state(q)
    assert state["next_epoch"] == 1 and "pre_norm_eps" in state["model"]
    got = _model(seed=123)                                # a fresh module with other weights
    got_hist = train.fit(got, tr, te, epochs=EPOCHS, state_path=q, resume=True, log=lambda msg: None)
    assert got_hist == ref_hist
    assert torch.equal(U.bits(U.flat_params(got)), U.bits(ref_flat))
    a, b = train.load_training_state(p), train.load_training_state(q)
    assert list(a["model"]) == list(b["model"])
    for k in a["model"]:
        assert torch.equal(a["model"][k], b["model"][k]), k
    # a state file of the option is refused by a model without it (the key), and the other way round
    with pytest.raises(RuntimeError, match="pre_norm_eps"):
        train.fit(_model(pre_norm=False), tr, te, epochs=EPOCHS, state_path=q, resume=True, log=lambda msg: None)
    # the best checkpoint: into a model with the option, not into one without
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    assert "pre_norm_eps" in sd
    m = train.load_checkpoint(_model(seed=7), ck)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items())
    with pytest.raises(RuntimeError, match="pre_norm_eps"):
        train.load_checkpoint(_model(pre_norm=False), ck)
