"""The staggered stage loop of the d = 256 fp32 weight-gradient kernel (wgrad.hip pgemm_x6w_kernel<3, 256>).

Waves 4 .. 7 of a workgroup (the SIMD partners of waves 0 .. 3) run their row hand-over -- counted wait, read of
the raw slot, scale request, refill DMA -- after half of the iteration's MFMA groups and stage all eight points
beside the other half.  The arithmetic, its order and every wave's order of vector-memory operations are those
of the single ordering, so every result is bit for bit what it was; what can go wrong is a wait that no longer
covers its data (a run-to-run difference) or a slot refilled before its read (a wrong value).

Model as in test_gpu_moe_streams.py: d = 256, 8 heads, one block, one input function, fp32; 2 and 8 experts;
n_mlp_num_layers 1 and 4.  With serial weight gradients (GNOT_WGRAD_OVERLAP=0) the soft-MoE's last Linear runs
scaled jobs (GELU'd input at nl = 4: the scaled interleaved loop); the forked default keeps the stored dz, so
the same Linears run the unscaled GELU loop; every chain's first hidden Linear after a plain input and the
attention projections run the unscaled plain loop.

Point counts, for the staged loop's edges (a split-K range covers at least 128 points, so a small sample is one
range of ceil(n / 16) stages; the loop body runs stages - 1 times):
  16        one stage: the loop body never runs
  17        two stages, the last partial
  40        three stages: both raw slots used and the first refill read back
  129       a partial last chain block and wave
  77 + 123  a sample boundary inside a block
  2064      balanced ranges ending inside a job: several ranges per workgroup with a barrier between them

Checks per case:
  1. float64 (the stock-torch port): golden_util.check_parity at its existing bars on the output and every
     parameter gradient, serial and forked; input gradients finite;
  2. bitwise: serial = forked = MoE recompute;
  3. bitwise: three forward + backward runs on one model give identical arrays.

Widths below 256 (test_padded_width): jobs with out or in below 256 take the masked interleaved loop on the waves
whose row and column blocks are all present.  test_gpu_widths.py's d = 208 and 224 leave row block 3 of waves
4 .. 7 and column block 1 of waves 3 and 7 empty, so there only waves 0 .. 2 run the masked interleaved loop (the
early ordering) beside the plain loop on the others: no width of that file reaches the late masked loop.  d = 240
(15 heads of 16; out = in = 240 > 224 fills every block) does, on all eight waves, and is added here for it.
"""
import functools

import numpy as np
import pytest

import test_gpu_moe_streams as S
import test_gpu_widths as W
from golden_util import check_parity, model_args, port_reference
from test_gpu_geometry import _run, _same_bits
from test_gpu_parity import _random_case, build_model, run_packed

pytestmark = pytest.mark.gpu

GEOMS = {"one_stage": [16], "two_stages": [17], "three_stages": [40], "one_block_plus_one": [129],
         "two_samples": [77, 123], "split_in_job": [2064]}
KEYS = ("out", "loss", "dx", "dtheta")


@functools.lru_cache(maxsize=None)
def _case(nl, E, geom):
    """one float64 reference per case; the geometries test_gpu_moe_streams.py has share its reference"""
    if geom in S.GEOMS:
        assert S.GEOMS[geom] == GEOMS[geom]
        return S._case(nl, E, geom)
    from gnot_amd import GNOT
    import torch
    cfg = S._cfg(nl, E)
    Ns = GEOMS[geom]
    torch.manual_seed(31)
    params = {k: v.double().numpy() for k, v in GNOT(*model_args(cfg)).state_dict().items()}
    rng = np.random.default_rng(31)
    xs = [rng.random((n, cfg["input_dim"])) for n in Ns]
    thetas = [rng.random(cfg["theta_dim"]) for _ in Ns]
    fns_ps = [[rng.random((S.M_FN, cfg["input_func_dim"]))] for _ in Ns]
    Gs = [rng.standard_normal((n, cfg["out_dim"])) for n in Ns]
    samples, grads, e32 = port_reference(cfg, params, xs, thetas, fns_ps, Gs)
    off = lambda L: np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    return dict(cfg=cfg, params=params, samples=samples, grads=grads, e32=e32, x=np.concatenate(xs),
                x_off=off(Ns), theta=np.stack(thetas), fns=[np.concatenate([f[0] for f in fns_ps])],
                fn_offs=[off([S.M_FN] * len(Ns))], G=np.concatenate(Gs), out=np.concatenate([s["out"] for s in samples]))


def _with_loss(got, fx):
    got["loss"] = np.float64((got["out"] * fx["G"]).sum())
    return got


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("E", [2, 8])
@pytest.mark.parametrize("nl", [1, 4])
def test_wave_stagger(nl, E, geom, monkeypatch):
    fx = _case(nl, E, geom)
    # serial weight gradients: the scaled jobs
    m, serial = S._fresh_run(fx, monkeypatch, "0", None)
    errs = check_parity(serial["out"], serial["grads"], fx)
    print(f"\nWAVE_STAGGER nl={nl} E={E} {geom}: serial parity errors {errs}")
    assert not errs, errs
    assert all(np.isfinite(a).all() for a in (serial["dx"], serial["dtheta"], *serial["dfns"]))
    # the same model twice more: a wait that is one too loose shows as a run-to-run difference
    for rep in (1, 2):
        again = _with_loss(_run(m, fx), fx)
        assert not _same_bits(serial, again, KEYS), f"serial run {rep} differs from run 0"
    # the default (forked) choice of a small plan: stored dz, the unscaled loops
    m, forked = S._fresh_run(fx, monkeypatch, None, None)
    errs = check_parity(forked["out"], forked["grads"], fx)
    print(f"WAVE_STAGGER nl={nl} E={E} {geom}: forked parity errors {errs}")
    assert not errs, errs
    assert all(np.isfinite(a).all() for a in (forked["dx"], forked["dtheta"], *forked["dfns"]))
    assert not _same_bits(serial, forked, KEYS), "forked plan differs from the serial one"
    for rep in (1, 2):
        again = _with_loss(_run(m, fx), fx)
        assert not _same_bits(forked, again, KEYS), f"forked run {rep} differs from run 0"
    # MoE recompute: its backward re-runs the experts in front of the same weight-gradient jobs
    _, rec = S._fresh_run(fx, monkeypatch, "0", None, recompute=True)
    assert not _same_bits(serial, rec, KEYS), "MoE recompute differs"


D240 = W._cfg(240, 15, 2, 1)


@functools.lru_cache(maxsize=None)
def _width_case(name):
    if name in W.CASES:
        return W._case(name)               # the reference test_gpu_widths.py computed
    return _random_case(13, D240, [300, 173], [[120, 77]])


@pytest.mark.parametrize("name", ["d208_h13", "d240_h15"])
def test_padded_width(name, monkeypatch):
    """the masked interleaved loop (module docstring): oracle parity at check_parity's bars, serial and forked,
    serial = forked bitwise, and three runs of one model bitwise equal"""
    fx, G = _width_case(name)
    runs = {}
    for tag, overlap in (("serial", "0"), ("forked", None)):
        if overlap is None:
            monkeypatch.delenv("GNOT_WGRAD_OVERLAP", raising=False)
        else:
            monkeypatch.setenv("GNOT_WGRAD_OVERLAP", overlap)
        m = build_model(fx["params"], fx["cfg"])
        out, grads = run_packed(m, fx, G)
        errs = check_parity(out, grads, fx)
        print(f"\nWAVE_STAGGER {name} {tag}: parity errors {errs}")
        assert not errs, errs
        for rep in (1, 2):
            out2, grads2 = run_packed(m, fx, G)
            assert np.array_equal(out, out2), f"{tag} run {rep}: out differs"
            bad = [k for k in grads if not np.array_equal(grads[k], grads2[k])]
            assert not bad, f"{tag} run {rep}: {bad} differ"
        runs[tag] = (out, grads)
    assert np.array_equal(runs["serial"][0], runs["forked"][0])
    bad = [k for k in runs["serial"][1] if not np.array_equal(runs["serial"][1][k], runs["forked"][1][k])]
    assert not bad, f"serial and forked differ: {bad}"
