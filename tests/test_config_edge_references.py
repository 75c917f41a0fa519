"""The float64 references of tests/test_gpu_config_edges.py, checked on the CPU: no device needed.

Building a case through the GPU file's own _case runs golden_util.port_reference and _assemble's sharpness
condition: for the output, per sample and per row, 20 e32 (the port's own fp32 error) stays within a quarter
of the 1e-4 term of the parity rule.  A GPU test can therefore never pass because its reference is vague, and
a case whose reference cannot be built (an input the output does not depend on, a zero-width theta) fails
here, on a machine with no GPU.
"""
import numpy as np
import pytest

from golden_util import reference_sharpness
from test_gpu_config_edges import CASES, NS, _case, _fn_points, _padded_theta0_case, unused_encoder_nonzeros


@pytest.mark.parametrize("family,edge", CASES)
def test_config_edge_references(family, edge):
    fx = _case(family, edge)         # asserts the sharpness condition (test_gpu_geometry._assert_reference_is_sharp)
    cfg = fx["cfg"]
    ws, wr = reference_sharpness(fx["samples"])
    print(f"\nCFGE reference {family}/{edge}: 20 e32 over the 1e-4 term, worst sample {ws:.3f}, worst row {wr:.3f}")
    assert ws <= 0.25 and wr <= 0.25, (ws, wr)
    # the case is the batch the GPU file describes
    assert [s["N"] for s in fx["samples"]] == NS
    Ms = _fn_points(cfg["n_input_functions"])
    assert [s["M"] for s in fx["samples"]] == [[M[b] for M in Ms] for b in range(len(NS))]
    assert fx["theta"].shape == (len(NS), cfg["theta_dim"])
    assert all(s["dtheta"].shape == (cfg["theta_dim"],) for s in fx["samples"])
    assert np.isfinite(fx["out"]).all() and np.linalg.norm(fx["out"]) > 0
    if cfg["n_attn_layers"] == 0 and cfg["n_input_functions"] > 0:
        # the input functions do not reach the output: exact zeros, not small numbers
        dfns = [np.concatenate([s["dfns"][i] for s in fx["samples"]]) for i in range(cfg["n_input_functions"])]
        assert not unused_encoder_nonzeros(fx["grads"], dfns)
    else:
        # every other gradient is live (the gate's is zero with one expert or no block)
        for k, g in fx["grads"].items():
            if not k.startswith("gating."):
                assert np.linalg.norm(g) > 0, k


def test_theta0_padded_reference():
    fx = _padded_theta0_case()
    ws, wr = reference_sharpness(fx["samples"])
    assert ws <= 0.25 and wr <= 0.25, (ws, wr)
    assert fx["theta"].shape == (3, 0)
