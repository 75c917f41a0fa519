"""The constants of tests/test_gpu_prenorm_kernel.py, measured on the CPU (no GPU): how far torch's own float32
LayerNorm (forward, rstd, autograd backward) lies from float64 on the row kernels' test inputs
(tests/prenorm_util.py: every width, row count and row family), as ratios to the test's error scales.  The
kernels get 4 times the ratio.

    python scripts/prenorm_bounds.py > profiles/prenorm_kernel_bounds.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnot-replication_amd"), os.path.join(ROOT, "tests"), ROOT]

import torch  # noqa: E402

import prenorm_util as PU  # noqa: E402


def main():
    worst = {f: [(0.0, None)] * 3 for f in PU.FAMILIES}
    for C in PU.WIDTHS:
        for rows in PU.ROWS:
            for fam in PU.FAMILIES:
                r = PU.torch_ratios(C, rows, fam)
                worst[fam] = [max(w, (v, (C, rows)), key=lambda t: t[0]) for w, v in zip(worst[fam], r)]
    print(f"torch {torch.__version__} float32 layer_norm on the CPU against float64, inputs of tests/prenorm_util.py")
    print(f"widths {PU.WIDTHS}\nrows {PU.ROWS}")
    print("largest ratio per row family (at C, rows):")
    print("  forward  |y - y64| / (2^-24 (rstd64 max_j |x_rj| + |y64|))")
    print("  rstd     |rstd - rstd64| / (2^-24 rstd64)")
    print("  backward |dx - dx64(y, rstd)| / (2^-24 rstd (|dy_r|_1 / C (1 + |y|) + |dy|))")
    for fam in PU.FAMILIES:
        f, r, b = worst[fam]
        print(f"  {fam:9s} forward {f[0]:.4g} at {f[1]}   rstd {r[0]:.4g} at {r[1]}   backward {b[0]:.4g} at {b[1]}")
    fwd = max(worst[f][0][0] for f in PU.FAMILIES)
    bwd_all = max(worst[f][2][0] for f in PU.FAMILIES)
    bwd = max(worst[f][2][0] for f in PU.FAMILIES if f != "offset")
    print(f"forward, all families: {fwd:.4g}  ->  C_FWD = 4 x = {4 * fwd:.4g} (also the bound of rstd, relative)")
    print(f"backward, all families: {bwd_all:.4g} (4 x = {4 * bwd_all:.4g}): torch's backward forms dx = a dy + b x + c "
          "from the raw x, which cancels\n  catastrophically on the rows with a common offset of 1e4 -- a bound from "
          "it would check nothing")
    print(f"backward, the families without a common offset: {bwd:.4g}  ->  C_BWD = 4 x = {4 * bwd:.4g}, which the "
          "test applies to all four families")


if __name__ == "__main__":
    main()
