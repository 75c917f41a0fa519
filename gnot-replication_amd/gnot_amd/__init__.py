"""gnot_amd — MI355X-native GNOT core (drop-in for aloe101/GNOT-Replication's model.py).

    from gnot_amd import GNOT
    model = GNOT(input_dim, theta_dim, input_func_dim, out_dim, n_attn_layers, n_attn_hidden_dim,
                 n_mlp_num_layers, n_mlp_hidden_dim, n_input_hidden_dim, n_expert, n_head,
                 n_input_functions).cuda()

The training step around it lives in `gnot_amd.train` (`RelL2Loss`, `MSELoss`, `LpLoss` -- the rel2 / rel1 / relinf /
mse / l1 / linf family with component weights -- `evaluate_table` for per-sample errors, `FlatAdamW` with optional
global-norm gradient clipping, `OneCycle`, `fit`), datasets, loaders and unit-Gaussian normalisation
(`Normalizer`, `DeviceDataset`, `DeviceLoader`) in `gnot_amd.data`, and the multi-GPU glue in
`gnot_amd.parallel`.  `GNOT(..., x_fourier=n, fn_fourier=n)` embeds x and the input functions in multi-scale
Fourier features inside the model (`gnot_amd.fourier`: `fourier_features` is the same map in plain torch,
`fourier_embed` the library's kernel).  `GNOT(..., pre_norm=True)` normalises the inputs of every attention call
with a parameter-free LayerNorm (`gnot_amd.norm` holds the two row kernels' wrappers).
`GNOT(..., attn_dropout=p, dropout_seed=s)` drops the attention outputs in training mode with a keyed mask that is
never stored (`gnot_amd.dropout` holds the threshold arithmetic and the row kernel's wrapper).
"""
from .model import GNOT, MLP, LinearAttention, HeterogeneousNormalizedAttentionBlock  # noqa: F401
from . import _lib  # noqa: F401
from .data import Normalizer  # noqa: F401
from .fourier import fourier_embed, fourier_features  # noqa: F401
from .train import LpLoss, evaluate_table  # noqa: F401

__all__ = ["GNOT", "MLP", "LinearAttention", "HeterogeneousNormalizedAttentionBlock", "Normalizer",
           "fourier_features", "fourier_embed", "LpLoss", "evaluate_table"]
