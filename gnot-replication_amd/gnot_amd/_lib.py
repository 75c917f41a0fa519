"""ctypes binding of libgnot_hip.so (C ABI: include/gnot_hip.h).

This is the reference-side binding a maintainer adds to aloe101/GNOT-Replication (see
INTEGRATION.md): plain pointers and sizes, one `gnot_plan` per model.  There is deliberately no
fallback: if the shared library is missing or cannot be loaded, importing the product path fails.
"""
import ctypes
import hashlib
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)                      # gnot-replication_amd/
LIB_PATH = os.path.join(PKG_ROOT, "lib", "libgnot_hip.so")
CSRC = os.path.join(PKG_ROOT, "csrc")


class GnotConfig(ctypes.Structure):
    """gnot_config: the 12 GNOT constructor arguments (reference model.py:143)."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "input_dim", "theta_dim", "input_func_dim", "out_dim", "n_attn_layers", "n_attn_hidden_dim",
        "n_mlp_num_layers", "n_mlp_hidden_dim", "n_input_hidden_dim", "n_expert", "n_head",
        "n_input_functions")]


EXPORTS = [
    "gnot_plan_create", "gnot_plan_destroy", "gnot_plan_num_linears", "gnot_plan_linear_dims",
    "gnot_plan_bind_params", "gnot_plan_set_batch", "gnot_plan_workspace_bytes",
    "gnot_plan_bind_workspace", "gnot_plan_bind_workspace_async", "gnot_plan_set_moe_recompute", "gnot_plan_set_precision",
    "gnot_plan_set_input_grads", "gnot_input_grads", "gnot_plan_grad_offsets", "gnot_pack_weights", "gnot_forward",
    "gnot_backward", "gnot_profile_enable", "gnot_profile_read", "gnot_debug_buffer", "gnot_last_error",
    "gnot_version", "gnot_plan_set_shard", "gnot_plan_set_grad_comm", "gnot_shard_range", "gnot_shard_exchange",
    "gnot_rel_l2_work_floats", "gnot_rel_l2_loss", "gnot_adamw_step",
    "gnot_mse_work_floats", "gnot_mse_loss", "gnot_grad_clip_work_floats", "gnot_grad_clip", "gnot_adamw_step_clipped",
    "gnot_plan_set_grad_arena", "gnot_backward_ex", "gnot_grad_norm", "gnot_adamw_step_guarded",
    "gnot_ema_update", "gnot_adamw_step_ema", "gnot_gather_rows", "gnot_debug_gelu",
    "gnot_channel_stats_work_floats", "gnot_channel_stats", "gnot_gather_rows_affine", "gnot_rel_l2_loss_affine",
    "gnot_mse_loss_affine", "gnot_plan_set_fourier", "gnot_fourier_embed", "gnot_fourier_embed_bwd",
    "gnot_debug_kernel_forms", "gnot_plan_set_pre_norm", "gnot_layer_norm", "gnot_layer_norm_bwd",
    "gnot_lp_loss_work_floats", "gnot_lp_loss",
    "gnot_plan_set_dropout", "gnot_plan_set_dropout_active", "gnot_dropout_rows",
    "gnot_adamw_step_groups", "gnot_grad_norm_groups", "gnot_grad_clip_groups",
    "gnot_plan_set_trainable", "gnot_debug_backward_plan",
    "gnot_lp_loss_weighted_work_floats", "gnot_lp_loss_weighted",
    "gnot_channel_stats_weighted_work_floats", "gnot_channel_stats_weighted",
]
# (the header's int / void / size_t / const char* functions; gnot_plan_grad_floats returns int64_t and is
# declared in _declare like the rest)

# gnot_backward_ex flags (include/gnot_hip.h)
BWD_ACCUMULATE = 1
BWD_SKIP_GRAD_COMM = 2

# gnot_lp_loss kinds (include/gnot_hip.h GNOT_LP_*)
LP_KINDS = {"rel2": 0, "rel1": 1, "relinf": 2, "mse": 3, "l1": 4, "linf": 5}

# gnot_comm callbacks (include/gnot_hip.h)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)
ALLTOALLV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p)


class GnotComm(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("allreduce_sum", ALLREDUCE_FN), ("alltoallv", ALLTOALLV_FN)]


def build(jobs=8, quiet=True):
    """Compile the HIP sources for gfx950 into lib/libgnot_hip.so (hipcc cross-compiles, no GPU)."""
    cmd = ["make", "-C", CSRC, f"-j{jobs}"]
    res = subprocess.run(cmd, capture_output=quiet, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libgnot_hip.so failed:\n" + (res.stdout or "") + (res.stderr or ""))
    return LIB_PATH


# every file the library's code depends on (csrc/Makefile's SRCS, its headers and its flags)
SOURCES = ["Makefile", "gnot_common.h", "gnot_kernels.h", "x6_core.h", "pack.hip", "linear.hip", "linear2.hip",
           "chain.hip", "chain2.hip", "chainw.hip", "wgrad.hip", "state.hip", "attn.hip", "attn_mfma.hip", "misc.hip",
           "fourier.hip", "norm.hip", "dropout.hip", "train.hip", "gather.hip", "stats.hip", "engine.cpp", "tuning.cpp"]


def source_hash():
    """16 hex digits of sha256 over the library's sources (SOURCES + include/gnot_hip.h): the identity of
    the kernels a measurement was taken on.  profiles/pmc_traffic.json stores it per entry, and bench.py
    reports an entry's traffic only for the same hash (a changed kernel or launch sequence prints null).
    None when an experiment build is loaded instead (GNOT_LIB)."""
    if os.environ.get("GNOT_LIB"):
        return None
    h = hashlib.sha256()
    for f in [os.path.join(CSRC, n) for n in SOURCES] + [os.path.join(os.path.dirname(PKG_ROOT), "include", "gnot_hip.h")]:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _declare(lib):
    P = ctypes.c_void_p
    i32, i64, sz = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    lib.gnot_plan_create.argtypes = [ctypes.POINTER(GnotConfig), ctypes.POINTER(P)]
    lib.gnot_plan_destroy.argtypes = [P]
    lib.gnot_plan_destroy.restype = None
    lib.gnot_plan_num_linears.argtypes = [P]
    lib.gnot_plan_linear_dims.argtypes = [P, ctypes.POINTER(ctypes.c_int32)]
    lib.gnot_plan_bind_params.argtypes = [P, ctypes.POINTER(P), ctypes.POINTER(P)]
    lib.gnot_plan_set_batch.argtypes = [P, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), i32]
    lib.gnot_plan_workspace_bytes.argtypes = [P]
    lib.gnot_plan_workspace_bytes.restype = sz
    lib.gnot_plan_bind_workspace.argtypes = [P, P, sz]
    lib.gnot_plan_bind_workspace_async.argtypes = [P, P, sz, P]
    lib.gnot_plan_set_moe_recompute.argtypes = [P, ctypes.c_int]
    lib.gnot_plan_set_precision.argtypes = [P, ctypes.c_int]
    lib.gnot_plan_set_input_grads.argtypes = [P, ctypes.c_int]
    lib.gnot_input_grads.argtypes = [P, P, P, ctypes.POINTER(P), P]
    lib.gnot_plan_grad_offsets.argtypes = [P, ctypes.POINTER(i64)]
    lib.gnot_pack_weights.argtypes = [P, P]
    lib.gnot_forward.argtypes = [P, P, P, ctypes.POINTER(P), P, P]
    lib.gnot_backward.argtypes = [P, P, P]
    lib.gnot_backward_ex.argtypes = [P, P, i32, P]
    lib.gnot_plan_grad_floats.argtypes = [P]
    lib.gnot_plan_grad_floats.restype = i64
    lib.gnot_plan_set_grad_arena.argtypes = [P, P, i64]
    lib.gnot_profile_enable.argtypes = [P, ctypes.c_char_p]
    lib.gnot_profile_read.argtypes = [P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64),
                                      ctypes.POINTER(ctypes.c_double)]
    lib.gnot_debug_buffer.argtypes = [P, ctypes.c_char_p, ctypes.POINTER(P), ctypes.POINTER(i64)]
    lib.gnot_debug_kernel_forms.argtypes = [P, ctypes.c_char_p, sz]
    lib.gnot_plan_set_shard.argtypes = [P, i32, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(GnotComm)]
    lib.gnot_plan_set_grad_comm.argtypes = [P, ctypes.POINTER(GnotComm)]
    lib.gnot_shard_range.argtypes = [i64, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.gnot_shard_exchange.argtypes = [i32, ctypes.POINTER(i64), i32, i32, i32, i32, ctypes.POINTER(i64),
                                        ctypes.POINTER(i64), ctypes.POINTER(i64), i64, ctypes.POINTER(i64)]
    lib.gnot_rel_l2_work_floats.argtypes = [ctypes.POINTER(i64), i32, i32]
    lib.gnot_rel_l2_work_floats.restype = sz
    lib.gnot_rel_l2_loss.argtypes = [P, P, P, ctypes.POINTER(i64), i32, i32, P, P, P, P]
    lib.gnot_adamw_step.argtypes = [P, P, P, P, i64, P, P]
    lib.gnot_mse_work_floats.argtypes = [ctypes.POINTER(i64), i32, i32]
    lib.gnot_mse_work_floats.restype = sz
    lib.gnot_mse_loss.argtypes = [P, P, P, ctypes.POINTER(i64), i32, i32, P, P, P, P]
    lib.gnot_grad_clip_work_floats.argtypes = [i64]
    lib.gnot_grad_clip_work_floats.restype = sz
    lib.gnot_grad_clip.argtypes = [P, i64, P, ctypes.c_float, P, P, P]
    lib.gnot_adamw_step_clipped.argtypes = [P, P, P, P, i64, P, P, P]
    lib.gnot_grad_norm.argtypes = [P, i64, P, P, P, P]
    lib.gnot_adamw_step_guarded.argtypes = [P, P, P, P, i64, P, P, P, P]
    lib.gnot_ema_update.argtypes = [P, P, i64, P, P]
    lib.gnot_adamw_step_ema.argtypes = [P, P, P, P, P, i64, P, P, P, P]
    lib.gnot_gather_rows.argtypes = [P, i32, P, ctypes.POINTER(i64), i32, P, P]
    lib.gnot_debug_gelu.argtypes = [P, P, P, P, P, i64, P]
    lib.gnot_channel_stats_work_floats.argtypes = [i64, i32]
    lib.gnot_channel_stats_work_floats.restype = sz
    lib.gnot_channel_stats.argtypes = [P, i64, i32, ctypes.c_float, P, P, P]
    lib.gnot_gather_rows_affine.argtypes = [P, i32, P, ctypes.POINTER(i64), i32, P, P, P]
    lib.gnot_rel_l2_loss_affine.argtypes = [P, P, P, ctypes.POINTER(i64), i32, i32, P, P, P, P, P]
    lib.gnot_mse_loss_affine.argtypes = [P, P, P, ctypes.POINTER(i64), i32, i32, P, P, P, P, P]
    lib.gnot_plan_set_fourier.argtypes = [P, i32, i32]
    lib.gnot_fourier_embed.argtypes = [P, i64, i32, i32, P, i64, P]
    lib.gnot_fourier_embed_bwd.argtypes = [P, i64, P, i64, P, i64, i64, i32, i32, P, P]
    lib.gnot_plan_set_pre_norm.argtypes = [P, i32, ctypes.c_float]
    lib.gnot_layer_norm.argtypes = [P, i64, i64, i32, ctypes.c_float, P, i64, P, P]
    lib.gnot_layer_norm_bwd.argtypes = [P, i64, P, P, i64, i64, i32, P, i64, i32, P]
    lib.gnot_lp_loss_work_floats.argtypes = [ctypes.POINTER(i64), i32, i32]
    lib.gnot_lp_loss_work_floats.restype = sz
    lib.gnot_lp_loss.argtypes = [P, P, P, ctypes.POINTER(i64), i32, i32, i32, P, P, P, P, P, P, P]
    lib.gnot_plan_set_dropout.argtypes = [P, ctypes.c_float, P]
    lib.gnot_plan_set_dropout_active.argtypes = [P, i32]
    lib.gnot_dropout_rows.argtypes = [P, i64, i64, i32, P, P, i32, P, ctypes.c_uint32, ctypes.c_float, P]
    lib.gnot_adamw_step_groups.argtypes = [P, P, P, P, P, i64, P, P, i32, P, ctypes.POINTER(i64), i64, P, P, P]
    lib.gnot_grad_norm_groups.argtypes = [P, i64, P, P, ctypes.POINTER(i64), i64, P, P, P]
    lib.gnot_grad_clip_groups.argtypes = [P, i64, P, ctypes.c_float, P, ctypes.POINTER(i64), i64, P, P, P]
    lib.gnot_plan_set_trainable.argtypes = [P, P]
    lib.gnot_debug_backward_plan.argtypes = [P, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.gnot_lp_loss_weighted_work_floats.argtypes = [ctypes.POINTER(i64), i32, i32]
    lib.gnot_lp_loss_weighted_work_floats.restype = sz
    lib.gnot_lp_loss_weighted.argtypes = [P, P, P, P, ctypes.POINTER(i64), i32, i32, i32, P, P, P, P, P, P, P]
    lib.gnot_channel_stats_weighted_work_floats.argtypes = [i64, i32]
    lib.gnot_channel_stats_weighted_work_floats.restype = sz
    lib.gnot_channel_stats_weighted.argtypes = [P, P, i64, i32, ctypes.c_float, P, P, P]
    lib.gnot_last_error.restype = ctypes.c_char_p
    lib.gnot_last_error.argtypes = []
    lib.gnot_version.restype = ctypes.c_char_p
    lib.gnot_version.argtypes = []
    return lib


_LIB = None


def load():
    """Load libgnot_hip.so (raises if it is missing: there is no CPU fallback)."""
    global _LIB
    if _LIB is None:
        path = os.environ.get("GNOT_LIB", LIB_PATH)      # experiment builds of the same library
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: build it with `make -C {CSRC}` "
                              "(gnot_amd has no CPU fallback)")
        _LIB = _declare(ctypes.CDLL(path))
    return _LIB


def check(rc):
    if rc != 0:
        raise RuntimeError(f"libgnot_hip error {rc}: {load().gnot_last_error().decode()}")


def kernel_forms(plan):
    """gnot_debug_kernel_forms of a plan whose batch is set, as a dict of its key=value pairs (host only)."""
    text = ctypes.create_string_buffer(512)
    check(load().gnot_debug_kernel_forms(plan, text, len(text)))
    return dict(kv.split("=") for kv in text.value.decode().split())


def backward_plan(plan):
    """gnot_debug_backward_plan of a plan whose batch is set: (weight-gradient jobs over all groups, the lowest
    stage the backward enters: -1 encoders, l block l, L the decoder alone, L + 1 nothing).  Host only."""
    jobs, stage = ctypes.c_int(), ctypes.c_int()
    check(load().gnot_debug_backward_plan(plan, ctypes.byref(jobs), ctypes.byref(stage)))
    return jobs.value, stage.value


def probe_plan(cfg, nx=0, nf=0, dropout=None):
    """Create and destroy a plan for `cfg` (the gnot_config as a dict) with the Fourier orders nx / nf and, if
    given, the dropout probability (gnot_plan_set_dropout with a placeholder key that nothing reads): host
    only.  ValueError with the library's message if it refuses the configuration."""
    lib = load()
    c = GnotConfig(**cfg)
    plan = ctypes.c_void_p()
    rc = lib.gnot_plan_create(ctypes.byref(c), ctypes.byref(plan))
    if rc == 0:
        rc = lib.gnot_plan_set_fourier(plan, nx, nf)
        if rc == 0 and dropout is not None:
            key = (ctypes.c_uint32 * 4)()
            rc = lib.gnot_plan_set_dropout(plan, dropout, ctypes.addressof(key))
        msg = lib.gnot_last_error().decode() if rc != 0 else ""
        lib.gnot_plan_destroy(plan)
    else:
        msg = lib.gnot_last_error().decode()
    if rc != 0:
        raise ValueError(f"libgnot_hip refuses this model ({rc}): {msg}")
