"""The kernel forms a plan chooses (gnot_debug_kernel_forms after gnot_plan_set_batch; host only, no GPU): the
attention passes' rule (attn_kernel, csrc/attn_mfma.hip), the state groups' (finish_state_group,
csrc/engine.cpp), and that the GNOT_* switches behind them are read once, when the plan is created.

The attention rule: fp32 MFMA at head widths 16 / 32 / 64 without padded heads, from GNOT_APPLY_MFMA_MIN (512)
64-point chunks, while the state images fit 160 KiB of LDS:
    ((bwd ? 2 : 1) * nsrc * H * (dh / 16)^2 * 64 * 4 + nsrc * H * dh) * 4 bytes;
otherwise the VALU kernels, 'wide' above a head width of 64 and 'narrow' up to it.  The state groups: MFMA from
GNOT_STATE_MFMA_MIN (65,536) points where state_mfma_ok(d, dh) holds (gnot_kernels.h)."""
import ctypes

import pytest

from gnot_amd import _lib

ATTN = ("apply_fwd.self", "apply_fwd.cross", "apply_bwd.self", "apply_bwd.cross", "kv_bwd", "kv_bwd_batch")


class Plan:
    """One plan of hidden width d with H heads and I input functions; forms(n, m): its forms for one sample of n
    points and m points per input function."""

    def __init__(self, d, H, I=0):
        self.lib = _lib.load()
        self.I = I
        cfg = _lib.GnotConfig(input_dim=2, theta_dim=1, input_func_dim=3, out_dim=1, n_attn_layers=1,
                              n_attn_hidden_dim=d, n_mlp_num_layers=2, n_mlp_hidden_dim=d, n_input_hidden_dim=d,
                              n_expert=2, n_head=H, n_input_functions=I)
        self.plan = ctypes.c_void_p()
        _lib.check(self.lib.gnot_plan_create(ctypes.byref(cfg), ctypes.byref(self.plan)))

    def forms(self, n, m=64):
        xo = (ctypes.c_int64 * 2)(0, n)
        fo = (ctypes.c_int64 * (2 * self.I))(*([0, m] * self.I))
        _lib.check(self.lib.gnot_plan_set_batch(self.plan, 1, xo, fo if self.I else None, 1))
        return _lib.kernel_forms(self.plan)

    def workspace_bytes(self):
        return self.lib.gnot_plan_workspace_bytes(self.plan)

    def __del__(self):
        self.lib.gnot_plan_destroy(self.plan)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in ("GNOT_APPLY_MFMA_MIN", "GNOT_STATE_MFMA_MIN", "GNOT_WGRAD_OVERLAP", "GNOT_MOE_STORED_STREAMS"):
        monkeypatch.delenv(name, raising=False)


def query_passes(f):
    """the forms of the passes over the query points; without input functions there is no batched K/V backward"""
    assert f["kv_bwd_batch"] == "none"
    return {f[k] for k in ATTN if k != "kv_bwd_batch"}


def test_chunk_threshold(monkeypatch):
    p = Plan(256, 8)                                   # dh = 32
    assert query_passes(p.forms(511 * 64)) == {"narrow"}
    assert query_passes(p.forms(512 * 64)) == {"mfma"}
    assert query_passes(p.forms(511 * 64 + 1)) == {"mfma"}      # a last chunk of one point counts
    assert query_passes(p.forms(64)) == {"narrow"}
    monkeypatch.setenv("GNOT_APPLY_MFMA_MIN", "0")
    assert query_passes(Plan(256, 8).forms(64)) == {"mfma"}
    assert {Plan(256, 8, I=1).forms(64)[k] for k in ATTN} == {"mfma"}


def test_batched_kv_backward_counts_every_job():
    """its chunk count is the largest job's times the number of (block, input function) jobs"""
    p = Plan(256, 8, I=2)                              # one block: 2 jobs
    assert p.forms(64, m=255 * 64)["kv_bwd_batch"] == "narrow"   # 510 chunks
    assert p.forms(64, m=256 * 64)["kv_bwd_batch"] == "mfma"     # 512
    assert p.forms(64, m=256 * 64)["kv_bwd"] == "narrow"          # the query points' own pass: 1 chunk


def test_lds_cap_dh64():
    f = Plan(256, 4, I=2).forms(32768)                 # dh = 64, two sets of states
    assert f["apply_fwd.cross"] == "mfma"              # 130 KiB
    assert f["apply_bwd.cross"] == "narrow"            # 258 KiB
    assert f["apply_fwd.self"] == f["apply_bwd.self"] == "mfma"
    assert f["kv_bwd"] == "mfma"


def test_lds_cap_five_input_functions():
    assert Plan(256, 8, I=5).forms(32768)["apply_fwd.cross"] == "narrow"   # 160 KiB of images + 5 KiB
    assert Plan(256, 8, I=4).forms(32768)["apply_fwd.cross"] == "mfma"     # 132 KiB


@pytest.mark.parametrize("d,H,form", [(100, 4, "narrow"),    # heads of 25 padded to 28 (the d100_h4_padheads fixture)
                                       (60, 4, "narrow"),     # heads of 15 padded to 16: an MFMA width, but padded
                                       (256, 2, "wide"),      # dh = 128
                                       (144, 3, "narrow")])   # dh = 48
def test_other_head_widths(monkeypatch, d, H, form):
    monkeypatch.setenv("GNOT_APPLY_MFMA_MIN", "0")
    for I in (0, 2):
        f = Plan(d, H, I).forms(32768)
        assert {f[k] for k in ATTN if k.startswith("apply")} == {form}, f
        if d != 60:   # the K/V backward runs whole internal heads: padding does not concern it
            assert (f["kv_bwd"], f["kv_bwd_batch"]) == (form, form if I else "none"), f


def test_state_groups(monkeypatch):
    p = Plan(256, 8, I=1)
    f = p.forms(65535, m=65535)
    assert (f["state.query"], f["state.fn"]) == ("valu", "valu")
    f = p.forms(65536, m=64)
    assert (f["state.query"], f["state.fn"]) == ("mfma", "valu")
    f = p.forms(64, m=65536)
    assert (f["state.query"], f["state.fn"]) == ("valu", "mfma")
    assert Plan(256, 8).forms(65536)["state.fn"] == "none"
    assert Plan(192, 12).forms(65536)["state.query"] == "valu"     # 12 heads of 16: no MFMA form (3 per wave)
    monkeypatch.setenv("GNOT_STATE_MFMA_MIN", "0")
    f = Plan(256, 8, I=1).forms(64)
    assert (f["state.query"], f["state.fn"]) == ("mfma", "mfma")
    assert Plan(192, 12).forms(64)["state.query"] == "valu"
    assert Plan(144, 3).forms(64)["state.query"] == "valu"         # dh = 48


def test_stream_forms(monkeypatch):
    f = Plan(256, 8).forms(64)                         # below 65,536 points the weight gradients fork
    assert (f["serial_wgrad"], f["moe_direct_out"], f["moe_direct_dz"]) == ("0", "1", "0")
    f = Plan(256, 8).forms(65536)
    assert (f["serial_wgrad"], f["moe_direct_out"], f["moe_direct_dz"]) == ("1", "1", "1")
    assert Plan(128, 8).forms(64)["moe_direct_out"] == "0"
    monkeypatch.setenv("GNOT_WGRAD_OVERLAP", "0")
    f = Plan(256, 8).forms(64)
    assert (f["serial_wgrad"], f["moe_direct_dz"]) == ("1", "1")
    monkeypatch.setenv("GNOT_MOE_STORED_STREAMS", "1")
    f = Plan(256, 8).forms(64)
    assert (f["serial_wgrad"], f["moe_direct_out"], f["moe_direct_dz"]) == ("1", "0", "0")


def test_switches_read_once(monkeypatch):
    """A switch changed after gnot_plan_create does not reach that plan: same forms, same workspace."""
    p = Plan(256, 8, I=1)
    before = p.forms(4096, m=4096)
    size = p.workspace_bytes()
    assert {before[k] for k in ATTN} == {"narrow"} and before["state.query"] == before["state.fn"] == "valu"
    monkeypatch.setenv("GNOT_APPLY_MFMA_MIN", "0")
    monkeypatch.setenv("GNOT_STATE_MFMA_MIN", "0")
    monkeypatch.setenv("GNOT_WGRAD_OVERLAP", "0")
    monkeypatch.setenv("GNOT_MOE_STORED_STREAMS", "1")
    assert p.forms(4096, m=4096) == before
    assert p.workspace_bytes() == size
    after = Plan(256, 8, I=1).forms(4096, m=4096)
    assert {after[k] for k in ATTN} == {"mfma"} and after["state.query"] == after["state.fn"] == "mfma"
    assert (after["serial_wgrad"], after["moe_direct_out"]) == ("1", "0")


def test_query_needs_a_batch():
    p = Plan(64, 4)
    text = ctypes.create_string_buffer(512)
    assert p.lib.gnot_debug_kernel_forms(p.plan, text, len(text)) != 0       # no batch yet
    p.forms(64)
    assert p.lib.gnot_debug_kernel_forms(p.plan, text, 8) != 0               # buffer too small
    assert p.lib.gnot_debug_kernel_forms(p.plan, text, len(text)) == 0
