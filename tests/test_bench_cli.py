"""bench.py's rank handling (CPU only, no GPU call): `--gpus N` without a launcher spawns N rank
processes; a launcher's WORLD_SIZE must agree with --gpus; more ranks than visible GPUs is refused
unless every rank is told to share cuda:0 (GNOT_BENCH_ONE_GPU)."""
import argparse
import os
import sys
import textwrap

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _args(gpus):
    return argparse.Namespace(gpus=gpus)


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GNOT_BENCH_ONE_GPU", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_single_rank_default(clean_env):
    assert bench.resolve_world(_args(None)) == (1, 0, 0)
    assert bench.resolve_world(_args(1)) == (1, 0, 0)


def test_launcher_world_must_match_flag(clean_env):
    clean_env.setenv("WORLD_SIZE", "2")
    clean_env.setenv("RANK", "1")
    clean_env.setenv("LOCAL_RANK", "1")
    clean_env.setenv("GNOT_BENCH_ONE_GPU", "1")
    assert bench.resolve_world(_args(2)) == (2, 1, 1)
    assert bench.resolve_world(_args(None)) == (2, 1, 1)
    with pytest.raises(SystemExit, match="--gpus 4 but WORLD_SIZE=2"):
        bench.resolve_world(_args(4))


def test_more_ranks_than_gpus_refused(clean_env):
    # this container has no GPU: device_count() == 0
    with pytest.raises(SystemExit, match="GPU\\(s\\) visible"):
        bench.resolve_world(_args(2))
    clean_env.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="GPU\\(s\\) visible"):
        bench.resolve_world(_args(2))


def test_spawn_ranks_runs_n_children(clean_env, tmp_path):
    out = tmp_path / "ranks"
    out.mkdir()
    script = tmp_path / "rank.py"
    script.write_text(textwrap.dedent(f"""
        import os, sys
        r = os.environ["RANK"]
        open(os.path.join({str(out)!r}, r), "w").write(
            " ".join(os.environ[k] for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR")) + " " + " ".join(sys.argv[1:]))
    """))
    assert bench.spawn_ranks(3, str(script), ["--gpus", "3"]) == 0
    got = sorted(p.read_text() for p in out.iterdir())
    assert got == [f"{r} {r} 3 127.0.0.1 --gpus 3" for r in range(3)]


def test_dump_outputs_writes_float32_and_a_fixed_sample(tmp_path, monkeypatch):
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    small = torch.arange(12, dtype=torch.float64).view(3, 4)
    big = torch.arange(5000, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    a_small, a_big = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert a_small.dtype == np.float32 and a_big.dtype == np.float32
    assert a_small.tolist() == list(range(12))
    # the sample: 1000 distinct elements in index order, the same ones in every run
    assert a_big.shape == (1000,) and (np.diff(a_big) > 0).all() and a_big.max() < 5000
    assert (a_big == np.load(tmp_path / "b" / "big.npy")).all()


@pytest.mark.parametrize("flag", [["--breakdown"], ["--roofline-kernel", "wgrad"]])
def test_profile_options_need_full(clean_env, monkeypatch, capsys, flag):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + flag)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and "--full" in capsys.readouterr().err


def test_spawn_ranks_reports_failure(clean_env, tmp_path):
    script = tmp_path / "rank.py"
    script.write_text(textwrap.dedent("""
        import os, sys, time
        if os.environ["RANK"] == "1":
            sys.exit(3)
        time.sleep(60)          # the surviving rank is ended by PID once rank 1 fails
    """))
    assert bench.spawn_ranks(2, str(script), []) == 3
