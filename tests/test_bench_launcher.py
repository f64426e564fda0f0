"""CPU: `python bench.py --gpus N` must itself start N ranks when no torch.distributed environment is present (round-1 defect:
--gpus was parsed and ignored), with the driver's own torchrun launch left untouched; plus the pure helpers of the bench line."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    return importlib.import_module("bench")


def test_gpus_n_relaunches_under_torchrun(bench, monkeypatch):
    calls = {}

    def fake_call(cmd, env=None):
        calls["cmd"], calls["env"] = cmd, env
        return 7

    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "20", "--warmup", "5"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                                              # the launcher's return code is ours
    cmd = calls["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "20", "--warmup", "5"]  # every rank sees the same flags
    assert calls["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_config4_queue_launch_reaches_device_selection(bench, monkeypatch):
    """config 4 (`bench.py --gpus 8 --total-prompts 15`): the launcher fans out eight ranks with the queue flags intact, and a rank (WORLD_SIZE
    set, as under the driver's torchrun) gets as far as device selection on this GPU-less box -- it must fail THERE, not in the argument
    plumbing or by fanning out again (dataset_tools/multi_gpu_infer_with_prompt.py:146-172)."""
    calls = {}
    monkeypatch.setattr(bench.subprocess, "call", lambda cmd, env=None: calls.update(cmd=cmd, env=env) or 0)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--total-prompts", "15"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and "--nproc-per-node=8" in calls["cmd"]
    i = calls["cmd"].index(os.path.join(ROOT, "bench.py"))
    assert calls["cmd"][i + 1:] == ["--gpus", "8", "--total-prompts", "15"]
    a = bench.parse(["--gpus", "8", "--total-prompts", "15"])
    assert a.gpus == 8 and a.total_prompts == 15 and a.prompts_per_gpu == 1
    import torch
    if torch.cuda.is_available():
        return
    monkeypatch.setattr(bench.subprocess, "call", lambda *a, **k: pytest.fail("a rank must not relaunch"))
    for k, v in dict(WORLD_SIZE="8", RANK="3", LOCAL_RANK="3", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533").items():
        monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "LOCAL_RANK 3" in str(e.value.code) and "GPU(s) visible" in str(e.value.code)          # device selection, nothing earlier


def test_no_relaunch_inside_a_torchrun_rank(bench, monkeypatch):
    """under the driver's `python -m torch.distributed.run ... bench.py --gpus N` WORLD_SIZE is set: no second fan-out"""
    monkeypatch.setattr(bench.subprocess, "call", lambda *a, **k: pytest.fail("must not relaunch"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "5")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    with pytest.raises((SystemExit, RuntimeError, AssertionError)):     # no GPU here: it must fail at device selection, not fan out again
        bench.main()


def test_per_kv_table_uses_window_iterations_near_each_point(bench):
    log, t = [], 0.0
    for i in range(400):
        kv = 60 + 6 * i
        t += 0.004 + 1e-6 * kv
        log.append((kv, 16, 2, t))
    tab = bench.per_kv_table(log, [64, 1216, 2368])
    assert set(tab) == {"64", "1216", "2368"}
    assert tab["64"]["ms_per_step"] < tab["1216"]["ms_per_step"] < tab["2368"]["ms_per_step"]
    assert abs(tab["1216"]["ms_per_step"] - (4.0 + 1.216)) < 0.1


def test_plain_run_is_lean_and_full_is_opt_in(bench):
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "out_dir"])
    assert a.full is True and a.dump_outputs == "out_dir"


def test_dump_outputs_writes_float64_npy(bench, tmp_path):
    np = pytest.importorskip("numpy")
    bench.dump_outputs(str(tmp_path / "d"), {"tokens": [1, 8197, 65535], "last_step_accepted": [3]})
    t = np.load(tmp_path / "d" / "tokens.npy")
    assert t.dtype == np.float64 and t.tolist() == [1.0, 8197.0, 65535.0]
    assert np.load(tmp_path / "d" / "last_step_accepted.npy").tolist() == [3.0]
    bench.dump_outputs(str(tmp_path / "d"), {"tokens": [5]}, rank=1, world=2)
    assert np.load(tmp_path / "d" / "tokens_rank1.npy").tolist() == [5.0]
