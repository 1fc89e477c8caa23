"""bench.py --gpus N starts its own ranks: the parent spawns the launcher before it has
imported torch, passes the ranks' JSON line on and leaves with their exit code."""
import json
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_parent_spawns_the_launcher_before_touching_the_gpu(monkeypatch, capsys):
    bench = _load_bench()
    seen = {}

    def fake_run(cmd, stdout=None, text=None):
        seen["cmd"] = cmd
        seen["torch_loaded_by_bench"] = "torch" in sys.modules and getattr(sys.modules["torch"], "_bench_marker", False)
        return types.SimpleNamespace(returncode=0, stdout='NCCL banner\n{"metric": "x", "value": 1.0, "n_gpus": 4}\n')

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert os.path.basename(cmd[cmd.index("--master-port") + 2]) == "bench.py"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and json.loads(out[0])["n_gpus"] == 4          # ONE line on stdout, the ranks' result


def test_parent_passes_a_failure_on(monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr(subprocess, "run", lambda cmd, stdout=None, text=None: types.SimpleNamespace(returncode=3, stdout=""))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 3


@pytest.mark.gpu
def test_bench_gpus_2_runs_by_itself_on_one_gpu():
    """Two ranks on the one GPU of the test box (gloo moves the tensors: RCCL refuses two ranks on one device): the
    launch, the strong-scaled frame, the re-cut bands, the JSON line."""
    env = dict(os.environ, LENTIL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--width", "960", "--height", "540", "--samples", "64", "--f-hi", "0.001", "--full", "--no-config5"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_joined"] == 2 and d["scaling"] == "strong"
    assert d["value"] > 0 and d["config"]["visits_per_gpu"] > 0
    assert "960x540 frame tiled over 2 GPU(s)" in d["config"]["workload"]
    assert isinstance(d["ranks"], list) and len(d["ranks"]) == 2


def test_dump_outputs_is_a_fixed_sample_below_64_mb(tmp_path):
    """--dump-outputs on a frame too large to write whole: the same seeded pixels every time, the values those pixels hold,
    fp32 images and fp64 indices, under 64 MB in all; a small frame is written whole."""
    import numpy as np
    bench = _load_bench()

    class Ctx:
        def __init__(self, n):
            self.n = n

        def sync(self):
            pass

        def download_aov(self, a):
            return np.arange(4 * self.n, dtype=np.float32).reshape(self.n, 4) + np.float32(a)

    def dump(W, H, aovs, out):
        b = types.SimpleNamespace(ctx=Ctx(W * H), p=types.SimpleNamespace(xres=W, yres=H), band=None, aovs=aovs, world=1, rank=0)
        bench.dump_outputs(b, str(out))
        return {f: np.load(os.path.join(str(out), f)) for f in sorted(os.listdir(str(out)))}

    for aovs in (0, 8):
        a, b = dump(3840, 2161, aovs, tmp_path / ("a%d" % aovs)), dump(3840, 2161, aovs, tmp_path / ("b%d" % aovs))
        assert sorted(a) == ["aov%d.npy" % k for k in range(1 + aovs)] + ["pixel_index.npy"]
        assert sum(os.path.getsize(str(tmp_path / ("a%d" % aovs) / f)) for f in a) <= 64 * 10 ** 6
        assert all(np.array_equal(a[f], b[f]) for f in a)
        idx = a["pixel_index.npy"]
        assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 3840 * 2161
        assert len(idx) < 3840 * 2161
        for k in range(1 + aovs):
            assert a["aov%d.npy" % k].dtype == np.float32
            assert np.array_equal(a["aov%d.npy" % k][:, 0], (4 * idx + k).astype(np.float32))
    small = dump(64, 49, 0, tmp_path / "small")
    assert np.array_equal(small["pixel_index.npy"], np.arange(64 * 49, dtype=np.float64))


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_one(tmp_path):
    """A plain run: one JSON line with the headline keys, exactly --steps timed passes, none of what --full adds; and
    --dump-outputs writes the last timed step's images -- the same, to fp32 summation order, from runs of a different
    length that end on the same visit stream."""
    import numpy as np
    dumps = []
    for steps in (3, 5):
        out = tmp_path / ("s%d" % steps)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--width", "320", "--height", "180", "--samples", "64", "--f-hi", "0.001", "--dump-outputs", str(out)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == steps and d["passes"]["timed"] == steps and d["value"] > 0 and d["ms_per_step"] > 0
        assert not any(k in d for k in ("configs", "regimes", "pcie_inclusive", "cpu_baseline", "parity_checked"))
        dumps.append({f: np.load(os.path.join(str(out), f)) for f in sorted(os.listdir(str(out)))})
    a, b = dumps
    assert sorted(a) == sorted(b) == ["aov0.npy", "pixel_index.npy"]
    img = a["aov0.npy"]
    assert img.dtype == np.float32 and img.shape == (len(a["pixel_index.npy"]), 4) and np.isfinite(img).all() and img.any()
    assert np.array_equal(a["pixel_index.npy"], b["pixel_index.npy"])
    assert np.abs(img - b["aov0.npy"]).max() <= 1e-5 * np.abs(img).max()
