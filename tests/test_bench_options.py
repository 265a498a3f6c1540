"""bench.py's options and its output dump, without a GPU: a plain run leaves the extra measurements to --full, --steps is
validated before anything starts, and --dump-outputs writes float32 / float64 arrays within its budget, sampling the same
elements from run to run."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr and not r.stdout.strip()


def test_step_outputs_and_budget(tmp_path):
    import bench
    from yoloseries_amd import models
    torch.manual_seed(0)
    m = models.YOLOV5Small(3, 80)

    class _Ema:
        ema = m
    arrays = bench.step_outputs({"tot_loss": torch.tensor(2.5), "tar_nums": torch.tensor(17.0)}, m, _Ema())
    assert sorted(arrays) == ["ema_state", "loss_tar_nums", "loss_tot_loss", "model_state"]
    n = sum(v.numel() for v in m.state_dict().values() if v.is_floating_point())
    assert arrays["model_state"].numel() == n
    # whole when it fits
    bench.write_outputs(str(tmp_path / "a"), arrays)
    st = np.load(tmp_path / "a" / "model_state.npy")
    assert st.dtype == np.float32 and st.size == n
    assert np.load(tmp_path / "a" / "loss_tot_loss.npy").dtype == np.float64
    np.testing.assert_array_equal(st, arrays["model_state"].numpy())
    # a budget below the total: small arrays whole, large ones a fixed sample of their share
    budget = 8 << 20
    for d in ("b", "c"):
        bench.write_outputs(str(tmp_path / d), arrays, budget=budget)
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["ema_state.npy", "loss_tar_nums.npy", "loss_tot_loss.npy", "model_state.npy"]
    data = sum(np.load(tmp_path / "b" / f).nbytes for f in files)
    assert data <= budget and sum(os.path.getsize(tmp_path / "b" / f) for f in files) < budget + 4096
    assert np.load(tmp_path / "b" / "loss_tar_nums.npy")[0] == 17.0
    s1, s2 = np.load(tmp_path / "b" / "model_state.npy"), np.load(tmp_path / "c" / "model_state.npy")
    np.testing.assert_array_equal(s1, s2)                                     # the same elements every run
    assert s1.size < n and np.isin(s1, arrays["model_state"].numpy()).all()


def test_detections_dump(tmp_path):
    import bench
    dets = [None, torch.tensor([[1, 2, 3, 4, 0.9, 5], [2, 3, 4, 5, 0.5, 7]], dtype=torch.float32), None]
    arrays = bench.step_outputs({"tot_loss": torch.zeros(()), "dets": dets})
    assert sorted(arrays) == ["detections", "detections_per_image"]
    bench.write_outputs(str(tmp_path), arrays)
    d = np.load(tmp_path / "detections.npy")
    assert d.dtype == np.float32 and d.shape == (2, 7) and (d[:, 0] == 1).all()
    np.testing.assert_array_equal(np.load(tmp_path / "detections_per_image.npy"), [0, 2, 0])
