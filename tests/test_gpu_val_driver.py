"""--device-metric on the drivers: the validation pass with the match table kept on the device reports what the host loop reports.
The same Training object runs its step twice on the same weights and the same seeded loader, flag off then on; the figures must be
equal exactly (tests/test_gpu_val_metric.py holds the two paths to each other on controlled detections; this is the wiring)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("map", "map50", "precision", "recall", "n_pred", "images")


def _training(driver):
    """the driver's Training on random weights, with the evaluator's thresholds at 0: random heads then give detections (the
    shipped 0.001 gives none), NMS keeps its 300 per image"""
    import torch
    from config.config import Config
    from yoloseries_amd.utils.synth import COCO_ANCHORS
    mod = __import__(driver)
    hyp = Config().get_config(os.path.join(ROOT, "config", "train_yolox.yaml" if driver == "val_yolox" else "train_yolov5.yaml"))
    hyp.update(input_img_size=[128, 128], batch_size=4, val_batches=2, compute_metric_conf_threshold=0., compute_metric_cls_threshold=0.)
    if driver == "val_yolox":          # its random boxes are a cell wide: none has the second overlapping candidate that the merge filter asks for
        hyp['postprocess_bbox'] = False
    torch.manual_seed(3)
    return mod.Training(hyp) if driver == "val_yolox" else mod.Training(torch.from_numpy(COCO_ANCHORS.copy()), hyp)


@pytest.mark.parametrize("driver", ["val_yolov5", "val_yolox"])
def test_validation_driver_reports_the_same_metric(dev, tmp_path, monkeypatch, driver):
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    v = _training(driver)
    host = dict(v.step())
    assert host["images"] == 8 and host["n_pred"] > 100
    called = []
    orig = type(v).preds_postprocess
    monkeypatch.setattr(type(v), "preds_postprocess", staticmethod(lambda *a: called.append(1) or orig(*a)))
    v.hyp["device_metric"] = True
    got = v.step()
    assert called == [], "the device path went through the host transforms"
    assert [got[k] for k in KEYS] == [host[k] for k in KEYS], (got, host)
    v2 = __import__(driver).main(["--img", "128", "--batch", "4", "--val-batches", "2", "--device-metric"])
    assert v2.hyp["device_metric"] is True and v2.metrics["images"] == 8
    assert all(np.isfinite([v2.metrics[k] for k in KEYS]))


def test_training_driver_evaluates_on_the_device(dev, tmp_path, monkeypatch):
    """after_epoch with the flag: the metric comes from the match table (no row crosses to the host per image), in both data modes"""
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    import train_yolov5
    calls = []
    for data in ("tensor", "dataset"):
        t = train_yolov5.main(["--epochs", "1", "--img", "128", "--batch", "4", "--steps-per-epoch", "2", "--data", data, "--device-metric"])
        assert t.hyp["device_metric"] is True
        assert set(t.last_metrics) == {"map", "map50", "precision", "recall", "n_pred"}
        t.validate.conf_threshold = t.validate.cls_threshold = 0.        # detections from a net of two steps
        monkeypatch.setattr(type(t.validate), "__call__", lambda self, x: calls.append(1))
        t.after_epoch(1)
        assert calls == [] and t.last_metrics["n_pred"] > 100 and all(np.isfinite(list(t.last_metrics.values())))
