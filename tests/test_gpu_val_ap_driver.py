"""--device-ap on the drivers: the validation pass whose AP and precision / recall curves come from the device (yh_val_ap through
MatchAccumulator.finish_ap and mAP_v2.from_curves) reports what the --device-metric pass reports on the same batches: the four
figures within 1e-12 (the AP sum is added left to right on the device and pairwise by np.sum; everything else is bit-equal), the
same n_pred and images.  tests/test_gpu_val_ap.py holds the kernel to its restatement; this is the wiring.

Two sets of batches.  The drivers' own (`main` at --img 128 --batch 4 --val-batches 2, the same weights for both flags).  And, since
random weights give a handful of distinct confidences (2 400 rows share four values, a true positive tied with hundreds of false
ones: the order among those comes from an unstable sort on the host and is outside the contract), the stub heads and the ground
truth of tests/test_gpu_val_metric.py put in place of the driver's loader and evaluator: some fifty detections per image with
pairwise distinct confidences, a third of them matched, the batch given twice (its repeated rows carry identical masks)."""
import os
import sys

import numpy as np
import pytest

from test_gpu_val_metric import JITTER_SEEDS, _id, ground_truth_from, host_metric_inputs, info_for, make_ev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = ("map", "map50", "precision", "recall")
ARGS = ["--img", "128", "--batch", "4", "--val-batches", "2"]


def assert_same_report(got, want, images):
    np.testing.assert_allclose([got[k] for k in FIGURES], [want[k] for k in FIGURES], rtol=1e-12, atol=1e-12)
    assert got["n_pred"] == want["n_pred"] and got["images"] == want["images"] == images


@pytest.mark.parametrize("driver", ["val_yolov5", "val_yolox"])
def test_validation_driver_reports_the_same_metric(dev, tmp_path, monkeypatch, driver):
    import torch
    from test_gpu_val_driver import _training
    from yoloseries_amd.trainer import MatchAccumulator
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    mod = __import__(driver)
    torch.manual_seed(5)                                              # the flags on the driver's own batches, the same weights
    m = mod.main(ARGS + ["--device-metric"])
    torch.manual_seed(5)
    a = mod.main(ARGS + ["--device-ap"])
    assert a.hyp["device_ap"] is True and a.hyp["device_metric"] is True and "device_ap" not in m.hyp
    assert_same_report(a.metrics, m.metrics, 8)

    cfg = ("320x320", driver == "val_yolox", False, False)           # detections that rank: stub heads, ground truth from them
    ev, _, x = make_ev(dev, cfg)
    info = info_for(cfg[0])
    ann = ground_truth_from(host_metric_inputs(ev(x), torch.zeros(len(x), 1, 5), info)[1], info, JITTER_SEEDS[_id(cfg)])
    v = _training(driver)
    v.hyp["num_class"] = ev.num_class
    v.val_dataloader = [dict(img=x, ann=ann, resize_info=info)] * 2
    v.build_evaluator = lambda model: ev
    v.hyp["device_metric"] = True
    want = dict(v.step())
    assert want["n_pred"] > 60 and 0 < want["map"] < want["map50"] < 1 and want["recall"] > 0
    called = []
    orig = MatchAccumulator.finish
    monkeypatch.setattr(MatchAccumulator, "finish", lambda self: called.append(1) or orig(self))
    v.hyp["device_ap"] = True
    assert_same_report(v.step(), want, 4)
    assert called == [], "the device-ap pass brought the match table to the host"
    del v.hyp["device_metric"]                                        # the key alone is enough
    assert_same_report(v.step(), want, 4)


def test_training_driver_evaluates_with_device_ap(dev, tmp_path, monkeypatch):
    """one epoch with the flag sets the keys and evaluates through finish_ap.  A net of two steps gives a few distinct confidences
    (see above), so across the two paths only what no tie can move is compared: the number of boxes."""
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    import train_yolov5
    from yoloseries_amd.trainer import MatchAccumulator
    calls = []
    orig = MatchAccumulator.finish_ap
    monkeypatch.setattr(MatchAccumulator, "finish_ap", lambda self: calls.append(1) or orig(self))
    t = train_yolov5.main(["--epochs", "1", "--img", "128", "--batch", "4", "--steps-per-epoch", "2", "--device-ap"])
    assert t.hyp["device_ap"] is True and t.hyp["device_metric"] is True and calls == [1]
    assert set(t.last_metrics) == {"map", "map50", "precision", "recall", "n_pred"}
    t.validate.conf_threshold = t.validate.cls_threshold = 0.            # detections from a net of two steps
    t.after_epoch(1)
    got = dict(t.last_metrics)
    assert calls == [1, 1] and got["n_pred"] > 100 and all(np.isfinite(list(got.values())))
    t.hyp["device_ap"] = False                                           # the same evaluation through the match table
    t.after_epoch(1)
    assert calls == [1, 1] and t.last_metrics["n_pred"] == got["n_pred"]
