"""train_yolov5.py --loss yolov7: the YOLOv5 driver trains YOLOv5s with YOLOV7Loss (same heads, same step, same log line);
without the switch the driver builds YOLOV5Loss as before."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_train_yolov5_with_the_yolov7_loss(dev, capsys, tmp_path, monkeypatch):
    import train_yolov5
    from yoloseries_amd.loss import YOLOV7Loss
    monkeypatch.chdir(tmp_path)
    t = train_yolov5.main(["--loss", "yolov7", "--epochs", "1", "--img", "128", "--batch", "4", "--steps-per-epoch", "3"])
    assert isinstance(t.loss_fcn, YOLOV7Loss) and (t.hyp["topk"], t.hyp["use_iou_as_tar_cof"]) == (15, True)
    losses = [h["tot_loss"] for h in t.history]
    print(t.history)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert all(np.isfinite([h["iou_loss"], h["cof_loss"], h["cls_loss"]]).all() and h["tar_nums"] > 0 for h in t.history)
    out = capsys.readouterr().out
    assert "epoch 1/1 step 1/3 tot " in out and " box " in out and " cof " in out and " cls " in out and " tars " in out


def test_default_driver_still_builds_the_yolov5_loss(dev):
    import train_yolov5
    from yoloseries_amd.loss import YOLOV5Loss, YOLOV7Loss
    from yoloseries_amd.utils.synth import COCO_ANCHORS
    hyp = dict(device=str(dev), input_img_size=[128, 128], num_class=3)
    me = types.SimpleNamespace(hyp=hyp, anchors=torch.from_numpy(COCO_ANCHORS.copy()), device=dev)
    assert type(train_yolov5.Training.build_loss(me)) is YOLOV5Loss
    me.hyp = dict(hyp, loss="yolov7", topk=15, use_iou_as_tar_cof=True)
    assert type(train_yolov5.Training.build_loss(me)) is YOLOV7Loss
    with pytest.raises(SystemExit):
        train_yolov5.main(["--loss", "yolov8"])
