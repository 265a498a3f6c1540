"""hyp['wfb'] on the evaluators: with use_tta the three passes are merged by weighted box fusion on the device.

The stub models of tests/test_gpu_tta_fused.py (three calls, three sets of heads written into one set of tensors) feed the
evaluator; the oracle is fuse_table (fp64, host) of rows built here from ev.test_time_augmentation(x)[1], the decoded tensors of
the passes, by the candidate rule of the reference's do_wfb: obj > t, cls *= obj, xywh -> xyxy, then the arg-max class if > t, or —
mutil_label — one row per (prediction, class) with cls * obj > t; both comparisons STRICT, in fp32; passes stacked, each row with its
pass's weight.  Bars: those of tests/test_gpu_wbf.py (counts and classes equal, boxes and scores within one float32 ulp)."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_tta_fused import SHAPES, make_ev
from test_gpu_val_metric import info_for
from yoloseries_amd.utils import fuse_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
WEIGHTS = [1.0, 2.0, 0.5]
SKIP = {"96x160": 0.001, "320x320": 0.3}


def wfb_ev(dev, shape, yolox, bf16, **kw):
    hyp = dict(wfb=True, wfb_weights=WEIGHTS, wfb_iou_threshold=0.5, wfb_skip_box_threshold=SKIP[shape])
    hyp.update(kw)
    return make_ev(dev, shape, yolox, bf16, **hyp)


def host_rows(passes, thr, weights, multi):
    """decoded tensors of the passes [(B, X, 5 + nc), ...] -> per image (n, 7) float32 rows by do_wfb's rule"""
    t = np.float32(thr)
    B = passes[0].shape[0]
    images = []
    for b in range(B):
        rows = [np.zeros((0, 7), np.float32)]
        for p, w in zip(passes, weights):
            x = p[b].detach().cpu().numpy().astype(np.float32)
            x = x[x[:, 4] > t]
            sc = x[:, 5:] * x[:, 4:5]
            half_w, half_h = x[:, 2] / np.float32(2), x[:, 3] / np.float32(2)
            box = np.stack((x[:, 0] - half_w, x[:, 1] - half_h, x[:, 0] + half_w, x[:, 1] + half_h), axis=1)
            if multi:
                r, c = np.nonzero(sc > t)
                out = np.concatenate((box[r], sc[r, c][:, None], c[:, None].astype(np.float32)), axis=1)
            else:
                c = sc.argmax(axis=1) if len(sc) else np.zeros(0, np.int64)
                best = sc[np.arange(len(sc)), c]
                out = np.concatenate((box, best[:, None], c[:, None].astype(np.float32)), axis=1)[best > t]
            rows.append(np.concatenate((out, np.full((len(out), 1), w, np.float32)), axis=1).astype(np.float32))
        images.append(np.concatenate(rows))
    return images


def assert_rows(got, rows7, thr, box_mean='reference'):
    """one image: the evaluator's (n, 6) tensor or None against fuse_table of the host rows"""
    ref, _ = fuse_table(rows7, thr, box_mean)
    if len(ref) == 0:
        assert got is None
        return 0
    assert got is not None and got.dtype == torch.float32 and got.device.type == "cpu" and tuple(got.shape) == (len(ref), 6)
    g = got.numpy()
    np.testing.assert_array_equal(g[:, 5], ref[:, 5].astype(np.float32))
    np.testing.assert_array_max_ulp(g[:, :5], ref[:, :5].astype(np.float32), maxulp=1)
    return len(ref)


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16_cell_major", "f32_nchw"])
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_call_with_wfb_equals_fusion_of_the_host_candidates(dev, shape, yolox, bf16):
    ev, stub, x = wfb_ev(dev, shape, yolox, bf16)
    images = host_rows(ev.test_time_augmentation(x)[1], SKIP[shape], WEIGHTS, False)
    assert all(len(r) >= 3 for r in images) and all(len(set(r[:, 6])) == 3 for r in images), [len(r) for r in images]
    ev, stub, x = wfb_ev(dev, shape, yolox, bf16)
    res = ev(x)
    assert stub.calls == 3 and len(res) == len(images)
    assert ev.last_ncand == [len(r) for r in images]
    assert sum(assert_rows(o, r, 0.5) for o, r in zip(res, images)) > 0


@gpu
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
def test_weighted_box_mean_and_multi_label(dev, yolox):
    shape = "96x160"
    for kw, multi, mean in ((dict(wfb_box_mean='weighted'), False, 'weighted'), (dict(mutil_label=True), True, 'reference'),
                            (dict(mutil_label=True, wfb_box_mean='weighted'), True, 'weighted')):
        ev, stub, x = wfb_ev(dev, shape, yolox, True, **kw)
        images = host_rows(ev.test_time_augmentation(x)[1], SKIP[shape], WEIGHTS, multi)
        ev, stub, x = wfb_ev(dev, shape, yolox, True, **kw)
        res = ev(x)
        assert ev.last_ncand == [len(r) for r in images]
        n = sum(assert_rows(o, r, 0.5, mean) for o, r in zip(res, images))
        assert n > 0
        if mean == 'weighted' and not yolox:       # clusters grow past the two of the reference mean (the YOLOX stub's boxes are a cell wide)
            assert max(fuse_table(r, 0.5, mean)[1].max() for r in images) > 2


@gpu
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi_label"])
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
def test_do_wfb_is_strict_at_the_threshold(dev, yolox, multi):
    """decoded tensors where an obj and a cls * obj equal the threshold EXACTLY: do_wfb drops them (the NMS filter's >= keeps them);
    the nesting is the reference's: per image None or a list per class of fused rows"""
    t = np.float32(0.25)
    nc = 3
    ev, stub, x = wfb_ev(dev, "96x160", yolox, True, wfb_skip_box_threshold=float(t), mutil_label=multi)

    def pred(cx, cy, w, h, obj, *cls):
        return [cx, cy, w, h, obj, *cls]
    a = [pred(50, 50, 20, 20, 0.25, 2, 2, 2),                   # obj == t: dropped, whatever its classes say
         pred(50, 50, 20, 20, 0.5, 0.5, 0.25, 0.125),           # cls * obj == t exactly for class 0: dropped
         pred(50, 50, 20, 20, 0.5, 0.25, 1.0, 0.75),            # classes 1 (0.5) and 2 (0.375) pass; single label keeps class 1
         pred(90, 50, 20, 20, float(np.nextafter(t, np.float32(1))), 1, 0, 0)]      # just above: kept, class 0
    b = [pred(51, 50, 20, 20, 0.5, 0, 0.75, 0), pred(0, 0, 1, 1, 0.25, 1, 1, 1), pred(0, 0, 1, 1, 1.0, 0.25, 0.25, 0.25),
         pred(0, 0, 1, 1, 0.2, 1, 1, 1)]
    passes = [torch.tensor([a, [pred(0, 0, 1, 1, 0.25, 1, 1, 1)] * 4], dtype=torch.float32, device=dev),
              torch.tensor([b, [pred(0, 0, 1, 1, 0.1, 1, 1, 1)] * 4], dtype=torch.float32, device=dev)]
    assert passes[0].shape == (2, 4, 5 + nc)
    images = host_rows(passes, t, WEIGHTS, multi)
    assert [len(r) for r in images] == [4 if multi else 3, 0]
    nested = ev.do_wfb(passes)
    assert nested[1] is None and len(nested) == 2
    ref, _ = fuse_table(images[0], 0.5)
    assert [len(per_class) for per_class in nested[0]] == [int((ref[:, 5] == c).sum()) for c in np.unique(ref[:, 5])]
    flat = np.asarray([r for per_class in nested[0] for r in per_class])
    np.testing.assert_array_equal(flat[:, 5], ref[:, 5].astype(np.float32))
    np.testing.assert_array_max_ulp(flat[:, :5], ref[:, :5].astype(np.float32), maxulp=1)
    # today's inclusive obj filter on the same tensors keeps the first row (multi label: the second's class 0 too)
    ev.conf_threshold = ev.cls_threshold = float(t)
    _cand, ncand, _B, _cap = ev._filter_decoded(passes[0], mode=ev._WFB_FILTER_MODES[1 if multi else 0])
    assert int(ncand[0]) > len(host_rows(passes[:1], t, WEIGHTS, multi)[0])


@gpu
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
def test_evaluate_matches_returns_the_fusion_rows_unletterboxed(dev, yolox):
    sys.path.insert(0, ROOT)
    from val_yolov5 import Training
    shape = "96x160"
    info = info_for(shape)
    ev, stub, x = wfb_ev(dev, shape, yolox, True)
    outs = ev(x)
    assert all(o is not None and len(o) >= 3 for o in outs)
    want = Training.preds_postprocess(outs, info)
    ann = torch.tensor([[[10, 10, 40, 40, 0]], [[20, 20, 60, 50, 1]]], dtype=torch.float32)
    ev, stub, x = wfb_ev(dev, shape, yolox, True)
    m = ev.evaluate_matches(x, ann, info)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(m['nrow'].cpu().numpy(), [len(o) for o in outs])
    for b, w in enumerate(want):
        n = len(w)
        np.testing.assert_array_equal(m['box'][b, :n].cpu().numpy(), w[:, :4])
        np.testing.assert_array_equal(m['conf'][b, :n].cpu().numpy(), w[:, 4])
        np.testing.assert_array_equal(m['cls'][b, :n].cpu().numpy(), w[:, 5].astype(np.int32))


@gpu
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
def test_without_wfb_nothing_changes(dev, yolox):
    """wfb False, and wfb True without use_tta (ignored, as in the reference): the rows of an evaluator built without any fusion key"""
    for tta in (True, False):
        ev, stub, x = make_ev(dev, "96x160", yolox, True, use_tta=tta)
        ev.hyp.pop('wfb')
        plain = type(ev)(stub, ev.hyp) if yolox else type(ev)(stub, ev.anchors, ev.hyp)
        want = plain(x)
        assert any(w is not None and len(w) for w in want)
        for kw in ((dict(wfb=False, wfb_weights=WEIGHTS, wfb_iou_threshold=0.5, wfb_skip_box_threshold=0.001),) +
                   (() if tta else (dict(wfb=True, wfb_iou_threshold=0.5, wfb_skip_box_threshold=0.001),))):
            ev, stub, x = make_ev(dev, "96x160", yolox, True, use_tta=tta, **kw)
            got = ev(x)
            assert not ev.wfb and len(got) == len(want)
            for g, w in zip(got, want):
                assert (g is None) == (w is None)
                if w is not None:
                    assert torch.equal(g, w)


@gpu
@pytest.mark.parametrize("driver", ["val_yolov5", "val_yolox"])
def test_driver_runs_with_wfb(dev, tmp_path, monkeypatch, driver):
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    v = __import__(driver).main(["--wfb", "--img", "128", "--batch", "4", "--val-batches", "1"])
    assert v.hyp["wfb"] is True and v.hyp["use_tta"] is True and v.metrics["images"] == 4
    assert all(np.isfinite([v.metrics[k] for k in ("map", "map50", "precision", "recall", "n_pred")]))
    v = __import__(driver).main(["--wfb", "--wfb-box-mean", "weighted", "--device-ap", "--img", "128", "--batch", "4", "--val-batches", "1"])
    assert v.hyp["wfb_box_mean"] == "weighted" and v.hyp["device_metric"] is True and v.metrics["images"] == 4
    assert all(np.isfinite([v.metrics[k] for k in ("map", "map50", "precision", "recall", "n_pred")]))
