"""Weighted box fusion on the host (yoloseries_amd/utils/weighted_fusion_bbox.py) against tests/golden/g21_wbf.npz, the result the
reference's utils.weighted_fusion_bbox recorded (tools/gen_golden_wbf.py: no equal scores within a class, every IoU at least 1e-9
from the threshold).  Bars: cluster count and sizes exact; boxes and scores 1e-12 relative — both sides are fp64 and differ only in
the order of their sums.  Also the evaluator's argument errors and the config keys of the fusion path."""
import os

import numpy as np
import pytest
import torch

from yoloseries_amd.utils import fuse_table, weighted_fusion_bbox
from yoloseries_amd.utils.synth import COCO_ANCHORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "g21_wbf.npz"))
IMAGES = range(4)


def golden(i):
    return GOLDEN[f"rows_{i}"], GOLDEN[f"fusion_{i}"], GOLDEN[f"sizes_{i}"], float(GOLDEN["iou_thr"])


def test_golden_is_what_the_tests_assume():
    for i in IMAGES:
        rows, fusion, sizes, thr = golden(i)
        assert rows.dtype == np.float32 and rows.shape[1] == 7 and 350 <= len(rows) <= 450
        assert fusion.shape == (len(sizes), 6) and sizes.sum() >= len(rows) and (sizes > 1).any()
        assert len(np.unique(rows[:, 5])) == 5 and set(np.unique(rows[:, 6])) == {0.5, 1.0, 2.0}


@pytest.mark.parametrize("i", IMAGES)
def test_fuse_table_equals_the_reference(i):
    rows, fusion, sizes, thr = golden(i)
    out, members = fuse_table(rows, thr)
    np.testing.assert_array_equal(members, sizes)
    np.testing.assert_array_equal(out[:, 5], fusion[:, 5])
    np.testing.assert_allclose(out[:, :5], fusion[:, :5], rtol=1e-12, atol=0)


@pytest.mark.parametrize("i", IMAGES)
def test_weighted_fusion_bbox_equals_the_reference(i):
    rows, fusion, sizes, thr = golden(i)
    cluster, fused = weighted_fusion_bbox(rows, thr)
    assert len(cluster) == len(fused) == 5
    np.testing.assert_array_equal([len(c) for per_class in cluster for c in per_class], sizes)
    flat = np.asarray([f for per_class in fused for f in per_class])
    np.testing.assert_array_equal(flat[:, 5], fusion[:, 5])
    np.testing.assert_allclose(flat[:, :5], fusion[:, :5], rtol=1e-12, atol=0)
    for per_class, lab in zip(cluster, np.unique(rows[:, 5])):         # members are whole rows of their class, in arrival order
        for c in per_class:
            m = np.asarray(c)
            assert m.shape[1] == 7 and (m[:, 5] == lab).all() and (np.diff(m[:, 4]) <= 0).all()


def test_weighted_box_is_the_reference_box_times_the_member_count():
    """'weighted' vs 'reference' on a table where the clusters are the same in both modes: single rows and exact duplicates (a
    duplicate pair's reference box is half the box, which the next, disjoint, object cannot meet either way)"""
    rng = np.random.RandomState(3)
    k = 40
    x, y = 200.0 * np.arange(k), rng.uniform(100, 200, k)
    box = np.stack((x + 50, y, x + 150, y + 80), axis=1)
    rows = np.concatenate((np.concatenate((box, rng.uniform(0.5, 1, (k, 1)), rng.randint(0, 3, (k, 1)), np.ones((k, 1))), axis=1),) * 2)
    rows[k:, 4] *= 0.5
    rows[k:, 6] = 2.0
    rows = rows[rng.permutation(2 * k)].astype(np.float32)
    ref, n_ref = fuse_table(rows, 0.5, 'reference')
    wtd, n_wtd = fuse_table(rows, 0.5, 'weighted')
    np.testing.assert_array_equal(n_ref, np.full(k, 2))
    np.testing.assert_array_equal(n_wtd, n_ref)
    np.testing.assert_allclose(wtd[:, :4], ref[:, :4] * n_ref[:, None], rtol=1e-15, atol=0)
    np.testing.assert_array_equal(wtd[:, 4:], ref[:, 4:])


def test_fuse_table_rules():
    """start empty, join EVERY cluster at or above the threshold (inclusive), stable order of equal scores, holes dropped"""
    a, b = [0, 0, 2, 2, 0.5, 0, 1], [0, 0, 2, 1, 0.25, 0, 1]                  # IoU exactly 0.5; the founder's fused box is exact
    out, n = fuse_table([a, b], 0.5)
    np.testing.assert_array_equal(n, [2])
    out, n = fuse_table([a, b], np.nextafter(0.5, 1))
    np.testing.assert_array_equal(n, [1, 1])
    two = [[0, 0, 10, 10, 0.9, 1, 1], [6, 0, 16, 10, 0.8, 1, 1], [3, 0, 13, 10, 0.7, 1, 1]]      # IoU 0.25 apart; 7/13 with the third
    out, n = fuse_table(two, 0.5, 'weighted')
    np.testing.assert_array_equal(n, [2, 2])
    tie = [[0, 0, 10, 10, 0.5, 0, 1], [100, 0, 110, 10, 0.5, 0, 1]]
    out, n = fuse_table(tie, 0.5)
    np.testing.assert_array_equal(out[:, 0], [0, 100])                          # table order
    out, n = fuse_table([a, [0, 0, 2, 2, 0.9, 0, 0], [0, 0, 2, 2, 0.0, 0, 1]], 0.5)
    np.testing.assert_array_equal(n, [1])
    out, n = fuse_table(np.zeros((0, 7)), 0.5)
    assert out.shape == (0, 6) and n.shape == (0,)
    with pytest.raises(ValueError, match="box_mean"):
        fuse_table([a], 0.5, 'mean')


def _hyp(**kw):
    hyp = dict(device="cpu", num_class=3, input_img_size=[96, 160], iou_threshold=0.2, conf_threshold=0.3, cls_threshold=0.3,
               max_predictions_per_img=300, iou_type="iou", mutil_label=False, agnostic=True, postprocess_bbox=True, wfb=True,
               use_tta=True, half=False, compute_metric_conf_threshold=0.001, compute_metric_iou_threshold=0.65,
               compute_metric_cls_threshold=0.001, num_anchors=1, num_stage=3, wfb_iou_threshold=0.5, wfb_skip_box_threshold=0.001)
    hyp.update(kw)
    return hyp


@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
def test_evaluator_rejects_bad_fusion_keys(yolox):
    from yoloseries_amd.trainer import YOLOV5Evaluator, YOLOXEvaluator

    def build(**kw):
        return YOLOXEvaluator(None, _hyp(**kw)) if yolox else YOLOV5Evaluator(None, torch.from_numpy(COCO_ANCHORS), _hyp(**kw))
    ev = build()
    assert ev.wfb and ev.wfb_weights == [1.0, 1.0, 1.0] and ev.wfb_box_mean == 'reference'
    assert build(wfb_weights=[1, 2, 0.5], wfb_box_mean='weighted').wfb_weights == [1.0, 2.0, 0.5]
    assert not build(use_tta=False).wfb                                 # wfb without use_tta is ignored, as in the reference
    for bad in ([1, 1], [], [1, 0, 1], [1, 1, -2.0], [1, float("nan"), 1]):
        with pytest.raises(ValueError, match="wfb_weights"):
            build(wfb_weights=bad)
    with pytest.raises(ValueError, match="wfb_box_mean"):
        build(wfb_box_mean='mean')
    with pytest.raises(ValueError, match="wfb_skip_box_threshold"):
        build(wfb_skip_box_threshold=-0.5)


@pytest.mark.parametrize("cfg", ["train_yolov5.yaml", "train_yolox.yaml"])
def test_config_carries_the_reference_values_of_the_fusion_keys(cfg):
    from config.config import Config
    hyp = Config().get_config(os.path.join(ROOT, "config", cfg))
    assert hyp['wfb'] is False and hyp['use_tta'] is True
    assert hyp['wfb_weights'] == [1, 1, 1] and hyp['wfb_iou_threshold'] == 0.5 and hyp['wfb_skip_box_threshold'] == 0.001
    assert 'wfb_box_mean' not in hyp                                    # the one key the reference does not have: 'reference' by default


def test_no_trace_of_the_unbuilt_branch():
    for name in ("eval_yolov5.py", "eval_yolox.py"):
        text = open(os.path.join(ROOT, "yoloseries_amd", "trainer", name)).read()
        assert "outside the HIP hot path" not in text
