"""The validation metric on the device, end to end on stub heads: evaluate_matches -> MatchAccumulator -> mAP_v2.from_matches against
the host loop it replaces — __call__ + preds_postprocess + gt_bbox_postprocess (on CPU tensors) + mAP_v2(gts, preds) — which stays
the oracle.  Bars: ap, precision, recall and the four means exactly (assert_array_equal): both paths hold the same fp32 operations
in the same order, and the AP curves are the same NumPy code on the same tables.

Stub models as in tests/test_gpu_tta_fused.py (synth_nms_heads; with use_tta three sets of heads written into one set of device
tensors), the 96x160 / 3-class and 320x320 / 80-class shapes, B = 2, fp32 NCHW and bf16 cell-major heads, both evaluators, with and
without test-time augmentation.  The ground truth is made from the host path's own detections: every third box in the original
frame, moved by a seeded few pixels and mapped into the letterboxed frame with an `info` whose pads, sizes and scales all differ.
The jitter seeds were picked on the CPU with oracle/postproc.py (`oracle_dets`, `find_seeds`) so that the margin condition of
tests/test_val_match_host.py holds; the test asserts it again on what the GPU returned."""
import numpy as np
import pytest
import torch

from test_gpu_tta_fused import PASSES, SEEDS, SHAPES, _hyp, heads_for
from test_val_match_host import MARGIN, assert_margins, margins
from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_nms_heads

gpu = pytest.mark.gpu
THR = 0.3
CONFIGS = [(shape, yolox, bf16, tta) for shape in SHAPES for yolox in (False, True) for bf16 in (True, False) for tta in (False, True)]
# jitter seed per configuration (find_seeds)
JITTER_SEEDS = {'320x320-v5-bf16-plain': 1, '320x320-v5-bf16-tta': 0, '320x320-v5-f32-plain': 1, '320x320-v5-f32-tta': 0,
                '320x320-yolox-bf16-plain': 1, '320x320-yolox-bf16-tta': 1, '320x320-yolox-f32-plain': 1, '320x320-yolox-f32-tta': 1,
                '96x160-v5-bf16-plain': 0, '96x160-v5-bf16-tta': 0, '96x160-v5-f32-plain': 0, '96x160-v5-f32-tta': 0,
                '96x160-yolox-bf16-plain': 0, '96x160-yolox-bf16-tta': 3, '96x160-yolox-f32-plain': 0, '96x160-yolox-f32-tta': 3}


def stub_heads(shape, yolox, seed):
    """heads_for of tests/test_gpu_tta_fused.py; for YOLOX ten times as many live cells (its boxes are a cell or two wide, and the
    merge filter keeps a box only where a second candidate overlaps it: at 0.05 an image can end up without a detection)"""
    if not yolox:
        return heads_for(shape, yolox, seed)
    B, H, W, nc = SHAPES[shape]
    hs = synth_nms_heads(B, W, nc, 1, seed=seed, clusters=10, frac=0.5)
    return [np.ascontiguousarray(h[:, :, :H // s]) for h, s in zip(hs, (8, 16, 32))]


def _id(cfg):
    shape, yolox, bf16, tta = cfg
    return f"{shape}-{'yolox' if yolox else 'v5'}-{'bf16' if bf16 else 'f32'}-{'tta' if tta else 'plain'}"


def info_for(shape):
    """resize_info of the two images: pads, scales and original sizes all different; the content area is smaller than the network
    input, so detections near the border clamp"""
    _, H, W, _ = SHAPES[shape]
    out = []
    for scale, pad_top, pad_left in ((0.83, 6, 11), (1.25, 3, 8)):
        out.append(dict(scale=scale, pad_top=pad_top, pad_left=pad_left,
                        org_shape=(int((H - 2 * pad_top) / scale), int((W - 2 * pad_left) / scale))))
    return out


def ground_truth_from(preds, info, seed):
    """every third detection of the host path (original frame), jittered, back in the letterboxed frame: (B, maxbox, 5) float32, -1 padded"""
    rng = np.random.default_rng(seed)
    rows = []
    for p, r in zip(preds, info):
        if p is None or len(p) == 0:
            rows.append(np.zeros((0, 5), np.float32))
            continue
        g = p[::3, :4] + rng.uniform(-3, 3, (len(p[::3]), 4)).astype(np.float32)
        g = g * np.float32(r['scale']) + np.array([r['pad_left'], r['pad_top']] * 2, np.float32)
        rows.append(np.concatenate((g, p[::3, 5:6]), axis=1).astype(np.float32))
    ann = np.full((len(rows), max(1, max(len(r) for r in rows)) + 2, 5), -1, np.float32)
    for b, r in enumerate(rows):
        ann[b, 1:1 + len(r)] = r                                   # a padding row in front
    return torch.from_numpy(ann)


def host_metric_inputs(outs, ann, info):
    """the host loop of val_yolov5.Training.step on CPU tensors -> (all_gts, all_preds)"""
    from val_yolov5 import Training
    preds = Training.preds_postprocess(outs, info)
    gt_bbox, gt_cls = Training.gt_bbox_postprocess(ann, info)
    all_preds = [p if p is not None else np.zeros((0, 6), np.float32) for p in preds]
    all_gts = [np.concatenate((gt_bbox[j], gt_cls[j][:, None]), axis=1) for j in range(len(preds))]
    return all_gts, all_preds


# ---------------------------------------------------------------------------------------------------- CPU: the choice of seeds
def oracle_dets(cfg):
    """the evaluator's rows for the stub's heads by oracle/postproc.py (CPU; exp and sigmoid differ from the device's by ulps)"""
    from oracle import postproc
    shape, yolox, bf16, tta = cfg
    B, H, W, nc = SHAPES[shape]
    dec = []
    for (s, f), seed in list(zip(PASSES, SEEDS))[:3 if tta else 1]:
        heads = stub_heads(shape, yolox, seed)
        if bf16:
            heads = [torch.from_numpy(h).bfloat16().float().numpy() for h in heads]
        d = postproc.decode_yolox([h[:, None] for h in heads], H) if yolox else postproc.decode_v5(heads, COCO_ANCHORS, (8, 16, 32))
        d[..., :4] *= np.float32(1) / np.float32(s)
        if f == 2:
            d[..., 1] = np.float32(H) - d[..., 1]
        if f == 3:
            d[..., 0] = np.float32(W) - d[..., 0]
        dec.append(d)
    dec = np.concatenate(dec, axis=1)
    cands = [(postproc.candidates_yolox if yolox else postproc.candidates_v5)(dec[b], THR, THR) for b in range(B)]
    return [postproc.nms_image(c, 0.2, True, 300, True)[0] for c in cands]


def find_seeds():
    """the search that produced JITTER_SEEDS"""
    seeds = {}
    for cfg in CONFIGS:
        info = info_for(cfg[0])
        outs = [None if o is None else torch.from_numpy(o) for o in oracle_dets(cfg)]
        for seed in range(5000):
            ann = ground_truth_from(host_metric_inputs(outs, torch.zeros(len(outs), 1, 5), info)[1], info, seed)
            if min(margins(*host_metric_inputs(outs, ann, info))) >= 3 * MARGIN:       # room for the device's ulps
                seeds[_id(cfg)] = seed
                break
    return seeds


# ---------------------------------------------------------------------------------------------------- GPU
class StubModel:
    """heads of the stub's seeds, one set per call in turn (`period` 3 with use_tta: the three passes; 1 otherwise), written into
    ONE set of device tensors as the engine does with its head buffers"""

    def __init__(self, dev, shape, yolox, bf16, period):
        from yoloseries_amd.layout import to_cell_major
        self.sets = [[torch.from_numpy(h).to(dev) for h in stub_heads(shape, yolox, sd)] for sd in SEEDS[:period]]
        if bf16:
            self.out = [to_cell_major(torch.zeros_like(h, dtype=torch.bfloat16))[0] for h in self.sets[0]]
        else:
            self.out = [torch.zeros_like(h) for h in self.sets[0]]
        self.calls = 0

    def __call__(self, x):
        for o, h in zip(self.out, self.sets[self.calls % len(self.sets)]):
            o.copy_(h)
        self.calls += 1
        return self.out


def make_ev(dev, cfg):
    from yoloseries_amd.trainer import YOLOV5Evaluator, YOLOXEvaluator
    shape, yolox, bf16, tta = cfg
    B, H, W, nc = SHAPES[shape]
    stub = StubModel(dev, shape, yolox, bf16, 3 if tta else 1)
    hyp = _hyp(dev, nc, H, W, THR, use_tta=tta)
    ev = YOLOXEvaluator(stub, hyp) if yolox else YOLOV5Evaluator(stub, torch.from_numpy(COCO_ANCHORS), hyp)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    return ev, stub, x


@gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_device_metric_equals_host_loop(dev, cfg):
    from yoloseries_amd.trainer import MatchAccumulator
    from yoloseries_amd.utils.mAP import mAP_v2
    shape = cfg[0]
    nc = SHAPES[shape][3]
    info = info_for(shape)
    ev, stub, x = make_ev(dev, cfg)
    outs = ev(x)                                                    # the host path, before
    assert all(o is not None and len(o) >= 3 for o in outs), [None if o is None else len(o) for o in outs]
    ann = ground_truth_from(host_metric_inputs(outs, torch.zeros(len(outs), 1, 5), info)[1], info, JITTER_SEEDS[_id(cfg)])
    all_gts, all_preds = host_metric_inputs(outs, ann, info)
    assert_margins(all_gts, all_preds)
    want = mAP_v2(all_gts, all_preds)
    w = want.compute_ap_per_class()
    assert w["ap"][:, 0].max() > 0 and w["ap"].min() < 1, "a metric of all zeros or all ones compares nothing"

    acc = MatchAccumulator(nc, dev)
    for k in range(2):                                              # two batches: the same one twice
        m = ev.evaluate_matches(x, ann.to(dev), info if k == 0 else torch.from_numpy(
            np.array([[r['scale'], r['pad_top'], r['pad_left'], *r['org_shape']] for r in info], np.float32)), gt_hist=acc.gt_hist)
        acc.append(m)
    conf, cls, tp, hist = acc.finish()
    n = sum(len(p) for p in all_preds)
    assert len(conf) == 2 * n and tp.shape == (2 * n, 10) and hist.sum() == 2 * sum(len(g) for g in all_gts)
    got = mAP_v2.from_matches(conf[:n], cls[:n], tp[:n], hist // 2)
    g = got.compute_ap_per_class()
    for k in ("ap", "precision", "recall", "f1", "unique_cls"):
        np.testing.assert_array_equal(g[k], w[k], err_msg=k)
    np.testing.assert_array_equal(np.array(got.get_mean_metrics()), np.array(want.get_mean_metrics()))
    two = mAP_v2.from_matches(conf, cls, tp, hist).compute_ap_per_class()      # the doubled set, as the host loop sees it
    np.testing.assert_array_equal(two["ap"], mAP_v2(all_gts * 2, all_preds * 2).compute_ap_per_class()["ap"])
    # the match table itself: the detections in the original frame are the host transform's, bit for bit
    for b, p in enumerate(all_preds):
        assert int(m["nrow"][b]) == len(p)
        np.testing.assert_array_equal(m["box"][b, :len(p)].cpu().numpy(), p[:, :4])
        np.testing.assert_array_equal(m["conf"][b, :len(p)].cpu().numpy(), p[:, 4])

    again = ev(x)                                                   # the host path, after: no state left behind
    assert stub.calls == (3 if cfg[3] else 1) * 4
    for a, o in zip(again, outs):
        np.testing.assert_array_equal(a.numpy(), o.numpy())


@gpu
def test_multi_label_path_and_images_that_do_not_count(dev):
    """hyp['mutil_label'] goes through the decoded tensor on both paths; an image whose ground truth is all padding adds nothing"""
    from yoloseries_amd.trainer import MatchAccumulator, YOLOV5Evaluator
    from yoloseries_amd.utils.mAP import mAP_v2
    shape = "96x160"
    B, H, W, nc = SHAPES[shape]
    info = info_for(shape)
    stub = StubModel(dev, shape, False, True, 1)
    ev = YOLOV5Evaluator(stub, torch.from_numpy(COCO_ANCHORS), _hyp(dev, nc, H, W, THR, use_tta=False, mutil_label=True))
    x = torch.zeros(B, 3, H, W, device=dev)
    outs = ev(x)
    ann = ground_truth_from(host_metric_inputs(outs, torch.zeros(B, 1, 5), info)[1], info, 0)
    ann[1, :, 4] = -1                                               # image 1: padding only
    all_gts, all_preds = host_metric_inputs(outs, ann, info)
    acc = MatchAccumulator(nc, dev)
    m = ev.evaluate_matches(x, ann.to(dev), info, gt_hist=acc.gt_hist)
    acc.append(m)
    conf, cls, tp, hist = acc.finish()
    assert m["nrow"].tolist() == [len(all_preds[0]), 0] and len(conf) == len(all_preds[0]) and hist.sum() == len(all_gts[0])
    want = mAP_v2(all_gts, all_preds)
    np.testing.assert_array_equal(mAP_v2.from_matches(conf, cls, tp, hist).compute_ap_per_class()["ap"], want.compute_ap_per_class()["ap"])
    np.testing.assert_array_equal(np.concatenate([want.compute_tp(g, p) for g, p in zip(want.gt, want.pred)]), tp)
