"""ORACLE (test infrastructure, never imported by the product path).

Shared reading side of tests/golden/g15_loss_edges.npz (loss kernels on hyper-parameter and target edge cases): every case
of the file is a JSON `spec` (sizes, hyper-parameter overrides, head seeds) plus its target arrays verbatim; this module
turns a spec back into the hyper-parameter dict and the head tensors, for tools/gen_golden.py (which runs the reference on
them), tests/test_oracle_golden.py (oracle vs file) and the GPU edge tests (HIP vs file, HIP vs oracle)."""
import json
import os

import numpy as np

from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_head_outputs, synth_yolox_heads

G15 = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g15_loss_edges.npz")

V5_BASE = dict(num_class=80, use_focal_loss=True, focal_loss_gamma=1.5, focal_loss_alpha=0.25, iou_loss_scale=0.05,
               cls_loss_scale=0.5, cof_loss_scale=1.0, anchor_match_thr=4.0, class_smooth_factor=1.0, cls_pos_weight=1.0,
               cof_pos_weight=1.0)
X_BASE = dict(num_class=80, use_focal_loss=False, focal_loss_gamma=1.5, focal_loss_alpha=0.25, iou_loss_scale=5.0, use_l1=True,
              l1_loss_scale=1.0, cls_loss_scale=1.0, cof_loss_scale=1.0, class_smooth_factor=1.0, cls_pos_weight=1.0,
              cof_pos_weight=1.0, num_anchors=1, iou_type="ciou", topk=13, center_radius=3, num_stage=3)
# a fourth anchor row for stage_num = 4 (stride 64): the reference constructor takes any (S, 3, 2) tensor
ANCHORS4 = np.concatenate([COCO_ANCHORS, np.array([[[436, 615], [739, 380], [925, 792]]], np.float32)], 0)


def load():
    return np.load(G15, allow_pickle=False)


def spec_of(g, name):
    return json.loads(str(g[f"{name}_spec"]))


def hyp_of(spec, device):
    h = dict(V5_BASE if spec["kind"] == "v5" else X_BASE)
    h.update(spec["hyp"])
    h["device"] = device
    h["input_img_size"] = [spec["img"], spec["img"]]
    return h


def anchors_of(spec):
    return ANCHORS4 if spec.get("stages", 3) == 4 else COCO_ANCHORS


def heads_of(spec, seed):
    """v5: list of (B, 3*(5+nc), h, w); yolox: OrderedDict of (B, 1, 5+nc, h, w) — float32, reference layout"""
    nc = hyp_of(spec, "cpu")["num_class"]
    if spec["kind"] == "v5":
        strides = (8, 16, 32, 64)[:spec.get("stages", 3)]
        return synth_head_outputs(spec["B"], spec["img"], nc, 3, seed=seed, scale=spec["pscale"], strides=strides)
    return synth_yolox_heads(spec["B"], spec["img"], nc, seed=seed)


def grad_sample(flat, s):
    """indices pinned for a gradient too large to store whole: 128 drawn at random and its 64 largest entries"""
    rs = np.random.RandomState(1500 + s)
    return np.unique(np.concatenate([rs.randint(0, flat.size, 128), np.argsort(-np.abs(flat), kind="stable")[:64]])).astype(np.int32)


def nan_equal_close(got, ref, rtol, atol=0.0):
    """assert_allclose where NaN is allowed exactly where the reference has it"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    m = ~np.isnan(ref)
    np.testing.assert_allclose(got[m], ref[m], rtol=rtol, atol=atol)


def fallback_plan(targets_xyxy, img, strides=(8, 16, 32)):
    """{(stage, image): (nearest cell of every ground truth, choose_num)} for every image and stage on which no cell centre lies
    inside any box, i.e. where the reference's select_grid draws `choose_num` of those nearest cells at random"""
    import torch
    from .yoloxloss import YOLOXLossOracle
    probe = YOLOXLossOracle(dict(X_BASE))
    plan = {}
    for s, st in enumerate(strides):
        n = img // st
        ys, xs = torch.meshgrid(torch.arange(n), torch.arange(n), indexing='ij')
        grid = torch.stack((xs, ys), dim=2).float().reshape(-1, 2)
        for b, rows in enumerate(np.asarray(targets_xyxy, np.float32)):
            v = torch.from_numpy(rows[rows[:, 4] >= 0])
            if len(v) == 0:
                continue
            xywh = torch.cat([(v[:, :2] + v[:, 2:4]) / 2, v[:, 2:4] - v[:, :2]], 1)
            try:
                probe.select_grid(xywh, grid, float(st))
            except RuntimeError:
                near, choose = YOLOXLossOracle.nearest_cells(xywh, grid, float(st))
                plan[(s, b)] = (near.tolist(), choose)
    return plan
