"""Inputs of the YOLOv8 post-processing tests (tests/test_v8post_host.py, tests/test_gpu_v8post.py, tests/test_gpu_v8post_edges.py)
and of the fixture generator tools/gen_golden_v8post.py, which stores only the seed of a case.  NumPy only.

Heads are yoloseries_amd.utils.synth.synth_v8_heads(seed) ~ N(0, 1) with `bias` added to every class logit, so that a few per
cent to about half of the cells pass the class threshold.  A stub model returns the heads of seed + call index on its call-th
call (a TTA run sees three different heads).

Square cases, compared with the reference (SQUARE):
  a    64^2, strides 4/8/16/32 (16^2, 8^2, 4^2, 2^2: N = 340), B 2, nc 5, reg 16, fp32: the last stage is smaller than one 64-cell chunk
  b    128^2, strides 8/16/32 (N = 336), B 3, nc 80, reg 16, heads rounded to bf16: 288-byte aligned rows
  c32  64^2, nc 3, reg 4, B 2, fp32: rows of 19 elements          c16  the same rounded to bf16: 38-byte rows, unaligned
  d    256^2, 4 stages (N = 5440), B 2, nc 5, reg 16: several blocks per stage
  e    a with mutil_label                   f1   a with agnostic false          f2   a with postprocess_bbox false
  g    a with the class logits of the last image lowered by 20: no cell passes, the image gives None
  h    a with one cell whose class logits 1 and 3 are 20 and 25: both sigmoids are 1.0f, class 1 wins (candidate level only)
  t    a under use_tta
  m    b's shape under the compute_metric thresholds (0.001 / 0.65), heads NOT rounded: at 0.001 every cell is a candidate, bf16 logits
       repeat, and torch's CPU sigmoid returns values one ulp apart for EQUAL logits (vector body and scalar tail differ), so the order
       of the reference's NMS among such rows is its own rounding noise — no seed of a rounded m meets the score-gap condition
  p    a with every head a channel slice of a wider cell-major tensor (ldp > 4*reg + nc; NaN around the slice)
  q2 / q32   a with reg 2 / reg 32
Compared with the restatement only (RESTATED_ONLY): r, 96 x 160, strides 8/16/32 (12 x 20 = 240 cells = 3.75 chunks, 6 x 10, 3 x 5):
the reference scrambles the grid of rectangular maps.
"""
from collections import OrderedDict

import numpy as np

from tools.postproc_cases import bf16_round

F32 = np.float32

HYP0 = dict(cls_threshold=0.25, iou_threshold=0.45, max_predictions_per_img=300, agnostic=True, postprocess_bbox=True,
            mutil_label=False, use_tta=False, wfb=False, compute_metric_cls_threshold=0.001, compute_metric_iou_threshold=0.65)

_A = dict(img=(64, 64), strides=(4, 8, 16, 32), B=2, nc=5, reg=16, bf16=0, bias=-2.5)
_B = dict(img=(128, 128), strides=(8, 16, 32), B=3, nc=80, reg=16, bf16=1, bias=-4.0)
CASES = OrderedDict([
    ("a", dict(_A)),
    ("b", dict(_B)),
    ("c32", dict(_A, nc=3, reg=4, bias=-2.2)),
    ("c16", dict(_A, nc=3, reg=4, bias=-2.2, bf16=1)),
    ("d", dict(_A, img=(256, 256), bias=-3.6)),
    ("e", dict(_A, hyp=dict(mutil_label=True))),
    ("f1", dict(_A, bias=-3.0, hyp=dict(agnostic=False))),
    ("f2", dict(_A, hyp=dict(postprocess_bbox=False))),
    ("g", dict(_A, empty_last=1)),
    ("h", dict(_A, tie_cell=1)),
    ("t", dict(_A, bias=-3.2, hyp=dict(use_tta=True))),
    ("m", dict(_B, metric=1, bf16=0)),
    ("p", dict(_A, sliced=1)),
    ("q2", dict(_A, reg=2)),
    ("q32", dict(_A, reg=32)),
    ("r", dict(_A, img=(96, 160), strides=(8, 16, 32))),
])
RESTATED_ONLY = ("r",)
SQUARE = tuple(n for n in CASES if n not in RESTATED_ONLY)
NEED_SUPPRESSION = ("a", "b", "d")          # at least one suppressed box and one row removed by the merge filter
TIE_CELL = (0, 0, 1, 2, 1, 3)               # case h: image, stage, row, column, class with logit 20, class with logit 25
SLICE_LEAD = 8                              # case p: channels of the wider tensor in front of the head's


def case(name):
    c = dict(metric=0, empty_last=0, tie_cell=0, sliced=0, hyp={})
    c.update(CASES[name])
    return c


def make_hyp(name, device="cpu"):
    c = case(name)
    hyp = dict(HYP0, device=device, num_class=c["nc"], reg=c["reg"], input_img_size=list(c["img"]))
    hyp.update(c["hyp"])
    return hyp


def thresholds(name):
    """(cls_threshold, iou_threshold) the evaluator of the case works with"""
    hyp = make_hyp(name)
    k = "compute_metric_" if case(name)["metric"] else ""
    return hyp[k + "cls_threshold"], hyp[k + "iou_threshold"]


def ncell(name):
    c = case(name)
    return sum((c["img"][0] // s) * (c["img"][1] // s) for s in c["strides"])


def heads(name, seed, call=0):
    """OrderedDict of (B, 4*reg + nc, h, w) float32 head tensors of the case's call-th forward (bf16 cases: bf16-representable values)"""
    from yoloseries_amd.utils.synth import synth_v8_heads
    c = case(name)
    out = synth_v8_heads(c["B"], c["img"], c["nc"], c["reg"], seed=seed + call, strides=c["strides"])
    for k, v in out.items():
        v[:, 4 * c["reg"]:] += F32(c["bias"])
        if c["empty_last"]:
            v[-1, 4 * c["reg"]:] -= F32(20)
    if c["tie_cell"]:
        b, s, y, x, c20, c25 = TIE_CELL
        v = list(out.values())[s]
        v[b, 4 * c["reg"]:, y, x] = F32(-3)
        v[b, 4 * c["reg"] + c20, y, x] = F32(20)
        v[b, 4 * c["reg"] + c25, y, x] = F32(25)
    if c["bf16"]:
        out = OrderedDict((k, bf16_round(v)) for k, v in out.items())
    return out


def inputs(name):
    """the (B, 3, h, w) float32 network input of the case: the stub ignores its values, the evaluators read its shape"""
    c = case(name)
    return np.zeros((c["B"], 3) + tuple(c["img"]), F32)


class StubYolo:
    """callable model of a case for torch evaluators: the call-th call returns heads(name, seed, call) as tensors on `device`;
    bf16 cases as torch.bfloat16 when as_bf16 (the product path) or as the same values in float32 (the reference).  With `period` the
    heads repeat every `period` calls (an evaluator that runs its passes a second time sees the same heads again)."""

    def __init__(self, name, seed, device="cpu", as_bf16=False, period=None):
        self.name, self.seed, self.device, self.as_bf16, self.period, self.calls = name, seed, device, as_bf16, period, 0

    def __call__(self, x):
        import torch
        c = case(self.name)
        hs = heads(self.name, self.seed, self.calls % self.period if self.period else self.calls)
        self.calls += 1
        out = OrderedDict()
        for k, v in hs.items():
            t = torch.from_numpy(v).to(self.device)
            if c["bf16"] and self.as_bf16:
                t = t.bfloat16()
            if c["sliced"]:
                t = slice_of_wider(t)
            out[k] = t
        return out


def slice_of_wider(t):
    """(B, C, h, w) -> the same values as channels SLICE_LEAD .. SLICE_LEAD + C of a cell-major [B][h][w][ld] buffer that is NaN
    everywhere else: a view whose cells are ld > C elements apart"""
    import torch
    B, C, h, w = t.shape
    ld = ((SLICE_LEAD + C + 8 + 7) // 8) * 8
    buf = torch.full((B, h, w, ld), float("nan"), dtype=t.dtype, device=t.device)
    buf[..., SLICE_LEAD:SLICE_LEAD + C] = t.permute(0, 2, 3, 1)
    return buf.as_strided((B, ld, h, w), (h * w * ld, 1, w * ld, ld))[:, SLICE_LEAD:SLICE_LEAD + C]
