#!/usr/bin/env python3
"""YOLOv8 post-processing at the workload's size: B = 64, 640 x 640, 4 stages (160^2 .. 20^2, N = 34 000 cells), 80 classes, reg 16,
bf16 cell-major heads ~ N(0, 1) with the class logits lowered so that about 1 % of the cells pass cls_threshold 0.25.  Timed with
device events, one pair per run, 50 runs after 10 warm-ups; the median is the figure, min and max its spread.  The heads (627 MB) do
not fit the 256 MB Infinity Cache, so every run reads them from HBM.  Algorithmic bytes: the heads read once.
  decode_filter   yh_v8_decode_filter with its workspace (scan + gather), the path YOLOV8Evaluator takes
  one_workgroup   the same entry point without a workspace (one workgroup per image), for scale
  nms             yh_nms_batched on the table decode_filter left
  torch           for context, not a gate: the reference's decode (:88-102) and candidate mask (:175) restated with torch ON THE GPU
                  (the reference itself takes the softmax on the host) from fp32 copies of the same heads
Writes one JSON file.
usage: bench_v8post.py [--out profiles/v8post_bench.json] [--runs 50] [--warmup 10] [--batch 64]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from yoloseries_amd import _lib  # noqa: E402
from yoloseries_amd._lib import check, lib  # noqa: E402
from yoloseries_amd.layout import cell_major_view  # noqa: E402
from yoloseries_amd.trainer import YOLOV8Evaluator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "v8post_bench.json"))
ap.add_argument("--runs", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_v8post.py measures on an MI355X: no GPU found")
dev = torch.device("cuda:0")
IMG, NC, REG, STRIDES = 640, 80, 16, (4, 8, 16, 32)
C_ALL = 4 * REG + NC
CLS_THR, IOU_THR, BIAS = 0.25, 0.45, -4.76        # P(N(0,1) >= 3.66) = 1.26e-4 per class: 1 % of the cells have one of 80 above 0.25


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": runs}


B = args.batch
gen = torch.Generator(device=dev).manual_seed(7)
heads = {}
for name, s in zip(("pred_xs", "pred_s", "pred_m", "pred_l"), STRIDES):
    buf = torch.randn(B, IMG // s, IMG // s, C_ALL, generator=gen, device=dev, dtype=torch.float32)
    buf[..., 4 * REG:] += BIAS
    heads[name] = cell_major_view(buf.bfloat16(), C_ALL)
    del buf
hyp = dict(device=dev, num_class=NC, reg=REG, input_img_size=[IMG, IMG], use_tta=False, cls_threshold=CLS_THR, iou_threshold=IOU_THR,
           max_predictions_per_img=300, agnostic=True, postprocess_bbox=True, mutil_label=False,
           compute_metric_cls_threshold=0.001, compute_metric_iou_threshold=0.65)
ev = YOLOV8Evaluator(lambda x: heads, hyp)
d, canon, ptrs = ev._desc(heads, IMG)
N = ev._ncell(d)
L = lib()
head_bytes = sum(c.shape[0] * c.shape[2] * c.shape[3] * c.stride(3) * c.element_size() for c in canon)
cap = 4096
cand = torch.empty(B, cap, 6, dtype=torch.float32, device=dev)
ncand = torch.zeros(B, dtype=torch.int32, device=dev)
ws_bytes = int(L.yh_v8_decode_filter_ws_bytes(C.byref(d)))
ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)


def decode_filter():
    check(L.yh_v8_decode_filter(C.byref(d), ptrs, None, CLS_THR, cand.data_ptr(), ncand.data_ptr(), cap, ws.data_ptr(), _lib.stream_ptr()),
          "yh_v8_decode_filter")


decode_filter()
counts = ncand.cpu()
assert int(counts.max()) <= cap, "raise cap: the table of the timed run must hold every candidate"
two_pass_table = cand.clone()
t_df = timed(decode_filter, args.runs, args.warmup)
t_one = timed(lambda: check(L.yh_v8_decode_filter(C.byref(d), ptrs, None, CLS_THR, cand.data_ptr(), ncand.data_ptr(), cap, None,
                                                  _lib.stream_ptr()), "yh_v8_decode_filter"), 10, 2)
same = torch.equal(ncand.cpu(), counts) and all(torch.equal(cand[b, :n], two_pass_table[b, :n]) for b, n in enumerate(counts.tolist()))

max_keep = 300
out = torch.empty(B, max_keep, 6, dtype=torch.float32, device=dev)
nkeep = torch.zeros(B, dtype=torch.int32, device=dev)
keep = torch.empty(B, max_keep, dtype=torch.int32, device=dev)
nws = torch.empty(L.yh_nms_ws_bytes(B, cap), dtype=torch.uint8, device=dev)
t_nms = timed(lambda: check(L.yh_nms_batched(cand.data_ptr(), ncand.data_ptr(), B, cap, IOU_THR, 1, 1, max_keep, 1, out.data_ptr(),
                                             nkeep.data_ptr(), keep.data_ptr(), nws.data_ptr(), _lib.stream_ptr()), "yh_nms_batched"),
              args.runs, args.warmup)

res = {
    "config": {"B": B, "img": IMG, "stages": [IMG // s for s in STRIDES], "cells": N, "num_class": NC, "reg": REG, "dtype": "bf16",
               "cls_threshold": CLS_THR, "iou_threshold": IOU_THR, "class_bias": BIAS, "cap": cap},
    "candidates_per_image": {"mean": float(counts.float().mean()), "min": int(counts.min()), "max": int(counts.max())},
    "kept_per_image_mean": float(nkeep.float().mean()),
    "head_bytes": head_bytes, "ws_bytes": ws_bytes,
    "decode_filter": dict(t_df, TBps=head_bytes / (t_df["median_ms"] * 1e-3) / 1e12),
    "one_workgroup": dict(t_one, same_table=bool(same)),
    "nms": t_nms,
}
print(json.dumps(res), flush=True)

# context: the reference's decode and candidate mask with torch on the GPU, fp32, at the largest batch that fits
rb = B
while rb >= 1:
    try:
        hp = [c[:rb].float() for c in canon]
        grid, strd = ev.make_grid([[c.shape[2], c.shape[3]] for c in canon], [IMG / c.shape[2] for c in canon], dev)
        bins = torch.arange(1, REG + 1, dtype=torch.float32, device=dev)

        def restated():
            allp = torch.cat([x.reshape(rb, C_ALL, -1) for x in hp], dim=2).permute(0, 2, 1).contiguous()
            reg, cls = allp.split((4 * REG, NC), -1)
            tblr = reg.view(rb, reg.size(1), 4, -1).softmax(-1).matmul(bins)
            t, b_, l, r = tblr.chunk(4, -1)
            gx, gy = grid[:, [0]][None], grid[:, [1]][None]
            dec = torch.cat((torch.cat((gx - l, gy - t, gx + r, gy + b_), -1) * strd[None], cls.sigmoid()), -1).contiguous()
            return dec, dec[..., 4:].amax(-1) >= CLS_THR
        torch.cuda.reset_peak_memory_stats()
        t_r = timed(restated, 10, 2)
        res["torch_restatement_fp32"] = dict(t_r, B=rb, peak_alloc_bytes=int(torch.cuda.max_memory_allocated()),
                                             note="decode + candidate mask only; the reference copies the decoded tensor to the host next")
        break
    except torch.OutOfMemoryError:
        hp = None
        torch.cuda.empty_cache()
        rb //= 2
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res.get("torch_restatement_fp32")), flush=True)
