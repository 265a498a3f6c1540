#!/usr/bin/env python3
"""YOLOV7Loss forward + backward at the workload's size: B = 64, 640 x 640, 3 stages (80^2, 40^2, 20^2), 80 classes, bf16 cell-major
heads, about 20 boxes per image (utils/synth.py), loss_items_on_device; beside it, in the same process and on the same heads,
YOLOV5Loss: the yardstick.  Timed with device events after warm-up.  The share of each YOLOv7 kernel (the SimOTA kernel among
them) comes from one profiled forward + backward (torch.profiler, device activities only); where the profiler gives no kernel
records the shares are left out.  Writes one JSON file.
usage: bench_v7loss.py [--out profiles/v7loss_bench.json] [--iters 20] [--batch 64]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from yoloseries_amd.layout import cell_major_view  # noqa: E402
from yoloseries_amd.loss import YOLOV5Loss, YOLOV7Loss  # noqa: E402
from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_targets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "v7loss_bench.json"))
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_v7loss.py measures on an MI355X: no GPU found")
dev = torch.device("cuda:0")
IMG, NC, STRIDES = 640, 80, (8, 16, 32)
C_ALL, LD = 3 * (5 + NC), 256


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


B = args.batch
gen = torch.Generator(device=dev).manual_seed(7)
preds = []
for s in STRIDES:
    buf = torch.randn(B, IMG // s, IMG // s, LD, generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16)
    preds.append(cell_major_view(buf, C_ALL).requires_grad_(True))
hyp = dict(num_class=NC, use_focal_loss=True, focal_loss_gamma=1.5, focal_loss_alpha=0.25, iou_loss_scale=0.05, cls_loss_scale=0.5,
           cof_loss_scale=1.0, anchor_match_thr=4.0, class_smooth_factor=1.0, cls_pos_weight=1.0, cof_pos_weight=1.0, topk=15,
           use_iou_as_tar_cof=True, input_img_size=[IMG, IMG], device=dev, loss_items_on_device=True)
tars = torch.from_numpy(synth_targets(B, IMG, NC, 40, seed=1)).to(dev)           # 1..40 boxes per image: about 20
anchors = torch.from_numpy(COCO_ANCHORS.copy()).to(dev)
res = {"config": {"B": B, "img": IMG, "stages": [IMG // s for s in STRIDES], "num_class": NC, "topk": 15, "dtype": "bf16",
                  "max_boxes": int(tars.shape[1]), "valid_boxes": int((tars[..., 4] >= 0).sum()), "iters": args.iters}}
for name, cls in (("yolov7", YOLOV7Loss), ("yolov5", YOLOV5Loss)):
    lf = cls(anchors, dict(hyp))

    def fwd():
        return lf(preds, tars)

    def fwd_bwd():
        torch.autograd.grad(lf(preds, tars)["tot_loss"], preds)
    out = fwd()
    res[name] = {"tar_nums": int(out["tar_nums"]), "tot_loss": out["tot_loss"].item(),
                 "fwd_ms": timed(fwd, args.iters), "fwd_bwd_ms": timed(fwd_bwd, args.iters)}
    if name == "yolov7":
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fwd_bwd()
                torch.cuda.synchronize()
            ker = {}
            for ev in prof.events():
                # the library's own kernels of this loss only (fill_u32_kernel is yh_fill_u32; torch's fill kernels have other names)
                m = re.search(r"v7_\w+_kernel|v5_assign_kernel|fill_u32_kernel", ev.name)
                if m:
                    ker[m.group(0)] = ker.get(m.group(0), 0.0) + ev.device_time_total / 1e3
            if ker:
                tot = sum(ker.values())
                res[name]["kernel_ms"] = ker
                res[name]["simota_share_of_kernel_time"] = sum(v for k, v in ker.items() if "simota" in k) / tot
        except Exception as e:                      # the timing above stands without the breakdown
            res[name]["kernel_ms_error"] = f"{type(e).__name__}: {e}"
    print(json.dumps({name: res[name]}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
