#!/usr/bin/env python3
"""Weighted box fusion at the validation workload's size: B = 64, 640 x 640, 80 classes, the three test-time-augmentation passes
from three sets of synth_nms_heads (bf16 cell-major, about 1 % of the anchors above 0.001, in overlapping groups), skip threshold
0.001, pass weights (1, 1, 1), IoU threshold 0.5 — the shipped config's values.  The candidate table is built once by the
evaluator's own path (yh_decode_filter_view per pass); timed on it, with device events, one pair per run, the median the figure:
  sort_fuse   hipk.wbf: the key, the stable sort, the workspace and yh_wbf_batched (what the evaluator runs per batch)
  fuse        yh_wbf_batched alone on the sorted table (two launches)
  nms         yh_nms_batched on the same table, for scale (iou 0.65, class aware, merge filter, 300 rows kept)
Nobody has measured this kernel before and the parent commit raises on this path, so the figures are a record, not a bar.
Worst case, not measured here: every row its own cluster in one class is n^2 / 256 IoU steps in one workgroup.
usage: bench_wbf.py [--out profiles/wbf_b64_640.json] [--runs 30] [--warmup 5] [--batch 64] [--box-mean reference]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from yoloseries_amd import _lib, hipk  # noqa: E402
from yoloseries_amd._lib import check, lib  # noqa: E402
from yoloseries_amd.layout import to_cell_major  # noqa: E402
from yoloseries_amd.trainer import YOLOV5Evaluator  # noqa: E402
from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_nms_heads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wbf_b64_640.json"))
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--box-mean", default="reference", choices=sorted(hipk.WBF_BOX_MEANS))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_wbf.py measures on an MI355X: no GPU found")
dev = torch.device("cuda:0")
IMG, NC, SKIP, IOU_THR, WEIGHTS, SEEDS = 640, 80, 0.001, 0.5, [1, 1, 1], (21, 22, 23)


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


class Stub:
    """three calls, three sets of heads, one set of device tensors, as the engine's head buffers"""

    def __init__(self, B):
        self.sets = [[torch.from_numpy(h).to(dev) for h in synth_nms_heads(B, IMG, NC, 3, seed=s)] for s in SEEDS]
        self.out = [to_cell_major(torch.zeros_like(h, dtype=torch.bfloat16))[0] for h in self.sets[0]]
        self.calls = 0

    def __call__(self, x):
        for o, h in zip(self.out, self.sets[self.calls % 3]):
            o.copy_(h)
        self.calls += 1
        return self.out


B = args.batch
hyp = dict(device=dev, num_class=NC, input_img_size=[IMG, IMG], iou_threshold=0.2, conf_threshold=0.3, cls_threshold=0.3,
           max_predictions_per_img=300, iou_type="iou", mutil_label=False, agnostic=True, postprocess_bbox=True, half=False,
           compute_metric_conf_threshold=0.001, compute_metric_iou_threshold=0.65, compute_metric_cls_threshold=0.001,
           use_tta=True, wfb=True, wfb_weights=WEIGHTS, wfb_iou_threshold=IOU_THR, wfb_skip_box_threshold=SKIP, wfb_box_mean=args.box_mean)
ev = YOLOV5Evaluator(Stub(B), torch.from_numpy(COCO_ANCHORS), hyp, compute_metric=True)
x = torch.rand(B, 3, IMG, IMG, device=dev)
cand, ncand, _B, cap, weight = ev._tta_table(x, ev._wfb_thresholds(True), ev.wfb_weights)
rows_in = (weight > 0).sum(dim=1)

out, nout, members = hipk.wbf(cand, weight, IOU_THR, args.box_mean, num_class=NC)
t_all = timed(lambda: hipk.wbf(cand, weight, IOU_THR, args.box_mean, num_class=NC), args.runs, args.warmup)

# the kernel alone, on the sorted order of the same table
order, nvalid = hipk.wbf_order(cand, weight, NC)
L = lib()
ws_bytes = int(L.yh_wbf_ws_bytes(B, cap))
ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
out2, nout2, mem2 = torch.empty_like(out), torch.zeros_like(nout), torch.zeros_like(members)


def fuse():
    check(L.yh_wbf_batched(cand.data_ptr(), weight.data_ptr(), order.data_ptr(), nvalid.data_ptr(), B, cap, NC, IOU_THR,
                           hipk.WBF_BOX_MEANS[args.box_mean], out2.data_ptr(), nout2.data_ptr(), mem2.data_ptr(), ws.data_ptr(),
                           _lib.stream_ptr()), "yh_wbf_batched")


t_fuse = timed(fuse, args.runs, args.warmup)
same = torch.equal(nout2, nout) and all(torch.equal(out2[b, :n], out[b, :n]) for b, n in enumerate(nout.tolist()))
t_nms = timed(lambda: ev._nms_device(cand, ncand, B, cap), args.runs, args.warmup)
_det, nkeep = ev._nms_device(cand, ncand, B, cap)

seg = torch.stack([((weight > 0) & (cand[:, :, 5] == c)).sum(dim=1) for c in range(NC)], dim=1)          # rows per (image, class)
mem_h = torch.cat([members[b, :n] for b, n in enumerate(nout.tolist())]).float()
res = {
    "device": torch.cuda.get_device_name(0),
    "config": {"B": B, "img": IMG, "num_class": NC, "passes": 3, "heads": "synth_nms_heads seeds %s, bf16 cell-major" % (SEEDS,),
               "wfb_skip_box_threshold": SKIP, "wfb_iou_threshold": IOU_THR, "wfb_weights": WEIGHTS, "box_mean": args.box_mean,
               "cap": cap, "lds_clusters": hipk.wbf_lds_clusters()},
    "rows_in_per_image": {"mean": float(rows_in.float().mean()), "min": int(rows_in.min()), "max": int(rows_in.max())},
    "rows_out_per_image": {"mean": float(nout.float().mean()), "min": int(nout.min()), "max": int(nout.max())},
    "rows_per_image_class_max": int(seg.max()),
    "members_per_cluster": {"mean": float(mem_h.mean()), "max": int(mem_h.max())},
    "ws_bytes": ws_bytes,
    "sort_fuse": t_all,
    "fuse": dict(t_fuse, same_rows_as_sort_fuse=bool(same)),
    "nms": dict(t_nms, kept_per_image_mean=float(nkeep.float().mean())),
}
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
