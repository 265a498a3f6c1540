#!/usr/bin/env python3
"""YOLOV8Loss forward + backward at the workload's size: B = 64, 640 x 640, 4 stages (160^2 .. 20^2, N = 34 000 cells), 80 classes,
reg 16, bf16 cell-major heads, targets from utils/synth.py.  Timed with device events after warm-up; the heads (627 MB) do not fit
the 256 MB Infinity Cache, so every pass reads them from HBM.  Algorithmic bytes: the logits read once by the forward, read and
written once by the backward.  For context (not a gate) the fp32 torch restatement (tools/v8loss_restated.py) is timed on the same
GPU at the largest batch of 64, 32, ... that fits in memory.  Writes one JSON file.
usage: bench_v8loss.py [--out profiles/v8loss_bench.json] [--iters 20] [--batch 64]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tools.v8loss_restated import v8loss_restated  # noqa: E402
from yoloseries_amd._lib import lib  # noqa: E402
from yoloseries_amd.layout import cell_major_view  # noqa: E402
from yoloseries_amd.loss import YOLOV8Loss  # noqa: E402
from yoloseries_amd.utils.synth import synth_targets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "v8loss_bench.json"))
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_v8loss.py measures on an MI355X: no GPU found")
dev = torch.device("cuda:0")
IMG, NC, REG, STRIDES = 640, 80, 16, (4, 8, 16, 32)
C_ALL = 4 * REG + NC


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


def heads(B, dtype):
    gen = torch.Generator(device=dev).manual_seed(7)
    out = {}
    for name, s in zip(("pred_xs", "pred_s", "pred_m", "pred_l"), STRIDES):
        buf = torch.randn(B, IMG // s, IMG // s, C_ALL, generator=gen, device=dev, dtype=torch.float32).to(dtype)
        out[name] = cell_major_view(buf, C_ALL).requires_grad_(True)
    return out


B = args.batch
hyp = dict(alpha=0.5, beta=6.0, topk=13, reg=REG, input_img_size=[IMG, IMG], num_class=NC, device=dev, loss_items_on_device=True)
tars = torch.from_numpy(synth_targets(B, IMG, NC, 20, seed=1)).to(dev)
preds = heads(B, torch.bfloat16)
lf = YOLOV8Loss(hyp)
plist = list(preds.values())


def fwd():
    return lf(preds, tars)


def fwd_bwd():
    torch.autograd.grad(lf(preds, tars)["tot_loss"], plist)


out = fwd()
desc = lf._last[0]
logit_bytes = sum(p.shape[0] * p.shape[2] * p.shape[3] * p.stride(3) * p.element_size() for p in plist)
t_fwd, t_all = timed(fwd, args.iters), timed(fwd_bwd, args.iters)
res = {
    "config": {"B": B, "img": IMG, "stages": [IMG // s for s in STRIDES], "num_class": NC, "reg": REG, "topk": 13, "dtype": "bf16",
               "max_boxes": int(tars.shape[1]), "valid_boxes": int((tars[..., 4] >= 0).sum()), "iters": args.iters},
    "tar_nums": int(out["tar_nums"]), "tot_loss": out["tot_loss"].item(),
    "fwd_ms": t_fwd, "fwd_bwd_ms": t_all,
    "logit_bytes": logit_bytes, "algorithmic_bytes_fwd": logit_bytes, "algorithmic_bytes_fwd_bwd": 3 * logit_bytes,
    "fwd_TBps": logit_bytes / (t_fwd * 1e-3) / 1e12, "fwd_bwd_TBps": 3 * logit_bytes / (t_all * 1e-3) / 1e12,
    "ws_bytes": int(lib().yh_v8loss_ws_bytes(C.byref(desc))), "saved_bytes": int(lib().yh_v8loss_saved_bytes(C.byref(desc))),
}
print(json.dumps(res), flush=True)
del preds, plist, lf

# context: the fp32 torch restatement, forward + backward, at the largest batch that fits
rb = B
while rb >= 1:
    try:
        rp = [p.detach().float().contiguous().requires_grad_(True) for p in heads(rb, torch.float32).values()]
        rt = tars[:rb]
        rhyp = dict(hyp, device=dev)

        def restated():
            torch.autograd.grad(v8loss_restated(rp, rt, rhyp, torch.float32)["tot_loss"], rp)
        torch.cuda.reset_peak_memory_stats()
        t_r = timed(restated, 3)
        res["restatement_fp32"] = {"B": rb, "fwd_bwd_ms": t_r, "peak_alloc_bytes": int(torch.cuda.max_memory_allocated())}
        break
    except torch.OutOfMemoryError:
        rp = None
        torch.cuda.empty_cache()
        rb //= 2
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res.get("restatement_fp32")), flush=True)
