#!/usr/bin/env python3
"""What --device-metric buys a validation pass: the loop of val_yolov5.Training.step over the same batches, host tail
(evaluator -> rows to the host -> preds_postprocess / gt_bbox_postprocess -> mAP_v2(gts, preds)) against device tail
(evaluate_matches -> MatchAccumulator -> mAP_v2.from_matches), and the yh_val_match launch alone.

YOLOv5s with random weights, the shipped configuration (test-time augmentation on unless --no-tta), --batches batches of the
synthetic loader, letterboxed once and kept on the device, so that the loader's host work (the same in both modes) is not in the
window.  The evaluator's confidence / class threshold is picked from a grid on the first batch so that NMS keeps on the order of
100 rows per image; where random weights reach that at no threshold, the heads come from synth_nms_heads through a stub that still
runs the network (its forward stays in the window) — the result says which ("heads").  The two modes alternate; each figure is the
median of --reps runs after one warm-up, a run timed from its first batch to the synchronize behind its last, the metric behind it
timed on its own ("metric_s": compute_tp is in it on the host path and on the device on the other).  The kernel: events around 50
launches after 10 warm-ups on the first batch's tables.

    python tools/bench_val.py [--img 640] [--batch 64] [--batches 16] [--reps 5] [--no-tta] [--out profiles/val_metric.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                                  # noqa: E402
import torch                                                                        # noqa: E402
import val_yolov5                                                                   # noqa: E402
from config.config import Config                                                    # noqa: E402
from yoloseries_amd import _lib                                                     # noqa: E402
from yoloseries_amd.trainer import MatchAccumulator                                 # noqa: E402
from yoloseries_amd.trainer.eval_yolov5 import IOU_THRESHOLDS, info_tensor          # noqa: E402
from yoloseries_amd.utils import mAP_v2                                             # noqa: E402
from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_nms_heads                # noqa: E402

GRID = (0., 1e-5, 1e-4, 0.001, 0.003, 0.01, 0.03, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)
WANTED = (30, 250)              # "on the order of 100" rows per image, and under the cap of 300


class StubHeads:
    """runs the network, returns synth_nms_heads: the same heads for every call, as device tensors of the reference's layout"""

    def __init__(self, model, batch, img, num_class, dev):
        self.model = model
        parts = []
        for c0 in range(0, batch, 16):
            parts.append([torch.from_numpy(h) for h in synth_nms_heads(min(16, batch - c0), img, num_class, 3, seed=2 + c0 // 16, wh_shift=1.2)])
        self.heads = [torch.cat([p[s] for p in parts]).to(dev) for s in range(3)]

    def __call__(self, x):
        self.model(x)
        return self.heads


@torch.no_grad()
def rows_per_image(ev, img, thr):
    ev.conf_threshold = ev.cls_threshold = thr
    _, nkeep = ev._nms_device(*ev._candidates(img))
    return float(nkeep.float().mean())


def pick_threshold(ev, img):
    """-> (threshold, mean rows per image, every threshold tried) with the mean closest to 100 on a log scale: the grid, then up to
    12 geometric bisections between the neighbours where the count falls through the wanted range (random weights put all their
    confidences within a factor of a few)"""
    grid = {thr: rows_per_image(ev, img, thr) for thr in GRID}
    for lo, hi in zip(GRID[:-1], GRID[1:]):
        if grid[lo] > WANTED[1] and grid[hi] < WANTED[0]:
            lo = max(lo, 1e-7)
            for _ in range(12):
                mid = float(np.sqrt(lo * hi))
                grid[mid] = rows_per_image(ev, img, mid)
                if WANTED[0] <= grid[mid] <= WANTED[1]:
                    break
                lo, hi = (mid, hi) if grid[mid] > WANTED[1] else (lo, mid)
            break
    thr = min(grid, key=lambda t: abs(np.log(max(grid[t], 1e-3) / 100.)) + (10. if grid[t] >= 299 else 0.))
    return thr, grid[thr], dict(sorted(grid.items()))


def host_pass(ev, batches):
    all_preds, all_gts = [], []
    for x in batches:
        gt_bbox, gt_cls = val_yolov5.Training.gt_bbox_postprocess(x['ann'], x['resize_info'])
        preds = val_yolov5.Training.preds_postprocess(ev(x['img']), x['resize_info'])
        for j in range(len(preds)):
            all_preds.append(preds[j] if preds[j] is not None else np.zeros((0, 6)))
            all_gts.append(np.concatenate((gt_bbox[j], gt_cls[j][:, None]), axis=1))
    torch.cuda.synchronize()
    return lambda: mAP_v2(all_gts, all_preds).get_mean_metrics(), int(sum(len(p) for p in all_preds))


def device_pass(ev, batches, num_class, dev):
    acc = MatchAccumulator(num_class, dev)
    for x in batches:
        acc.append(ev.evaluate_matches(x['img'], x['ann'], x['resize_info'], gt_hist=acc.gt_hist))
    conf, cls, tp, hist = acc.finish()
    torch.cuda.synchronize()
    return lambda: mAP_v2.from_matches(conf, cls, tp, hist).get_mean_metrics(), len(conf)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metric, n_pred = fn()
    t1 = time.perf_counter()
    m = metric()
    return t1 - t0, time.perf_counter() - t1, n_pred, [float(v) for v in m]


@torch.no_grad()
def kernel_ms(ev, x, num_class, launches=50, warm=10):
    det, nkeep = ev._nms_device(*ev._candidates(x['img']))
    dev = det.device
    B, K = det.shape[:2]
    ann = x['ann'].to(device=dev, dtype=torch.float32).contiguous()
    info = info_tensor(x['resize_info']).to(dev)
    o = [torch.empty(B, K, 4, dtype=torch.float32, device=dev), torch.empty(B, K, dtype=torch.float32, device=dev),
         torch.empty(B, K, dtype=torch.int32, device=dev), torch.empty(B, K, dtype=torch.float32, device=dev),
         torch.empty(B, K, dtype=torch.int32, device=dev), torch.empty(B, K, dtype=torch.int16, device=dev),
         torch.empty(B, dtype=torch.int32, device=dev), torch.zeros(num_class, dtype=torch.int32, device=dev)]
    thr = (C.c_double * len(IOU_THRESHOLDS))(*IOU_THRESHOLDS)

    def launch():
        _lib.check(_lib.lib().yh_val_match(det.data_ptr(), nkeep.data_ptr(), ann.data_ptr(), info.data_ptr(), B, K, ann.shape[1], ann.shape[2],
                                           num_class, thr, len(IOU_THRESHOLDS), *[t.data_ptr() for t in o], _lib.stream_ptr()), "yh_val_match")
    for _ in range(warm):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches, dict(B=B, max_keep=K, maxbox=int(ann.shape[1]), rows_per_image=float(nkeep.float().mean()),
                                                matched=int((o[4][torch.arange(K, device=dev)[None] < o[6][:, None]] >= 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-tta", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_val.py measures on an MI355X: no device found")
    hyp = Config().get_config(os.path.join(ROOT, "config", "train_yolov5.yaml"))
    hyp.update(input_img_size=[args.img, args.img], batch_size=args.batch, val_batches=args.batches, model_type='small')
    hyp.setdefault('num_workers', 8)           # the loader runs once, before the window
    if args.no_tta:
        hyp['use_tta'] = False
    torch.manual_seed(0)
    v = val_yolov5.Training(torch.from_numpy(COCO_ANCHORS.copy()), hyp)
    v.model.eval()
    dev, nc = v.device, hyp['num_class']
    batches = [dict(img=x['img'].clone(), ann=x['ann'].clone(), resize_info=x['resize_info']) for x in v.val_dataloader]
    assert len(batches) == args.batches and tuple(batches[0]['img'].shape) == (args.batch, 3, args.img, args.img)

    ev = v.build_evaluator(v.model)
    thr, rows, grid = pick_threshold(ev, batches[0]['img'])
    heads = "model"
    if not WANTED[0] <= rows <= WANTED[1]:
        model_grid = grid
        ev = v.build_evaluator(StubHeads(v.model, args.batch, args.img, nc, dev))
        thr, rows, grid = pick_threshold(ev, batches[0]['img'])
        heads = "stub"
    ev.conf_threshold = ev.cls_threshold = thr
    print(json.dumps({"heads": heads, "threshold": thr, "rows_per_image": rows, "grid": grid}), flush=True)

    modes = {"host": lambda: host_pass(ev, batches), "device": lambda: device_pass(ev, batches, nc, dev)}
    runs = {k: [] for k in modes}
    for rep in range(args.reps + 1):
        for k, fn in modes.items():
            r = timed(fn)
            if rep:
                runs[k].append(r)
            print(json.dumps({"rep": rep, "mode": k, "loop_s": r[0], "metric_s": r[1], "n_pred": r[2], "metrics": r[3]}), flush=True)
    k_ms, k_info = kernel_ms(ev, batches[0], nc)
    res = {"box": torch.cuda.get_device_name(0), "cpus": len(os.sched_getaffinity(0)), "model": "yolov5s, random weights", "img": args.img,
           "batch": args.batch, "batches": args.batches, "reps": args.reps, "use_tta": bool(hyp['use_tta']), "heads": heads,
           "threshold": thr, "rows_per_image_first_batch": rows, "threshold_grid": {str(t): n for t, n in grid.items()}}
    if heads == "stub":
        res["threshold_grid_model_heads"] = {str(t): n for t, n in model_grid.items()}
    for k, rs in runs.items():
        res[k] = {"loop_s": statistics.median(r[0] for r in rs), "metric_s": statistics.median(r[1] for r in rs),
                  "total_s": statistics.median(r[0] + r[1] for r in rs), "loop_s_all": [r[0] for r in rs], "metric_s_all": [r[1] for r in rs],
                  "n_pred": rs[0][2], "metrics": rs[0][3]}
        res[k]["img_per_s"] = args.batch * args.batches / res[k]["total_s"]
    res["metrics_equal"] = res["host"]["metrics"] == res["device"]["metrics"] and res["host"]["n_pred"] == res["device"]["n_pred"]
    res["yh_val_match"] = dict(ms_per_launch=k_ms, **k_info)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
