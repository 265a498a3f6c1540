#!/usr/bin/env python3
"""What --device-metric buys a validation pass: the loop of val_yolov5.Training.step over the same batches, host tail
(evaluator -> rows to the host -> preds_postprocess / gt_bbox_postprocess -> mAP_v2(gts, preds)) against device tail
(evaluate_matches -> MatchAccumulator -> mAP_v2.from_matches), against the device tail with the AP on the device too (--device-ap:
MatchAccumulator.finish_ap -> mAP_v2.from_curves), and the yh_val_match and yh_val_ap launches alone.

YOLOv5s with random weights, the shipped configuration (test-time augmentation on unless --no-tta), --batches batches of the
synthetic loader, letterboxed once and kept on the device, so that the loader's host work (the same in both modes) is not in the
window.  The evaluator's confidence / class threshold is picked from a grid on the first batch so that NMS keeps on the order of
100 rows per image; where random weights reach that at no threshold, the heads come from synth_nms_heads through a stub that still
runs the network (its forward stays in the window) — the result says which ("heads").  The three modes alternate; each figure is the
median of --reps runs after one warm-up, a run timed from its first batch to the synchronize behind its last, the metric behind it
timed on its own ("metric_s": compute_tp is in it on the host path and on the device on the others; with device_ap the sort, the
yh_val_ap launch and the copy of the curves are in "loop_s", like finish(), and "metric_s" is what is left for the host).  The kernels:
events around 50 launches after 10 warm-ups, yh_val_match on the first batch's tables, yh_val_ap on the whole pass's compacted table
(its key build + sort timed the same way next to it).

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
from yoloseries_amd.trainer.eval_yolov5 import AP_GRID, IOU_THRESHOLDS, PR_GRID, info_tensor   # noqa: E402
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


def device_ap_pass(ev, batches, num_class, dev):
    acc = MatchAccumulator(num_class, dev)
    for x in batches:
        acc.append(ev.evaluate_matches(x['img'], x['ann'], x['resize_info'], gt_hist=acc.gt_hist))
    ap, precision, recall, npred, hist = acc.finish_ap()
    torch.cuda.synchronize()
    return lambda: mAP_v2.from_curves(ap, precision, recall, hist).get_mean_metrics(), int(npred.sum())


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


def tie_report(conf, cls, tp):
    """how far the pass's table is from the condition under which the host's unstable argsort and the device's stable order must
    agree: rows that share (class, confidence) with another row, and those of them whose group holds different TP masks"""
    bits = (tp.astype(np.int64) << np.arange(tp.shape[1])).sum(1)
    key = (cls.astype(np.int64) << 32) | conf.view(np.uint32).astype(np.int64)
    order = np.lexsort((bits, key))
    k, b = key[order], bits[order]
    first = np.nonzero(np.r_[True, k[1:] != k[:-1]])[0]
    size = np.diff(np.r_[first, len(k)])
    mixed = np.minimum.reduceat(b, first) != np.maximum.reduceat(b, first)
    return dict(rows=len(k), distinct_class_conf=len(first), rows_in_tied_groups=int(size[size > 1].sum()),
                rows_in_tied_groups_with_different_masks=int(size[mixed].sum()))


def restatement_check(ev, batches, num_class, dev):
    """the device's curves on the pass's table against the NumPy restatement of the tests (stable order, left-to-right sum): bit for bit"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_val_ap_host import order_ref, val_ap_ref
    acc = MatchAccumulator(num_class, dev)
    for x in batches:
        acc.append(ev.evaluate_matches(x['img'], x['ann'], x['resize_info'], gt_hist=acc.gt_hist))
    conf, cls, tp, hist = acc.finish()
    ap, precision, recall, npred, _ = acc.finish_ap()
    bits = (tp.astype(np.uint16) << np.arange(tp.shape[1], dtype=np.uint16)).sum(1).astype(np.uint16)
    ref = val_ap_ref(conf, cls, bits, order_ref(conf, cls), hist)
    same = all(np.array_equal(a.view(np.uint64), ref[k].view(np.uint64)) for a, k in ((ap, "ap"), (precision, "precision"), (recall, "recall")))
    return dict(tie_report(conf, cls, tp), device_equals_restatement_bit_for_bit=bool(same and np.array_equal(npred, ref["npred"])))


def _event_ms(fn, launches, warm):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


@torch.no_grad()
def ap_kernel_ms(ev, batches, num_class, dev, launches=50, warm=10):
    """yh_val_ap alone on the compacted table of the whole pass, and the key build + stable sort in front of it"""
    acc = MatchAccumulator(num_class, dev)
    for x in batches:
        acc.append(ev.evaluate_matches(x['img'], x['ann'], x['resize_info'], gt_hist=acc.gt_hist))
    conf, cls, tp = (t.contiguous() for t in acc._compact())
    n, nt = conf.numel(), len(IOU_THRESHOLDS)

    def sort():
        key = (cls.to(torch.int64) << 32) | (0xFFFFFFFF - (conf.view(torch.int32).to(torch.int64) & 0xFFFFFFFF))
        return torch.sort(key, stable=True)[1].to(torch.int32)
    order = sort()
    xs = torch.from_numpy(np.concatenate((np.linspace(0, 1, AP_GRID), np.linspace(0, 1, PR_GRID)))).to(dev)
    o = [torch.empty(num_class * nt, dtype=torch.float64, device=dev), torch.empty(num_class * PR_GRID, dtype=torch.float64, device=dev),
         torch.empty(num_class * PR_GRID, dtype=torch.float64, device=dev), torch.empty(num_class, dtype=torch.int32, device=dev),
         torch.empty(max(int(_lib.lib().yh_val_ap_ws_bytes(n, nt)), 16), dtype=torch.uint8, device=dev)]

    def launch():
        _lib.check(_lib.lib().yh_val_ap(conf.data_ptr(), cls.data_ptr(), tp.data_ptr(), order.data_ptr(), n, acc.gt_hist.data_ptr(), num_class,
                                        nt, xs.data_ptr(), AP_GRID, xs[AP_GRID:].data_ptr(), PR_GRID, *[t.data_ptr() for t in o],
                                        _lib.stream_ptr()), "yh_val_ap")
    k_ms = _event_ms(launch, launches, warm)
    s_ms = _event_ms(sort, launches, warm)
    seg = torch.bincount(cls.clamp(0, num_class - 1), minlength=num_class)
    return dict(ms_per_launch=k_ms, key_and_sort_ms=s_ms, rows=n, num_class=num_class, n_thr=nt, longest_segment=int(seg.max()),
                classes_with_rows=int((seg > 0).sum()))


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

    modes = {"host": lambda: host_pass(ev, batches), "device": lambda: device_pass(ev, batches, nc, dev),
             "device_ap": lambda: device_ap_pass(ev, batches, nc, dev)}
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
    # the AP sum is added left to right on the device and pairwise by np.sum: the four figures agree to 1e-12, not to the bit —
    # where no two rows of a class with different TP masks share a confidence ("table": how many rows of this pass do; among those
    # the host's argsort is unstable and the device takes table order, and the device's curves are then held to the restatement)
    res["device_ap_metrics_close"] = res["device_ap"]["n_pred"] == res["device"]["n_pred"] and bool(
        np.allclose(res["device_ap"]["metrics"], res["device"]["metrics"], rtol=1e-12, atol=1e-12))
    res["device_ap_metrics_max_abs_diff"] = float(np.abs(np.subtract(res["device_ap"]["metrics"], res["device"]["metrics"])).max())
    res["table"] = restatement_check(ev, batches, nc, dev)
    res["device_ap_no_slower"] = res["device_ap"]["total_s"] <= res["device"]["total_s"]
    res["yh_val_match"] = dict(ms_per_launch=k_ms, **k_info)
    res["yh_val_ap"] = ap_kernel_ms(ev, batches, nc, dev)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
