#!/usr/bin/env python3
"""Ingest rate of the dataset layer: images/s that the prefetcher delivers with nothing consuming them, host letterbox
(fixed_imgsize_collate_fn -> DataPrefetcher) against device letterbox (raw_imgsize_collate_fn -> DeviceLetterboxPrefetcher), on the
synthetic dataset, plus the letterbox kernel's own rate (events around 50 launches after 10 warm-ups, output bytes per second).

The two paths alternate on the same machine and each figure is the median of --reps runs.  A run is timed from the creation of the
loader's iterator (worker start-up included: with 8 workers a later start of the clock would count the batches that the workers
queued before it) to the synchronize after its last batch.

    python tools/bench_ingest.py [--src 480 640] [--img 640] [--batch 64] [--workers 0 8] [--reps 5] [--out profiles/ingest_letterbox.json]

--multiscale measures the multi-scale ingest instead (utils/multiscale.py): a (batch, 3, img, img) fp32 batch resized to each of
--sizes and written as the stem's bf16 space-to-depth input, three ways -- (a) F.interpolate on the device + yh_input_s2d, the only
route before the resize kernels, (b) yh_resize_bilinear + yh_input_s2d, (c) yh_resize_bilinear_s2d -- alternating, medians of --reps
runs of 20 launches after 5 warm-ups, with the bytes each route has to move and the share of the 8 TB/s HBM peak that this amounts to;
and what a miss of the program cache costs: the first training step of YOLOv5s at a shape it has not seen, against a later one.

    python tools/bench_ingest.py --multiscale [--img 640] [--batch 64] [--sizes 320 608 960] [--out profiles/ingest_multiscale.json]

--augment measures the augmentation kernel (hipk.augment_batch: mosaic + warp + flips + HSV in one launch): --batch outputs of
--img x --img from 2 --img x 2 --img mosaic canvases of four --src images each, plans drawn with the shipped data_aug_* values, events
around 50 launches after 10 warm-ups, medians of --reps runs alternating with its variants (HSV off; affine, i.e. no divide; a canvas
with no tile, i.e. the stores alone) and with the letterbox kernel at the same output size, which is the comparison.

    python tools/bench_ingest.py --augment [--src 480 640] [--img 640] [--batch 64] [--out profiles/ingest_augment.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                        # noqa: E402
from functools import partial                                                       # noqa: E402
from torch.utils.data import DataLoader                                             # noqa: E402
from yoloseries_amd import hipk                                                     # noqa: E402
from yoloseries_amd.dataset import (DataPrefetcher, DeviceLetterboxPrefetcher, SyntheticDetectionDataset, fixed_imgsize_collate_fn,
                                    raw_imgsize_collate_fn)                        # noqa: E402


def loader_rate(device_path, src_hw, img, batch, workers, batches, seed):
    ds = SyntheticDetectionDataset(batches * batch, img_hw=src_hw, seed=seed)
    collate = raw_imgsize_collate_fn if device_path else fixed_imgsize_collate_fn
    loader = DataLoader(ds, batch_size=batch, shuffle=False, num_workers=workers, drop_last=True, pin_memory=True,
                        collate_fn=partial(collate, dst_size=[img, img]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pf = (DeviceLetterboxPrefetcher if device_path else DataPrefetcher)(loader)
    n = 0
    for _ in range(batches):
        x = pf.next()
        assert x['img'] is not None and tuple(x['img'].shape) == (batch, 3, img, img)
        n += batch
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def kernel_rate(src_hw, img, batch, reps):
    ds = SyntheticDetectionDataset(batch, img_hw=src_hw, seed=5)
    host = raw_imgsize_collate_fn([ds[i] for i in range(batch)], dst_size=[img, img])
    t = [host[k].cuda() for k in ('raw', 'img_off', 'src_hw', 'rows', 'cols')]
    out = torch.empty(batch, 3, t[3].shape[1], t[4].shape[1], device='cuda')
    border = [t[0], t[1], t[2], torch.full_like(t[3], -1), torch.full_like(t[4], -1)]     # no source reads: the kernel's store rate
    ms = {"gather": [], "border_only": []}
    for _ in range(reps):
        for what, tabs in (("gather", t), ("border_only", border)):                      # alternate
            for _ in range(10):
                hipk.letterbox_batch(*tabs, out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                hipk.letterbox_batch(*tabs, out)
            e1.record()
            torch.cuda.synchronize()
            ms[what].append(e0.elapsed_time(e1) / 50)
    med = statistics.median(ms["gather"])
    nbytes = out.numel() * 4
    return {"ms_per_launch": med, "ms_all": ms["gather"], "output_bytes": nbytes, "source_bytes": t[0].numel(),
            "output_TB_per_s": nbytes / med / 1e9, "images_per_s": batch / med * 1e3,
            "border_only_ms_per_launch": statistics.median(ms["border_only"]),
            "border_only_output_TB_per_s": nbytes / statistics.median(ms["border_only"]) / 1e9}


def augment_rate(src_hw, img, batch, reps):
    import random
    import numpy as np
    from yoloseries_amd.utils import augment as A
    ds = SyntheticDetectionDataset(16, img_hw=src_hw, seed=5)
    items = [ds[i] for i in range(len(ds))]
    hyp = A.check_aug_hyp({})                                                         # the shipped values (config/train_yolov5.yaml)
    rng, np_rng = random.Random(5), np.random.RandomState(5)

    def tables(hyp):
        plans = [A.draw_plan(b % len(items), len(items), lambda i: items[i][0].shape[:2], [img, img], hyp, rng, np_rng) for b in range(batch)]
        raw, tiles, canvas_hw, minv, gains = A.plan_tables(plans, [[items[i][0] for i in p['indices']] for p in plans])
        dev = [torch.from_numpy(raw).cuda(), torch.from_numpy(tiles.view(np.uint8).reshape(batch, 4, 40)).cuda(),
               torch.from_numpy(canvas_hw).cuda(), torch.from_numpy(minv).cuda(), None if gains is None else torch.from_numpy(gains).cuda()]
        return dev

    full = tables(hyp)
    affine = tables(dict(hyp, data_aug_prespective=0.0))
    variants = {"shipped": full, "hsv_off": full[:4] + [None], "affine": affine, "affine_hsv_off": affine[:4] + [None],
                "no_tile": [full[0], torch.zeros_like(full[1]), full[2], full[3], None]}
    out = torch.empty(batch, 3, img, img, device='cuda')
    lb_host = raw_imgsize_collate_fn([items[b % len(items)] for b in range(batch)], dst_size=[img, img])
    lb = [lb_host[k].cuda() for k in ('raw', 'img_off', 'src_hw', 'rows', 'cols')]
    fns = {k: (lambda v=v: hipk.augment_batch(*v, out, hyp['data_aug_fill_value'])) for k, v in variants.items()}
    fns["letterbox"] = lambda: hipk.letterbox_batch(*lb, out)
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():                                                        # alternate
            ms[k].append(_timed(fn, launches=50, warmup=10))
    nbytes = out.numel() * 4
    res = {"output_bytes": nbytes, "source_bytes": full[0].numel(), "canvas": [2 * img, 2 * img]}
    for k, v in ms.items():
        med = statistics.median(v)
        res[k] = {"ms_per_launch": med, "ms_all": v, "output_TB_per_s": nbytes / med / 1e9, "images_per_s": batch / med * 1e3}
    for k in variants:
        res[k]["over_letterbox"] = res[k]["ms_per_launch"] / res["letterbox"]["ms_per_launch"]
    return res


HBM_PEAK_B_PER_S = 8e12             # MI355X specification; about 6.3e12 is achievable by a streaming kernel


def _timed(fn, launches=20, warmup=5):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def multiscale_rates(img, batch, sizes, reps):
    import torch.nn.functional as F
    x = torch.rand(batch, 3, img, img, device='cuda')
    out = {}
    for size in sizes:
        mid = torch.empty(batch, 3, size, size, device='cuda')
        s2d = torch.empty(batch, size // 2, size // 2, 16, dtype=torch.bfloat16, device='cuda')
        parts = {
            "interpolate": lambda: F.interpolate(x, size=(size, size), mode='bilinear', align_corners=False),
            "resize_bilinear": lambda: hipk.resize_bilinear(x, mid),
            "input_s2d": lambda: hipk.input_s2d(mid, s2d),
            "a_interpolate_then_s2d": lambda: hipk.input_s2d(F.interpolate(x, size=(size, size), mode='bilinear', align_corners=False), s2d),
            "b_resize_then_s2d": lambda: (hipk.resize_bilinear(x, mid), hipk.input_s2d(mid, s2d)),
            "c_resize_s2d_fused": lambda: hipk.resize_bilinear_s2d(x, s2d),
        }
        ms = {k: [] for k in parts}
        for _ in range(reps):
            for k, fn in parts.items():                                                  # alternate
                ms[k].append(_timed(fn))
        in_b, mid_b, out_b = x.numel() * 4, mid.numel() * 4, s2d.numel() * 2
        moved = {"interpolate": in_b + mid_b, "resize_bilinear": in_b + mid_b, "input_s2d": mid_b + out_b,
                 "a_interpolate_then_s2d": in_b + 2 * mid_b + out_b, "b_resize_then_s2d": in_b + 2 * mid_b + out_b,
                 "c_resize_s2d_fused": in_b + out_b}
        entry = {}
        for k, v in ms.items():
            med = statistics.median(v)
            entry[k] = {"ms": med, "ms_all": v, "bytes_moved": moved[k], "GB_per_s": moved[k] / med / 1e6,
                        "share_of_hbm_peak": moved[k] / (med * 1e-3) / HBM_PEAK_B_PER_S}
        out[f"{img}_to_{size}"] = entry
        print(json.dumps({f"{img}_to_{size}": {k: round(e["ms"], 4) for k, e in entry.items()}}), flush=True)
        del mid, s2d
    return out


def program_build_cost(batch, sizes):
    """seconds of the first training step (forward, loss-free backward) of YOLOv5s at a shape the model has not run, which builds
    the program, its training buffers and its backward, against the median of five later steps"""
    from yoloseries_amd import models
    torch.manual_seed(0)
    m = models.YOLOV5Small(3, 80).cuda().train()
    m._yh_program_budget_bytes = 1 << 50
    out = {}
    for size in sizes:
        x = torch.rand(batch, 3, size, size, device='cuda')
        times = []
        for _ in range(6):
            for p_ in m.parameters():
                p_.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sum((o.float() ** 2).mean() for o in m(x)).backward()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        prog = m._yh_state()['progs'][(batch, size, size)]
        out[str(size)] = {"first_step_s": times[0], "later_step_s": statistics.median(times[1:]), "later_all_s": times[1:],
                          "program_owned_bytes": prog.owned_bytes()}
        print(json.dumps({f"program_{size}": out[str(size)]}), flush=True)
        m._yh_state()['progs'].clear()
        del prog, x
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multiscale", action="store_true")
    ap.add_argument("--augment", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[320, 608, 960])
    ap.add_argument("--program-sizes", type=int, nargs="*", default=[640, 960])
    ap.add_argument("--src", type=int, nargs=2, default=[480, 640])
    ap.add_argument("--img", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--workers", type=int, nargs="+", default=[0, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-batches", type=int, default=1, help="batches per worker (at least one) in a host-path run")
    ap.add_argument("--device-batches", type=int, default=4, help="batches per worker (at least one) in a device-path run")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.augment:
        res = {"box": torch.cuda.get_device_name(0), "src_hw": args.src, "img": args.img, "batch": args.batch, "reps": args.reps,
               "kernel": augment_rate(tuple(args.src), args.img, args.batch, args.reps)}
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if args.multiscale:
        res = {"box": torch.cuda.get_device_name(0), "img": args.img, "batch": args.batch, "reps": args.reps,
               "hbm_peak_B_per_s": HBM_PEAK_B_PER_S, "resize": multiscale_rates(args.img, args.batch, args.sizes, args.reps),
               "program_build": program_build_cost(args.batch, args.program_sizes)}
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    res = {"box": torch.cuda.get_device_name(0), "cpus": len(os.sched_getaffinity(0)), "src_hw": args.src, "img": args.img, "batch": args.batch,
           "reps": args.reps, "kernel": kernel_rate(tuple(args.src), args.img, args.batch, args.reps), "loader_img_per_s": {}}
    print(json.dumps({"kernel": res["kernel"]}), flush=True)
    for w in args.workers:
        runs = {"host": [], "device": []}
        for rep in range(args.reps):
            for path in ("host", "device"):                                          # alternate the two paths
                nb = (args.device_batches if path == "device" else args.host_batches) * max(w, 1)
                runs[path].append(loader_rate(path == "device", tuple(args.src), args.img, args.batch, w, nb, seed=1 + rep))
                print(f"workers {w} run {rep} {path}: {nb} batches, {runs[path][-1]:.1f} img/s", flush=True)
        entry = {p: {"median": statistics.median(v), "all": v} for p, v in runs.items()}
        entry["device_over_host"] = entry["device"]["median"] / entry["host"]["median"]
        res["loader_img_per_s"][f"workers_{w}"] = entry
        print(json.dumps({f"workers_{w}": entry}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
