#!/usr/bin/env python3
"""Ingest rate of the dataset layer: images/s that the prefetcher delivers with nothing consuming them, host letterbox
(fixed_imgsize_collate_fn -> DataPrefetcher) against device letterbox (raw_imgsize_collate_fn -> DeviceLetterboxPrefetcher), on the
synthetic dataset, plus the letterbox kernel's own rate (events around 50 launches after 10 warm-ups, output bytes per second).

The two paths alternate on the same machine and each figure is the median of --reps runs.  A run is timed from the creation of the
loader's iterator (worker start-up included: with 8 workers a later start of the clock would count the batches that the workers
queued before it) to the synchronize after its last batch.

    python tools/bench_ingest.py [--src 480 640] [--img 640] [--batch 64] [--workers 0 8] [--reps 5] [--out profiles/ingest_letterbox.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=int, nargs=2, default=[480, 640])
    ap.add_argument("--img", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--workers", type=int, nargs="+", default=[0, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-batches", type=int, default=1, help="batches per worker (at least one) in a host-path run")
    ap.add_argument("--device-batches", type=int, default=4, help="batches per worker (at least one) in a device-path run")
    ap.add_argument("--out")
    args = ap.parse_args()
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
