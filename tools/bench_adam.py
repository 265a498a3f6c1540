#!/usr/bin/env python3
"""HBM-rate check of the two optimizer step kernels side by side: yh_sgd_step_dev (21 B per element) and yh_adam_step_dev (29 B per
element; alone, and with yh_adam_advance in front of it as in a step) at the arena sizes of YOLOv5s / m / l / x.  The two alternate inside every
round, and each walks a ring of buffer sets larger than the 256 MB Infinity Cache, so that a pass reads from HBM as it does in a
train step.  Prints the median over the rounds and their spread.
usage: bench_adam.py [iters] [rounds]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from yoloseries_amd import hipk

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 400
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
RING_BYTES = 1 << 30


def timeit(fn):
    for k in range(4):
        fn(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for name, n in (("yolov5s", 7235389), ("yolov5m", 21190557), ("yolov5l", 46563709), ("yolov5x", 86749405)):
    nset = max(2, -(-RING_BYTES // (16 * n)))
    gen = torch.Generator(device=dev).manual_seed(0)
    sets = [[torch.randn(n, generator=gen, device=dev) * s for s in (1.0, 0.01, 0.0, 0.0)] for _ in range(nset)]    # p, g, m / buf, v
    group = (torch.arange(n, device=dev) % 3).to(torch.uint8)
    scal = torch.tensor([1e-3, 1e-3, 1e-3, 0.0, 1e-4, 0.0, 0.937, 0.0], device=dev)
    blk = torch.zeros(hipk.ADAM_BLK_FLOATS, device=dev)
    blk[:hipk.ADAM_BLK_HOST] = torch.tensor([1e-3, 1e-3, 1e-3, 0.0, 1e-4, 0.0, 0.937, 0.999, 1e-8])

    def sgd(k):
        p, g, b, _ = sets[k % nset]
        hipk.sgd_step_dev(p, g, b, group, scal, True)

    def adam(k):
        p, g, m, v = sets[k % nset]
        hipk.adam_step_dev(p, g, m, v, group, blk)

    def adam_adv(k):
        hipk.adam_advance(blk)
        adam(k)

    hipk.adam_advance(blk)                        # bias corrections of step 1 for the passes timed without the advance kernel
    t = {"sgd": [], "adam": [], "adam+advance": []}
    for _ in range(rounds):
        for k, fn in (("sgd", sgd), ("adam", adam), ("adam+advance", adam_adv)):
            t[k].append(timeit(fn))
    out = []
    for k, nb in (("sgd", 21), ("adam", 29), ("adam+advance", 29)):
        ts = sorted(t[k])
        med = ts[len(ts) // 2]
        out.append(f"{k}: {med * 1000:7.1f} us ({ts[0] * 1000:.1f}..{ts[-1] * 1000:.1f}) {nb * n / med / 1e9:5.2f} TB/s")
    ratio = sorted(t["adam"])[rounds // 2] / sorted(t["sgd"])[rounds // 2]
    print(f"{name:8s} n={n:9d} ring of {nset} sets | " + " | ".join(out) + f" | adam / sgd {ratio:.2f} (bytes: 1.38)", flush=True)
    del sets
