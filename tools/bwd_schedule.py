#!/usr/bin/env python3
"""Schedule digest of the compiled backward arrays (engine/backward.py, engine/executor.py): for every (two streams, bucket hook,
frozen BatchNorm) combination, what the array replayed by yh_exec holds — entry point and label, stream, slot count, the slot
values below 2^32 (dimensions and flags; pointers and doubles are shown as `*`), the bucket breaks and the kinds of the head-gradient
patches.  Read from `prog._compiled[key]` only, after one backward of that combination.

    YH_CONV_TUNE=0 YH_WGRAD_TUNE=0 tools/bwd_schedule.py OUT.json [COMMIT]      (needs an MI355X)

writes the record tests/test_gpu_backward_schedule.py compares against (tests/golden/bwd_schedule_v5s_2x128.json): YOLOv5s at
2 x 3 x 128 x 128, the full rendering of (two, hooked, not frozen), a SHA-256 and the entry count of the other seven combinations,
of YOLOXSmall and of YOLOv5s in deterministic mode (two, not hooked, not frozen).  A change of the schedule regenerates the record
with the code BEFORE the change; COMMIT names it in the file."""
import hashlib
import itertools
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE = (2, 3, 128, 128)
COMBOS = list(itertools.product((True, False), repeat=3))          # (two, hooked, frozen)
FULL = (True, True, False)
PLAIN = (True, False, False)


def combo_name(combo):
    return "two=%d,hooked=%d,frozen=%d" % tuple(int(v) for v in combo)


def render(comp):
    """the lines of one `prog._compiled[('bwd', two, hooked, frozen)]` entry"""
    cc, breaks, patches = comp
    lines = []
    for i in range(cc.n):
        c = cc.arr[i]
        slots = ",".join(str(int(v)) if int(v) < 1 << 32 else "*" for v in c.slots[:c.nslots])
        lines.append(f"{i} s{c.stream} {cc.names[i]} n{c.nslots} {slots}")
    lines.append("breaks " + ",".join(str(b) for b in breaks))
    lines.append("patches " + ",".join(p[0] for p in patches))
    return lines


def digest(lines):
    return {"sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(), "entries": len(lines) - 2}


def _schedules(model, x, combos):
    """{combo name: lines} of `model`'s program for SHAPE: one forward + backward per combination, then the compiled array is read"""
    import torch

    def passes():
        outs = model(x)
        outs = list(outs.values()) if isinstance(outs, dict) else outs
        sum(o.float().sum() for o in outs).backward()
        torch.cuda.synchronize()
    model.train()
    passes()                                   # builds the backward: two_streams is read at every backward() after this
    prog = model._yh_program(SHAPE[0], SHAPE[2], SHAPE[3])
    two0, out = prog.two_streams, {}
    try:
        for two, hooked, frozen in combos:
            prog.two_streams = two
            model.train(not frozen)
            if hooked:
                model._yh_bucket_hook = lambda part: None
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                passes()
            model.__dict__.pop("_yh_bucket_hook", None)
            out[combo_name((two, hooked, frozen))] = render(prog._compiled[('bwd', two, hooked, frozen)])
    finally:
        prog.two_streams = two0
        model.train()
    return out


def schedules(dev):
    """{'v5s' | 'yolox_s' | 'v5s_deterministic': {combo name: lines}}; the caller sets YH_CONV_TUNE=0 and YH_WGRAD_TUNE=0"""
    import torch
    import yoloseries_amd
    from yoloseries_amd import models
    x = torch.rand(*SHAPE, generator=torch.Generator().manual_seed(5)).to(dev)
    torch.manual_seed(0)
    out = {"v5s": _schedules(models.YOLOV5Small(3, 80).to(dev), x, COMBOS),
           "yolox_s": _schedules(models.YOLOXSmall(1, 3, 80).to(dev), x, [PLAIN])}
    yoloseries_amd.set_deterministic(True)
    try:
        out["v5s_deterministic"] = _schedules(models.YOLOV5Small(3, 80).to(dev), x, [PLAIN])
    finally:
        yoloseries_amd.set_deterministic(False)
    return out


def document(scheds):
    """the record: the full rendering of v5s FULL, digests of everything else"""
    doc = {"shape": list(SHAPE), "v5s_full": {combo_name(FULL): scheds["v5s"][combo_name(FULL)]}}
    for name, by_combo in scheds.items():
        doc[name] = {k: digest(v) for k, v in by_combo.items() if not (name == "v5s" and k == combo_name(FULL))}
    return doc


if __name__ == "__main__":
    import torch
    os.environ["YH_CONV_TUNE"] = os.environ["YH_WGRAD_TUNE"] = "0"
    doc = document(schedules(torch.device("cuda:0")))
    doc["produced_by"] = sys.argv[2] if len(sys.argv) > 2 else "working tree"
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print({k: (len(v) if isinstance(v, (list, dict)) else v) for k, v in doc.items()})
