#!/usr/bin/env python3
"""Generate tests/golden/g19_v8loss.npz by RUNNING THE REFERENCE's YOLOV8Loss (loss/yolov8_loss.py) on the CPU.

Runs only where /root/reference exists; the reference is imported read-only with the shims of tools/gen_golden.py.  Only data
is written: per case the arguments and the head seed (yoloseries_amd.utils.synth.synth_v8_heads), the targets verbatim, the
five outputs, the gradient of tot_loss w.r.t. every head tensor and the matched target row per cell.

Hyp of every case: alpha 0.5, beta 6.0, topk 13 (case e: topk 1), the reference's default scales.  Cases:
  a  128^2, 4 stages (32^2, 16^2, 8^2, 4^2; N = 1360), B 2, M 4, 5 classes, reg 16
  b  64^2, 4 stages (16^2, 8^2, 4^2, 2^2; N = 340), B 3, M 3, 3 classes, reg 16
  c  128^2, 3 stages (16^2, 8^2, 4^2), otherwise as a, reg 8
  d  as a, logits x 3
  e  as a, topk 1, one valid box in one image: a single foreground cell (gpu_CIoU squeezes to a scalar)
  f  as a, every target row padding (the reference runs it: only the class term is non-zero)
  g  as a, inputs rounded to bf16 first
  h  as a, with cls_pos_weight 2.5, focal gamma 2.0 / alpha 0.4 and the scales 5.0 / 1.0 / 0.5 (stored as `h_hyp`, JSON): beyond
     the cases asked for, so that the reference pins every field of the descriptor
Odd images have one padding row (except e, f).  Boxes are 0.15-0.55 x img, centred in the middle 60 %, logits N(0, 1).

The seed of a case is searched until the fixture sits on no decision boundary and not on the first departure of
csrc/loss_v8.hip; ASSERTED for the stored seed:
  - every valid ground truth has at least topk strictly positive metrics;
  - the relative gap between its topk-th and (topk+1)-th metric is >= 1e-3;
  - at every multiply-chosen cell the best and the second-best IoU differ by >= 1e-3 relative;
  - cases a and b have at least one multiply-chosen cell.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_v8.py
"""
import json
import os
import sys

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g19_v8loss.npz")

CASES = {   # img, B, M, nc, reg, strides, scale, topk, bf16, boxes per image (None: M, odd images M - 1)
    "a": dict(img=128, B=2, M=4, nc=5, reg=16, strides=(4, 8, 16, 32), scale=1.0, topk=13, bf16=0, boxes=None),
    "b": dict(img=64, B=3, M=3, nc=3, reg=16, strides=(4, 8, 16, 32), scale=1.0, topk=13, bf16=0, boxes=None),
    "c": dict(img=128, B=2, M=4, nc=5, reg=8, strides=(8, 16, 32), scale=1.0, topk=13, bf16=0, boxes=None),
    "d": dict(img=128, B=2, M=4, nc=5, reg=16, strides=(4, 8, 16, 32), scale=3.0, topk=13, bf16=0, boxes=None),
    "e": dict(img=128, B=2, M=4, nc=5, reg=16, strides=(4, 8, 16, 32), scale=1.0, topk=1, bf16=0, boxes=[1, 0]),
    "f": dict(img=128, B=2, M=4, nc=5, reg=16, strides=(4, 8, 16, 32), scale=1.0, topk=13, bf16=0, boxes=[0, 0]),
    "g": dict(img=128, B=2, M=4, nc=5, reg=16, strides=(4, 8, 16, 32), scale=1.0, topk=13, bf16=1, boxes=None),
    "h": dict(img=128, B=2, M=4, nc=5, reg=16, strides=(4, 8, 16, 32), scale=1.0, topk=13, bf16=0, boxes=None,
              hyp=dict(cls_pos_weight=2.5, focal_loss_gamma=2.0, focal_loss_alpha=0.4, iou_loss_scale=5.0, cls_loss_scale=1.0,
                       dfl_loss_scale=0.5)),
}
ARG_NAMES = ("img", "B", "M", "nc", "reg", "nstage", "topk", "bf16", "seed", "stride0")


def make_hyp(c, device="cpu"):
    return dict(alpha=0.5, beta=6.0, topk=c["topk"], reg=c["reg"], input_img_size=[c["img"], c["img"]], num_class=c["nc"],
                device=device, **c.get("hyp", {}))


def make_targets(c, seed):
    rs = np.random.RandomState(seed)
    img, B, M = c["img"], c["B"], c["M"]
    t = -np.ones((B, M, 6), np.float32)
    for b in range(B):
        n = c["boxes"][b] if c["boxes"] is not None else (M - 1 if b % 2 else M)
        wh = rs.uniform(0.15, 0.55, (n, 2)) * img
        ctr = rs.uniform(0.2, 0.8, (n, 2)) * img
        t[b, :n, 0:2] = np.clip(ctr - wh / 2, 0, img)
        t[b, :n, 2:4] = np.clip(ctr + wh / 2, 0, img)
        t[b, :n, 4] = rs.randint(0, c["nc"], n)
        t[b, :n, 5] = b
    return t


def make_heads(c, seed):
    import torch
    from yoloseries_amd.utils.synth import synth_v8_heads
    heads = synth_v8_heads(c["B"], c["img"], c["nc"], c["reg"], seed=seed, scale=c["scale"], strides=c["strides"])
    out = {k: torch.from_numpy(v) for k, v in heads.items()}
    if c["bf16"]:
        out = {k: v.bfloat16().float() for k, v in out.items()}
    return out


def conditions(lf, preds, tars, topk, need_multi):
    """-> None where the asserted conditions hold, else the name of the first that does not"""
    import torch
    with torch.no_grad():
        _, pred_xyxy, pred_cls = lf.pred_preprocessing(preds)
        tar_xyxy, tar_cls = tars[..., :4], tars[..., 4]
        mask_gt = tar_cls >= 0
        in_gt = lf.select_grids_in_gt_bbox(tar_xyxy, mask_gt)
        metric, iou = lf.compute_metric(pred_xyxy, pred_cls, tar_xyxy, tar_cls, in_gt)
        mask_topk = lf.select_topk_candidates(metric, mask_gt)
    if mask_gt.any():
        v = metric[mask_gt].sort(-1, descending=True)[0]
        if not bool((v[:, topk - 1] > 0).all()):
            return "fewer than topk positive metrics"
        if float(((v[:, topk - 1] - v[:, topk]) / v[:, topk - 1]).min()) < 1e-3:
            return "topk gap"
    multi = mask_topk.sum(1) > 1                                   # (B, N)
    if need_multi and not bool(multi.any()):
        return "no multiply-chosen cell"
    if multi.any():
        top2 = iou.permute(0, 2, 1)[multi].sort(-1, descending=True)[0][:, :2]
        if float(((top2[:, 0] - top2[:, 1]) / top2[:, 0]).min()) < 1e-3:
            return "iou gap at a multiply-chosen cell"
    return None


def run_case(ref_loss, c, seed, need_multi):
    import torch
    tars = torch.from_numpy(make_targets(c, seed + 1))
    lf = ref_loss.YOLOV8Loss(make_hyp(c))
    preds = {k: v.clone().requires_grad_(True) for k, v in make_heads(c, seed).items()}
    out = lf(preds, tars.clone())
    why = conditions(lf, preds, tars, c["topk"], need_multi)
    if why is not None:
        return why
    grads = torch.autograd.grad(out["tot_loss"], list(preds.values()))
    with torch.no_grad():
        _, pred_xyxy, pred_cls = lf.pred_preprocessing(preds)
        mask_assign, _, _ = lf.label_assign(pred_cls, pred_xyxy, tars[..., 4], tars[..., :4])
    owner = torch.where(mask_assign.sum(1) > 0, mask_assign.argmax(1), torch.full((), -1, dtype=torch.long))
    vals = np.array([out["tot_loss"].item(), out["cls_loss"], out["iou_loss"], out["dfl_loss"], out["tar_nums"]], np.float64)
    assert np.isfinite(vals).all()
    return dict(targets=tars.numpy(), vals=vals, owner=owner.numpy().astype(np.int16), grads=[g.numpy() for g in grads])


def main():
    if not os.path.isdir(REF):
        sys.exit("tools/gen_golden_v8.py needs /root/reference (build container only)")
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_golden import install_shims
    install_shims()
    sys.path.insert(0, REF)
    sys.path.insert(1, ROOT)
    import torch
    import loss as ref_loss
    torch.set_num_threads(8)
    g = {}
    for name, c in CASES.items():
        seed0 = 1900 + 100 * (ord(name) - ord("a"))
        for seed in range(seed0, seed0 + 100):
            r = run_case(ref_loss, c, seed, need_multi=name in ("a", "b"))
            if isinstance(r, dict):
                break
            print(f"case {name}: seed {seed} rejected ({r})")
        else:
            sys.exit(f"case {name}: no seed in {seed0}..{seed0 + 99} meets the conditions")
        g[f"{name}_args"] = np.array([c["img"], c["B"], c["M"], c["nc"], c["reg"], len(c["strides"]), c["topk"], c["bf16"], seed,
                                      c["strides"][0]], np.int64)
        g[f"{name}_scale"] = np.array([c["scale"]], np.float64)
        if "hyp" in c:
            g[f"{name}_hyp"] = np.array(json.dumps(c["hyp"]))
        g[f"{name}_targets"], g[f"{name}_vals"], g[f"{name}_owner"] = r["targets"], r["vals"], r["owner"]
        for s, gr in enumerate(r["grads"]):
            g[f"{name}_grad{s}"] = gr
        print(f"case {name}: seed {seed}, vals {r['vals']}, assigned {int((r['owner'] >= 0).sum())}")
    g["arg_names"] = np.array(ARG_NAMES)
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
