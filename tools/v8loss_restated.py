"""Plain-torch restatement of the YOLOv8 loss as csrc/loss_v8.hip computes it, in any float dtype (fp64 for the edge-case
tests, fp32 for the golden cases).  Written from the description of the semantics, three departures from the reference included:

  1. a ground truth takes its `topk` largest STRICTLY POSITIVE metrics, ties to the lower cell index (stages as given); one
     with fewer positive metrics takes fewer cells (the reference lets torch.topk fill up with zero-metric cells);
  2. the grid of an (h, w) map is x = col + 0.5, y = row + 0.5 with stride img_size[0] / h (the reference's make_grid agrees on
     square maps only);
  3. no NaN prompt: NaNs propagate.

Only rows with class id >= 0 count as ground truths anywhere, the arg-max that settles a multiply-chosen cell included.
It materialises (B, M, N) matrices, as the reference does: a yardstick for tests and tools, never a product path."""
import json
import math

import torch
import torch.nn.functional as F


def golden_case(g, name, device="cpu"):
    """One case of tests/golden/g19_v8loss.npz (tools/gen_golden_v8.py) -> (hyp, OrderedDict of fp32 head tensors, targets)"""
    from yoloseries_amd.utils.synth import synth_v8_heads
    img, B, M, nc, reg, nstage, topk, bf16, seed, stride0 = (int(v) for v in g[f"{name}_args"])
    hyp = dict(alpha=0.5, beta=6.0, topk=topk, reg=reg, input_img_size=[img, img], num_class=nc, device=device)
    if f"{name}_hyp" in g.files:
        hyp.update(json.loads(str(g[f"{name}_hyp"])))
    heads = synth_v8_heads(B, img, nc, reg, seed=seed, scale=float(g[f"{name}_scale"][0]), strides=[stride0 << s for s in range(nstage)])
    heads = {k: torch.from_numpy(v) for k, v in heads.items()}
    if bf16:
        heads = {k: v.bfloat16().float() for k, v in heads.items()}
    return hyp, heads, torch.from_numpy(g[f"{name}_targets"].copy())


def make_grid(shapes, img_size0, dtype=torch.float32, device="cpu"):
    """[(h, w), ...] -> grid (N, 2) [x, y] in cells, stride (N,)"""
    g, s = [], []
    for h, w in shapes:
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype, device=device) + 0.5, torch.arange(w, dtype=dtype, device=device) + 0.5, indexing="ij")
        g.append(torch.stack((xs, ys), -1).reshape(-1, 2))
        s.append(torch.full((h * w,), img_size0 / h, dtype=dtype, device=device))
    return torch.cat(g), torch.cat(s)


def ciou_assign(a, b):
    """the loss class's own ciou (eps 1e-6) of broadcastable xyxy boxes a (ground truth), b (prediction); no gradient needed"""
    eps = 1e-6
    w1, h1, w2, h2 = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1], b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
    inter = ((torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp(min=0)
             * (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp(min=0))
    union = ((w1 * h1).clamp(min=0) + (w2 * h2).clamp(min=0) - inter).clamp(min=eps)
    iou = inter / union
    cw = torch.maximum(a[..., 2], b[..., 2]) - torch.minimum(a[..., 0], b[..., 0])
    ch = torch.maximum(a[..., 3], b[..., 3]) - torch.minimum(a[..., 1], b[..., 1])
    diag = (ch ** 2 + cw ** 2).clamp(min=eps)
    dist = ((a[..., 2] + a[..., 0] - (b[..., 2] + b[..., 0])) ** 2 + (a[..., 3] + a[..., 1] - (b[..., 1] + b[..., 3])) ** 2) / 4
    v = 4 / math.pi ** 2 * (torch.atan(w1 / h1) - torch.atan(w2 / h2)) ** 2
    alpha = v / (1 - iou + v).clamp(min=eps)
    return iou - (dist / diag + v * alpha)


def ciou_loss_term(b1, b2):
    """pairwise CIoU (eps 1e-9, alpha constant) of (X, 4) xyxy boxes, differentiable in b1"""
    eps = 1e-9
    w1, h1, w2, h2 = b1[:, 2] - b1[:, 0], b1[:, 3] - b1[:, 1], b2[:, 2] - b2[:, 0], b2[:, 3] - b2[:, 1]
    iw = (torch.min(b1[:, 2], b2[:, 2]) - torch.max(b1[:, 0], b2[:, 0])).clamp(min=0)
    ih = (torch.min(b1[:, 3], b2[:, 3]) - torch.max(b1[:, 1], b2[:, 1])).clamp(min=0)
    inter = iw * ih
    iou = inter / (w1 * h1 + w2 * h2 - inter).clamp(min=eps)
    cw = torch.max(b1[:, 2], b2[:, 2]) - torch.min(b1[:, 0], b2[:, 0])
    ch = torch.max(b1[:, 3], b2[:, 3]) - torch.min(b1[:, 1], b2[:, 1])
    diag = (cw ** 2 + ch ** 2).clamp(min=eps)
    dist = ((b1[:, 1] + b1[:, 3]) / 2 - (b2[:, 1] + b2[:, 3]) / 2) ** 2 + ((b1[:, 0] + b1[:, 2]) / 2 - (b2[:, 0] + b2[:, 2]) / 2) ** 2
    v = (4 / math.pi ** 2) * (torch.atan(w1 / h1.clamp(min=eps)) - torch.atan(w2 / h2.clamp(min=eps))) ** 2
    with torch.no_grad():
        alpha = v / (1 - iou + v).clamp(min=eps)
    return iou - (dist / diag + v * alpha)


def v8loss_restated(preds, tars, hyp, dtype=torch.float32):
    """preds: list (or dict) of (B, 4*reg + nc, h, w) tensors (they may require grad); tars (B, M, 6).
    -> dict: tot_loss (tensor with graph), cls_loss / iou_loss / dfl_loss (floats), tar_nums, score_sum, assignment (per stage a
    (B, h*w) int64 tensor: matched target row per cell, -1 none)"""
    if isinstance(preds, dict):
        preds = list(preds.values())
    reg, nc, topk = int(hyp["reg"]), int(hyp["num_class"]), int(hyp["topk"])
    a_exp, b_exp = float(hyp["alpha"]), float(hyp["beta"])
    B, M = tars.shape[0], tars.shape[1]
    dev = preds[0].device
    shapes = [(p.shape[2], p.shape[3]) for p in preds]
    grid, stride = make_grid(shapes, float(hyp["input_img_size"][0]), dtype, dev)
    N = grid.shape[0]
    allp = torch.cat([p.to(dtype).reshape(B, p.shape[1], -1) for p in preds], -1).permute(0, 2, 1)          # (B, N, C)
    box_logits, cls_logits = allp[..., :4 * reg].reshape(B, N, 4, reg), allp[..., 4 * reg:4 * reg + nc]
    proj = torch.arange(1, reg + 1, dtype=dtype, device=dev)
    dist = (box_logits.softmax(-1) * proj).sum(-1)                                                           # (B, N, 4) t, b, l, r
    gx, gy = grid[:, 0][None], grid[:, 1][None]
    xyxy = torch.stack((gx - dist[..., 2], gy - dist[..., 0], gx + dist[..., 3], gy + dist[..., 1]), -1)     # grid units
    tars = tars.to(device=dev, dtype=dtype)
    tb, tcls = tars[..., :4], tars[..., 4]

    with torch.no_grad():
        valid = tcls >= 0                                                                                    # (B, M)
        cx, cy = (grid[:, 0] * stride)[None, None], (grid[:, 1] * stride)[None, None]
        sides = torch.stack((cy - tb[..., 1, None], tb[..., 3, None] - cy, cx - tb[..., 0, None], tb[..., 2, None] - cx), -1)
        cand = (sides.amin(-1) > 1e-9) & valid[..., None]                                                    # (B, M, N)
        pbox = xyxy * stride[None, :, None]
        iou = torch.where(cand, ciou_assign(tb[:, :, None, :], pbox[:, None, :, :]).clamp(min=0), torch.zeros((), dtype=dtype, device=dev))
        ci = tcls.clamp(min=0).long()                                                                        # (B, M)
        score = cls_logits.sigmoid().permute(0, 2, 1)[torch.arange(B, device=dev)[:, None], ci]              # (B, M, N)
        metric = torch.where(cand, iou.pow(b_exp) * score.pow(a_exp), torch.zeros((), dtype=dtype, device=dev))
        k = min(topk, N)
        val, idx = torch.sort(metric, dim=-1, descending=True, stable=True)                                  # equal values: lower cell first
        chosen = torch.zeros(B, M, N, dtype=torch.bool, device=dev)
        chosen.scatter_(2, idx[..., :k], val[..., :k] > 0)                                                   # departure 1
        claims = chosen.sum(1)                                                                               # (B, N)
        best = iou.argmax(1)                                                                                 # first of equal maxima
        assign = torch.where((claims > 1)[:, None, :], F.one_hot(best, M).permute(0, 2, 1).bool(), chosen)
        fg = assign.any(1)                                                                                   # (B, N)
        owner = torch.where(fg, assign.int().argmax(1), torch.full((), -1, dtype=torch.long, device=dev))
        m_a, i_a = metric * assign, iou * assign
        norm = ((m_a * i_a.amax(-1, True)) / (m_a.amax(-1, True) + 1e-9)).amax(1)                            # (B, N)
        bi = torch.arange(B, device=dev)[:, None].expand(B, N)
        own0 = owner.clamp(min=0)
        cls_target = F.one_hot(tcls[bi, own0].clamp(min=0).long(), nc).to(dtype) * (norm * fg)[..., None]    # (B, N, nc)
        box_target = tb[bi, own0]                                                                            # (B, N, 4) pixels
        den = max(float(cls_target.sum()), 1.0)

    pw = float(hyp.get("cls_pos_weight", 1.0))
    gamma, alpha = float(hyp.get("focal_loss_gamma", 1.5)), float(hyp.get("focal_loss_alpha", 0.25))
    x, t = cls_logits, cls_target
    bce = (1 - t) * x + (1 + (pw - 1) * t) * F.softplus(-x)
    prob = x.sigmoid()
    factor = (1 - (t * prob + (1 - t) * (1 - prob))) ** gamma * (t * alpha + (1 - t) * (1 - alpha))
    cls_loss = (bce * factor).sum() / den

    w = norm[fg]
    tgt = (box_target / stride[None, :, None])[fg]                                                           # (X, 4) grid units
    iou_loss = ((1 - ciou_loss_term(xyxy[fg], tgt)) * w).sum() / den
    gxf, gyf = gx.expand(B, N)[fg], gy.expand(B, N)[fg]
    tdist = torch.stack((gyf - tgt[:, 1], tgt[:, 3] - gyf, gxf - tgt[:, 0], tgt[:, 2] - gxf), -1).clamp(0, reg - 1 - 0.01)
    left = tdist.long()
    w_left = (left + 1).to(dtype) - tdist
    logp = box_logits[fg].log_softmax(-1)                                                                    # (X, 4, reg)
    ce = -(logp.gather(-1, left[..., None])[..., 0] * w_left + logp.gather(-1, left[..., None] + 1)[..., 0] * (1 - w_left))
    dfl_loss = (ce.mean(-1) * w).sum() / den

    scale = [float(hyp.get("cls_loss_scale", 0.5)), float(hyp.get("iou_loss_scale", 7.5)), float(hyp.get("dfl_loss_scale", 1.5))]
    tc, ti, td = cls_loss * scale[0] * B, iou_loss * scale[1] * B, dfl_loss * scale[2] * B
    offs = [0]
    for h, w_ in shapes:
        offs.append(offs[-1] + h * w_)
    return {"tot_loss": tc + ti + td, "cls_loss": tc.item(), "iou_loss": ti.item(), "dfl_loss": td.item(),
            "tar_nums": int(fg.sum()), "score_sum": float(cls_target.sum()),
            "assignment": [owner[:, offs[s]:offs[s + 1]].clone() for s in range(len(shapes))]}
