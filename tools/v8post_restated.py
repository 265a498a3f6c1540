"""NumPy restatement of the YOLOv8 evaluator's post-processing as csrc/postproc_v8.hip and YOLOV8Evaluator compute it, in float32
or float64.  Written from the description of the semantics:

  1. cells: stages in the order given, row-major inside a stage;
  2. per cell and side [t, b, l, r]: softmax(reg logits) . [1, 2, ..., reg] (1-based bins);
  3. box = (gx - l, gy - t, gx + r, gy + b) * (img_h / h) with gx = col + 0.5, gy = row + 0.5 — for rectangular maps too, where the
     reference's make_grid scrambles the grid;
  4. scores = sigmoid of every class logit, no objectness;
  5. single label: score = the largest sigmoid, class = the first index that reaches it (compared on the values of the working
     dtype), candidate iff score >= threshold; rows [xmin, ymin, xmax, ymax, score, cls] in cell order;
  6. multi label: one row per (cell, class) with sigmoid >= threshold, in (cell, class) order;
  7. NMS: oracle.postproc.nms_image (class offset cls * 4096 when agnostic, inclusive threshold, cap, merge filter); an image
     without candidates gives None;
  8. TTA: passes (1, none), (0.83, rows flipped), (0.67, columns flipped); boxes times the reciprocal of the scale taken once in the
     working dtype; a flip mirrors AND swaps the corner pair; the passes' candidates are appended in pass order.
A yardstick for tests and tools, never a product path."""
import numpy as np

from oracle.postproc import nms_image

TTA_PASSES = ((1, None), (0.83, 2), (0.67, 3))


def decode(heads, img_h, reg, dtype=np.float32):
    """list of (B, 4*reg + nc, h, w) -> (B, N, 4 + nc) [xmin, ymin, xmax, ymax, sigmoid(cls)...] in `dtype`"""
    out = []
    bins = np.arange(1, reg + 1, dtype=dtype)
    for p in heads:
        B, E, h, w = p.shape
        x = np.ascontiguousarray(np.asarray(p, dtype=dtype).transpose(0, 2, 3, 1)).reshape(B, h * w, E)
        z = x[..., :4 * reg].reshape(B, h * w, 4, reg)
        e = np.exp(z - z.max(-1, keepdims=True))
        dist = ((e / e.sum(-1, keepdims=True)) * bins).sum(-1).astype(dtype)               # (B, hw, 4) [t, b, l, r]
        gy, gx = np.meshgrid(np.arange(h, dtype=dtype) + dtype(0.5), np.arange(w, dtype=dtype) + dtype(0.5), indexing="ij")
        gx, gy = gx.reshape(-1), gy.reshape(-1)
        st = dtype(dtype(img_h) / dtype(h))
        box = np.stack((gx - dist[..., 2], gy - dist[..., 0], gx + dist[..., 3], gy + dist[..., 1]), -1) * st
        cls = dtype(1) / (dtype(1) + np.exp(-x[..., 4 * reg:]))
        out.append(np.concatenate((box, cls), -1).astype(dtype))
    return np.concatenate(out, 1)


def unview(dec, scale, flip, img_h, img_w):
    """one TTA pass back to the original image, in place"""
    dtype = dec.dtype.type
    if scale != 1:
        dec[..., :4] *= dtype(1) / dtype(scale)
    if flip == 2:
        ymin, ymax = dtype(img_h) - dec[..., 3], dtype(img_h) - dec[..., 1]
        dec[..., 1], dec[..., 3] = ymin, ymax
    if flip == 3:
        xmin, xmax = dtype(img_w) - dec[..., 2], dtype(img_w) - dec[..., 0]
        dec[..., 0], dec[..., 2] = xmin, xmax
    return dec


def candidates(dec_img, cls_thr, multi_label=False):
    """(N, 4 + nc) of one image -> (M, 6) rows in the dtype of dec_img"""
    dtype = dec_img.dtype.type
    sc = dec_img[:, 4:]
    if multi_label:
        r, c = np.nonzero(sc >= dtype(cls_thr))
        return np.concatenate((dec_img[r, :4], sc[r, c][:, None], c[:, None].astype(dtype)), 1)
    best, cls = sc.max(1), sc.argmax(1)
    keep = best >= dtype(cls_thr)
    return np.concatenate((dec_img[keep, :4], best[keep, None], cls[keep, None].astype(dtype)), 1)


def decoded_of(head_sets, hyp, img_hw, dtype=np.float32):
    """the tensor the filter sees: head_sets is [heads] without TTA, the heads of the three passes with it (list of lists of arrays)"""
    img_h, img_w = img_hw
    if not hyp["use_tta"]:
        return decode(head_sets[0], img_h, hyp["reg"], dtype)
    net_h = int(np.ceil(img_h / 32) * 32)             # scale_img pads every pass back to this height
    parts = [unview(decode(hs, net_h, hyp["reg"], dtype), s, f, img_h, img_w) for hs, (s, f) in zip(head_sets, TTA_PASSES)]
    return np.concatenate(parts, 1)


def postprocess(dec, cls_thr, iou_thr, hyp):
    """decoded (B, N, 4 + nc) -> (candidate rows per image, final rows per image or None); the NMS decides in float32, as every
    implementation does, and the rows it keeps are returned in the dtype of `dec`"""
    cands = [candidates(dec[b], cls_thr, bool(hyp["mutil_label"])) for b in range(dec.shape[0])]
    outs = []
    for x in cands:
        rows, keep = nms_image(x.astype(np.float32), iou_thr, bool(hyp["agnostic"]), int(hyp["max_predictions_per_img"]), bool(hyp["postprocess_bbox"]))
        outs.append(None if rows is None else x[keep])
    return cands, outs


def run_case(name, seed, dtype=np.float32):
    """a case of tools/v8post_cases.py -> (decoded, candidate rows per image, final rows per image)"""
    from tools import v8post_cases as vc
    hyp = vc.make_hyp(name)
    ncall = 3 if hyp["use_tta"] else 1
    sets = [list(vc.heads(name, seed, k).values()) for k in range(ncall)]
    dec = decoded_of(sets, hyp, vc.case(name)["img"], dtype)
    cls_thr, iou_thr = vc.thresholds(name)
    cands, outs = postprocess(dec, cls_thr, iou_thr, hyp)
    return dec, cands, outs


# ------------------------------------------------------------------------------------------------- conditions on a fixture
def offset_iou(x, agnostic):
    """pairwise IoU (float64) of candidate rows with the class offset of the NMS"""
    b = x[:, :4].astype(np.float64) + (x[:, 5:6].astype(np.float64) * 4096 if agnostic else 0)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.clip(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), 0, None)
    h = np.clip(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), 0, None)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area[:, None] + area[None, :] - inter)


def conditions(name, dec, cands, outs, max_logit=None):
    """-> None where the conditions a stored seed must meet hold, else the name of the first that does not:
    every candidate decision >= 1e-5 away from the class threshold; outside case h no two candidates of an image with scores closer
    than 1e-6 — except scores that are EQUAL because their logits are equal (max_logit: per image the largest class logit of every
    row's cell; heads rounded to bf16 repeat logits, every implementation then computes the same score twice and breaks the tie by
    index); every pairwise class-offset IoU >= 1e-4 away from the IoU threshold; cases a, b, d: a suppressed box and a row removed
    by the merge filter."""
    from tools import v8post_cases as vc
    hyp = vc.make_hyp(name)
    cls_thr, iou_thr = vc.thresholds(name)
    sc = dec[..., 4:].astype(np.float64)
    decided = sc if hyp["mutil_label"] else sc.max(-1)
    if np.abs(decided - cls_thr).min() < 1e-5:
        return "a candidate decision within 1e-5 of the class threshold"
    for b, x in enumerate(cands):
        if len(x) < 2:
            continue
        if name != "h":
            o = np.argsort(x[:, 4], kind="stable")
            gap = np.diff(x[o, 4].astype(np.float64))
            close = gap < 1e-6
            if max_logit is not None and not hyp["mutil_label"]:
                ml = max_logit[b][o]
                close &= ~((gap == 0) & (ml[1:] == ml[:-1]))
            if close.any():
                return "two scores closer than 1e-6"
        iou = offset_iou(x, bool(hyp["agnostic"]))
        iou = iou[np.triu_indices(len(x), 1)]
        if (np.abs(iou[np.isfinite(iou)] - iou_thr) < 1e-4).any():
            return "an IoU within 1e-4 of the threshold"
    if name in vc.NEED_SUPPRESSION:
        supp = merged = False
        for x in cands:
            if len(x) == 0:
                continue
            keep = nms_image(x.astype(np.float32), iou_thr, bool(hyp["agnostic"]), int(hyp["max_predictions_per_img"]), False)[1]
            kept = nms_image(x.astype(np.float32), iou_thr, bool(hyp["agnostic"]), int(hyp["max_predictions_per_img"]), True)[1]
            supp |= len(keep) < len(x)
            merged |= len(kept) < len(keep)
        if not (supp and merged):
            return "no suppressed box or no row removed by the merge filter"
    return None


def cell_max_logit(name, seed, dec, cls_thr):
    """per image the largest class logit of the cell behind every single-label candidate row, in row order"""
    from tools import v8post_cases as vc
    hyp = vc.make_hyp(name)
    ncall = 3 if hyp["use_tta"] else 1
    reg = hyp["reg"]
    ml = np.concatenate([np.concatenate([p[:, 4 * reg:].max(1).reshape(p.shape[0], -1) for p in vc.heads(name, seed, k).values()], 1)
                         for k in range(ncall)], 1)
    keep = dec[..., 4:].max(-1) >= dec.dtype.type(cls_thr)
    return [ml[b][keep[b]] for b in range(dec.shape[0])]
