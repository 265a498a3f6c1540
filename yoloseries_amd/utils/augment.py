"""Train-time augmentation: mosaic, random perspective, HSV jitter and flips (utils/data_aug.py of the reference: mosaic :579-671,
RandomPerspective :482-576, RandomHSV :363-389, RandomFlipLR / RandomFlipUD :434-478; drawn per item by
dataset/CommonDataloader.py:213-246, :404-429).

The reference runs these per image on the host as a chain of full-image passes over a 2H x 2W canvas.  Here an item is a *plan*: which
images are pasted where on the canvas ("tiles"), one 3 x 3 matrix for warp + flips, three HSV gains.  The pixels are produced from the
plan by one gather per output pixel, `hipk.augment_batch` on the GPU or `augment_batch_host` below, which is the written definition of
that kernel (csrc/augment.hip) and agrees with it bit for bit.  The labels follow the reference's own NumPy arithmetic on the host.

Operation order of the pixel path, every operation one correctly rounded float32 operation:
    xf = float(x), yf = float(y)
    nu = (m0*xf + m1*yf) + m2      nv = (m3*xf + m4*yf) + m5      w = (m6*xf + m7*yf) + m8
    u = nu / w,  v = nv / w
    fu = min(max(floor(u), -2), 2^30),  fv likewise          (fmax / fmin: a NaN coordinate becomes -2, i.e. outside)
    ax = u - fu,  ay = v - fv,  bx = 1 - ax,  by = 1 - ay
    taps p00 p01 | p10 p11 at (fu + {0, 1}, fv + {0, 1}): the byte of the highest tile whose rectangle holds the tap, else fill_value
    top = p00*bx + p01*ax,  bot = p10*bx + p11*ax,  val = top*by + bot*ay        (0..255 scale, no rounding to uint8)
    HSV gains, if given (hsv_jitter below), on the three channels of val
    out = val / 255
Pixel i sits at coordinate i (OpenCV's convention), so the identity matrix reproduces the canvas exactly.

Departures from the reference ("Documented deviations"): the warp's output is not rounded to uint8; the HSV jitter is
float arithmetic without OpenCV's two uint8 quantisations; an item that loses all its boxes is redrawn (MAX_TRIES plans, the last one
kept) instead of being replaced by an un-augmented random item; an item for which the mosaic is not drawn is warped too (its own
image is the canvas); mixup, cutout and scale jitting are not built."""
import math

import numpy as np

__all__ = ['TILE_DTYPE', 'MAX_TRIES', 'check_aug_hyp', 'mosaic_rects', 'warp_matrix', 'draw_plan', 'identity_plan', 'mosaic_labels',
           'warp_labels', 'flip_labels', 'valid_bbox', 'plan_labels', 'plan_tables', 'validate_tables', 'hsv_jitter',
           'augment_batch_host', 'build_canvas']

# NumPy form of yh_aug_tile (include/yolohip.h), 40 bytes
TILE_DTYPE = np.dtype([('off', '<i8'), ('src_h', '<i4'), ('src_w', '<i4'), ('sx0', '<i4'), ('sy0', '<i4'),
                       ('ox0', '<i4'), ('oy0', '<i4'), ('ox1', '<i4'), ('oy1', '<i4')])
MAX_TRIES = 8                    # plans drawn for one item until one keeps a box
_NOT_BUILT = ('data_aug_mixup_p', 'data_aug_cutout_p', 'data_aug_scale_jitting_p')
_DEFAULTS = dict(data_aug_mosaic_p=1.0, data_aug_degree=0.0, data_aug_translate=0.1, data_aug_scale=0.5, data_aug_shear=0.0,
                 data_aug_prespective=0.0005, data_aug_fill_value=114, data_aug_hsv_p=1.0, data_aug_hsv_hgain=0.015,
                 data_aug_hsv_sgain=0.7, data_aug_hsv_vgain=0.4, data_aug_fliplr_p=0.3, data_aug_flipud_p=0.0)   # config/train_yolov5.yaml


def check_aug_hyp(hyp):
    """the data_aug_* keys of a hyper-parameter dict with the defaults filled in; the augmentations that are not built must be off"""
    hyp = hyp or {}
    for key in _NOT_BUILT:
        if float(hyp.get(key, 0.0) or 0.0) != 0.0:
            raise ValueError(f"{key}={hyp[key]}: this augmentation is not built yet (only 0 is accepted)")
    out = dict(_DEFAULTS)
    out.update({k: hyp[k] for k in _DEFAULTS if k in hyp and hyp[k] is not None})
    fill = out['data_aug_fill_value']
    if int(fill) != fill or not 0 <= int(fill) <= 255:
        raise ValueError(f"data_aug_fill_value={fill} is not a byte")
    out['data_aug_fill_value'] = int(fill)
    return out


# ------------------------------------------------------------------------------------------------ geometry of a plan
def mosaic_rects(xc, yc, sizes, mosaic_shape):
    """the four paste rectangles of the mosaic (utils/data_aug.py:601-616): image i of `sizes` [(h, w)] x 4 goes to the quadrant
    i of the centre (xc, yc), its centre region cut out where it is larger than the quadrant.
    Returns [(sx0, sy0, ox0, oy0, ox1, oy1)] x 4: source pixel at the rectangle's corner, rectangle in canvas pixels (half open)."""
    mh, mw = int(mosaic_shape[0]), int(mosaic_shape[1])
    rects = []
    for i, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        if i == 0:
            ox0, oy0, ox1, oy1 = max(xc - w, 0), max(yc - h, 0), xc, yc
        elif i == 1:
            ox0, oy0, ox1, oy1 = xc, max(yc - h, 0), min(xc + w, mw), yc
        elif i == 2:
            ox0, oy0, ox1, oy1 = max(xc - w, 0), yc, xc, min(yc + h, mh)
        else:
            ox0, oy0, ox1, oy1 = xc, yc, min(xc + w, mw), min(yc + h, mh)
        sx0 = w // 2 - (ox1 - ox0) // 2
        sy0 = h // 2 - (oy1 - oy0) // 2
        rects.append((sx0, sy0, ox0, oy0, ox1, oy1))
    return rects


def warp_matrix(canvas_hw, dst_hw, perspective_xy, angle, scale, shear_xy, translate_xy):
    """M = T S R P C of RandomPerspective (utils/data_aug.py:511-538), float64, canvas -> output: C centres the canvas, P the
    perspective terms, R rotation by `angle` degrees and `scale` (cv2.getRotationMatrix2D about the origin), S the shears (degrees),
    T the translation as fractions of the output size"""
    C = np.eye(3)
    C[0, 2] = -canvas_hw[1] / 2
    C[1, 2] = -canvas_hw[0] / 2
    P = np.eye(3)
    P[2, 0], P[2, 1] = perspective_xy
    R = np.eye(3)
    rad = angle * math.pi / 180
    alpha, beta = scale * math.cos(rad), scale * math.sin(rad)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = alpha, beta, -beta, alpha
    S = np.eye(3)
    S[0, 1] = math.tan(shear_xy[0] * math.pi / 180)
    S[1, 0] = math.tan(shear_xy[1] * math.pi / 180)
    T = np.eye(3)
    T[0, 2] = translate_xy[0] * dst_hw[1]
    T[1, 2] = translate_xy[1] * dst_hw[0]
    return T @ S @ R @ P @ C


def _finish_plan(plan, dst_hw):
    """compose the flips on the left of the warp and invert: the matrix the kernel applies to an output pixel"""
    H, W = int(dst_hw[0]), int(dst_hw[1])
    M = plan['M']
    if plan['fliplr']:
        M = np.array([[-1.0, 0, W - 1], [0, 1, 0], [0, 0, 1]]) @ M
    if plan['flipud']:
        M = np.array([[1.0, 0, 0], [0, -1, H - 1], [0, 0, 1]]) @ M
    plan['M_total'] = M
    plan['minv'] = np.linalg.inv(M).astype(np.float32).reshape(9)
    return plan


def draw_plan(index, n_items, hw_of, input_dim, aug_hyp, rng, np_rng):
    """One plan for dataset item `index`, drawn in the reference's order of draws (CommonDataloader.py:408-409, :225-226,
    data_aug.py:595, :498-535, :376-377, :446, :469).  rng: a random.Random, np_rng: a numpy RandomState; hw_of(i) -> (h, w) of
    dataset image i.  Returns a dict: 'indices' (1 or 4 dataset indices, one per tile), 'canvas_hw', 'rects' (mosaic_rects' format),
    'M' (warp, canvas -> output, float64), 'scale' (the warp's scale draw), 'perspective', 'fliplr', 'flipud', 'M_total' (flips
    composed), 'minv' float32 (9,) output -> canvas, 'hsv_gain' float32 (3,) or None, 'dst_hw'."""
    hyp = aug_hyp
    H, W = int(input_dim[0]), int(input_dim[1])
    plan = {'dst_hw': (H, W)}
    if rng.random() < hyp['data_aug_mosaic_p']:
        indices = [index] + [rng.randint(0, n_items - 1) for _ in range(3)]
        rng.shuffle(indices)
        mosaic_shape = [2 * H, 2 * W]
        # the reference draws xc from the canvas height and yc from its width (data_aug.py:595 iterates [h, w])
        xc, yc = [int(rng.uniform(2 * x / 5, 4 * x / 5)) for x in np.array(mosaic_shape)]
        plan.update(indices=indices, canvas_hw=(2 * H, 2 * W), centre=(xc, yc), mosaic=True,
                    rects=mosaic_rects(xc, yc, [hw_of(i) for i in indices], mosaic_shape))
    else:
        h, w = hw_of(index)
        plan.update(indices=[index], canvas_hw=(int(h), int(w)), mosaic=False, rects=[(0, 0, 0, 0, int(w), int(h))])
    rng.random()                                                     # RandomPerspective's own p = 1.0 draw
    persp = hyp['data_aug_prespective']
    pxy = (rng.uniform(-persp, persp), rng.uniform(-persp, persp))
    angle = rng.uniform(-hyp['data_aug_degree'], hyp['data_aug_degree'])
    scale = rng.uniform(1 - hyp['data_aug_scale'], 1 + hyp['data_aug_scale'])
    shear = (rng.uniform(-hyp['data_aug_shear'], hyp['data_aug_shear']), rng.uniform(-hyp['data_aug_shear'], hyp['data_aug_shear']))
    tr = hyp['data_aug_translate']
    txy = (rng.uniform(0.5 - tr, 0.5 + tr), rng.uniform(0.5 - tr, 0.5 + tr))
    plan.update(M=warp_matrix(plan['canvas_hw'], (H, W), pxy, angle, scale, shear, txy), scale=scale, perspective=bool(persp))
    plan['hsv_gain'] = None
    if rng.random() < hyp['data_aug_hsv_p']:
        gains = np_rng.uniform(-1, 1, 3) * [hyp['data_aug_hsv_hgain'], hyp['data_aug_hsv_sgain'], hyp['data_aug_hsv_vgain']] + 1
        plan['hsv_gain'] = gains.astype(np.float32)
    plan['fliplr'] = rng.random() < hyp['data_aug_fliplr_p']
    plan['flipud'] = rng.random() < hyp['data_aug_flipud_p']
    return _finish_plan(plan, (H, W))


def identity_plan(index, src_hw, input_dim):
    """the un-augmented item as a plan: the letterbox (utils/letterbox.py, training form) as one tile and an affine matrix, sampled
    bilinearly at pixel centres (the host letterbox samples the nearest pixel; at scale 1 the two are the same copy)"""
    from .letterbox import _letterbox_geometry
    h, w = int(src_hw[0]), int(src_hw[1])
    _, (H, W), record = _letterbox_geometry((h, w), list(input_dim), 64, False, True)
    s = record['scale']
    M = np.array([[s, 0, record['pad_left'] + 0.5 * s - 0.5], [0, s, record['pad_top'] + 0.5 * s - 0.5], [0, 0, 1.0]])
    plan = {'dst_hw': (H, W), 'indices': [index], 'canvas_hw': (h, w), 'mosaic': False, 'rects': [(0, 0, 0, 0, w, h)], 'M': M,
            'scale': s, 'perspective': False, 'fliplr': False, 'flipud': False, 'hsv_gain': None, 'record': record}
    return _finish_plan(plan, (H, W))


# ------------------------------------------------------------------------------------------------ labels
def _iou_with_window(box, window):
    """IoU of (n, 4) boxes with one xyxy window, (n,): the filter of data_aug.py:624-626 keeps the boxes where it is > 0"""
    window = np.asarray(window)
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    warea = (window[2] - window[0]) * (window[3] - window[1])
    iw = np.maximum(0., np.minimum(box[:, 2], window[2]) - np.maximum(box[:, 0], window[0]))
    ih = np.maximum(0., np.minimum(box[:, 3], window[3]) - np.maximum(box[:, 1], window[1]))
    inter = iw * ih
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / (area + warea - inter)


def mosaic_labels(bboxes, labels, rects, mosaic_shape):
    """labels of the mosaic (utils/data_aug.py:619-671): per image, the boxes that touch the pasted window, rounded, clipped to the
    window, moved onto the canvas, kept where at least 0.3 (rounded to one decimal) of their area is left; the result clipped to
    [0, mosaic_shape[0]].  bboxes: four (n, 4) xyxy arrays, labels: four (n,) arrays.  Returns ((k, 4) float32, (k,)); k may be 0."""
    out_b, out_l = [], []
    for box_i, lab_i, (sx0, sy0, ox0, oy0, ox1, oy1) in zip(bboxes, labels, rects):
        sx1, sy1 = sx0 + (ox1 - ox0), sy0 + (oy1 - oy0)
        box = np.round(np.array(box_i).astype(np.float32), decimals=3).reshape(-1, 4)
        org = box.copy()
        keep = _iou_with_window(box, np.array([sx0, sy0, sx1, sy1])) > 0
        if keep.sum() == 0:
            continue
        box = box[keep]
        box[:, [0, 2]] = np.clip(np.round(box[:, [0, 2]], decimals=2), sx0, sx1 - 1)
        box[:, [1, 3]] = np.clip(np.round(box[:, [1, 3]], decimals=2), sy0, sy1 - 1)
        box[:, [0, 2]] -= sx0
        box[:, [1, 3]] -= sy0
        box[:, [0, 2]] += ox0
        box[:, [1, 3]] += oy0
        org_area = np.prod(org[keep][:, 2:4] - org[keep][:, 0:2], axis=1)
        cur_area = np.prod(box[:, 2:4] - box[:, 0:2], axis=1)
        with np.errstate(divide='ignore', invalid='ignore'):
            valid = np.round(cur_area / org_area, decimals=1) >= 0.3
        out_b.append(box[valid])
        out_l.extend(np.array(lab_i)[keep][valid])
    if not out_b:
        return np.zeros((0, 4), np.float32), np.zeros((0,), np.float32)
    return np.clip(np.concatenate(out_b, axis=0), 0, mosaic_shape[0]), np.array(out_l)


def box_candidates(box1, box2, wh_thr=2, ar_thr=20, area_thr=0.1):
    """utils/bbox_tools.py:342-355: box1 (4, n) before, box2 (4, n) after the warp; True where the warped box is worth keeping"""
    w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
    w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
    ar = np.maximum(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
    return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + 1e-16) > area_thr) & (ar < ar_thr)


def warp_labels(bboxes, labels, M, scale, perspective, dst_hw):
    """label half of RandomPerspective (utils/data_aug.py:547-574): the four corners of every box through M, their bounding box,
    clipped to the output, filtered by box_candidates against the box before the warp times `scale`"""
    height, width = dst_hw
    bboxes, labels = np.array(bboxes), np.array(labels)
    n = len(bboxes)
    if not n:
        return bboxes, labels
    xy = np.ones((n * 4, 3))
    xy[:, :2] = bboxes[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)
    xy = xy @ M.T
    xy = (xy[:, :2] / xy[:, 2:3]).reshape(n, 8) if perspective else xy[:, :2].reshape(n, 8)
    x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
    xy = np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1))).reshape(4, n).T
    xy[:, [0, 2]] = xy[:, [0, 2]].clip(0, width)
    xy[:, [1, 3]] = xy[:, [1, 3]].clip(0, height)
    keep = box_candidates(box1=bboxes[:, :4].T * scale, box2=xy.T)
    bboxes, labels = bboxes[keep], labels[keep]
    bboxes[:, :4] = xy[keep]
    return bboxes, labels


def flip_labels(bboxes, dst_hw, fliplr, flipud):
    """utils/data_aug.py:446-477: xmin' = w - xmax, xmax' = w - xmin (and the same in y)"""
    h, w = dst_hw
    bboxes = np.array(bboxes)
    if fliplr and len(bboxes):
        xmax, xmin = w - bboxes[:, 0], w - bboxes[:, 2]
        bboxes[:, 0], bboxes[:, 2] = xmin, xmax
    if flipud and len(bboxes):
        ymax, ymin = h - bboxes[:, 1], h - bboxes[:, 3]
        bboxes[:, 1], bboxes[:, 3] = ymin, ymax
    return bboxes


def valid_bbox(bboxes, wh_thr=2, ar_thr=10, area_thr=16):
    """utils/bbox_tools.py:358-389 for xyxy boxes: positive extent, sides > wh_thr, area >= area_thr, aspect ratio < ar_thr"""
    b = np.array(bboxes)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    ar_1, ar_2 = w / (h + 1e-16), h / (w + 1e-16)
    ar = np.where(ar_1 > ar_2, ar_1, ar_2)
    return (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1]) & (ar < ar_thr) & ((w * h) >= area_thr) & (h > wh_thr) & (w > wh_thr)


def plan_labels(plan, anns):
    """labels of a drawn plan: anns = [{'bboxes': (n, 4) xyxy, 'classes': (n,)}] per tile -> (bboxes (k, 4), classes (k,)) in the
    output frame, in the reference's order: mosaic, warp, flips, valid_bbox"""
    if plan['mosaic']:
        mshape = [plan['canvas_hw'][0], plan['canvas_hw'][1]]
        boxes, classes = mosaic_labels([a['bboxes'] for a in anns], [a['classes'] for a in anns], plan['rects'], mshape)
    else:
        boxes, classes = np.array(anns[0]['bboxes']).reshape(-1, 4), np.array(anns[0]['classes']).reshape(-1)
    boxes, classes = warp_labels(boxes, classes, plan['M'], plan['scale'], plan['perspective'], plan['dst_hw'])
    boxes = flip_labels(boxes, plan['dst_hw'], plan['fliplr'], plan['flipud'])
    if len(classes) > 0:
        keep = valid_bbox(boxes)
        boxes, classes = boxes[keep], classes[keep]
    return boxes, classes


# ------------------------------------------------------------------------------------------------ tables of a batch
def plan_tables(plans, images):
    """plans and their images ([[(h, w, 3) uint8] per tile] per plan) -> what hipk.augment_batch reads, as NumPy arrays: raw uint8
    (the images concatenated), tiles TILE_DTYPE (B, 4) (unused tiles empty), canvas_hw int32 (B, 2), minv float32 (B, 9),
    hsv_gain float32 (B, 3) or None (gains (1, 1, 1) where a plan of a batch with HSV has none: multiplying by 1 and the round trip
    through HSV are then applied to that image too).  Raises ValueError (validate_tables) before anything is concatenated."""
    B = len(plans)
    if B == 0:
        raise ValueError("plan_tables: empty batch")
    tiles = np.zeros((B, 4), dtype=TILE_DTYPE)
    canvas_hw = np.zeros((B, 2), dtype=np.int32)
    minv = np.zeros((B, 9), dtype=np.float32)
    flat, pos = [], 0
    for b, (plan, imgs) in enumerate(zip(plans, images)):
        if len(imgs) != len(plan['rects']) or not 1 <= len(imgs) <= 4:
            raise ValueError(f"image {b}: {len(imgs)} images for {len(plan['rects'])} tiles (1..4 allowed)")
        canvas_hw[b] = plan['canvas_hw']
        minv[b] = plan['minv']
        for k, (img, (sx0, sy0, ox0, oy0, ox1, oy1)) in enumerate(zip(imgs, plan['rects'])):
            img = np.asarray(img)
            if img.ndim != 3 or img.shape[-1] != 3 or img.dtype != np.uint8:
                raise ValueError(f"image {b}, tile {k}: images are (h, w, 3) uint8 arrays, got {img.dtype} {img.shape}")
            tiles[b, k] = (pos, img.shape[0], img.shape[1], sx0, sy0, ox0, oy0, ox1, oy1)
            flat.append(img)
            pos += img.size
    validate_tables(pos, tiles, canvas_hw)
    if not np.isfinite(minv).all():
        raise ValueError(f"image {int(np.argwhere(~np.isfinite(minv))[0, 0])}: the plan's matrix is not finite")
    raw = np.concatenate([np.ascontiguousarray(i).reshape(-1) for i in flat])
    gains = None
    if any(p['hsv_gain'] is not None for p in plans):
        gains = np.stack([np.ones(3, np.float32) if p['hsv_gain'] is None else np.asarray(p['hsv_gain'], np.float32) for p in plans])
    return raw, tiles, canvas_hw, minv, gains


def validate_tables(raw_bytes, tiles, canvas_hw):
    """every non-empty rectangle inside its canvas, its source window inside its image, the image inside the raw buffer; ValueError
    naming the image otherwise.  The kernel trusts this (it only clamps source indices into the image the tile names)."""
    tiles = np.asarray(tiles)
    for b in range(tiles.shape[0]):
        ch, cw = int(canvas_hw[b][0]), int(canvas_hw[b][1])
        if ch <= 0 or cw <= 0 or ch >= 2 ** 30 or cw >= 2 ** 30:
            raise ValueError(f"image {b}: canvas {ch}x{cw} is empty or too large")
        used = 0
        for k in range(tiles.shape[1]):
            t = tiles[b, k]
            off, sh, sw, sx0, sy0, ox0, oy0, ox1, oy1 = (int(t[n]) for n in TILE_DTYPE.names)
            if ox1 <= ox0 or oy1 <= oy0:
                continue
            used += 1
            if ox0 < 0 or oy0 < 0 or ox1 > cw or oy1 > ch:
                raise ValueError(f"image {b}, tile {k}: rectangle x {ox0}..{ox1}, y {oy0}..{oy1} is outside its {ch}x{cw} canvas")
            if sh <= 0 or sw <= 0 or sx0 < 0 or sy0 < 0 or sx0 + (ox1 - ox0) > sw or sy0 + (oy1 - oy0) > sh:
                raise ValueError(f"image {b}, tile {k}: source window x {sx0}..{sx0 + ox1 - ox0}, y {sy0}..{sy0 + oy1 - oy0} is outside "
                                 f"its {sh}x{sw} image")
            if sh * sw >= 2 ** 31:
                raise ValueError(f"image {b}, tile {k}: a {sh}x{sw} image has 2^31 pixels or more (the kernel's 32-bit pixel index)")
            if off < 0 or off + sh * sw * 3 > raw_bytes:
                raise ValueError(f"image {b}, tile {k}: bytes {off}..{off + sh * sw * 3} are outside the raw buffer of {raw_bytes}")
        if not used:
            raise ValueError(f"image {b}: no tile has a non-empty rectangle")


# ------------------------------------------------------------------------------------------------ pixels
_F = np.float32


def hsv_jitter(r, g, b, gains):
    """the HSV gains on float32 arrays r, g, b (0..255): RandomHSV (utils/data_aug.py:363-389) in float arithmetic, H on OpenCV's
    8-bit 0..180 scale, S and V on 0..255, without its uint8 quantisations.  One float32 operation per line of csrc/augment.hip's
    aug_hsv.  Returns the new (r, g, b)."""
    r, g, b = (np.asarray(c, dtype=_F) for c in (r, g, b))
    g0, g1, g2 = (_F(x) for x in gains)
    with np.errstate(divide='ignore', invalid='ignore'):
        V = np.fmax(r, np.fmax(g, b))
        m = np.fmin(r, np.fmin(g, b))
        d = V - m
        S = np.where(V > 0, (_F(255) * d) / V, _F(0)).astype(_F)
        hr = (_F(30) * (g - b)) / d
        hg = _F(60) + (_F(30) * (b - r)) / d
        hb = _F(120) + (_F(30) * (r - g)) / d
        H = np.where(d == 0, _F(0), np.where(V == r, hr, np.where(V == g, hg, hb))).astype(_F)
        H = np.where(H < 0, H + _F(180), H).astype(_F)
        H2 = np.fmod(H * g0, _F(180))
        S2 = np.fmin(S * g1, _F(255))
        V2 = np.fmin(V * g2, _F(255))
        s = S2 / _F(255)
        h6 = H2 / _F(30)
        fi = np.fmin(np.fmax(np.floor(h6), _F(0)), _F(5))
        f = h6 - fi
        p = V2 * (_F(1) - s)
        q = V2 * (_F(1) - s * f)
        t = V2 * (_F(1) - s * (_F(1) - f))
    i = fi.astype(np.int32)
    ro = np.where((i == 0) | (i == 5), V2, np.where(i == 1, q, np.where(i == 4, t, p)))
    go = np.where((i == 1) | (i == 2), V2, np.where(i == 0, t, np.where(i == 3, q, p)))
    bo = np.where((i == 3) | (i == 4), V2, np.where(i == 2, t, np.where(i == 5, q, p)))
    return ro.astype(_F), go.astype(_F), bo.astype(_F)


def _tap(raw, tiles_b, ch, cw, tx, ty, fill_value):
    """(H, W, 3) float32 canvas values at integer canvas positions tx, ty (int64 arrays)"""
    hit = np.zeros(tx.shape, dtype=bool)
    off = np.zeros(tx.shape, dtype=np.int64)
    sel_h = np.zeros(tx.shape, dtype=np.int64)
    sel_w = np.zeros(tx.shape, dtype=np.int64)
    dx = np.zeros(tx.shape, dtype=np.int64)
    dy = np.zeros(tx.shape, dtype=np.int64)
    for t in tiles_b:                                                # later tiles are pasted over earlier ones
        o, sh, sw, sx0, sy0, ox0, oy0, ox1, oy1 = (int(t[n]) for n in TILE_DTYPE.names)
        inside = (tx >= ox0) & (tx < ox1) & (ty >= oy0) & (ty < oy1) & (sh > 0) & (sw > 0)
        sel_h[inside], sel_w[inside], dx[inside], dy[inside], off[inside] = sh, sw, sx0 - ox0, sy0 - oy0, o
        hit |= inside
    hit &= (tx >= 0) & (tx < cw) & (ty >= 0) & (ty < ch)
    sx = np.minimum(np.maximum(dx + tx, 0), sel_w - 1)
    sy = np.minimum(np.maximum(dy + ty, 0), sel_h - 1)
    addr = np.where(hit, off + (sy * sel_w + sx) * 3, 0)
    vals = raw[addr[..., None] + np.arange(3)].astype(_F)
    return np.where(hit[..., None], vals, _F(fill_value))


def augment_batch_host(raw, tiles, canvas_hw, minv, hsv_gain, H, W, fill_value=128):
    """The definition of hipk.augment_batch in NumPy float32 (operation order: module docstring): raw uint8 (n,), tiles TILE_DTYPE
    (B, 4), canvas_hw (B, 2), minv (B, 9), hsv_gain (B, 3) or None -> (B, 3, H, W) float32.  The tables are the caller's
    (validate_tables)."""
    raw = np.asarray(raw, dtype=np.uint8).reshape(-1)
    tiles = np.asarray(tiles)
    if tiles.dtype != TILE_DTYPE:
        tiles = np.ascontiguousarray(tiles).view(TILE_DTYPE).reshape(tiles.shape[0], 4)
    minv = np.asarray(minv, dtype=_F).reshape(-1, 9)
    B = minv.shape[0]
    out = np.empty((B, 3, H, W), dtype=_F)
    xf = np.arange(W, dtype=_F)[None, :]
    yf = np.arange(H, dtype=_F)[:, None]
    for b in range(B):
        m = minv[b]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            nu = (m[0] * xf + m[1] * yf) + m[2]
            nv = (m[3] * xf + m[4] * yf) + m[5]
            w = (m[6] * xf + m[7] * yf) + m[8]
            u, v = nu / w, nv / w
            fu = np.fmin(np.fmax(np.floor(u), _F(-2)), _F(2 ** 30))
            fv = np.fmin(np.fmax(np.floor(v), _F(-2)), _F(2 ** 30))
            ax, ay = (u - fu)[..., None], (v - fv)[..., None]
            bx, by = _F(1) - ax, _F(1) - ay
            tx, ty = fu.astype(np.int64), fv.astype(np.int64)
            ch, cw = int(canvas_hw[b][0]), int(canvas_hw[b][1])
            p00 = _tap(raw, tiles[b], ch, cw, tx, ty, fill_value)
            p01 = _tap(raw, tiles[b], ch, cw, tx + 1, ty, fill_value)
            p10 = _tap(raw, tiles[b], ch, cw, tx, ty + 1, fill_value)
            p11 = _tap(raw, tiles[b], ch, cw, tx + 1, ty + 1, fill_value)
            top = p00 * bx + p01 * ax
            bot = p10 * bx + p11 * ax
            val = top * by + bot * ay
            if hsv_gain is not None:
                val = np.stack(hsv_jitter(val[..., 0], val[..., 1], val[..., 2], hsv_gain[b]), axis=-1)
            out[b] = (val / _F(255)).transpose(2, 0, 1)
    return out


def build_canvas(images, rects, canvas_hw, fill_value=128):
    """the canvas a plan describes, built explicitly (tests and debugging; the kernel never builds it)"""
    canvas = np.full((int(canvas_hw[0]), int(canvas_hw[1]), 3), fill_value, dtype=np.uint8)
    for img, (sx0, sy0, ox0, oy0, ox1, oy1) in zip(images, rects):
        canvas[oy0:oy1, ox0:ox1] = img[sy0:sy0 + (oy1 - oy0), sx0:sx0 + (ox1 - ox0)]
    return canvas
