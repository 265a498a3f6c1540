"""Letterbox geometry: the transform between a dataset image and the (3, H, W) network input, and its record
(`scale`, `pad_top/left/bottom/right`, `org_shape`) that the evaluators use to map predictions back.  Behaviour of the
reference's utils/data_aug.py:21-70 (letter_resize_img) and utils/bbox_tools.py:38-49 (letter_resize_bbox).

The reference resizes with OpenCV (`cv2.resize(..., interpolation=0)`, INTER_NEAREST) and pads with
`cv2.copyMakeBorder`; OpenCV is not a dependency here: nearest sampling is restated from its index rule
``src = min(floor(dst * src_size / dst_size), src_size - 1)`` and the border is a constant fill."""
import numpy as np

__all__ = ['letter_resize_img', 'letter_resize_bbox', 'resize_nearest', 'letterbox_tables', 'pack_raw_batch', 'letter_resize_batch']


def _nearest_index(src, dst):
    """source index of each of `dst` output positions along an axis of `src` pixels (float64: not `(i * src) // dst`)"""
    return np.minimum(np.floor(np.arange(dst) * (src / dst)).astype(np.int64), src - 1)


def resize_nearest(img, resize_w, resize_h):
    """nearest-neighbour resize with OpenCV's INTER_NEAREST index rule"""
    h, w = img.shape[:2]
    ys = _nearest_index(h, resize_h)
    xs = _nearest_index(w, resize_w)
    return img[ys][:, xs]


def _round_up(v, stride):
    rem = int(np.remainder(v, stride))
    return int(v + (stride - rem if rem > 0 else 0))


def _letterbox_geometry(src_hw, dst_size, stride, only_ds, training):
    """the scale / padding arithmetic of the letterbox: ((new_h, new_w) of the resized body, (out_h, out_w) of the canvas, record)"""
    target = [dst_size, dst_size] if isinstance(dst_size, int) else list(dst_size)
    target = [_round_up(target[0], stride), _round_up(target[1], stride)]
    src_h, src_w = int(src_hw[0]), int(src_hw[1])
    scale = float(np.min([target[0] / src_h, target[1] / src_w]))
    if only_ds:
        scale = min(scale, 1.0)
    if scale != 1.:
        new_h, new_w = int(src_h * scale), int(src_w * scale)
    else:
        new_h, new_w = src_h, src_w
    slack_h, slack_w = target[0] - new_h, target[1] - new_w
    if training:
        top, left = slack_h // 2, slack_w // 2
        out_h, out_w = target
    else:
        slack_h, slack_w = int(np.remainder(slack_h, stride)), int(np.remainder(slack_w, stride))
        top, left = int(round(slack_h / 2)), int(round(slack_w / 2))
        out_h, out_w = new_h + slack_h, new_w + slack_w
    bottom, right = slack_h - top, slack_w - left
    record = {'scale': scale, 'pad_top': top, 'pad_left': left, 'pad_bottom': bottom, 'pad_right': right,
              'org_shape': (src_h, src_w)}
    return (new_h, new_w), (out_h, out_w), record


def letter_resize_img(img, dst_size, stride=64, fill_value=128, only_ds=False, training=True):
    """Scale `img` (h, w, 3) uint8 by one factor so that it fits `dst_size` (int or [h, w], rounded up to a multiple of
    `stride`) and pad with `fill_value`.

    training=True: the output always has the full target size (batches need one shape), padding split evenly, the odd
    pixel at the bottom / right.  training=False: only as much padding as the next multiple of `stride` needs.
    only_ds=True never enlarges.  Returns (uint8 image, record dict)."""
    src_h, src_w = img.shape[:2]
    (new_h, new_w), (out_h, out_w), record = _letterbox_geometry((src_h, src_w), dst_size, stride, only_ds, training)
    body = resize_nearest(img, new_w, new_h) if record['scale'] != 1. else img
    top, left = record['pad_top'], record['pad_left']
    canvas = np.empty((out_h, out_w, 3), dtype=np.uint8)
    canvas[...] = np.asarray(fill_value, dtype=np.int64).astype(np.uint8)
    canvas[top:top + new_h, left:left + new_w] = body
    return canvas, record


def letter_resize_bbox(bboxes, letter_info):
    """xyxy boxes of the original image -> of the letterboxed image"""
    boxes = np.asarray(bboxes) * letter_info['scale']
    boxes[:, [0, 2]] += letter_info['pad_left']
    boxes[:, [1, 3]] += letter_info['pad_top']
    return boxes


def letterbox_tables(src_hw, dst_size, stride=64, only_ds=False, training=True):
    """The letterbox of a (src_h, src_w) image as index tables: `rows` int32 (H,) and `cols` int32 (W,) hold the source row /
    column of every output row / column of `letter_resize_img(img, dst_size, stride, ..., only_ds, training)`, -1 on the border, so
    that  out[y, x] = img[rows[y], cols[x]]  (or the fill value).  Returns (rows, cols, record), the record being the same dict.
    A source so thin that its resized body has a side of 0 pixels raises ValueError."""
    src_h, src_w = int(src_hw[0]), int(src_hw[1])
    (new_h, new_w), (out_h, out_w), record = _letterbox_geometry((src_h, src_w), dst_size, stride, only_ds, training)
    if new_h < 1 or new_w < 1:
        raise ValueError(f"letterbox of a {src_h}x{src_w} image into {dst_size}: the resized body would be {new_h}x{new_w} pixels")
    resized = record['scale'] != 1.
    rows = np.full(out_h, -1, dtype=np.int32)
    cols = np.full(out_w, -1, dtype=np.int32)
    top, left = record['pad_top'], record['pad_left']
    rows[top:top + new_h] = _nearest_index(src_h, new_h) if resized else np.arange(src_h)
    cols[left:left + new_w] = _nearest_index(src_w, new_w) if resized else np.arange(src_w)
    return rows, cols, record


def pack_raw_batch(images, dst_size):
    """A list of (h, w, 3) uint8 images -> what the device letterbox (hipk.letterbox_batch) reads, as NumPy arrays:
    raw uint8 (sum of h*w*3,) the images concatenated, img_off int64 (B,) their byte offsets, src_hw int32 (B, 2),
    rows int32 (B, H), cols int32 (B, W) (letterbox_tables, training form: every image gets the full target), and the records."""
    if len(images) == 0:
        raise ValueError("pack_raw_batch: empty batch")
    flat, offs, hw, rows, cols, records = [], [], [], [], [], []
    pos = 0
    for img in images:
        img = np.asarray(img)
        if img.ndim != 3 or img.shape[-1] != 3 or img.dtype != np.uint8:
            raise ValueError(f"pack_raw_batch: images are (h, w, 3) uint8 arrays, got {img.dtype} {img.shape}")
        r, c, record = letterbox_tables(img.shape[:2], dst_size)
        flat.append(np.ascontiguousarray(img).reshape(-1))
        offs.append(pos)
        pos += flat[-1].size
        hw.append(img.shape[:2])
        rows.append(r); cols.append(c); records.append(record)
    return (np.concatenate(flat), np.asarray(offs, dtype=np.int64), np.asarray(hw, dtype=np.int32).reshape(-1, 2),
            np.stack(rows), np.stack(cols), records)


def letter_resize_batch(images, dst_size, fill_value=128, device=None):
    """`letter_resize_img` + `normal_normalization` of a list of (h, w, 3) uint8 arrays in one kernel launch on the GPU:
    returns ((B, 3, H, W) float32 tensor on `device`, [records]), bit-identical to the host functions."""
    import torch
    from .. import hipk
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    *tables, records = pack_raw_batch(images, dst_size)
    with torch.cuda.device(device):
        raw, img_off, src_hw, rows, cols = (torch.from_numpy(t).to(device) for t in tables)
        out = torch.empty(len(images), 3, rows.shape[1], cols.shape[1], dtype=torch.float32, device=device)
        hipk.letterbox_batch(raw, img_off, src_hw, rows, cols, out, fill_value)
    return out, records
