"""Batch assembly — the tensor format between a dataset and the hot path, as the reference's
dataset/data_collater.py:16-82 produces it:

    'img'          (B, 3, H, W) float32 in [0, 1], channel order as loaded
    'ann'          (B, maxbox, 6) float32 rows [xmin, ymin, xmax, ymax, cls, index of the image in the batch], -1 padded
    'resize_info'  one letterbox record per image (utils/letterbox.py)
    'img_id'       the dataset's ids

`YOLOV5Loss` / `YOLOXLoss` and the evaluators of this package consume exactly this (loss/yolov5_loss.py:30-60)."""
import numpy as np
import torch

from ..utils.letterbox import letter_resize_bbox, letter_resize_img, pack_raw_batch

__all__ = ['fixed_imgsize_collate_fn', 'test_dataset_collate_fn', 'normal_normalization', 'raw_imgsize_collate_fn',
           'raw_test_collate_fn', 'augment_collate_fn']


def normal_normalization(img):
    """uint8 HWC image -> CHW tensor scaled to [0, 1] (float64 like the reference; the batch tensor is float32)"""
    return torch.from_numpy(img / 255.0).permute(2, 0, 1).contiguous()


def _annotation_rows(ann, info, index):
    """(n, 6) float32 rows of one image, boxes moved into the letterboxed frame"""
    n = len(ann['classes'])
    if len(ann['bboxes']) != n:
        raise AssertionError("every box needs a class")
    rows = torch.empty(n, 6)
    if n:
        rows[:, :4] = torch.from_numpy(np.asarray(letter_resize_bbox(ann['bboxes'], info), dtype=np.float64)).float()
        rows[:, 4] = torch.as_tensor([float(c) for c in ann['classes']])
        rows[:, 5] = float(index)
    return rows


def fixed_imgsize_collate_fn(data_in, dst_size):
    """data_in: sequence of (image (h,w,3) uint8, {'bboxes': (n,4) xyxy, 'classes': n}, image id); dst_size: [h, w]"""
    first = data_in[0][0]
    assert first.ndim == 3 and first.shape[-1] == 3, f"data's formate should be (h, w, 3), but got {first.shape}"
    batch = torch.zeros(len(data_in), 3, dst_size[0], dst_size[1])
    infos, rows, ids = [], [], []
    for index, (img, ann, img_id) in enumerate(data_in):
        boxed, info = letter_resize_img(img, dst_size)
        batch[index] = normal_normalization(boxed)
        infos.append(info)
        rows.append(_annotation_rows(ann, info, index))
        ids.append(img_id)
    return {'img': batch, 'ann': _padded_annotations(rows), 'resize_info': infos, 'img_id': ids}


def _padded_annotations(rows):
    """per-image (n, 6) rows -> (B, maxbox, 6)"""
    ann_out = torch.full((len(rows), max(len(r) for r in rows), 6), -1.0)      # -1 rows = padding
    for index, r in enumerate(rows):
        ann_out[index, :len(r)] = r
    return ann_out


def _raw_batch(images, dst_size):
    raw, img_off, src_hw, rows, cols, infos = pack_raw_batch(images, dst_size)
    return {'raw': torch.from_numpy(raw), 'img_off': torch.from_numpy(img_off), 'src_hw': torch.from_numpy(src_hw),
            'rows': torch.from_numpy(rows), 'cols': torch.from_numpy(cols)}, infos


def raw_imgsize_collate_fn(data_in, dst_size):
    """fixed_imgsize_collate_fn for the device letterbox (DeviceLetterboxPrefetcher): the same items in, but the images leave
    the worker as they are, uint8 and concatenated ('raw', 'img_off', 'src_hw'), with the letterbox as index tables ('rows', 'cols':
    utils/letterbox.py letterbox_tables); 'ann', 'resize_info' and 'img_id' are those of fixed_imgsize_collate_fn."""
    first = data_in[0][0]
    assert first.ndim == 3 and first.shape[-1] == 3, f"data's formate should be (h, w, 3), but got {first.shape}"
    batch, infos = _raw_batch([item[0] for item in data_in], dst_size)
    rows = [_annotation_rows(ann, info, index) for index, ((_, ann, _), info) in enumerate(zip(data_in, infos))]
    batch.update(ann=_padded_annotations(rows), resize_info=infos, img_id=[item[2] for item in data_in])
    return batch


def test_dataset_collate_fn(data_in):
    """items: (already letterboxed (3,h,w) tensor, letterbox record)"""
    img = torch.stack([item[0].to(torch.float32) for item in data_in])
    return {'img': img, 'resize_info': [item[1] for item in data_in]}


def raw_test_collate_fn(data_in, dst_size):
    """items: (h, w, 3) uint8 images as the dataset holds them -> the raw batch of raw_imgsize_collate_fn without annotations"""
    batch, infos = _raw_batch(list(data_in), dst_size)
    batch['resize_info'] = infos
    return batch


def _box_rows(boxes, classes, index):
    """(n, 6) float32 rows of one image from boxes that are already in the network input's frame"""
    n = len(classes)
    rows = torch.empty(n, 6)
    if n:
        rows[:, :4] = torch.from_numpy(np.asarray(boxes, dtype=np.float64).reshape(n, 4)).float()
        rows[:, 4] = torch.as_tensor([float(c) for c in classes])
        rows[:, 5] = float(index)
    return rows


def augment_collate_fn(data_in, dst_size):
    """collate of AugmentedDataset (dataset/augmented.py) for DeviceAugmentPrefetcher.  Items: ([raw uint8 images], plan, labels in
    the output frame, id), or the plain (image, annotation, id) of an un-augmented item, which becomes the letterbox as a plan
    (utils/augment.py identity_plan), so one kernel serves the batch.  Out: the images concatenated ('raw') and the plan tables
    ('tiles' as bytes (B, 4, 40), 'canvas_hw', 'minv', 'hsv_gain' or None), checked here (ValueError naming the image, before
    anything is copied); 'ann', 'resize_info' and 'img_id' as fixed_imgsize_collate_fn builds them."""
    from ..utils import augment as A
    from ..utils.letterbox import letter_resize_bbox
    plans, images, rows, infos, ids = [], [], [], [], []
    for index, item in enumerate(data_in):
        if len(item) == 4:
            imgs, plan, ann, img_id = item
            if tuple(plan['dst_hw']) != (int(dst_size[0]), int(dst_size[1])):
                raise ValueError(f"image {index}: the plan was drawn for {plan['dst_hw']}, the batch is {list(dst_size)}")
            rows.append(_box_rows(ann['bboxes'], ann['classes'], index))
            infos.append({'augmented': True, 'M': plan['M_total'], 'org_shape': tuple(imgs[0].shape[:2])})
        else:
            img, ann, img_id = item
            imgs, plan = [img], A.identity_plan(index, img.shape[:2], dst_size)
            rows.append(_annotation_rows(ann, plan['record'], index))
            infos.append(plan['record'])
        plans.append(plan); images.append(imgs); ids.append(img_id)
    raw, tiles, canvas_hw, minv, gains = A.plan_tables(plans, images)
    return {'raw': torch.from_numpy(raw), 'tiles': torch.from_numpy(tiles.view(np.uint8).reshape(len(plans), 4, A.TILE_DTYPE.itemsize)),
            'canvas_hw': torch.from_numpy(canvas_hw), 'minv': torch.from_numpy(minv),
            'hsv_gain': None if gains is None else torch.from_numpy(gains), 'dst_size': (int(dst_size[0]), int(dst_size[1])),
            'ann': _padded_annotations(rows), 'resize_info': infos, 'img_id': ids}
