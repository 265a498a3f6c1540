"""Host side of the device letterbox (no GPU needed): the index tables of utils/letterbox.py letterbox_tables and the raw batch
of dataset/data_collater.py raw_imgsize_collate_fn, pushed through a NumPy emulation of yh_letterbox_batch's definition
(include/yolohip.h), reproduce fixed_imgsize_collate_fn bit for bit; and the C entry rejects bad arguments before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch

from yoloseries_amd.dataset import fixed_imgsize_collate_fn, raw_imgsize_collate_fn, raw_test_collate_fn
from yoloseries_amd.utils.letterbox import letter_resize_img, letterbox_tables

# 7x13: up-scale, the next image starts at byte 273 | 333x500: non-integer ratio | 64x128: scale exactly 1 | 700x20: tall, the odd
# slack puts the extra border pixel on the right | 65x129: just over the target | 1x1 | 18x26: floor(i * (src / dst)) in float64
# differs from (i * src) // dst
SIZES = [(7, 13), (333, 500), (64, 128), (700, 20), (65, 129), (1, 1), (18, 26)]
TARGET = [64, 128]


def make_items(sizes=SIZES, seed=3):
    rs = np.random.RandomState(seed)
    items = []
    for i, (h, w) in enumerate(sizes):
        img = rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8)
        n = i % 3                                           # images without boxes too
        x0, y0 = rs.uniform(0, w / 2, n), rs.uniform(0, h / 2, n)
        boxes = np.stack([x0, y0, x0 + rs.uniform(0.5, w / 2, n), y0 + rs.uniform(0.5, h / 2, n)], 1).astype(np.float32).reshape(n, 4)
        items.append((img, {'bboxes': boxes, 'classes': rs.randint(0, 80, n).tolist()}, 100 + i))
    items[1][1]['bboxes'] = np.array([[3., 4., 200., 300.]], np.float32); items[1][1]['classes'] = [5]      # at least one box in the batch
    return items


def emulate_kernel(batch, fill_value):
    """out[b][c][y][x] = float32(v) / float32(255), v = raw[img_off[b] + (rows[b][y] * src_w + cols[b][x]) * 3 + c] or fill_value"""
    raw, img_off, src_hw = batch['raw'].numpy(), batch['img_off'].numpy(), batch['src_hw'].numpy()
    rows, cols = batch['rows'].numpy(), batch['cols'].numpy()
    B, H, W = rows.shape[0], rows.shape[1], cols.shape[1]
    out = np.empty((B, 3, H, W), np.float32)
    for b in range(B):
        border = (rows[b][:, None] < 0) | (cols[b][None, :] < 0)
        pix = (np.maximum(rows[b], 0).astype(np.int64)[:, None] * src_hw[b, 1] + np.maximum(cols[b], 0)[None, :]) * 3 + img_off[b]
        for c in range(3):
            v = np.where(border, np.uint8(fill_value), raw[np.where(border, 0, pix + c)])
            out[b, c] = v.astype(np.float32) / np.float32(255.0)
    return torch.from_numpy(out)


def test_raw_collate_reproduces_the_host_batch():
    items = make_items()
    host = fixed_imgsize_collate_fn(items, dst_size=TARGET)
    raw = raw_imgsize_collate_fn(items, dst_size=TARGET)
    assert sorted(raw) == sorted(['raw', 'img_off', 'src_hw', 'rows', 'cols', 'ann', 'resize_info', 'img_id'])
    B = len(items)
    assert raw['raw'].dtype == torch.uint8 and raw['raw'].shape == (sum(h * w * 3 for h, w in SIZES),)
    assert raw['img_off'].dtype == torch.int64 and raw['img_off'].shape == (B,) and raw['img_off'][1].item() == 273
    assert raw['src_hw'].dtype == torch.int32 and raw['src_hw'].tolist() == [list(s) for s in SIZES]
    assert raw['rows'].dtype == torch.int32 and raw['rows'].shape == (B, 64)
    assert raw['cols'].dtype == torch.int32 and raw['cols'].shape == (B, 128)
    assert all(torch.is_tensor(v) or isinstance(v, list) for v in raw.values())            # what pin_memory=True can pin
    assert (raw['rows'][2] >= 0).all() and (raw['cols'][2] >= 0).all()                   # 64x128: no border
    assert (raw['cols'][3] >= 0).sum().item() == 1 and raw['cols'][3][63].item() == 0    # 700x20 -> 64x1 body, 63 left / 64 right
    got = emulate_kernel(raw, 128)
    assert got.dtype == host['img'].dtype and torch.equal(got, host['img'])
    assert torch.equal(raw['ann'], host['ann'])
    assert raw['resize_info'] == host['resize_info'] and raw['img_id'] == host['img_id']


def test_float64_index_rule_is_what_the_tables_hold():
    """18x26 into 64x128 (body 64x92): the integer rule gives other columns, so the table cannot come from (i * src) // dst"""
    rows, cols, _ = letterbox_tables((18, 26), TARGET)
    body = cols[cols >= 0]
    assert len(body) == 92 and (rows >= 0).all()
    assert (body != (np.arange(92) * 26) // 92).any()


def test_scale_is_the_correctly_rounded_fp32_quotient():
    v = np.arange(256)
    want = (v / 255.0).astype(np.float32)                  # normal_normalization: float64 division, float32 batch
    assert np.array_equal(want, v.astype(np.float32) / np.float32(255.0))
    assert np.array_equal(want, (torch.arange(256).float() / 255.0).numpy())            # the test loader's own scale (_ImagesOnly)
    assert (want != v.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))).sum() == 126


def test_tables_inference_form():
    img = np.random.RandomState(0).randint(0, 256, size=(333, 500, 3), dtype=np.uint8)
    want, info = letter_resize_img(img, TARGET, training=False)
    rows, cols, record = letterbox_tables((333, 500), TARGET, training=False)
    assert record == info and (len(rows), len(cols)) == want.shape[:2]
    got = np.where(((rows < 0)[:, None] | (cols < 0)[None, :])[..., None], np.uint8(128), img[np.maximum(rows, 0)][:, np.maximum(cols, 0)])
    assert np.array_equal(got, want)


def test_zero_pixel_body_raises():
    with pytest.raises(ValueError, match="200x3"):
        letterbox_tables((200, 3), TARGET)
    with pytest.raises(ValueError):
        raw_imgsize_collate_fn([(np.zeros((200, 3, 3), np.uint8), {'bboxes': np.zeros((0, 4), np.float32), 'classes': []}, 0)], dst_size=TARGET)


def test_target_rounds_up_to_the_stride():
    img = np.random.RandomState(1).randint(0, 256, size=(65, 129, 3), dtype=np.uint8)
    want, info = letter_resize_img(img, [64, 96])
    assert want.shape == (64, 128, 3)
    rows, cols, record = letterbox_tables((65, 129), [64, 96])
    assert (len(rows), len(cols)) == (64, 128) and record == info
    batch = raw_test_collate_fn([img], dst_size=[64, 96])
    assert sorted(batch) == sorted(['raw', 'img_off', 'src_hw', 'rows', 'cols', 'resize_info']) and batch['resize_info'] == [info]
    assert torch.equal(emulate_kernel(batch, 128)[0], torch.from_numpy((want / 255.0).astype(np.float32)).permute(2, 0, 1))


def test_c_abi_rejects_bad_arguments_before_any_launch():
    from yoloseries_amd import _lib
    L = _lib.lib()
    assert "yh_letterbox_batch" in _lib.EXPORTED_SYMBOLS
    buf = (C.c_uint8 * 4096)()                               # stands in for every pointer: no call below reaches a launch
    p = C.c_void_p((C.addressof(buf) + 63) // 64 * 64)

    def call(raw=p, B=1, W=8, fill=128):
        return L.yh_letterbox_batch(raw, p, p, p, p, B, 8, W, fill, p, None)

    for what, kw in (("null", dict(raw=None)), ("positive", dict(B=0)), ("multiple of 4", dict(W=6)), ("fill_value", dict(fill=256))):
        assert call(**kw) == -1, what                        # YH_EINVAL
        msg = L.yh_last_error().decode()
        assert "yh_letterbox_batch" in msg and what in msg, (what, msg)
