"""yh_letterbox_batch and everything above it (hipk.letterbox_batch, letter_resize_batch, DeviceLetterboxPrefetcher, the loaders'
device_letterbox switch, the drivers' --device-letterbox) against the host path that stays the default: letter_resize_img +
normal_normalization through fixed_imgsize_collate_fn.  Every comparison is bit equality."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_letterbox_host import SIZES, TARGET, make_items
from yoloseries_amd.dataset import build_dataloader, build_test_dataloader, fixed_imgsize_collate_fn, raw_imgsize_collate_fn
from yoloseries_amd.utils.letterbox import letter_resize_batch, letter_resize_img

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_batch(items, fill_value):
    """fixed_imgsize_collate_fn's image loop with another fill value (the collate itself has no such argument)"""
    from yoloseries_amd.dataset import normal_normalization
    return torch.stack([normal_normalization(letter_resize_img(img, TARGET, fill_value=fill_value)[0]).float() for img, _, _ in items])


@pytest.fixture(scope="module")
def seven():
    items = make_items()
    return items, fixed_imgsize_collate_fn(items, dst_size=TARGET), raw_imgsize_collate_fn(items, dst_size=TARGET)


def run_kernel(raw, dev, fill_value=128):
    from yoloseries_amd import hipk
    t = [raw[k].to(dev) for k in ('raw', 'img_off', 'src_hw', 'rows', 'cols')]
    out = torch.full((t[3].shape[0], 3, t[3].shape[1], t[4].shape[1]), float('nan'), device=dev)
    hipk.letterbox_batch(*t, out, fill_value)
    return out


def test_seven_image_batch(dev, seven):
    _, host, raw = seven
    out = run_kernel(raw, dev)
    assert torch.equal(out.cpu(), host['img'])


@pytest.mark.parametrize("fill_value", [0, 255])
def test_fill_values(dev, seven, fill_value):
    items, host, raw = seven
    want = host_batch(items, fill_value)
    assert not torch.equal(want, host['img'])
    assert torch.equal(run_kernel(raw, dev, fill_value).cpu(), want)


def test_padding_only_image_reads_nothing(dev):
    raw = {'raw': torch.full((1,), 7, dtype=torch.uint8), 'img_off': torch.zeros(1, dtype=torch.int64),
           'src_hw': torch.ones(1, 2, dtype=torch.int32), 'rows': torch.full((1, 64), -1, dtype=torch.int32),
           'cols': torch.full((1, 64), -1, dtype=torch.int32)}
    out = run_kernel(raw, dev, 128)
    assert torch.equal(out.cpu(), torch.full((1, 3, 64, 64), np.float32(128 / 255.0).item()))
    raw['raw'] = torch.full((3,), 7, dtype=torch.uint8)     # one pixel
    raw['rows'][0, 5] = 0                                   # a body row whose columns are all border: still only the fill value
    assert torch.equal(run_kernel(raw, dev, 128).cpu(), torch.full((1, 3, 64, 64), np.float32(128 / 255.0).item()))


def test_more_rows_than_one_grid_pass(dev):
    # one workgroup per output row (b, y), at most LB_GRID_CAP = 2048 workgroups per launch (csrc/preproc.hip): the grid-stride loop
    # runs a second time once B * H > 2048.  The letterbox target is a multiple of 64, so H = W = 64 is the smallest plane and
    # B = 33 (2112 rows) the smallest batch past the cap; workgroups 0..63 then own two rows each, of different images.
    rs = np.random.RandomState(11)
    items = [(rs.randint(0, 256, size=(8, 8, 3), dtype=np.uint8), {'bboxes': np.array([[1., 1., 5., 6.]], np.float32), 'classes': [1]}, i)
             for i in range(33)]
    assert len(items) * 64 > 2048 >= (len(items) - 1) * 64
    host = fixed_imgsize_collate_fn(items, dst_size=[64, 64])
    out = run_kernel(raw_imgsize_collate_fn(items, dst_size=[64, 64]), dev)
    assert torch.equal(out.cpu(), host['img'])


def test_non_default_stream(dev, seven):
    _, host, raw = seven
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        out = run_kernel(raw, dev)
    side.synchronize()
    assert torch.equal(out.cpu(), host['img'])


def test_letter_resize_batch(dev, seven):
    items, host, _ = seven
    out, records = letter_resize_batch([img for img, _, _ in items], TARGET, device=dev)
    assert out.device == dev and out.dtype == torch.float32 and tuple(out.shape) == (len(SIZES), 3, 64, 128)
    assert torch.equal(out.cpu(), host['img']) and records == host['resize_info']


def _three_batches(prefetcher, keys):
    got = []
    for _ in range(3):
        x = prefetcher.next()
        assert x['img'] is not None and x['img'].is_cuda
        got.append({k: x[k] for k in keys})
    torch.cuda.synchronize()
    return got


def test_loader_path(dev):
    args = dict(img_dir='synthetic', lab_dir=None, name_path=None, input_dim=[64, 64], aug_hyp=None, cache_num=0, enable_data_aug=False,
                seed=3, batch_size=4, num_workers=0, pin_memory=True, shuffle=False, drop_last=True)
    keys = ('img', 'ann', 'resize_info', 'img_id')
    host = _three_batches(build_dataloader(**args, device_letterbox=False)[2], keys)
    devb = _three_batches(build_dataloader(**args, device_letterbox=True)[2], keys)
    for h, d in zip(host, devb):
        assert d['img'].dtype == torch.float32 and torch.equal(h['img'], d['img']) and torch.equal(h['ann'], d['ann'])
        assert h['resize_info'] == d['resize_info'] and h['img_id'] == d['img_id']
    assert len({b['img'].data_ptr() for b in devb}) == 3                       # a fresh output per batch ...
    for h, d in zip(host, devb):                                               # ... that later batches did not write over
        assert torch.equal(h['img'], d['img'])
    assert not torch.equal(devb[0]['img'], devb[1]['img'])


def test_test_loader_path(dev):
    keys = ('img', 'resize_info')
    host = _three_batches(build_test_dataloader('synthetic', [64, 64], batch_size=4, device_letterbox=False)[2], keys)
    devb = _three_batches(build_test_dataloader('synthetic', [64, 64], batch_size=4, device_letterbox=True)[2], keys)
    for h, d in zip(host, devb):
        assert torch.equal(h['img'], d['img']) and h['resize_info'] == d['resize_info']
    assert len({b['img'].data_ptr() for b in devb}) == 3
    for h, d in zip(host, devb):
        assert torch.equal(h['img'], d['img'])


def _driver(args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train_yolov5.py")] + args, cwd=cwd, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=300)


def test_driver_device_letterbox(dev, tmp_path):
    """The first step's loss depends on the ingest path alone (the batch and the initial weights): it must be finite.  Later steps
    at 64 x 64 may print nan on either ingest path: the coarsest stage is a 2 x 2 map, and the class loss of a stage that no target
    was assigned to is the mean of an empty tensor, nan as in the reference (csrc/loss_v5.hip, v5_finalize_kernel)."""
    r = _driver(["--data", "dataset", "--device-letterbox", "--img", "64", "--batch", "4", "--epochs", "1", "--steps-per-epoch", "2"], tmp_path)
    assert r.returncode == 0, r.stdout[-3000:]
    losses = [float(v) for v in re.findall(r"step \d+/2 tot (\S+)", r.stdout)]
    assert len(losses) == 2 and math.isfinite(losses[0]), r.stdout[-3000:]


def test_driver_rejects_device_letterbox_without_images(dev, tmp_path):
    r = _driver(["--data", "tensor", "--device-letterbox", "--img", "64", "--batch", "4", "--epochs", "1", "--steps-per-epoch", "2"], tmp_path)
    assert r.returncode != 0 and "--device-letterbox needs --data dataset" in r.stdout, r.stdout[-3000:]
