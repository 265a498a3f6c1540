"""yh_augment_batch and everything above it (hipk.augment_batch, DeviceAugmentPrefetcher, the drivers' --augment) against the NumPy
statement of the same computation, utils/augment.py augment_batch_host: bit equality for the geometry and the interpolation, the
colorsys bound of tests/test_augment_host.py for the HSV jitter."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_augment_host import CASES, DST, FILL, G, HSV_BOUND, HYP, MOSAIC_CASES, TinyDataset, _hsv_colorsys, case_plan
from yoloseries_amd.utils import augment as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plans():
    return {name: case_plan(name) for name in CASES}


def tables_of(plans, names):
    return A.plan_tables([plans[n][0] for n in names], [[i[0] for i in plans[n][1]] for n in names])


def run_kernel(dev, raw, tiles, canvas_hw, minv, gains, H, W, fill_value=FILL):
    from yoloseries_amd import hipk
    t = [torch.from_numpy(np.ascontiguousarray(raw)).to(dev),
         torch.from_numpy(tiles.view(np.uint8).reshape(tiles.shape[0], 4, 40)).to(dev),
         torch.from_numpy(canvas_hw).to(dev), torch.from_numpy(np.ascontiguousarray(minv, dtype=np.float32).reshape(-1, 9)).to(dev),
         None if gains is None else torch.from_numpy(np.ascontiguousarray(gains, dtype=np.float32)).to(dev)]
    out = torch.full((tiles.shape[0], 3, H, W), float('nan'), device=dev)
    hipk.augment_batch(*t, out, fill_value)
    return out.cpu().numpy()


def assert_bits_equal(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} values differ, largest difference {np.abs(got - want).max():.3e}"


def _batches(plans):
    """name -> (plan names, H, W): every launch shape and matrix kind of the kernel"""
    single_variants = ["single"] * 3
    return {
        "fixture_3x64x64": (MOSAIC_CASES, DST, DST),                  # affine + fliplr, perspective + flipud, scale only
        "lane_tail_64x68": (MOSAIC_CASES[:2], DST, DST + 4),          # 17 lanes: not a whole wave
        "single_tile": (single_variants, DST, DST),                   # perspective and both flips on a one-tile canvas
        "mixed_1_and_4_tiles": (["single", "mosaic_affine", "single", "mosaic_persp"], DST, DST),
    }


@pytest.mark.parametrize("batch", ["fixture_3x64x64", "lane_tail_64x68", "single_tile", "mixed_1_and_4_tiles"])
def test_kernel_equals_the_numpy_statement(dev, plans, batch):
    names, H, W = _batches(plans)[batch]
    raw, tiles, canvas_hw, minv, _ = tables_of(plans, names)
    minv = minv.copy()
    for b in range(1, len(names)):                                    # repeated plans get different sampling positions
        minv[b, 2] += np.float32(0.37 * b)
        minv[b, 5] -= np.float32(0.21 * b)
    want = A.augment_batch_host(raw, tiles, canvas_hw, minv, None, H, W, FILL)
    assert np.abs(want - np.float32(FILL / 255)).max() > 0.1
    assert_bits_equal(run_kernel(dev, raw, tiles, canvas_hw, minv, None, H, W), want)


def test_more_rows_than_one_grid_pass(dev, plans):
    """one workgroup per output row (b, y), at most AUG_GRID_CAP = 2048 per launch (csrc/augment.hip): B = 40 at 64 x 64 is 2560 rows,
    so workgroups 0..511 own two rows each, of different images"""
    names = (MOSAIC_CASES + ["single"]) * 10
    assert len(names) * DST > 2048
    raw, tiles, canvas_hw, minv, _ = tables_of(plans, names)
    minv = minv.copy()
    minv[:, 2] += (np.arange(len(names)) * 0.13).astype(np.float32)
    want = A.augment_batch_host(raw, tiles, canvas_hw, minv, None, DST, DST, FILL)
    assert_bits_equal(run_kernel(dev, raw, tiles, canvas_hw, minv, None, DST, DST), want)


@pytest.mark.parametrize("name", MOSAIC_CASES)
def test_identity_matrix_is_the_reference_canvas(dev, plans, name):
    raw, tiles, canvas_hw, _, _ = tables_of(plans, [name])
    out = run_kernel(dev, raw, tiles, canvas_hw, np.eye(3, dtype=np.float32).reshape(1, 9), None, 2 * DST, 2 * DST)
    assert_bits_equal(out[0], np.ascontiguousarray((G[f"{name}_canvas"].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)))


GAINS = np.array([[1.015, 1.7, 1.4], [0.985, 0.3, 0.6], [1.0, 1.0, 1.0]], dtype=np.float32)


def test_hsv_within_the_colorsys_bound(dev, plans):
    """the kernel's HSV jitter against colorsys (float64) applied to the blended pixel (the NumPy statement with HSV off, which the
    kernel equals bit for bit), within the bound of test_augment_host.test_hsv_against_colorsys"""
    raw, tiles, canvas_hw, minv, _ = tables_of(plans, MOSAIC_CASES)
    got = run_kernel(dev, raw, tiles, canvas_hw, minv, GAINS, DST, DST).astype(np.float64)
    plain = A.augment_batch_host(raw, tiles, canvas_hw, minv, None, DST, DST, FILL).astype(np.float64) * 255.0
    ref = np.empty_like(plain)
    for b in range(plain.shape[0]):
        for y in range(DST):
            for x in range(DST):
                ref[b, :, y, x] = _hsv_colorsys(plain[b, 0, y, x], plain[b, 1, y, x], plain[b, 2, y, x], [float(g) for g in GAINS[b]])
    err = np.abs(got - ref).max()
    print(f"kernel HSV against colorsys: max err {err:.3e} (bound {HSV_BOUND:.3e})")
    # `plain` went through / 255 and * 255: one more float32 rounding of the input colour (2^-24 relative), inside the bound's factor 4
    assert err <= HSV_BOUND


def test_hsv_equals_the_numpy_statement(dev, plans):
    raw, tiles, canvas_hw, minv, _ = tables_of(plans, MOSAIC_CASES)
    want = A.augment_batch_host(raw, tiles, canvas_hw, minv, GAINS, DST, DST, FILL)
    assert_bits_equal(run_kernel(dev, raw, tiles, canvas_hw, minv, GAINS, DST, DST), want)


def test_bad_arguments_launch_nothing(dev, plans):
    from yoloseries_amd import _lib
    raw, tiles, canvas_hw, minv, _ = tables_of(plans, MOSAIC_CASES[:1])
    t_raw = torch.from_numpy(raw).to(dev)
    t_tiles = torch.from_numpy(tiles.view(np.uint8).reshape(1, 4, 40)).to(dev)
    t_hw, t_minv = torch.from_numpy(canvas_hw).to(dev), torch.from_numpy(minv).to(dev)
    buf = torch.full((3 * 64 * 72 + 8,), float('nan'), device=dev)
    L, st = _lib.lib(), _lib.stream_ptr()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)               # noqa: E731

    def call(raw=t_raw, tiles=t_tiles, hw=t_hw, minv=t_minv, W=64, fill=128, out_off=0):
        return L.yh_augment_batch(None if raw is None else p(raw), None if tiles is None else p(tiles), None if hw is None else p(hw),
                                  None if minv is None else p(minv), None, 1, 64, W, fill, p(buf, out_off), st)

    YH_EINVAL = -1
    assert call(W=70) == YH_EINVAL and b"multiple of 4" in L.yh_last_error()
    assert call(out_off=4) == YH_EINVAL and b"aligned" in L.yh_last_error()
    assert call(fill=256) == YH_EINVAL and b"not a byte" in L.yh_last_error()
    assert call(tiles=None) == YH_EINVAL and call(hw=None) == YH_EINVAL and call(minv=None) == YH_EINVAL and call(raw=None) == YH_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()                                     # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(buf[:3 * 64 * 64]).any() and torch.isnan(buf[3 * 64 * 64:]).all()


def test_device_augment_prefetcher(dev):
    from torch.utils.data import DataLoader
    from functools import partial
    from yoloseries_amd.dataset import AugmentedDataset, DeviceAugmentPrefetcher, augment_collate_fn

    def loader():
        ds = AugmentedDataset(TinyDataset(), [64, 64], HYP, seed=9)
        return DataLoader(ds, batch_size=4, shuffle=False, drop_last=True, num_workers=0, collate_fn=partial(augment_collate_fn, dst_size=[64, 64]))

    host = list(loader())[:2]
    pf = DeviceAugmentPrefetcher(loader(), fill_value=114)
    got = []
    for _ in range(2):
        x = pf.next()
        assert x['img'].is_cuda and x['ann'].is_cuda and x['img'].dtype == torch.float32
        total = x['img'].sum()                                        # consumed on this stream without a synchronize
        got.append((x, float(total)))
    torch.cuda.synchronize()
    assert got[0][0]['img'].data_ptr() != got[1][0]['img'].data_ptr()              # a fresh output per batch
    seen_hsv = False
    for (x, total), h in zip(got, host):
        gains = None if h['hsv_gain'] is None else h['hsv_gain'].numpy()
        seen_hsv |= gains is not None
        want = A.augment_batch_host(h['raw'].numpy(), h['tiles'].numpy(), h['canvas_hw'].numpy(), h['minv'].numpy(), gains, 64, 64, 114)
        img = x['img'].cpu().numpy()
        assert tuple(img.shape) == (4, 3, 64, 64)
        assert_bits_equal(img, want)
        assert abs(total - float(want.astype(np.float64).sum())) <= 0.05          # a float32 sum of 49152 values in [0, 1]
        assert torch.equal(x['ann'].cpu(), h['ann']) and x['img_id'] == h['img_id']
        ann = h['ann']
        assert ann.shape[0] == 4 and ann.shape[2] == 6 and (ann[ann[:, :, 4] < 0] == -1).all() and (ann[:, :, 4] < 0).any()
    assert seen_hsv


def _driver(script, args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=300)


@pytest.mark.parametrize("script,cfg", [("train_yolov5.py", "train_yolov5.yaml"), ("train_yolox.py", "train_yolox.yaml")])
def test_driver_augment(dev, tmp_path, script, cfg):
    """two epochs of two steps with no_data_aug_epoch: 1: the first epoch augmented, the second not, finite losses"""
    text = open(os.path.join(ROOT, "config", cfg)).read()
    assert "no_data_aug_epoch: 10" in text
    override = tmp_path / cfg
    override.write_text(text.replace("no_data_aug_epoch: 10", "no_data_aug_epoch: 1"))
    r = _driver(script, ["--cfg", str(override), "--data", "dataset", "--augment", "--img", "128", "--batch", "4", "--steps-per-epoch", "2",
                         "--epochs", "2"], tmp_path)
    assert r.returncode == 0, r.stdout[-3000:]
    losses = [float(v) for v in re.findall(r"step \d+/2 tot (\S+)", r.stdout)]
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses), r.stdout[-3000:]
    lines = r.stdout.splitlines()
    closed = [i for i, line in enumerate(lines) if "epoch 2/2: data augmentation closed" in line]
    first_e2 = [i for i, line in enumerate(lines) if line.startswith("epoch 2/2 step")]
    assert len(closed) == 1 and first_e2 and closed[0] < first_e2[0], r.stdout[-3000:]
    assert not any("data augmentation closed" in line for line in lines[:closed[0]])


def test_driver_rejects_augment_without_images(dev, tmp_path):
    r = _driver("train_yolov5.py", ["--data", "tensor", "--augment", "--img", "64", "--batch", "4", "--epochs", "1", "--steps-per-epoch", "2"],
                tmp_path)
    assert r.returncode != 0 and "needs --data dataset" in r.stdout, r.stdout[-3000:]
