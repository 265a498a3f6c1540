"""Train-time augmentation, host side (utils/augment.py, dataset/augmented.py, augment_collate_fn): the plan geometry and the label
arithmetic against vectors recorded from the reference (tests/golden/g17_augment.npz, tools/gen_golden_augment.py), the NumPy
statement of the pixel path against independent float64 evaluations, and the loader's behaviour.  No GPU."""
import colorsys
import math
import os

import numpy as np
import pytest

from yoloseries_amd.utils import augment as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_augment.npz")
G = np.load(GOLDEN)
DST, FILL = int(G["dst"]), int(G["fill_value"])
CASES = [str(c) for c in G["cases"]]
MOSAIC_CASES = [c for c in CASES if c.startswith("mosaic")]
EPS = 2.0 ** -24


class Replay:
    """the part of random.Random that draw_plan uses: random() returns recorded values, uniform() goes through it with
    random.Random's own expression, randint() returns given indices"""

    def __init__(self, values, ints=()):
        self.values, self.ints = list(values), list(ints)

    def random(self):
        return self.values.pop(0)

    def uniform(self, a, b):
        return a + (b - a) * self.random()

    def randint(self, a, b):
        return self.ints.pop(0)

    def shuffle(self, x):
        pass


def case_items(name):
    n = 4 if name in MOSAIC_CASES else 1
    return [(G[f"{name}_img{k}"], G[f"{name}_box{k}"], G[f"{name}_lab{k}"]) for k in range(n)]


def case_plan(name):
    """draw_plan fed the draws the reference made: mosaic (2), RandomPerspective (9), the flips (1 + 1)"""
    items = case_items(name)
    degree, translate, scale, shear, persp, lr_p, ud_p = (float(v) for v in G[f"{name}_hyp"])
    d = list(G[f"{name}_draws"])
    mosaic = len(items) == 4
    hyp = A.check_aug_hyp(dict(data_aug_mosaic_p=1.0 if mosaic else 0.0, data_aug_degree=degree, data_aug_translate=translate,
                               data_aug_scale=scale, data_aug_shear=shear, data_aug_prespective=persp, data_aug_hsv_p=0.0,
                               data_aug_fliplr_p=lr_p, data_aug_flipud_p=ud_p, data_aug_fill_value=FILL))
    nw = 11 if mosaic else 9                                          # draws up to the end of the warp
    rng = Replay([0.5] + d[:nw] + [0.5] + d[nw:], ints=[1, 2, 3])     # 0.5: the mosaic_p and the hsv_p draws
    plan = A.draw_plan(0, len(items), lambda i: items[i][0].shape[:2], [DST, DST], hyp, rng, np.random.RandomState(0))
    assert not rng.values
    return plan, items


@pytest.fixture(scope="module")
def plans():
    return {name: case_plan(name) for name in CASES}


# ---------------------------------------------------------------------------------------------- mosaic against the reference
@pytest.mark.parametrize("name", MOSAIC_CASES)
def test_mosaic_rectangles_and_identity_pixels(plans, name):
    plan, items = plans[name]
    assert plan['indices'] == [0, 1, 2, 3] and plan['canvas_hw'] == (2 * DST, 2 * DST)
    canvas = G[f"{name}_canvas"]
    np.testing.assert_array_equal(A.build_canvas([i[0] for i in items], plan['rects'], plan['canvas_hw'], FILL), canvas)
    ident = dict(plan, minv=np.eye(3, dtype=np.float32).reshape(9))
    raw, tiles, canvas_hw, minv, gains = A.plan_tables([ident], [[i[0] for i in items]])
    assert gains is None and any(int(t['off']) % 2 for t in tiles[0])          # an image starts at an odd byte
    out = A.augment_batch_host(raw, tiles, canvas_hw, minv, None, 2 * DST, 2 * DST, FILL)
    np.testing.assert_array_equal(out[0], (canvas.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def test_fixture_covers_fill_and_crop(plans):
    plan, items = plans["mosaic_affine"]
    (_, _, ox0, oy0, ox1, oy1), (h, w) = plan['rects'][0], items[0][0].shape[:2]
    assert (ox1 - ox0, oy1 - oy0) == (w, h) and ox0 > 0 and oy0 > 0             # smaller than its quadrant: fill shows
    (sx0, sy0, ox0, oy0, ox1, oy1), (h, w) = plan['rects'][1], items[1][0].shape[:2]
    assert sx0 > 0 and sy0 > 0 and ox1 - ox0 < w and oy1 - oy0 < h              # larger: its centre is cut out


@pytest.mark.parametrize("name", CASES)
def test_labels_equal_the_reference(plans, name):
    plan, items = plans[name]
    np.testing.assert_array_equal(plan['M'], G[f"{name}_M"])
    if name in MOSAIC_CASES:
        box, lab = A.mosaic_labels([i[1] for i in items], [i[2] for i in items], plan['rects'], [2 * DST, 2 * DST])
        np.testing.assert_array_equal(box, G[f"{name}_mosaic_box"])
        np.testing.assert_array_equal(lab, G[f"{name}_mosaic_lab"])
        assert box.dtype == G[f"{name}_mosaic_box"].dtype
    else:
        box, lab = items[0][1], items[0][2]
    wbox, wlab = A.warp_labels(box, lab, plan['M'], plan['scale'], plan['perspective'], plan['dst_hw'])
    np.testing.assert_array_equal(wbox, G[f"{name}_warp_box"])
    np.testing.assert_array_equal(wlab, G[f"{name}_warp_lab"])
    fbox, flab = A.plan_labels(plan, [{'bboxes': i[1], 'classes': i[2]} for i in items])
    np.testing.assert_array_equal(fbox, G[f"{name}_final_box"])
    np.testing.assert_array_equal(flab, G[f"{name}_final_lab"])


def test_fixture_drops_boxes_in_both_filters():
    n_in = sum(len(G[f"mosaic_persp_box{k}"]) for k in range(4))
    assert len(G["mosaic_persp_mosaic_box"]) < n_in                              # the mosaic's window / area filter
    assert len(G["mosaic_persp_warp_box"]) < len(G["mosaic_persp_mosaic_box"])   # box_candidates


def test_flip_matrix_moves_labels_with_the_pixels(plans):
    """the label flip is x -> w - x on box edges, the pixel flip x -> w - 1 - x on pixel indices (np.fliplr): M_total maps the
    canvas to the flipped output (float64: 1e-9 px), and minv, its inverse rounded to float32, back (2e-4 px: 2^-24 relative on
    coordinates up to 128 px through three terms and a divide; no label is computed through the inverse)"""
    plan, _ = plans["single"]
    assert plan['fliplr'] and plan['flipud']
    pts = np.array([[3.0, 60.0], [5.0, 7.0], [1.0, 1.0]])
    fwd = plan['M'] @ pts
    fwd /= fwd[2]
    flipped = plan['M_total'] @ pts
    flipped /= flipped[2]
    np.testing.assert_allclose(flipped[0], DST - 1 - fwd[0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(flipped[1], DST - 1 - fwd[1], rtol=0, atol=1e-9)
    back = plan['minv'].astype(np.float64).reshape(3, 3) @ flipped
    np.testing.assert_allclose(back[:2] / back[2], pts[:2], rtol=0, atol=2e-4)


# ---------------------------------------------------------------------------------------------- warp against float64
def _warp_reference(canvas, minv, H, W, fill):
    """independent evaluation: float64, pixel loop, explicit canvas; returns (out (3, H, W), per-pixel bound on the coordinate
    magnitudes: sum of the absolute terms of the map, after the divide)"""
    m = np.asarray(minv, dtype=np.float64).reshape(3, 3)
    ch, cw = canvas.shape[:2]
    out = np.empty((3, H, W))
    mag = 0.0

    def px(tx, ty):
        return canvas[ty, tx].astype(np.float64) if 0 <= tx < cw and 0 <= ty < ch else np.full(3, float(fill))

    for y in range(H):
        for x in range(W):
            w = m[2, 0] * x + m[2, 1] * y + m[2, 2]
            u = (m[0, 0] * x + m[0, 1] * y + m[0, 2]) / w
            v = (m[1, 0] * x + m[1, 1] * y + m[1, 2]) / w
            mag = max(mag, (abs(m[0, 0] * x) + abs(m[0, 1] * y) + abs(m[0, 2])) / abs(w), (abs(m[1, 0] * x) + abs(m[1, 1] * y) + abs(m[1, 2])) / abs(w))
            tx, ty = math.floor(u), math.floor(v)
            ax, ay = u - tx, v - ty
            top = px(tx, ty) * (1 - ax) + px(tx + 1, ty) * ax
            bot = px(tx, ty + 1) * (1 - ax) + px(tx + 1, ty + 1) * ax
            out[:, y, x] = (top * (1 - ay) + bot * ay) / 255.0
    return out, mag


def _warp_cases():
    tr = lambda dx, dy: np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1.0]])          # noqa: E731  (these are output -> canvas)
    sc = lambda s: np.array([[1 / s, 0, 0], [0, 1 / s, 0], [0, 0, 1.0]])         # noqa: E731
    persp = A.warp_matrix((128, 128), (DST, DST), (0.0005, -0.0004), 7.0, 0.8, (3.0, -2.0), (0.45, 0.55))
    flips = A._finish_plan({'M': A.warp_matrix((128, 128), (DST, DST), (0, 0), 0.0, 0.6, (0, 0), (0.5, 0.5)), 'fliplr': True,
                            'flipud': True}, (DST, DST))['M_total']
    return {"translate": tr(30.37, 41.61), "scale_0.5": sc(0.5), "scale_1.5": sc(1.5) @ tr(40, 50),
            "perspective": np.linalg.inv(persp), "flips": np.linalg.inv(flips)}


@pytest.mark.parametrize("case", list(_warp_cases()))
def test_warp_against_float64(plans, case):
    """augment_batch_host (float32) against the float64 pixel loop above on the 128 x 128 mosaic canvas of the fixture.
    Bound: bilinear interpolation is continuous and piecewise linear with slope at most D = the largest difference between
    neighbouring canvas values (fill border included; at most 255), so an error (du, dv) of the sampling position moves the value by
    at most (|du| + |dv|) * D.  In float32 each of nu, nv, w comes from two products and two sums, each rounding relative 2^-24 of a
    partial result bounded by A = |m0 x| + |m1 y| + |m2| (resp. the other rows): |d nu| <= 4 * 2^-24 * A; the quotient adds the
    relative error of w (<= 4 * 2^-24 here, its terms having one sign dominated by m8 = 1) and its own rounding: |du| <= 10 * 2^-24 *
    A / |w|.  The blend and the division by 255 are seven more roundings of values <= 255 (<= 1 after the division): 8 * 2^-24.  Both
    sides read the same float32 matrix.  tol = 2 * 10 * 2^-24 * max(A / |w|) * D / 255 + 8 * 2^-24 (about 1e-4 at these sizes)."""
    plan, items = plans["mosaic_affine"]
    minv = _warp_cases()[case].astype(np.float32)
    canvas = G["mosaic_affine_canvas"]
    raw, tiles, canvas_hw, _, _ = A.plan_tables([plan], [[i[0] for i in items]])
    got = A.augment_batch_host(raw, tiles, canvas_hw, minv.reshape(1, 9), None, DST, DST, FILL)[0]
    ref, mag = _warp_reference(canvas, minv, DST, DST, FILL)
    padded = np.pad(canvas.astype(np.int64), ((1, 1), (1, 1), (0, 0)), constant_values=FILL)
    D = max(np.abs(np.diff(padded, axis=0)).max(), np.abs(np.diff(padded, axis=1)).max())
    tol = 2 * 10 * EPS * mag * D / 255 + 8 * EPS
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"{case}: max err {err:.3e}, tol {tol:.3e}, |coord| {mag:.1f}, D {D}")
    assert tol < 5e-4 and err <= tol
    assert np.abs(ref - FILL / 255).max() > 0.1                                  # the case samples image content, not only fill


# ---------------------------------------------------------------------------------------------- HSV against colorsys
def _hsv_colorsys(r, g, b, gains):
    h, s, v = colorsys.rgb_to_hsv(r / 255.0, g / 255.0, b / 255.0)
    h2 = math.fmod(h * 180.0 * gains[0], 180.0) / 180.0
    s2 = min(s * 255.0 * gains[1], 255.0) / 255.0
    v2 = min(v * 255.0 * gains[2], 255.0) / 255.0
    return colorsys.hsv_to_rgb(h2, s2, v2)


def hsv_colours():
    rs = np.random.RandomState(17)
    greys = np.repeat(np.arange(0, 256, 5, dtype=np.float32)[:, None], 3, 1)
    special = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                        [1, 0, 0], [0, 0, 1], [114, 114, 114], [200, 200, 199], [10, 10.5, 10]], dtype=np.float32)
    return np.concatenate([rs.uniform(0, 255, (3000, 3)).astype(np.float32), rs.randint(0, 256, (3000, 3)).astype(np.float32), greys,
                           special])


# gains (1, 1, 1) and the extremes of the shipped hgain 0.015, sgain 0.7, vgain 0.4
HSV_GAINS = [(1.0, 1.0, 1.0), (1.015, 1.7, 1.4), (0.985, 0.3, 0.6), (1.015, 0.3, 1.4)]
# 4 x the largest error of hsv_jitter against colorsys on hsv_colours() x HSV_GAINS, output scale (0..1); the measured maximum was
# HSV_MEASURED (test_hsv_against_colorsys prints the current one)
HSV_MEASURED = 7.8e-7
HSV_BOUND = 4 * HSV_MEASURED


@pytest.mark.parametrize("gains", HSV_GAINS)
def test_hsv_against_colorsys(gains):
    """hsv_jitter (float32, utils/augment.py) against colorsys (float64) with the same gains, on the output scale.  The map is
    continuous (the hue wrap at 180 joins the same colour), so the error is rounding only; the bound is 4 x the largest error
    measured on these inputs (HSV_MEASURED above)."""
    col = hsv_colours()
    r, g, b = A.hsv_jitter(col[:, 0], col[:, 1], col[:, 2], gains)
    got = np.stack([r, g, b], 1).astype(np.float64) / 255.0
    ref = np.array([_hsv_colorsys(float(c[0]), float(c[1]), float(c[2]), gains) for c in col])
    err = np.abs(got - ref).max()
    print(f"gains {gains}: max err {err:.3e} (bound {HSV_BOUND:.3e})")
    assert err <= HSV_BOUND


# ---------------------------------------------------------------------------------------------- plans and the loader
class TinyDataset:
    """images of unequal odd sizes with a few boxes each"""

    def __init__(self, n=12):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        rs = np.random.RandomState(100 + i)
        h, w = 40 + 7 * (i % 5), 33 + 11 * (i % 4)
        img = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
        x0, y0 = rs.uniform(0, w * 0.4, 4), rs.uniform(0, h * 0.4, 4)
        boxes = np.stack([x0, y0, x0 + rs.uniform(w * 0.3, w * 0.5, 4), y0 + rs.uniform(h * 0.3, h * 0.5, 4)], 1).astype(np.float32)
        return img, {'bboxes': boxes, 'classes': rs.randint(0, 80, 4).astype(np.float32)}, i


HYP = dict(data_aug_mosaic_p=0.7, data_aug_scale=0.5, data_aug_translate=0.1, data_aug_prespective=0.0005, data_aug_fliplr_p=0.5,
           data_aug_hsv_p=0.8, data_aug_fill_value=114)


def _plans_of(ds, n=6):
    return [ds[i][1] for i in range(n)]


def _same(p, q):
    return p['indices'] == q['indices'] and np.array_equal(p['minv'], q['minv']) and p['rects'] == q['rects'] and \
        np.array_equal(p['hsv_gain'], q['hsv_gain'])


def test_same_seed_same_plans_and_workers_differ():
    from yoloseries_amd.dataset import AugmentedDataset
    a, b, c = (AugmentedDataset(TinyDataset(), [64, 64], HYP, seed=s) for s in (3, 3, 4))
    pa, pb, pc = _plans_of(a), _plans_of(b), _plans_of(c)
    assert all(_same(p, q) for p, q in zip(pa, pb))
    assert not all(_same(p, q) for p, q in zip(pa, pc))
    w1, w2 = (AugmentedDataset(TinyDataset(), [64, 64], HYP, seed=3) for _ in range(2))
    w1.seed_worker(1001)
    w2.seed_worker(1002)
    assert not all(_same(p, q) for p, q in zip(_plans_of(w1), _plans_of(w2)))
    assert {len(p['indices']) for p in pa + pc} == {1, 4}


def test_items_and_close_data_aug():
    from yoloseries_amd.dataset import AugmentedDataset
    base = TinyDataset()
    ds = AugmentedDataset(base, [64, 64], HYP, seed=5)
    imgs, plan, ann, img_id = ds[2]
    assert len(imgs) == len(plan['indices']) and all(i.dtype == np.uint8 for i in imgs) and img_id == 2
    assert 2 in plan['indices'] and len(ann['classes']) == len(ann['bboxes']) > 0
    assert (ann['bboxes'] >= 0).all() and (ann['bboxes'] <= 64).all()
    ds.close_data_aug()
    img, ann, img_id = ds[2]
    np.testing.assert_array_equal(img, base[2][0])
    np.testing.assert_array_equal(ann['bboxes'], base[2][1]['bboxes'])


@pytest.mark.parametrize("key", ["data_aug_mixup_p", "data_aug_cutout_p", "data_aug_scale_jitting_p"])
def test_unbuilt_augmentations_raise(key):
    from yoloseries_amd.dataset import AugmentedDataset
    with pytest.raises(ValueError, match=f"{key}.*not built yet"):
        AugmentedDataset(TinyDataset(), [64, 64], dict(HYP, **{key: 0.3}), seed=1)
    AugmentedDataset(TinyDataset(), [64, 64], dict(HYP, **{key: 0.0}), seed=1)


def test_collate_builds_and_validates_tables():
    from yoloseries_amd.dataset import AugmentedDataset, augment_collate_fn
    ds = AugmentedDataset(TinyDataset(), [64, 64], HYP, seed=5)
    items = [ds[i] for i in range(4)]
    ds.close_data_aug()
    items.append(ds[4])                                               # a plain item in the same batch
    batch = augment_collate_fn(items, dst_size=[64, 64])
    assert batch['tiles'].shape == (5, 4, 40) and batch['minv'].shape == (5, 9) and batch['canvas_hw'].shape == (5, 2)
    assert batch['raw'].numel() == sum(i.size for item in items[:4] for i in item[0]) + items[4][0].size
    ann = batch['ann']
    assert ann.shape[0] == 5 and ann.shape[2] == 6
    for b in range(5):
        n = int((ann[b, :, 4] >= 0).sum())
        assert (ann[b, :n, 5] == b).all() and (ann[b, n:] == -1).all()
    assert (ann[:, :, 4] < 0).any()                                   # some image has fewer boxes than the longest: -1 rows
    # the plain item is the letterbox: at scale 1 the same copy as letter_resize_img
    from yoloseries_amd.utils.letterbox import letter_resize_img
    img = np.random.RandomState(1).randint(0, 256, (64, 48, 3), dtype=np.uint8)
    one = augment_collate_fn([(img, {'bboxes': np.array([[1., 2, 30, 40]]), 'classes': [3]}, 'x')], dst_size=[64, 64])
    host = A.augment_batch_host(one['raw'].numpy(), one['tiles'].numpy(), one['canvas_hw'].numpy(), one['minv'].numpy(), None, 64, 64, 128)
    np.testing.assert_array_equal(host[0], (letter_resize_img(img, [64, 64])[0].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))

    imgs, plan, ann_i, img_id = items[0]
    bad = dict(plan, rects=[(sx0, sy0, ox0, oy0, ox1 + 500, oy1) for sx0, sy0, ox0, oy0, ox1, oy1 in plan['rects']])
    with pytest.raises(ValueError, match="image 1.*outside its .* canvas"):
        augment_collate_fn([items[1], (imgs, bad, ann_i, img_id)], dst_size=[64, 64])
    bad = dict(plan, rects=[(sx0 + 500, sy0, ox0, oy0, ox1, oy1) for sx0, sy0, ox0, oy0, ox1, oy1 in plan['rects']])
    with pytest.raises(ValueError, match="image 0.*source window.*outside"):
        augment_collate_fn([(imgs, bad, ann_i, img_id)], dst_size=[64, 64])
    tiles = np.zeros((1, 4), dtype=A.TILE_DTYPE)
    tiles[0, 0] = (10, 8, 8, 0, 0, 0, 0, 8, 8)
    with pytest.raises(ValueError, match="image 0.*outside the raw buffer"):
        A.validate_tables(8 * 8 * 3, tiles, np.array([[8, 8]]))


def test_tile_dtype_matches_the_c_struct(tmp_path):
    """TILE_DTYPE (what the collate writes) and _lib.AugTile against the C compiler's view of yh_aug_tile in include/yolohip.h"""
    import ctypes as C
    import subprocess
    from yoloseries_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [n for n, _ in _lib.AugTile._fields_]
    assert names == list(A.TILE_DTYPE.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "yolohip.h"', 'int main(void) {', '  printf("%zu\\n", sizeof(yh_aug_tile));']
    lines += [f'  printf("%zu\\n", offsetof(yh_aug_tile, {n}));' for n in names] + ["  return 0; }"]
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    size, *offsets = (int(v) for v in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split())
    assert A.TILE_DTYPE.itemsize == C.sizeof(_lib.AugTile) == size == 40
    for name, off in zip(names, offsets):
        assert A.TILE_DTYPE.fields[name][1] == getattr(_lib.AugTile, name).offset == off


def test_build_dataloader_with_augmentation():
    """fails before this feature: build_dataloader(enable_data_aug=True) raised NotImplementedError"""
    import torch
    from yoloseries_amd.dataset import AugmentedDataset, build_dataloader
    ds, loader, prefetcher = build_dataloader(TinyDataset(), None, None, [64, 64], HYP, 0, True, 11, 4, 0, False, True, True)
    assert isinstance(ds, AugmentedDataset) and (prefetcher is None) == (not torch.cuda.is_available())
    batch = next(iter(loader))
    assert batch['tiles'].shape == (4, 4, 40) and batch['ann'].shape[0] == 4 and batch['dst_size'] == (64, 64)
    with pytest.raises(ValueError, match="data_aug_mixup_p"):
        build_dataloader(TinyDataset(), None, None, [64, 64], dict(HYP, data_aug_mixup_p=0.3), 0, True, 11, 4, 0, False, True, True)
