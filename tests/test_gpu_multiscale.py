"""Multi-scale training on the device: yh_resize_bilinear / yh_resize_bilinear_s2d against the NumPy statement of their arithmetic
(utils/multiscale.py resize_bilinear_host) bit for bit, the losses at the size of the step against the oracles, the models'
forward(x, input_size=...) against the unfused route, the program cache under a byte budget, and the drivers' --multi-scale."""
import ctypes as C
import gc
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_multiscale_host import SIZES, load_case
from yoloseries_amd.utils.multiscale import mutil_scale_training, resize_bilinear, resize_bilinear_host
from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_targets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(x, size, dev):
    out = resize_bilinear(torch.from_numpy(x).to(dev), size)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------- plain kernel
@pytest.mark.parametrize("name", list(SIZES))
def test_plain_kernel_bit_for_bit(dev, name):
    x, size, _ = load_case(name)
    np.testing.assert_array_equal(_plain(x, size, dev), resize_bilinear_host(x, size))


def test_plain_kernel_clamps_no_value(dev):
    x = (np.random.RandomState(21).randn(2, 3, 24, 40) * 3).astype(np.float32)
    assert x.min() < -1 and x.max() > 1
    for size in ((40, 72), (16, 24), (24, 40)):
        np.testing.assert_array_equal(_plain(x, size, dev), resize_bilinear_host(x, size))


def test_plain_kernel_non_default_stream(dev):
    x, size, _ = load_case("small_up")
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        out = resize_bilinear(torch.from_numpy(x).to(dev), size)
    side.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), resize_bilinear_host(x, size))


def test_plain_kernel_more_tiles_than_one_grid_pass(dev):
    # one workgroup per tile of RS_ROWS = 4 output rows of an image, at most RS_GRID_CAP = 2048 workgroups per launch
    # (csrc/preproc.hip): 8200 rows are 2050 tiles, so workgroups 0 and 1 take a second tile in the grid-stride loop
    x = np.random.RandomState(22).rand(1, 1, 8, 8).astype(np.float32)
    assert math.ceil(8200 / 4) > 2048
    np.testing.assert_array_equal(_plain(x, (8200, 32), dev), resize_bilinear_host(x, (8200, 32)))


def test_plain_kernel_ragged_width_and_batch(dev):
    # a width that is no multiple of 4 takes the scalar-store form; several images and planes; down and up in one call
    x = np.random.RandomState(23).rand(3, 2, 19, 50).astype(np.float32)
    np.testing.assert_array_equal(_plain(x, (33, 27), dev), resize_bilinear_host(x, (33, 27)))


# ---------------------------------------------------------------- fused kernel
@pytest.mark.parametrize("hw,size", [((64, 96), (96, 160)), ((96, 128), (64, 96)), ((64, 64), (64, 64))])
def test_fused_kernel_equals_resize_then_s2d(dev, hw, size):
    from yoloseries_amd import hipk
    x = torch.from_numpy(np.random.RandomState(31).rand(2, 3, *hw).astype(np.float32)).to(dev)
    want = torch.full((2, size[0] // 2, size[1] // 2, 16), float('nan'), dtype=torch.bfloat16, device=dev)
    got = torch.full_like(want, float('nan'))
    hipk.input_s2d(resize_bilinear(x, size), want)
    hipk.resize_bilinear_s2d(x, got)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert (got[..., 12:] == 0).all() and got[..., :12].float().abs().max() > 0
    # and the plain half of `want` is the host statement
    np.testing.assert_array_equal(resize_bilinear(x, size).cpu().numpy(), resize_bilinear_host(x.cpu().numpy(), size))


def test_argument_checks(dev):
    from yoloseries_amd._lib import lib, stream_ptr
    L = lib()
    x = torch.zeros(1, 3, 8, 8, device=dev)
    out = torch.zeros(1 * 3 * 8 * 8 + 8, device=dev)
    xp, op, st = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), stream_ptr()

    def message(rc):
        assert rc != 0
        return L.yh_last_error().decode()
    assert "even" in message(L.yh_resize_bilinear_s2d(xp, 1, 3, 8, 8, 7, 8, op, st))
    assert "null" in message(L.yh_resize_bilinear_s2d(None, 1, 3, 8, 8, 8, 8, op, st))
    assert "null" in message(L.yh_resize_bilinear(xp, 1, 3, 8, 8, 8, 8, None, st))
    assert "aligned" in message(L.yh_resize_bilinear(xp, 1, 3, 8, 8, 8, 8, C.c_void_p(out.data_ptr() + 4), st))
    assert "aligned" in message(L.yh_resize_bilinear_s2d(xp, 1, 3, 8, 8, 8, 8, C.c_void_p(out.data_ptr() + 8), st))
    assert "positive" in message(L.yh_resize_bilinear(xp, 1, 3, 8, 8, 0, 8, op, st))
    assert "Cin" in message(L.yh_resize_bilinear_s2d(xp, 1, 5, 8, 8, 8, 8, op, st))
    torch.cuda.synchronize()
    assert (out == 0).all()


# ---------------------------------------------------------------- losses at the size of the step
def _scaled_targets(B, base_hw, scale, seed):
    """(B, 7, 6) targets of a base_hw image -- six boxes an image at most, sides log-uniform from 6 px to 0.6 of the image so that
    every stage's anchors match some, the rest padding (-1), the last row padding in every image -- times `scale` over ALL rows,
    padding included (train_yolov5.py:543)"""
    rs = np.random.RandomState(seed)
    t = -np.ones((B, 7, 6), np.float32)
    for b in range(B):
        n = rs.randint(4, 7)
        w = np.exp(rs.uniform(np.log(6), np.log(0.6 * base_hw[1]), n))
        h = np.exp(rs.uniform(np.log(6), np.log(0.6 * base_hw[0]), n))
        cx, cy = rs.uniform(w / 2, base_hw[1] - w / 2), rs.uniform(h / 2, base_hw[0] - h / 2)
        t[b, :n, :4] = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1)
        t[b, :n, 4], t[b, :n, 5] = rs.randint(0, 80, n), b
    assert (t[:, -1] == -1).all()
    t[:, :, :4] *= np.float32(scale)
    return t


def _v5_hyp(dev, hw, focal=True):
    return dict(device=dev, num_class=80, input_img_size=list(hw), use_focal_loss=focal, focal_loss_gamma=1.5,
                focal_loss_alpha=0.25, iou_loss_scale=0.05, cls_loss_scale=0.5, cof_loss_scale=1.0, anchor_match_thr=4.0,
                class_smooth_factor=1.0, cls_pos_weight=1.0, cof_pos_weight=1.0)


def _v5_compare(dev, lf, of, hw, t, seed):
    """one call of the HIP loss and of the oracle on bf16 cell-major heads of an hw image (tests/test_gpu_loss.py
    test_loss_vs_oracle_bf16_layout: same quantities, same tolerances)"""
    rs = np.random.RandomState(seed)
    heads_bf = [torch.from_numpy((rs.randn(t.shape[0], 255, hw[0] // s, hw[1] // s) * 1.5).astype(np.float32)).to(torch.bfloat16)
                for s in (8, 16, 32)]
    preds = []
    for h in heads_bf:
        Bn, Ct, hh, ww = h.shape
        buf = torch.zeros(Bn, hh, ww, 256, dtype=torch.bfloat16, device=dev)
        buf[..., :Ct] = h.to(dev).permute(0, 2, 3, 1)
        preds.append(buf.as_strided((Bn, Ct, hh, ww), (hh * ww * 256, 1, ww * 256, 256)).requires_grad_(True))
    out = lf(preds, torch.from_numpy(t.copy()).to(dev))
    grads = torch.autograd.grad(out["tot_loss"], preds)
    opreds = [h.float().requires_grad_(True) for h in heads_bf]
    oout = of(opreds, t.copy())
    ograds = torch.autograd.grad(oout["tot_loss"], opreds)
    got = [out["tot_loss"].item(), out["iou_loss"], out["cof_loss"], out["cls_loss"]]
    ref = [oout["tot_loss"].item(), oout["iou_loss"], oout["cof_loss"], oout["cls_loss"]]
    print(f"v5 loss at {hw}: tar_nums {out['tar_nums']} / {oout['tar_nums']}, got {got}, oracle {ref}")
    assert out["tar_nums"] == oout["tar_nums"] and out["tar_nums"] > 0
    np.testing.assert_allclose(got, ref, rtol=1e-4)
    np.testing.assert_allclose(lf.balances, of.balances, rtol=1e-5)
    for gr, og in zip(grads, ograds):
        r = og.numpy()
        np.testing.assert_allclose(gr.float().cpu().numpy(), r, rtol=6e-3, atol=1e-3 * np.abs(r).max())


def test_v5_loss_at_the_size_of_the_step(dev):
    from oracle import v5loss as ov5
    from yoloseries_amd.loss import YOLOV5Loss
    hyp = _v5_hyp(dev, [64, 96])
    lf = YOLOV5Loss(torch.from_numpy(COCO_ANCHORS).to(dev), hyp)
    ohyp = _v5_hyp("cpu", [96, 160])
    of = ov5.V5LossOracle(COCO_ANCHORS, ohyp)
    lf.set_input_img_size([96, 160])
    _v5_compare(dev, lf, of, (96, 160), _scaled_targets(2, (56, 96), 160 / 96, seed=41), seed=42)
    assert hyp['input_img_size'] == [64, 96]
    # a third size: nothing of 96 x 160 survives (the balances do: they are the loss's running state, in the oracle too)
    lf.set_input_img_size([160, 128])
    ohyp['input_img_size'] = [160, 128]
    _v5_compare(dev, lf, of, (160, 128), _scaled_targets(2, (120, 96), 4 / 3, seed=43), seed=44)
    assert hyp['input_img_size'] == [64, 96]


def _yolox_hyp(dev, hw):
    return dict(device=dev, num_class=80, input_img_size=list(hw), use_focal_loss=False, focal_loss_gamma=1.5, focal_loss_alpha=0.25,
                iou_loss_scale=5.0, use_l1=True, l1_loss_scale=1.0, cls_loss_scale=1.0, cof_loss_scale=1.0, class_smooth_factor=1.0,
                cls_pos_weight=1.0, cof_pos_weight=1.0, num_anchors=1, iou_type="ciou", topk=13, center_radius=3, num_stage=3)


def _yolox_heads(B, hw, seed):
    """utils/synth.py synth_yolox_heads for an image that need not be square"""
    from collections import OrderedDict
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for name, s in zip(("pred_s", "pred_m", "pred_l"), (8, 16, 32)):
        h, w = hw[0] // s, hw[1] // s
        t = rs.randn(B, 1, 85, h, w).astype(np.float32)
        t[:, :, 0:2] = (0.5 + 0.5 * rs.randn(B, 1, 2, h, w)).astype(np.float32)
        t[:, :, 2:4] = (np.log(3.0) + 0.5 * rs.randn(B, 1, 2, h, w)).astype(np.float32)
        out[name] = t
    return out


def _yolox_compare(dev, lf, of, hw, t, seed):
    """tests/test_gpu_yolox.py test_yolox_loss_vs_oracle_640_b8: same quantities, same tolerances"""
    heads = _yolox_heads(t.shape[0], hw, seed)
    opreds = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in heads.items()}
    oout = of(opreds, torch.from_numpy(t.copy()))
    preds = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in heads.items()}
    out = lf(preds, torch.from_numpy(t.copy()).to(dev))
    for s, (mk, ofg) in enumerate(zip(lf.foreground_masks(), of.last_fg)):
        np.testing.assert_array_equal(mk, ofg.numpy(), err_msg=f"foreground mask of stage {s}")
    got = np.array([out["tot_loss"].item(), out["iou_loss"], out["l1_loss"], out["cls_loss"], out["cof_loss"]])
    ref = np.array([oout["tot_loss"].item(), oout["iou_loss"], oout["l1_loss"], oout["cls_loss"], oout["cof_loss"]])
    print(f"yolox loss at {hw}: fg {out['fg_nums']} / {oout['fg_nums']}, got {got}, oracle {ref}")
    assert out["fg_nums"] == oout["fg_nums"] > 0 and out["tar_nums"] == oout["tar_nums"] > 0
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(lf.balances, of.balances, rtol=1e-5)
    grads = torch.autograd.grad(out["tot_loss"], list(preds.values()))
    ograds = torch.autograd.grad(oout["tot_loss"], list(opreds.values()))
    for gr, og in zip(grads, ograds):
        r = og.numpy()
        np.testing.assert_allclose(gr.cpu().numpy(), r, rtol=1e-4, atol=1e-4 * np.abs(r).max())


def test_yolox_loss_at_the_size_of_the_step(dev):
    from oracle.yoloxloss import YOLOXLossOracle
    from yoloseries_amd.loss import YOLOXLoss
    hyp = _yolox_hyp(dev, [64, 96])
    lf = YOLOXLoss(hyp)
    ohyp = _yolox_hyp("cpu", [96, 160])
    of = YOLOXLossOracle(ohyp, stable_ties=True)
    lf.set_input_img_size([96, 160])
    _yolox_compare(dev, lf, of, (96, 160), _scaled_targets(2, (56, 96), 160 / 96, seed=51), seed=52)
    assert hyp['input_img_size'] == [64, 96]
    lf.set_input_img_size([160, 128])
    ohyp['input_img_size'] = [160, 128]
    _yolox_compare(dev, lf, of, (160, 128), _scaled_targets(2, (120, 96), 4 / 3, seed=53), seed=54)
    assert hyp['input_img_size'] == [64, 96]


# ---------------------------------------------------------------- models
def test_fused_ingest_equals_plain_one_train_step(dev):
    """model(x, input_size) against model(resize_bilinear(x)) on the same weights and the same program: heads and flat gradient"""
    import yoloseries_amd
    from yoloseries_amd import models
    yoloseries_amd.set_deterministic(True)
    try:
        torch.manual_seed(0)
        m = models.YOLOV5Small(3, 80).to(dev).train()
        x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(61)).to(dev)
        runs = []
        for fused in (True, False):
            for p_ in m.parameters():
                p_.grad = None
            heads = m(x, input_size=(96, 96)) if fused else m(resize_bilinear(x, (96, 96)))
            assert [tuple(h.shape) for h in heads] == [(2, 255, 12, 12), (2, 255, 6, 6), (2, 255, 3, 3)]
            sum((h.float() ** 2).mean() for h in heads).backward()
            torch.cuda.synchronize()
            runs.append(([h.detach().clone() for h in heads], m._yh_last_flat_grad.clone()))
        assert list(m._yh_state()['progs']) == [(2, 96, 96)]
        (h_f, g_f), (h_p, g_p) = runs
        for a, b in zip(h_f, h_p):
            assert torch.equal(a, b)
        assert torch.isfinite(g_f).all() and g_f.abs().max() > 0 and torch.equal(g_f, g_p)
        # the reference's function, unfused: same images, targets scaled in place over every row
        t = torch.from_numpy(synth_targets(2, 64, 80, 4, seed=62)).to(dev)
        t0 = t.clone()
        imgs, t1 = mutil_scale_training(x, t, shape=[96, 96])
        assert t1 is t and torch.equal(t[:, :, :4], t0[:, :, :4] * 1.5) and torch.equal(t[:, :, 4:], t0[:, :, 4:])
        assert torch.equal(imgs, resize_bilinear(x, (96, 96)))
    finally:
        yoloseries_amd.set_deterministic(False)


def test_input_size_rejects_a_differentiable_image(dev):
    from yoloseries_amd import models
    from yoloseries_amd._lib import YoloHipError
    m = models.YOLOV5Small(3, 80).to(dev).train()
    x = torch.rand(1, 3, 64, 64, device=dev, requires_grad=True)
    with pytest.raises(YoloHipError, match="no gradient through the resize"):
        m(x, input_size=(96, 96))
    assert len(m._yh_state()['progs']) == 0


def test_program_cache_under_a_byte_budget(dev):
    from yoloseries_amd import models
    sizes, B = [64, 96, 128, 160, 192], 2
    torch.manual_seed(0)
    m = models.YOLOV5Small(3, 80).to(dev).eval()
    xs = {s: torch.rand(B, 3, s, s, generator=torch.Generator().manual_seed(s)).to(dev) for s in sizes}
    with torch.no_grad():
        # what each program owns: an unbounded budget keeps all five
        m._yh_program_budget_bytes = 1 << 50
        for s in sizes:
            m(xs[s])
        owned = {k[1]: p.owned_bytes() for k, p in m._yh_state()['progs'].items()}
        assert sorted(owned) == sizes and all(owned[a] < owned[b] for a, b in zip(sizes, sizes[1:])), owned
        assert m._yh_cached_bytes() == sum(owned.values())
        pack = m._yh_state()['pack']
        budget = owned[160] + owned[192]                     # holds any two of them
        m._yh_state()['progs'].clear()
        gc.collect()
        m._yh_program_budget_bytes = budget
        order = sizes * 2
        random.Random(71).shuffle(order)
        first, base = {}, None
        for i, s in enumerate(order):
            heads = [h.cpu() for h in m(xs[s])]
            assert m._yh_cached_bytes() <= budget and (B, s, s) in m._yh_state()['progs']
            if s in first:
                for a, b in zip(heads, first[s]):
                    assert torch.equal(a, b), f"size {s} changed on its revisit (visit {i})"
            else:
                first[s] = heads
            del heads
            if i == 1:
                gc.collect()
                base = torch.cuda.memory_allocated(dev)
        assert len(m._yh_state()['progs']) >= 2 and m._yh_state()['pack'] is pack
        gc.collect()
        assert torch.cuda.memory_allocated(dev) <= base + budget, (torch.cuda.memory_allocated(dev), base, budget)
        # without the attribute: four entries, the first inserted goes
        del m._yh_program_budget_bytes
        m._yh_state()['progs'].clear()
        for s in sizes:
            m(xs[s])
        assert list(m._yh_state()['progs']) == [(B, s, s) for s in sizes[1:]]


# ---------------------------------------------------------------- drivers
_DRIVER = """
import json, random, sys
sys.path.insert(0, {root!r})
random.seed(11)
import {module} as drv
t = drv.main({argv!r})
print("RESULT " + json.dumps(dict(sizes=t.size_history, losses=[h["tot_loss"] for h in t.history],
                                  evals=sorted(k[1:] for k in t.validate.yolo._yh_state()["progs"]), hyp_size=t.hyp["input_img_size"])))
"""


def _driver(module, extra, cwd):
    argv = ["--data", "shapes", "--img", "128", "--batch", "4", "--steps-per-epoch", "6", "--epochs", "1"] + extra
    r = subprocess.run([sys.executable, "-c", _DRIVER.format(root=ROOT, module=module, argv=argv)], cwd=cwd, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-3000:]
    return json.loads(line[0][len("RESULT "):]), r.stdout


@pytest.mark.parametrize("module", ["train_yolov5", "train_yolox"])
def test_driver_multi_scale(dev, tmp_path, module):
    res, log = _driver(module, ["--multi-scale"], tmp_path)
    print(res)
    assert len(res["sizes"]) == 6 and all(h == w and h % 32 == 0 and 64 <= h <= 192 for h, w in res["sizes"]), res
    assert len({h for h, _ in res["sizes"]}) >= 2, res
    assert len(res["losses"]) == 6 and all(math.isfinite(v) for v in res["losses"]), res
    # the evaluator ran on the EMA copy, which never trains: its programs are the sizes validation ran at (128 and the smaller
    # passes of test-time augmentation), none of the larger sizes the training drew
    assert res["hyp_size"] == [128, 128] and [128, 128] in res["evals"] and max(h for h, _ in res["evals"]) == 128, res
    assert "[eval] epoch 1: mAP" in log, log[-2000:]


def test_driver_without_multi_scale_is_unchanged(dev, tmp_path):
    res, log = _driver("train_yolov5", [], tmp_path)
    assert res["sizes"] == [] and "multi-scale" not in log
    assert len(res["losses"]) == 6 and math.isfinite(res["losses"][0]) and [128, 128] in res["evals"]
