"""YOLOv8 loss, host side: the plain-torch restatement (tools/v8loss_restated.py) in fp32 on the CPU reproduces every case the
reference produced (tests/golden/g19_v8loss.npz, tools/gen_golden_v8.py) — loss items within rtol 1e-4 / atol 1e-6, gradients
within rtol 1e-4 / atol 1e-4 * max|ref| (the loss tolerances of tests/test_gpu_yolox.py), assignment exact; the tblr <-> xyxy
helpers; the hyp defaults; and the memory condition on the library's workspace and saved state."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tools.v8loss_restated import golden_case, v8loss_restated

G = os.path.join(os.path.dirname(__file__), "golden", "g19_v8loss.npz")
CASES = ["a", "b", "c", "d", "e", "f", "g", "h"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    g = np.load(G)
    hyp, heads, tars = golden_case(g, name)
    preds = [v.clone().requires_grad_(True) for v in heads.values()]
    out = v8loss_restated(preds, tars, hyp, torch.float32)
    vals = g[f"{name}_vals"]
    got = np.array([out["tot_loss"].item(), out["cls_loss"], out["iou_loss"], out["dfl_loss"]])
    print(f"case {name}: got {got} tar_nums {out['tar_nums']}; reference {vals}")
    np.testing.assert_array_equal(np.concatenate([a.numpy() for a in out["assignment"]], axis=1), g[f"{name}_owner"])
    assert out["tar_nums"] == int(vals[4])
    np.testing.assert_allclose(got, vals[:4], rtol=1e-4, atol=1e-6)
    grads = torch.autograd.grad(out["tot_loss"], preds)
    for s, gr in enumerate(grads):
        ref = g[f"{name}_grad{s}"]
        assert tuple(gr.shape) == ref.shape
        np.testing.assert_allclose(gr.numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def test_golden_cases_cover_what_they_claim():
    g = np.load(G)
    assert int((g["e_owner"] >= 0).sum()) == 1 and int(g["e_vals"][4]) == 1          # a single foreground cell
    assert int((g["f_owner"] >= 0).sum()) == 0 and g["f_vals"][2] == 0 and g["f_vals"][3] == 0
    for name in ("a", "b", "c", "d", "g", "h"):
        t = g[f"{name}_targets"]
        assert (t[1::2, -1, 4] < 0).all() and (t[0::2, :, 4] >= 0).all()            # odd images: one padding row
    assert g["b_owner"].shape == (3, 340) and g["b_grad3"].shape == (3, 67, 2, 2) and g["a_owner"].shape == (2, 1360)
    assert (g["e_targets"][..., 4] >= 0).sum() == 1 and (g["f_targets"][..., 4] < 0).all()


def test_tblr_xyxy_round_trip():
    from yoloseries_amd.utils import tblr2xyxy, xyxy2tblr
    gen = torch.Generator().manual_seed(3)
    grid = torch.stack(torch.meshgrid(torch.arange(5.) + 0.5, torch.arange(7.) + 0.5, indexing="xy"), -1).reshape(-1, 2)
    # quarter-integer coordinates: every sum and difference below is exact in fp32
    lo = torch.randint(-40, 40, (2, 35, 2), generator=gen).float() / 4
    x = torch.cat([lo, lo + torch.randint(1, 40, (2, 35, 2), generator=gen).float() / 4], -1)
    tblr = xyxy2tblr(x, grid)
    assert tblr.shape == (2, 35, 4)
    assert torch.equal(tblr[0, 0], torch.stack([grid[0, 1] - x[0, 0, 1], x[0, 0, 3] - grid[0, 1], grid[0, 0] - x[0, 0, 0], x[0, 0, 2] - grid[0, 0]]))
    assert torch.equal(tblr2xyxy(tblr, grid), x)


def test_hyp_defaults():
    from yoloseries_amd.loss import YOLOV8Loss
    lf = YOLOV8Loss(dict(alpha=0.5, beta=6.0, topk=13, reg=16, input_img_size=[640, 640], num_class=80, device="cpu"))
    assert (lf.iou_loss_scale, lf.cls_loss_scale, lf.dfl_loss_scale) == (7.5, 0.5, 1.5)
    assert (lf.alpha, lf.beta, lf.topk, lf.reg, lf.num_class, lf.img_sz) == (0.5, 6.0, 13, 16, 80, [640, 640])
    tars = torch.zeros(2, 3, 6)
    d, _ = lf._make_desc([torch.zeros(2, 144, 8, 8), torch.zeros(2, 144, 4, 4)], tars)
    assert (d.focal_gamma, d.focal_alpha, d.cls_pos_weight) == (1.5, 0.25, 1.0)
    assert (d.iou_scale, d.cls_scale, d.dfl_scale) == (7.5, 0.5, 1.5)
    assert (d.B, d.maxbox, d.num_stage, list(d.H)[:2], list(d.ldp)[:2], d.pred_is_f32) == (2, 3, 2, [8, 4], [144, 144], 1)
    lf.set_input_img_size((320, 512))
    assert lf.img_sz == [320, 512] and lf.hyp["input_img_size"] == [640, 640]
    with pytest.raises(RuntimeError):
        lf({"p": torch.zeros(2, 144, 8, 8)}, tars)                                  # no CPU path


@pytest.mark.parametrize("B,maxbox", [(64, 20), (2, 64)])
def test_buffers_do_not_scale_with_B_M_N(B, maxbox):
    """doubling maxbox grows the workspace and the saved state by less than B * N * maxbox bytes (no (B, M, N) buffer)"""
    from yoloseries_amd._lib import V8LossDesc, lib

    def sizes(m):
        d = V8LossDesc()
        d.B, d.maxbox, d.num_class, d.num_stage, d.reg, d.topk = B, m, 80, 4, 16, 13
        for s, hw in enumerate((160, 80, 40, 20)):
            d.H[s], d.W[s], d.ldp[s] = hw, hw, 144
        return lib().yh_v8loss_ws_bytes(C.byref(d)), lib().yh_v8loss_saved_bytes(C.byref(d))
    N = 160 * 160 + 80 * 80 + 40 * 40 + 20 * 20
    (w1, s1), (w2, s2) = sizes(maxbox), sizes(2 * maxbox)
    assert w1 > 0 and s1 > 0
    assert (w2 - w1) + (s2 - s1) < B * N * maxbox
    assert w1 + s1 <= 48 * B * N + 16 * B * maxbox + 128 * 1024                    # a few dozen bytes per cell, a few per target row
