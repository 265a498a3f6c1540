"""YOLOv7 loss, host side: the plain-torch restatement (tools/v7loss_restated.py) in fp32 on the CPU reproduces every case the
reference produced (tests/golden/g22_v7loss.npz, tools/gen_golden_v7.py) — matched rows and tar_nums equal, loss items within
rtol 1e-4 / atol 1e-6, gradients within rtol 1e-4 / atol 1e-4 * max|ref| (the loss tolerances of tests/test_gpu_yolox.py), balances
within rtol 1e-6; the golden cases cover what they claim; the hyp defaults and the descriptor; the exported symbols; the topk
limit; no CPU path; and the memory condition on the library's workspace and saved state."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tools.v7loss_restated import golden_case, v7loss_restated

G = os.path.join(os.path.dirname(__file__), "golden", "g22_v7loss.npz")
CASES = ["a", "b", "c", "d", "e", "f", "g", "h", "i", "j", "k"]
ITEMS = ("tot_loss", "iou_loss", "cof_loss", "cls_loss")


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    g = np.load(G)
    anchors, hyp, calls, tars = golden_case(g, name)
    bal = None
    for heads in calls:                                               # case k: two calls, the second is stored
        preds = [v.clone().requires_grad_(True) for v in heads]
        out = v7loss_restated(preds, tars, anchors, hyp, torch.float32, balances=bal)
        bal = out["balances"]
    vals = g[f"{name}_vals"]
    got = np.array([out["tot_loss"].item()] + [out[k] for k in ITEMS[1:]])
    print(f"case {name}: got {got} tar_nums {out['tar_nums']} balances {bal}; reference {vals} {g[f'{name}_balances']}")
    for s, rows in enumerate(out["matches"]):
        np.testing.assert_array_equal(rows, g[f"{name}_rows{s}"])
        np.testing.assert_array_equal(out["src_rows"][s], g[f"{name}_src{s}"])
    assert out["tar_nums"] == int(vals[4])
    np.testing.assert_allclose(got, vals[:4], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(bal, g[f"{name}_balances"], rtol=1e-6)
    grads = torch.autograd.grad(out["tot_loss"], preds)
    for s, gr in enumerate(grads):
        ref = g[f"{name}_grad{s}"]
        assert tuple(gr.shape) == ref.shape
        np.testing.assert_allclose(gr.numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def test_golden_cases_cover_what_they_claim():
    g = np.load(G)
    for name in ("a", "b"):
        nstage = int(g[f"{name}_args"][4])
        dup_both = moved = False
        for s in range(nstage):
            rows, src = g[f"{name}_rows{s}"], g[f"{name}_src{s}"]
            cells, n = np.unique(rows[:, :4], axis=0, return_counts=True)
            dup_both |= bool((n > 1).any())                           # a duplicated cell, both copies matched
            moved |= bool((rows[:, 4] != src).any())                  # a candidate that went to another row than its own
        assert dup_both and moved, name
    d = g["j_dynk"]                                                    # (stage, image, row, dynamic_k, min(topk, Xp))
    assert (d[:, 3] < d[:, 4]).any() and (d[:, 3] >= 1).all()
    for s in range(3):                                                 # no row is matched more often than its dynamic_k
        for st, b, row, k, _ in d[d[:, 0] == s]:
            r = g[f"j_rows{s}"]
            assert int(((r[:, 0] == b) & (r[:, 4] == row)).sum()) <= k
    for name in ("a", "b", "c", "d", "g", "h", "i", "k"):
        t = g[f"{name}_targets"]
        assert (t[1::2, -1, 4] < 0).all() and (t[0::2, :, 4] >= 0).all()              # odd images: one padding row
    assert (g["e_targets"][..., 4] >= 0).sum() == 1 and int(g["e_args"][5]) == 1
    assert (g["f_targets"][..., 4] < 0).all() and g["f_vals"][4] == 0 and g["f_vals"][1] == 0 and g["f_vals"][3] == 0 and g["f_vals"][2] > 0
    assert all(len(g[f"f_rows{s}"]) == 0 for s in range(3))
    assert int(g["c_args"][4]) == 4 and g["c_grad3"].shape == (2, 30, 2, 2) and len(g["c_balances"]) == 4
    assert int(g["i_args"][3]) == 1 and int(g["k_args"][8]) == 2 and int(g["g_args"][6]) == 1
    assert (g["j_targets"][..., 4] >= 0).sum() == 2 and int(g["j_args"][0]) == 256


def _hyp(**kw):
    h = dict(num_class=80, use_focal_loss=False, iou_loss_scale=0.05, cls_loss_scale=0.5, cof_loss_scale=1.0, anchor_match_thr=4.0,
             cls_pos_weight=1.0, cof_pos_weight=1.0, topk=15, use_iou_as_tar_cof=True, input_img_size=[640, 640], device="cpu")
    h.update(kw)
    return h


def _anchors():
    from yoloseries_amd.utils.synth import COCO_ANCHORS
    return torch.from_numpy(COCO_ANCHORS.copy())


def test_hyp_defaults_and_descriptor():
    from yoloseries_amd.loss import YOLOV7Loss
    lf = YOLOV7Loss(_anchors(), _hyp())
    assert (lf.positive_smooth_cls, lf.negative_smooth_cls) == (0.95, 0.05) and lf.use_iou_as_tar_cof is True
    assert lf.balances == [4., 1., 0.4] and YOLOV7Loss(_anchors(), _hyp(), stage_num=4).balances == [4., 1., 0.4, 0.1]
    tars = torch.zeros(2, 3, 6)
    v, canon = lf._make_desc([torch.zeros(2, 255, 8, 8), torch.zeros(2, 255, 4, 4), torch.zeros(2, 255, 2, 2)], tars)
    d = v.v5
    assert (v.topk, v.use_iou_as_tar_cof, d.targets_xywhn) == (15, 1, 0)
    assert (d.B, d.maxbox, d.num_class, d.num_anchor, d.num_stage) == (2, 3, 80, 3, 3)
    assert (list(d.H)[:3], list(d.W)[:3], list(d.ldp)[:3], d.pred_is_f32) == ([8, 4, 2], [8, 4, 2], [256, 256, 256], 1)
    assert (d.focal_gamma, d.focal_alpha, d.use_focal, d.anchor_thr) == (1.5, 0.25, 0, 4.0)
    assert (d.img_size0, d.img_size1, d.cls_pos_weight, d.cof_pos_weight) == (640.0, 640.0, 1.0, 1.0)
    assert [d.anchors[i] for i in (0, 1, 6, 7, 16, 17)] == [10.0, 13.0, 30.0, 61.0, 373.0, 326.0]
    np.testing.assert_allclose([d.iou_scale, d.cof_scale, d.cls_scale], [0.05, 1.0, 0.5], rtol=1e-7)
    lf.set_input_img_size((320, 512))
    assert lf.input_img_size == [320, 512] and lf.hyp["input_img_size"] == [640, 640]
    f = lf.focal_loss_factor(torch.zeros(3), torch.ones(3))
    np.testing.assert_allclose(f.numpy(), 0.5 ** 1.5 * 0.25, rtol=1e-6)


def test_library_exports_the_new_symbols():
    from yoloseries_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for sym in ("yh_v7loss_ws_bytes", "yh_v7loss_saved_bytes", "yh_v7_loss_fwd", "yh_v7_loss_bwd", "yh_v7_matches"):
        assert hasattr(raw, sym) and sym in _lib.EXPORTED_SYMBOLS, sym
    assert C.sizeof(_lib.V7LossDesc) == C.sizeof(_lib.V5LossDesc) + 8                    # yh_v7loss_desc: the v5 fields, topk, use_iou_as_tar_cof
    assert _lib.V7LossDesc.topk.offset == C.sizeof(_lib.V5LossDesc)


@pytest.mark.parametrize("topk", [0, 25])
def test_topk_outside_1_24_is_refused(topk):
    from yoloseries_amd import _lib
    from yoloseries_amd.loss import YOLOV7Loss
    with pytest.raises(_lib.YoloHipError):
        YOLOV7Loss(_anchors(), _hyp(topk=topk))
    lf = YOLOV7Loss(_anchors(), _hyp())
    lf.hyp["topk"] = topk                                              # changed after construction: refused when the call is prepared
    with pytest.raises(_lib.YoloHipError):
        lf._make_desc([torch.zeros(2, 255, 8, 8)] * 3, torch.zeros(2, 3, 6))
    v = _lib.V7LossDesc()
    v.v5.B, v.v5.maxbox, v.v5.num_class, v.v5.num_anchor, v.v5.num_stage, v.topk = 1, 1, 1, 3, 3, topk
    for s in range(3):
        v.v5.H[s], v.v5.W[s], v.v5.ldp[s] = 2, 2, 24
    one = (C.c_void_p * 4)(16, 16, 16, 16)                             # never dereferenced: the descriptor is refused first
    assert _lib.lib().yh_v7_loss_fwd(C.byref(v), one, 16, 16, 16, 16, 16, None) != 0


def test_no_cpu_path():
    from yoloseries_amd.loss import YOLOV7Loss
    lf = YOLOV7Loss(_anchors(), _hyp(num_class=3))
    heads = {f"p{s}": torch.zeros(2, 24, n, n) for s, n in enumerate((8, 4, 2))}
    with pytest.raises(RuntimeError):
        lf(heads, torch.zeros(2, 3, 6))


@pytest.mark.parametrize("B,maxbox", [(64, 20), (2, 64)])
def test_buffers_do_not_scale_with_cells_times_targets(B, maxbox):
    """doubling maxbox grows workspace + saved state by less than B * sum(H W) * A * maxbox bytes: no per-cell x per-target buffer"""
    from yoloseries_amd._lib import V7LossDesc, lib

    def sizes(m):
        v = V7LossDesc()
        v.v5.B, v.v5.maxbox, v.v5.num_class, v.v5.num_anchor, v.v5.num_stage, v.topk = B, m, 80, 3, 3, 15
        for s, hw in enumerate((80, 40, 20)):
            v.v5.H[s], v.v5.W[s], v.v5.ldp[s] = hw, hw, 256
        return lib().yh_v7loss_ws_bytes(C.byref(v)), lib().yh_v7loss_saved_bytes(C.byref(v))
    cells = (80 * 80 + 40 * 40 + 20 * 20) * 3
    (w1, s1), (w2, s2) = sizes(maxbox), sizes(2 * maxbox)
    assert w1 > 0 and s1 > 0
    assert (w2 - w1) + (s2 - s1) < B * cells * maxbox
    assert w1 + s1 <= 4 * B * cells + 124 * 3 * 15 * B * maxbox + 256 * 1024       # 4 bytes per cell, 76 + 48 per stage and candidate row
