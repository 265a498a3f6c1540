"""GPU parity of YOLOV7Loss (csrc/loss_v7.hip) against the cases the reference produced (tests/golden/g22_v7loss.npz,
tools/gen_golden_v7.py): matched rows and tar_nums equal, loss items within rtol 1e-4 / atol 1e-6, gradients within rtol 1e-4 /
atol 1e-4 * max|ref|, balances within rtol 1e-6 (the tolerances of tests/test_v7loss_host.py); the bf16 case against the fp32
golden gradient within one bf16 ulp on top; NCHW, cell-major and the reference's 5-D layout bit-identical."""
import os

import numpy as np
import pytest
import torch

from tools.v7loss_restated import golden_case

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "g22_v7loss.npz")
ITEMS = ("iou_loss", "cof_loss", "cls_loss")


def _run(dev, name, dtype):
    from yoloseries_amd.loss import YOLOV7Loss
    g = np.load(G)
    anchors, hyp, calls, tars = golden_case(g, name, dev)
    lf = YOLOV7Loss(anchors.to(dev), hyp, stage_num=len(calls[0]))
    for heads in calls:                                               # case k: two calls on one instance, the second is stored
        preds = {f"p{s}": v.to(dev, dtype).requires_grad_(True) for s, v in enumerate(heads)}
        out = lf(preds, tars.to(dev))
        grads = torch.autograd.grad(out["tot_loss"], list(preds.values()))
    vals = g[f"{name}_vals"]
    got = np.array([out["tot_loss"].item()] + [out[k] for k in ITEMS])
    print(f"case {name} {dtype}: got {got} tar_nums {out['tar_nums']} balances {lf.balances}; reference {vals} {g[f'{name}_balances']}")
    for s, rows in enumerate(lf.matches()):
        np.testing.assert_array_equal(rows, g[f"{name}_rows{s}"])
    assert out["tar_nums"] == int(vals[4])
    np.testing.assert_allclose(lf.balances, g[f"{name}_balances"], rtol=1e-6)
    return g, got, vals, grads


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f", "g", "h", "i", "j", "k"])
def test_v7_loss_golden_fp32(dev, name):
    g, got, vals, grads = _run(dev, name, torch.float32)
    np.testing.assert_allclose(got, vals[:4], rtol=1e-4, atol=1e-6)
    for s, gr in enumerate(grads):
        ref = g[f"{name}_grad{s}"]
        assert tuple(gr.shape) == ref.shape and gr.dtype == torch.float32
        np.testing.assert_allclose(gr.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def test_v7_loss_golden_bf16(dev):
    """case g: the inputs are bf16 numbers, so the kernel reads what the reference read; its fp32 gradient is rounded to bf16
    once on the way out, and an fp32 difference may flip that rounding: one bf16 ulp (2^-7 relative) on top of the fp32 bound"""
    g, got, vals, grads = _run(dev, "g", torch.bfloat16)
    np.testing.assert_allclose(got, vals[:4], rtol=1e-4, atol=1e-6)
    for s, gr in enumerate(grads):
        ref = g[f"g_grad{s}"]
        assert tuple(gr.shape) == ref.shape and gr.dtype == torch.bfloat16
        np.testing.assert_allclose(gr.float().cpu().numpy(), ref, rtol=1e-4 + 2.0 ** -7, atol=1e-4 * np.abs(ref).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_v7_loss_layouts_bit_identical(dev, dtype):
    from yoloseries_amd.layout import is_cell_major, to_cell_major
    from yoloseries_amd.loss import YOLOV7Loss
    g = np.load(G)
    anchors, hyp, calls, tars = golden_case(g, "a", dev)
    nc = hyp["num_class"]
    res, grads = [], []
    for layout in ("nchw", "cell_major", "ref5d"):
        lf = YOLOV7Loss(anchors.to(dev), dict(hyp, loss_items_on_device=True))
        preds = [v.to(dev, dtype).contiguous() for v in calls[0]]
        if layout == "cell_major":
            preds = [to_cell_major(v)[0] for v in preds]
        elif layout == "ref5d":
            preds = [v.reshape(v.shape[0], 3, 5 + nc, v.shape[2], v.shape[3]).permute(0, 1, 3, 4, 2).contiguous() for v in preds]
        assert all(is_cell_major(v) == (layout == "cell_major") for v in preds)
        preds = [v.requires_grad_(True) for v in preds]
        out = lf(preds if layout != "ref5d" else {f"p{s}": v for s, v in enumerate(preds)}, tars.to(dev))
        res.append(torch.stack([out["tot_loss"][0].detach(), out["iou_loss"], out["cof_loss"], out["cls_loss"], out["tar_nums"]]).cpu())
        gr = torch.autograd.grad(out["tot_loss"], preds)
        if layout == "ref5d":                                          # (B, A, h, w, E) -> (B, A*E, h, w)
            assert all(x.shape == v.shape for x, v in zip(gr, preds))
            gr = [x.permute(0, 1, 4, 2, 3).reshape(x.shape[0], -1, x.shape[2], x.shape[3]) for x in gr]
        grads.append([x.contiguous().cpu() for x in gr])
    for i in (1, 2):
        assert torch.equal(res[0], res[i])
        for a, b in zip(grads[0], grads[i]):
            assert a.shape == b.shape and torch.equal(a, b)
