"""GPU parity of YOLOV8Loss (csrc/loss_v8.hip) against the cases the reference produced (tests/golden/g19_v8loss.npz,
tools/gen_golden_v8.py): assignment exact, loss items within rtol 1e-4 / atol 1e-6, gradients within rtol 1e-4 /
atol 1e-4 * max|ref| (the tolerances of tests/test_gpu_yolox.py); the bf16 case against the fp32 golden gradient within one
bf16 ulp; NCHW and cell-major inputs bit-identical."""
import os

import numpy as np
import pytest
import torch

from tools.v8loss_restated import golden_case

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "g19_v8loss.npz")


def _run(dev, name, dtype):
    from yoloseries_amd.loss import YOLOV8Loss
    g = np.load(G)
    hyp, heads, tars = golden_case(g, name, dev)
    lf = YOLOV8Loss(hyp)
    preds = {k: v.to(dev, dtype).requires_grad_(True) for k, v in heads.items()}
    out = lf(preds, tars.to(dev))
    grads = torch.autograd.grad(out["tot_loss"], list(preds.values()))
    vals = g[f"{name}_vals"]
    got = np.array([out["tot_loss"].item(), out["cls_loss"], out["iou_loss"], out["dfl_loss"]])
    print(f"case {name} {dtype}: got {got} tar_nums {out['tar_nums']}; reference {vals}")
    np.testing.assert_array_equal(np.concatenate(lf.assignment(), axis=1), g[f"{name}_owner"])
    assert out["tar_nums"] == int(vals[4])
    return g, got, vals, grads


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f", "h"])
def test_v8_loss_golden_fp32(dev, name):
    g, got, vals, grads = _run(dev, name, torch.float32)
    np.testing.assert_allclose(got, vals[:4], rtol=1e-4, atol=1e-6)
    for s, gr in enumerate(grads):
        ref = g[f"{name}_grad{s}"]
        assert tuple(gr.shape) == ref.shape and gr.dtype == torch.float32
        np.testing.assert_allclose(gr.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def test_v8_loss_golden_bf16(dev):
    """case g: the inputs are bf16 numbers, so the kernel reads what the reference read; its fp32 gradient is rounded to bf16
    once on the way out, and an fp32 difference may flip that rounding: one bf16 ulp (2^-7 relative) on top of the fp32 bound"""
    g, got, vals, grads = _run(dev, "g", torch.bfloat16)
    np.testing.assert_allclose(got, vals[:4], rtol=1e-4)
    for s, gr in enumerate(grads):
        ref = g[f"g_grad{s}"]
        assert tuple(gr.shape) == ref.shape and gr.dtype == torch.bfloat16
        np.testing.assert_allclose(gr.float().cpu().numpy(), ref, rtol=2.0 ** -7, atol=1e-4 * np.abs(ref).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_v8_loss_nchw_and_cell_major_bit_identical(dev, dtype):
    from yoloseries_amd.layout import is_cell_major, to_cell_major
    from yoloseries_amd.loss import YOLOV8Loss
    g = np.load(G)
    hyp, heads, tars = golden_case(g, "a", dev)
    res, grads = [], []
    for cell_major in (False, True):
        lf = YOLOV8Loss(dict(hyp, loss_items_on_device=True))
        preds = {k: v.to(dev, dtype).contiguous() for k, v in heads.items()}
        if cell_major:
            preds = {k: to_cell_major(v)[0] for k, v in preds.items()}
        assert all(is_cell_major(v) == cell_major for v in preds.values())
        preds = {k: v.requires_grad_(True) for k, v in preds.items()}
        out = lf(preds, tars.to(dev))
        res.append(torch.stack([out["tot_loss"][0].detach(), out["cls_loss"], out["iou_loss"], out["dfl_loss"], out["tar_nums"]]).cpu())
        grads.append([x.contiguous().cpu() for x in torch.autograd.grad(out["tot_loss"], list(preds.values()))])
    assert torch.equal(res[0], res[1])
    for a, b in zip(*grads):
        assert a.shape == b.shape and torch.equal(a, b)
