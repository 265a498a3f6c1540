"""YOLOV8Loss on the GPU (csrc/loss_v8.hip) at the edges the reference does not pin, each against the fp64 restatement
(tools/v8loss_restated.py) on the same inputs: assignment and tar_nums exact, loss items within rtol 1e-4 / atol 1e-6, gradients
within rtol 1e-4 / atol 1e-4 * max|ref| — the fp32 bounds of the golden tests, the restatement's own fp64 error being far below."""
import numpy as np
import pytest
import torch

from tools.v8loss_restated import v8loss_restated
from yoloseries_amd.utils.synth import synth_v8_heads

pytestmark = pytest.mark.gpu


def _hyp(dev, img_hw, nc=3, reg=16, topk=13, **kw):
    return dict(alpha=0.5, beta=6.0, topk=topk, reg=reg, input_img_size=list(img_hw), num_class=nc, device=dev, **kw)


def _heads(B, img_hw, nc, reg, seed, strides=(4, 8, 16), near=None):
    """N(0, 1) logits; near: boost the logit of distance `near` on every side, so that predicted boxes are about 2 * near cells wide"""
    heads = synth_v8_heads(B, img_hw, nc, reg, seed=seed, strides=strides)
    if near is not None:
        for v in heads.values():
            for side in range(4):
                v[:, side * reg + near - 1] += 5.0
    return heads


def _targets(rows, M=None):
    """rows: per image a list of (xmin, ymin, xmax, ymax, cls) -> (B, M, 6) padded with -1"""
    M = M or max(1, max(len(r) for r in rows))
    t = -np.ones((len(rows), M, 6), np.float32)
    for b, r in enumerate(rows):
        for m, box in enumerate(r):
            t[b, m, :5], t[b, m, 5] = box, b
    return t


def _check(dev, hyp, heads, tnp):
    from yoloseries_amd.loss import YOLOV8Loss
    lf = YOLOV8Loss(hyp)
    preds = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in heads.items()}
    out = lf(preds, torch.from_numpy(tnp.copy()).to(dev))
    grads = torch.autograd.grad(out["tot_loss"], list(preds.values()))
    rp = [torch.from_numpy(v).double().requires_grad_(True) for v in heads.values()]
    ref = v8loss_restated(rp, torch.from_numpy(tnp.copy()), dict(hyp, device="cpu"), torch.float64)
    rgrads = torch.autograd.grad(ref["tot_loss"], rp)
    got = np.array([out["tot_loss"].item(), out["cls_loss"], out["iou_loss"], out["dfl_loss"]])
    want = np.array([ref["tot_loss"].item(), ref["cls_loss"], ref["iou_loss"], ref["dfl_loss"]])
    print(f"got {got} tar_nums {out['tar_nums']}; restatement {want} tar_nums {ref['tar_nums']}")
    for s, (a, r) in enumerate(zip(lf.assignment(), ref["assignment"])):
        np.testing.assert_array_equal(a, r.numpy(), err_msg=f"assignment of stage {s}")
    assert out["tar_nums"] == ref["tar_nums"]
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
    for gr, rg in zip(grads, rgrads):
        r = rg.numpy()
        assert tuple(gr.shape) == r.shape
        np.testing.assert_allclose(gr.cpu().numpy(), r, rtol=1e-4, atol=1e-4 * np.abs(r).max())
    return out, ref


def test_box_with_fewer_than_topk_centres(dev):
    """departure 1: a 6-px box holds 4 cell centres at stride 4, none at stride 8, one at stride 16: it gets at most those 5 cells"""
    tnp = _targets([[(21, 21, 27, 27, 1), (8, 10, 50, 44, 0)], [(30, 12, 58, 40, 2)]])
    out, ref = _check(dev, _hyp(dev, (64, 64)), _heads(2, 64, 3, 16, seed=11, near=1), tnp)
    small = sum(int((a[0] == 0).sum()) for a in ref["assignment"])
    assert 1 <= small <= 5 and out["tar_nums"] < 3 * 13


def test_rectangular_input(dev):
    """departure 2: 64 x 96 image, maps 16 x 24, 8 x 12, 4 x 6; x = col + 0.5, y = row + 0.5, stride from the height"""
    tnp = _targets([[(50, 8, 90, 40, 0), (5, 20, 40, 60, 2)], [(30, 10, 70, 50, 1)]])
    out, _ = _check(dev, _hyp(dev, (64, 96)), _heads(2, (64, 96), 3, 16, seed=12, near=3), tnp)
    assert out["tar_nums"] > 0


def test_image_without_valid_rows_beside_one_with(dev):
    tnp = _targets([[], [(10, 10, 40, 50, 1), (20, 16, 60, 44, 0)]], M=2)
    out, ref = _check(dev, _hyp(dev, (64, 64)), _heads(2, 64, 3, 16, seed=13, near=3), tnp)
    assert out["tar_nums"] > 0 and all(int((a[0] >= 0).sum()) == 0 for a in ref["assignment"])


def test_box_touching_the_border(dev):
    tnp = _targets([[(0, 0, 30, 25, 0), (40, 30, 64, 64, 2)], [(0, 20, 64, 50, 1)]])
    out, _ = _check(dev, _hyp(dev, (64, 64)), _heads(2, 64, 3, 16, seed=14, near=3), tnp)
    assert out["tar_nums"] > 0


def test_single_class(dev):
    tnp = _targets([[(10, 10, 40, 50, 0), (20, 16, 60, 44, 0)], [(5, 5, 35, 30, 0)]])
    out, _ = _check(dev, _hyp(dev, (64, 64), nc=1, reg=8), _heads(2, 64, 1, 8, seed=15, near=3), tnp)
    assert out["tar_nums"] > 0


def _crowd(valid, M=130):
    rs = np.random.RandomState(16)
    ctr, wh = rs.uniform(8, 56, (valid, 2)), rs.uniform(8, 24, (valid, 2))
    rows = [(*np.clip(c - s / 2, 0, 64), *np.clip(c + s / 2, 0, 64), int(rs.randint(0, 3))) for c, s in zip(ctr, wh)]
    return _targets([rows, rows[:3]], M=M)


def test_more_than_128_valid_rows_is_refused_before_any_launch(dev):
    from yoloseries_amd._lib import YoloHipError
    from yoloseries_amd.loss import YOLOV8Loss
    lf = YOLOV8Loss(_hyp(dev, (64, 64)))
    preds = {k: torch.from_numpy(v).to(dev) for k, v in _heads(2, 64, 3, 16, seed=16).items()}
    with pytest.raises(YoloHipError, match="129 ground-truth boxes"):
        lf(preds, torch.from_numpy(_crowd(129)).to(dev))
    assert lf._last is None and lf._ws is None


def test_130_rows_with_128_valid(dev):
    tnp = _crowd(128)
    assert tnp.shape == (2, 130, 6) and (tnp[0, :, 4] >= 0).sum() == 128
    out, _ = _check(dev, _hyp(dev, (64, 64)), _heads(2, 64, 3, 16, seed=16, near=2), tnp)
    assert out["tar_nums"] > 0


def test_two_identical_calls_are_bit_identical(dev):
    from yoloseries_amd.loss import YOLOV8Loss
    tnp = _crowd(40, M=40)
    heads = _heads(2, 64, 3, 16, seed=17, near=2)
    runs = []
    for _ in range(2):
        lf = YOLOV8Loss(_hyp(dev, (64, 64), loss_items_on_device=True))
        preds = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in heads.items()}
        out = lf(preds, torch.from_numpy(tnp.copy()).to(dev))
        grads = torch.autograd.grad(out["tot_loss"], list(preds.values()))
        runs.append([out["tot_loss"].detach().cpu(), *[out[k].cpu() for k in ("cls_loss", "iou_loss", "dfl_loss", "tar_nums")],
                     *[x.cpu() for x in grads], *[torch.from_numpy(a) for a in lf.assignment()]])
    assert float(runs[0][4]) > 40                    # crowded enough for cells chosen by several ground truths
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_loss_items_on_device(dev):
    from yoloseries_amd.loss import YOLOV8Loss
    tnp = _targets([[(10, 10, 40, 50, 1)], [(5, 5, 35, 30, 0)]])
    heads = _heads(2, 64, 3, 16, seed=18, near=3)
    outs = []
    for on_dev in (True, False):
        lf = YOLOV8Loss(_hyp(dev, (64, 64), loss_items_on_device=on_dev))
        outs.append(lf({k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in heads.items()}, torch.from_numpy(tnp.copy()).to(dev)))
    d, h = outs
    assert d["tot_loss"].shape == (1,) and d["tot_loss"].requires_grad and h["tot_loss"].requires_grad
    for k in ("cls_loss", "iou_loss", "dfl_loss", "tar_nums"):
        assert isinstance(d[k], torch.Tensor) and d[k].is_cuda and d[k].dim() == 0
        assert not isinstance(h[k], torch.Tensor) and float(d[k]) == h[k]
    assert isinstance(h["tar_nums"], int) and h["tar_nums"] > 0
