"""YOLOV7Loss (csrc/loss_v7.hip) at the shapes and targets where the kernels branch, against the fp64 restatement
(tools/v7loss_restated.py): matched rows and tar_nums equal, loss items within rtol 1e-4 / atol 1e-6, gradients within rtol 1e-4 /
atol 1e-4 * max|ref|, balances within rtol 1e-6.  The restatement makes the index decisions of the anchor match in fp32 like
the library and everything else in fp64; the inputs are random, so no cost sits within fp32 rounding of another except the
exact duplicates, which both sides resolve by the same rule (lower candidate, lower target row)."""
import numpy as np
import pytest
import torch

from tools.v7loss_restated import BASE_HYP, anchors_for, v7loss_restated

pytestmark = pytest.mark.gpu
ITEMS = ("iou_loss", "cof_loss", "cls_loss")


def _hyp(h, w, nc, dev="cpu", **kw):
    return dict(BASE_HYP, topk=10, num_class=nc, input_img_size=[h, w], device=dev, **kw)


def _heads(B, nc, maps, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy((rs.randn(B, 3 * (5 + nc), h, w) * scale).astype(np.float32)) for h, w in maps]


def _boxes(rs, n, lo, hi, span, nc, b):
    """n rows [x1, y1, x2, y2, cls, b] with sides in [lo, hi] and centres inside the middle of a span x span square"""
    wh = rs.uniform(lo, hi, (n, 2))
    ctr = rs.uniform(0.2, 0.8, (n, 2)) * span
    return np.concatenate([np.clip(ctr - wh / 2, 0, span), np.clip(ctr + wh / 2, 0, span), rs.randint(0, nc, (n, 1)), np.full((n, 1), b)], 1).astype(np.float32)


def _targets(B, M, rows_per_image):
    t = -np.ones((B, M, 6), np.float32)
    for b, rows in enumerate(rows_per_image):
        if len(rows):
            t[b, :len(rows)] = rows
    return torch.from_numpy(t)


def _device_call(dev, heads, tars, hyp, dtype=torch.float32, **kw):
    from yoloseries_amd.loss import YOLOV7Loss
    lf = YOLOV7Loss(anchors_for(len(heads)).to(dev), dict(hyp, device=dev, **kw), stage_num=len(heads))
    preds = [v.to(dev, dtype).requires_grad_(True) for v in heads]
    out = lf(preds, tars.to(dev))
    grads = torch.autograd.grad(out["tot_loss"], preds)
    return lf, out, grads


def _check(dev, heads, tars, hyp):
    lf, out, grads = _device_call(dev, heads, tars, hyp)
    p64 = [v.double().requires_grad_(True) for v in heads]
    ref = v7loss_restated(p64, tars, anchors_for(len(heads)), hyp, torch.float64)
    rgrads = torch.autograd.grad(ref["tot_loss"], p64)
    got = np.array([out["tot_loss"].item()] + [out[k] for k in ITEMS])
    want = np.array([ref["tot_loss"].item()] + [ref[k] for k in ITEMS])
    print(f"got {got} tar_nums {out['tar_nums']} balances {lf.balances}; fp64 {want} {ref['tar_nums']} {ref['balances']}")
    for rows, rrows in zip(lf.matches(), ref["matches"]):
        np.testing.assert_array_equal(rows, rrows)
    assert out["tar_nums"] == ref["tar_nums"]
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(lf.balances, ref["balances"], rtol=1e-6)
    for gr, rg in zip(grads, rgrads):
        rg = rg.numpy()
        np.testing.assert_allclose(gr.cpu().numpy(), rg, rtol=1e-4, atol=1e-4 * np.abs(rg).max())
    return lf, out, ref


def test_rectangular_input(dev):
    """96 x 160 input, maps 12 x 20, 6 x 10, 3 x 5.  The size pair enters as in the reference's formulas (x / size[0], y / size[1],
    stride size[1] / map width): the boxes stay inside a 96 x 96 corner so that every centre falls inside every map"""
    rs = np.random.RandomState(71)
    tars = _targets(2, 4, [_boxes(rs, 4, 10, 50, 96, 4, 0), _boxes(rs, 3, 10, 50, 96, 4, 1)])
    _, out, _ = _check(dev, _heads(2, 4, [(12, 20), (6, 10), (3, 5)], 72), tars, _hyp(96, 160, 4))
    assert out["tar_nums"] > 0


def test_image_without_valid_rows_and_border_box(dev):
    """image 0 has only padding rows, image 1 a box touching the image's corner and one touching its right and lower border"""
    rs = np.random.RandomState(73)
    rows = _boxes(rs, 3, 16, 60, 128, 5, 1)
    rows[0, :4] = [0, 0, 40, 24]
    rows[1, :4] = [90, 70, 128, 128]
    tars = _targets(2, 4, [[], rows])
    lf, out, _ = _check(dev, _heads(2, 5, [(16, 16), (8, 8), (4, 4)], 74), tars, _hyp(128, 128, 5))
    assert out["tar_nums"] > 0 and all((r[:, 0] == 1).all() for r in lf.matches())


def test_stage_without_candidates(dev):
    """boxes of 8..14 pixels: below a quarter of every stride-32 anchor side, so the last stage has no candidate"""
    rs = np.random.RandomState(75)
    tars = _targets(2, 3, [_boxes(rs, 3, 8, 14, 128, 5, 0), _boxes(rs, 2, 8, 14, 128, 5, 1)])
    lf, out, _ = _check(dev, _heads(2, 5, [(16, 16), (8, 8), (4, 4)], 76), tars, _hyp(128, 128, 5))
    m = lf.matches()
    assert len(m[0]) > 0 and len(m[2]) == 0


def _crowd(nvalid, M, seed):
    rs = np.random.RandomState(seed)
    return _targets(2, M, [_boxes(rs, nvalid, 10, 40, 256, 5, 0), _boxes(rs, 5, 10, 40, 256, 5, 1)])


def test_128_valid_rows_more_than_1024_candidates(dev):
    """130 rows, 128 of them valid, at 256^2: more than 1024 candidates in one (image, stage), i.e. several passes of the
    256-thread workgroup over the candidate list and a row of the cost matrix longer than 1024"""
    tars = _crowd(128, 130, 77)
    heads = _heads(2, 5, [(32, 32), (16, 16), (8, 8)], 78)
    _, _, ref = _check(dev, heads, tars, _hyp(256, 256, 5))
    assert max(i["cost"].shape[1] for per in ref["info"] for i in per if i is not None) > 1024


def test_more_than_128_valid_rows_is_refused(dev):
    from yoloseries_amd._lib import YoloHipError
    with pytest.raises(YoloHipError, match="129 ground-truth boxes"):
        _device_call(dev, _heads(2, 5, [(32, 32), (16, 16), (8, 8)], 78), _crowd(129, 130, 77), _hyp(256, 256, 5))


def _small_case():
    rs = np.random.RandomState(79)
    tars = _targets(2, 4, [_boxes(rs, 4, 16, 70, 128, 5, 0), _boxes(rs, 3, 16, 70, 128, 5, 1)])
    return _heads(2, 5, [(16, 16), (8, 8), (4, 4)], 80), tars, _hyp(128, 128, 5)


def test_two_identical_calls_bit_identical_and_device_items(dev):
    heads, tars, hyp = _small_case()
    runs = []
    for _ in range(2):
        lf, out, grads = _device_call(dev, heads, tars, hyp, loss_items_on_device=True)
        assert all(isinstance(out[k], torch.Tensor) and out[k].is_cuda and out[k].dim() == 0 for k in ITEMS + ("tar_nums",))
        runs.append((torch.stack([out["tot_loss"][0].detach()] + [out[k] for k in ITEMS + ("tar_nums",)]).cpu(),
                     [g.cpu() for g in grads], lf.balances))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][2] == runs[1][2] and float(runs[0][0][4]) > 0
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


def test_graph_capture_matches_eager(dev):
    """one forward + backward captured on a single stream and replayed twice == the same two calls launched eagerly on a twin
    instance: results, gradients and the stateful balances (the first call of both twins runs eagerly: it creates the state)"""
    from yoloseries_amd.loss import YOLOV7Loss
    heads, tars, hyp = _small_case()
    hyp = dict(hyp, device=dev, loss_items_on_device=True)
    tars = tars.to(dev)

    def twin():
        lf = YOLOV7Loss(anchors_for(3).to(dev), dict(hyp))
        preds = [v.to(dev).requires_grad_(True) for v in heads]

        def step():
            out = lf(preds, tars)
            grads = torch.autograd.grad(out["tot_loss"], preds)
            return torch.stack([out["tot_loss"][0].detach()] + [out[k] for k in ITEMS + ("tar_nums",)]), grads
        return lf, step

    lf_e, step_e = twin()
    eager = []
    for _ in range(3):
        res, grads = step_e()
        eager.append((res.cpu(), [g.cpu() for g in grads], lf_e.balances))
    lf_g, step_g = twin()
    step_g()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, grads = step_g()
    for i in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(res.cpu(), eager[i][0]) and float(res[4]) > 0
        for a, b in zip(grads, eager[i][1]):
            assert torch.equal(a.cpu(), b)
        assert lf_g.balances == eager[i][2]
    assert eager[1][2] != eager[2][2]                                  # the balances did move between the two replays
