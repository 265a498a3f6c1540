"""YOLOV8Evaluator (trainer/eval_yolov8.py over csrc/postproc_v8.hip) end to end against tests/golden/g20_v8post.npz, the results
of the reference's evaluator on the same heads (tools/gen_golden_v8post.py; inputs tools/v8post_cases.py).

Bars: row counts, class sequence and order exact (tests/test_v8post_host.py shows the fixture sits on no decision boundary); scores
rtol = atol = 2e-5, the bar tests/test_gpu_postproc.py states for decoded sigmoid outputs; boxes within 4 * E_ref of the fp64
restatement (tools/v8post_restated.py), E_ref being the reference's own fp32 error against it, stored per case as box_err_ref — the
factor covers another expf and another summation order over at most 32 bins.  Case r (rectangular maps, where the reference
scrambles the grid) is compared with the fp32 restatement under the same bars."""
import os

import numpy as np
import pytest
import torch

from tools import v8post_cases as vc
from tools import v8post_restated as vr

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "g20_v8post.npz")
SCORE_TOL = dict(rtol=2e-5, atol=2e-5)
_R64 = {}


def unpack(g, name, what):
    n, body = g[f"{name}_n{what}"], g[f"{name}_{what}"]
    rows, at = [], 0
    for k in n:
        rows.append(None if k < 0 else body[at:at + k])
        at += max(int(k), 0)
    return rows


def restated64(g, name):
    """(decoded, candidates, finals) of the fp64 restatement, computed once per case and never modified"""
    if name not in _R64:
        _R64[name] = vr.run_case(name, int(g[f"{name}_seed"][0]), np.float64)
    return _R64[name]


def evaluator(g, name, dev):
    from yoloseries_amd.trainer import YOLOV8Evaluator
    c = vc.case(name)
    stub = vc.StubYolo(name, int(g[f"{name}_seed"][0]), device=dev, as_bf16=True)
    return YOLOV8Evaluator(stub, vc.make_hyp(name, device=str(dev)), compute_metric=bool(c["metric"])), torch.from_numpy(vc.inputs(name)).to(dev)


def assert_rows(got, want, want64, bar, what):
    assert (got is None) == (want is None), what
    if want is None:
        return
    assert got.shape == want.shape, f"{what}: {got.shape} rows, expected {want.shape}"
    np.testing.assert_array_equal(got[:, 5], want[:, 5], err_msg=what)
    np.testing.assert_allclose(got[:, 4], want[:, 4], err_msg=what, **SCORE_TOL)
    if len(got):
        err = np.abs(got[:, :4].astype(np.float64) - want64[:, :4]).max()
        print(f"{what}: {len(got)} rows, boxes {err:.3g} from the fp64 restatement, bar {bar:.3g}")
        assert err <= bar, f"{what}: boxes {err:.3g} from the fp64 restatement, bar {bar:.3g}"


@pytest.fixture(scope="module")
def g():
    return np.load(G)


@pytest.mark.parametrize("name", [n for n in vc.CASES if n != "t"])
def test_evaluator_end_to_end(dev, g, name):
    ev, x = evaluator(g, name, dev)
    outs = ev(x)
    assert len(outs) == vc.case(name)["B"]
    bar = 4.0 * float(g[f"{name}_box_err_ref"][0])
    _, cands64, outs64 = restated64(g, name)
    if name in vc.RESTATED_ONLY:
        _, want_c, want_o = vr.run_case(name, int(g[f"{name}_seed"][0]), np.float32)
    else:
        want_c, want_o = unpack(g, name, "cand"), unpack(g, name, "out")
    assert ev.last_ncand == [len(c) for c in want_c]
    if name == "h":                                    # compared at candidate level only: the tie rule
        ev, x = evaluator(g, name, dev)                 # a fresh stub: its first call returns the heads of the stored seed
        cand, ncand, B, cap = ev._candidates(x)
        tab = cand.cpu().numpy()
        for b in range(B):
            assert_rows(tab[b, :len(want_c[b])], want_c[b], cands64[b], bar, f"case h image {b} candidates")
        return
    for b, o in enumerate(outs):
        assert o is None or (o.dtype == torch.float32 and not o.is_cuda)
        assert_rows(None if o is None else o.numpy(), want_o[b], outs64[b], bar, f"case {name} image {b}")


def test_evaluator_tta(dev, g):
    """case t: three passes, each with other heads, appended to one table; and the decoded route (test_time_augmentation, then
    numba_nms on the concatenated tensor) gives the same rows bit for bit as the fused one"""
    ev, x = evaluator(g, "t", dev)
    outs = ev(x)
    assert ev.yolo.calls == 3
    bar = 4.0 * float(g["t_box_err_ref"][0])
    _, cands64, outs64 = restated64(g, "t")
    want_c, want_o = unpack(g, "t", "cand"), unpack(g, "t", "out")
    assert ev.last_ncand == [len(c) for c in want_c]
    for b, o in enumerate(outs):
        assert_rows(None if o is None else o.numpy(), want_o[b], outs64[b], bar, f"case t image {b}")
    ev2, _ = evaluator(g, "t", dev)
    merged, parts = ev2.test_time_augmentation(x)
    assert merged.shape == (2, 3 * vc.ncell("t"), 4 + 5) and len(parts) == 3
    for a, b in zip(ev2.numba_nms(merged), outs):
        np.testing.assert_array_equal(a, b.numpy())


@pytest.mark.parametrize("name", ["a", "b", "c32", "c16"])
def test_do_inference_against_the_reference(dev, g, name):
    ev, x = evaluator(g, name, dev)
    dec = ev.do_inference(x)
    assert dec.shape == (vc.case(name)["B"], vc.ncell(name), 4 + vc.case(name)["nc"]) and dec.dtype == torch.float32
    dec = dec.cpu().numpy()
    dec64 = restated64(g, name)[0]
    bar = 4.0 * float(g[f"{name}_box_err_ref"][0])
    err = np.abs(dec[..., :4].astype(np.float64) - dec64[..., :4]).max()
    print(f"case {name}: boxes {err:.3g} from the fp64 restatement, bar {bar:.3g}")
    assert err <= bar
    if name == "b":
        np.testing.assert_allclose(dec[0, :, 4:], g["b_decoded0"][:, 4:], **SCORE_TOL)
        np.testing.assert_allclose(dec[..., :4], g["b_boxes"], rtol=0, atol=bar + float(g["b_box_err_ref"][0]))
    else:
        ref = g[f"{name}_decoded"]
        np.testing.assert_allclose(dec[..., 4:], ref[..., 4:], **SCORE_TOL)
        np.testing.assert_allclose(dec[..., :4], ref[..., :4], rtol=0, atol=bar + float(g[f"{name}_box_err_ref"][0]))
    # the decoded route of the evaluator gives the rows of the fused one
    for a, b in zip(ev.numba_nms(torch.from_numpy(dec).to(dev)), evaluator(g, name, dev)[0](x)):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, b.numpy())


@pytest.mark.parametrize("name", ["d", "t"])
def test_cap_overflow_reruns_with_room_for_every_cell(dev, g, name):
    """a first table too small for the candidates (counted, not stored) makes the evaluator run again with one row per cell: same rows"""
    ev, x = evaluator(g, name, dev)
    want = ev(x)
    small, _ = evaluator(g, name, dev)
    small._FIRST_CAP, small.yolo.period = 16, ev.yolo.calls
    got = small(x)
    # the TTA path runs its three forwards again (their heads are gone by then), the plain path filters the same heads again
    assert small.yolo.calls == (6 if name == "t" else 1) and small.last_ncand == ev.last_ncand and max(ev.last_ncand) > 3 * 16
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.numpy(), b.numpy())


def test_post_processing_and_grid(dev, g):
    """the reference's helper methods: distances [t, b, l, r] of post_processing, the (col + 0.5, row + 0.5) grid"""
    ev, _ = evaluator(g, "a", dev)
    heads = list(vc.heads("a", int(g["a_seed"][0])).values())
    reg = 16
    z = np.concatenate([p[:, :4 * reg].reshape(2, 4 * reg, -1) for p in heads], 2).transpose(0, 2, 1)
    got = ev.post_processing(torch.from_numpy(np.ascontiguousarray(z)).to(dev)).cpu().numpy()
    z64 = z.astype(np.float64).reshape(2, -1, 4, reg)
    e = np.exp(z64 - z64.max(-1, keepdims=True))
    want = (e / e.sum(-1, keepdims=True) * np.arange(1, reg + 1)).sum(-1)
    np.testing.assert_allclose(got, want, rtol=0, atol=4.0 * float(g["a_box_err_ref"][0]))
    iou = ev.bbox_iou(torch.tensor([[0., 0., 2., 2.]], device=dev), torch.tensor([[1., 1., 3., 3.], [0., 0., 2., 2.]], device=dev))
    np.testing.assert_allclose(iou.cpu().numpy(), [[1 / 7, 1.0]], rtol=1e-6)
    assert tuple(ev.scale_img(torch.zeros(1, 3, 64, 64, device=dev), 0.83).shape) == (1, 3, 64, 64)
    grid, stride = ev.make_grid([[2, 3]], [8.0], dev)
    assert grid.cpu().tolist() == [[0.5, 0.5], [1.5, 0.5], [2.5, 0.5], [0.5, 1.5], [1.5, 1.5], [2.5, 1.5]] and stride.cpu().tolist() == [[8.0]] * 6


def test_host_tensors_are_refused(dev, g):
    from yoloseries_amd._lib import YoloHipError
    from yoloseries_amd.trainer import YOLOV8Evaluator
    ev = YOLOV8Evaluator(vc.StubYolo("a", 1, device="cpu"), vc.make_hyp("a", device=str(dev)))
    x = torch.from_numpy(vc.inputs("a"))
    for call in (lambda: ev(x), lambda: ev.do_inference(x), lambda: ev.numba_nms(torch.zeros(1, 4, 9))):
        with pytest.raises(YoloHipError, match="must live on an MI355X device"):
            call()
