"""GPU parity of the YOLOv5 loss kernels (csrc/loss_v5.hip) over hyper-parameter values and target edge cases: every case of
tests/golden/g15_loss_edges.npz against the reference's recorded outputs, and once more against the oracle on a seed that is not
in the file, with fp32 predictions and with the bf16 cell-major layout the models emit.

Bars (as in test_gpu_loss.py): tar_nums and — through YOLOV5Loss.assign — all indices and tar_box equal; loss
items rtol 1e-4, balances rtol 1e-5; fp32 gradients rtol 1e-4, atol 1e-4 * max|ref|; bf16 gradients rtol 6e-3, atol
1e-3 * max|ref| (stored in bf16: half an ulp is 2^-9) with the oracle evaluated on the same bf16 values, padding columns of
the gradient buffer exactly zero.  NaN (cls_loss / tot_loss when a stage has no positive: a mean of nothing in the reference,
loss/yolov5_loss.py:101) compares equal to NaN and is allowed only where the reference has it.

Backward scale: the kernels multiply by the incoming d tot as a device scalar.  3.75 is exact in bf16 and fp32, so the scaled
gradient differs from 3.75 x the unit gradient only by the rounding of one more fp32 product per term (a cell's gradient sums a
handful of terms): 16 ulp = 2e-6 relative for fp32 gradients; for bf16 gradients both sides are rounded to bf16 once, 2^-8 each.

Not covered: non-square `input_img_size`.  The reference divides x by img_size[0] but takes ds = img_size[1] / fm_w
(loss/yolov5_loss.py:66) and on a 256 x 128 input either returns NaN or trips its own assertion (:176): no defined behaviour.

Saturated logits (test_v5_saturated_logits): objectness and class logits of +30 / -30, where the fp32 sigmoid is exactly 1 or
1 - sigmoid is exactly 1, so that the focal factor's base (1 - acc) is 0 and its derivative takes the branch that is defined
to be 0 (csrc/exact_math.h focal_factor).  Same bars as above against the oracle; in addition the gradient of every
saturated-correct logit is 0 as a value.  The objectness target of a positive is its CIoU, never exactly 1, so the
saturated-correct sites here are the objectness of cells without a positive at -30 (t = 0) and the target class of a positive
at +30 (t = class_smooth_factor = 1)."""
import numpy as np
import pytest
import torch

from oracle import loss_cases as lc
from oracle import v5loss as ov5

pytestmark = pytest.mark.gpu

_G = lc.load()
NAMES = [str(n) for n in _G["case_names"] if lc.spec_of(_G, str(n))["kind"] == "v5"]
ORACLE_ONLY = ["nc124_refused", "bscale_f32", "bscale_bf16"]
_RAN_GOLDEN, _RAN_ORACLE = set(), set()


def _loss(spec, dev):
    from yoloseries_amd.loss import YOLOV5Loss
    return YOLOV5Loss(torch.from_numpy(lc.anchors_of(spec).copy()).to(dev), lc.hyp_of(spec, dev), stage_num=spec["stages"])


def _preds(heads, dev, bf16):
    """fp32: plain (B, C, h, w) tensors; bf16: views into [B][h][w][ld] buffers, ld = 256 for 255 channels, else padded to 8"""
    if not bf16:
        return [torch.from_numpy(h).to(dev).requires_grad_(True) for h in heads]
    out = []
    for h in heads:
        B, Ct, hh, ww = h.shape
        ld = ((Ct + 7) // 8) * 8
        buf = torch.zeros(B, hh, ww, ld, dtype=torch.bfloat16, device=dev)
        buf[..., :Ct] = torch.from_numpy(h).to(torch.bfloat16).to(dev).permute(0, 2, 3, 1)
        out.append(buf.as_strided((B, Ct, hh, ww), (hh * ww * ld, 1, ww * ld, ld)).requires_grad_(True))
    return out


def _items(out):
    return np.array([out["tot_loss"].item(), out["iou_loss"], out["cof_loss"], out["cls_loss"]], np.float64)


def _check_assign(lf, spec, targets, heads, dev):
    outs = lf.assign(torch.from_numpy(targets).to(dev), [tuple(h.shape[2:]) for h in heads])
    hyp = lc.hyp_of(spec, "cpu")
    total = 0
    for s, h in enumerate(heads):
        ref = ov5.match(targets, lc.anchors_of(spec)[s], h.shape[3], h.shape[2], hyp["input_img_size"], hyp["anchor_match_thr"])
        for name, got, want in zip(("tbox", "cls", "img", "anc", "gy", "gx"), outs[s], ref):
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"stage {s} {name}")
        total += len(ref[0])
    return total


@pytest.mark.parametrize("name", NAMES)
def test_v5_case_vs_reference(dev, name):
    _RAN_GOLDEN.add(name)
    spec = lc.spec_of(_G, name)
    lf = _loss(spec, dev)
    for call, seed in enumerate(spec["seeds"]):
        key = f"{name}_c{call}"
        t = _G[f"{key}_targets"]
        heads = lc.heads_of(spec, seed)
        preds = _preds(heads, dev, False)
        out = lf(preds, torch.from_numpy(t).to(dev))
        vals = _G[f"{key}_vals"]
        print(name, call, "hip", _items(out), out["tar_nums"], "ref", vals)
        assert out["tar_nums"] == vals[4] == _check_assign(lf, spec, t, heads, dev)
        lc.nan_equal_close(_items(out), vals[:4], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(lf.balances, _G[f"{key}_balances"], rtol=1e-5)
        for s, gr in enumerate(torch.autograd.grad(out["tot_loss"], preds)):
            gn = gr.cpu().numpy()
            assert np.isfinite(gn).all()
            if f"{key}_grad{s}" in _G:
                ref = _G[f"{key}_grad{s}"]
                np.testing.assert_allclose(gn, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
            else:
                flat, ref = gn.reshape(-1), _G[f"{key}_gval{s}"]
                np.testing.assert_allclose(flat[_G[f"{key}_gidx{s}"]], ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
                np.testing.assert_allclose([flat.astype(np.float64).sum(), np.abs(flat.astype(np.float64)).sum()], _G[f"{key}_gsum{s}"], rtol=1e-4)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16cm"])
@pytest.mark.parametrize("name", NAMES)
def test_v5_case_vs_oracle_fresh_seed(dev, name, bf16):
    _RAN_ORACLE.add((name, bf16))
    spec = lc.spec_of(_G, name)
    t = _G[f"{name}_f_targets"]
    heads = lc.heads_of(spec, spec["fresh_seed"])
    if bf16:
        heads = [torch.from_numpy(h).to(torch.bfloat16).float().numpy() for h in heads]
    lf = _loss(spec, dev)
    preds = _preds(heads, dev, bf16)
    out = lf(preds, torch.from_numpy(t).to(dev))
    grads = torch.autograd.grad(out["tot_loss"], preds)
    of = ov5.V5LossOracle(lc.anchors_of(spec), lc.hyp_of(spec, "cpu"), stage_num=spec["stages"])
    opreds = [torch.from_numpy(h).requires_grad_(True) for h in heads]
    oout = of(opreds, t)
    ograds = torch.autograd.grad(oout["tot_loss"], opreds)
    print(name, "bf16" if bf16 else "f32", "hip", _items(out), out["tar_nums"], "oracle", _items(oout), oout["tar_nums"])
    assert out["tar_nums"] == oout["tar_nums"] == _check_assign(lf, spec, t, heads, dev)
    lc.nan_equal_close(_items(out), _items(oout), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(lf.balances, of.balances, rtol=1e-5)
    for gr, og in zip(grads, ograds):
        ref = og.numpy()
        gn = gr.float().cpu().numpy()
        assert np.isfinite(gn).all()
        if bf16:
            np.testing.assert_allclose(gn, ref, rtol=6e-3, atol=1e-3 * np.abs(ref).max())
            B, Ct, hh, ww = gr.shape
            ld = gr.stride(3)
            assert ld == ((Ct + 7) // 8) * 8 and (ld == 256 or Ct != 255)
            whole = gr.as_strided((B, hh, ww, ld), (hh * ww * ld, ww * ld, ld, 1))
            assert (whole[..., Ct:] == 0).all()
        else:
            np.testing.assert_allclose(gn, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


SAT_SPEC = dict(kind="v5", img=128, B=2, stages=3, pscale=1.0, hyp=dict(num_class=3, use_focal_loss=True, focal_loss_gamma=1.5))


def saturated_case():
    """-> (heads, targets): synthetic heads whose objectness and class logits are +30 / -30 in a checkerboard over (row + column +
    channel); two boxes of class 1 and one padding row per image, sized so that every stage has positives"""
    heads = lc.heads_of(SAT_SPEC, 1601)
    E = 5 + SAT_SPEC["hyp"]["num_class"]
    for h in heads:
        yy, xx = np.mgrid[0:h.shape[2], 0:h.shape[3]]
        for ch in range(h.shape[1]):
            if ch % E >= 4:
                h[:, ch] = np.where((yy + xx + ch) % 2 == 0, 30.0, -30.0).astype(np.float32)
    t = np.full((2, 3, 6), -1.0, np.float32)
    t[0, 0] = [14, 20, 58, 70, 1, 0]
    t[0, 1] = [60, 36, 118, 110, 1, 0]
    t[1, 0] = [30, 12, 96, 64, 1, 1]
    t[1, 2] = [50, 66, 90, 120, 1, 1]          # row 1 of image 1 is the padding row
    return heads, t


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16cm"])
def test_v5_saturated_logits(dev, bf16):
    heads, t = saturated_case()          # +-30 and the targets are exact in bf16; the other logits are rounded for both sides
    if bf16:
        heads = [torch.from_numpy(h).to(torch.bfloat16).float().numpy() for h in heads]
    lf = _loss(SAT_SPEC, dev)
    preds = _preds(heads, dev, bf16)
    out = lf(preds, torch.from_numpy(t).to(dev))
    grads = torch.autograd.grad(out["tot_loss"], preds)
    of = ov5.V5LossOracle(lc.anchors_of(SAT_SPEC), lc.hyp_of(SAT_SPEC, "cpu"), stage_num=3)
    opreds = [torch.from_numpy(h).requires_grad_(True) for h in heads]
    oout = of(opreds, t)
    ograds = torch.autograd.grad(oout["tot_loss"], opreds)
    print("saturated", "bf16" if bf16 else "f32", "hip", _items(out), out["tar_nums"], "oracle", _items(oout), oout["tar_nums"])
    assert out["tar_nums"] == oout["tar_nums"] == _check_assign(lf, SAT_SPEC, t, heads, dev)
    assert np.isfinite(_items(out)).all()
    np.testing.assert_allclose(_items(out), _items(oout), rtol=1e-4, atol=1e-6)
    E = 5 + SAT_SPEC["hyp"]["num_class"]
    assigned = lf.assign(torch.from_numpy(t).to(dev), [tuple(h.shape[2:]) for h in heads])
    for s, (gr, og, h) in enumerate(zip(grads, ograds, heads)):
        ref, gn = og.numpy(), gr.float().cpu().numpy()
        assert np.isfinite(gn).all()
        if bf16:
            np.testing.assert_allclose(gn, ref, rtol=6e-3, atol=1e-3 * np.abs(ref).max())
        else:
            np.testing.assert_allclose(gn, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
        _, cls, img, anc, gy, gx = [a.cpu().numpy() for a in assigned[s]]
        assert len(cls) > 0
        obj_at_pos = h[img, anc * E + 4, gy, gx]
        assert (obj_at_pos == 30).any() and (obj_at_pos == -30).any()
        # saturated-correct class logits of the positives: t = 1, x = +30
        hot = h[img, anc * E + 5 + cls, gy, gx] == 30
        assert hot.any() and (~hot).any()
        assert (gn[img[hot], (anc * E + 5 + cls)[hot], gy[hot], gx[hot]] == 0).all()
        # saturated-correct objectness of the cells without a positive: t = 0, x = -30
        free = np.ones((h.shape[0], 3, h.shape[2], h.shape[3]), bool)
        free[img, anc, gy, gx] = False
        obj = h[:, 4::E]
        assert (gn[:, 4::E][free & (obj == -30)] == 0).all() and (free & (obj == -30)).any()
        assert (gn[:, 4::E][free & (obj == 30)] != 0).all()


def test_v5_hyper_parameters_change_the_result():
    """the one-at-a-time cases are only worth their name if each moves the reference's result away from the default's"""
    base = _G["h_default_c0_vals"]
    for name in NAMES:
        if name.startswith("h_") and name not in ("h_default", "h_stage4", "h_all"):
            assert not np.allclose(_G[f"{name}_c0_vals"], base, rtol=1e-5), name


def test_v5_num_class_124_is_refused(dev):
    """5 + nc <= 128 is the kernels' stated limit: 124 classes end in a YoloHipError from the argument check, not in a launch"""
    from yoloseries_amd._lib import YoloHipError
    _RAN_GOLDEN.add("nc124_refused")
    spec = dict(kind="v5", img=64, B=1, stages=3, pscale=1.0, hyp=dict(num_class=124))
    lf = _loss(spec, dev)
    t = torch.tensor([[[8., 8., 40., 40., 5., 0.]]], device=dev)
    with pytest.raises(YoloHipError, match="123"):
        lf(_preds(lc.heads_of(spec, 1), dev, False), t)
    with pytest.raises(YoloHipError, match="123"):
        lf.assign(t, [(8, 8), (4, 4), (2, 2)])


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_v5_backward_scale(dev, bf16):
    _RAN_GOLDEN.add("bscale_bf16" if bf16 else "bscale_f32")
    spec = lc.spec_of(_G, "h_all")
    t = _G["h_all_f_targets"]
    heads = lc.heads_of(spec, 1599)

    def run(how):
        preds = _preds(heads, dev, bf16)
        tot = _loss(spec, dev)(preds, torch.from_numpy(t).to(dev))["tot_loss"]
        if how == "unit":
            return torch.autograd.grad(tot, preds)
        if how == "mul":
            return torch.autograd.grad(tot * 3.75, preds)
        return torch.autograd.grad(tot, preds, grad_outputs=torch.tensor([3.75], dtype=torch.bfloat16, device=dev))
    unit = [g.float().cpu().numpy() for g in run("unit")]
    assert all(np.abs(u).max() > 0 for u in unit)
    rtol = 2.0 ** -7 if bf16 else 2e-6
    for how in ("mul", "grad_outputs"):
        for u, g in zip(unit, run(how)):
            np.testing.assert_allclose(g.float().cpu().numpy(), 3.75 * u, rtol=rtol, atol=rtol * 1e-3 * np.abs(u).max(), err_msg=how)


def test_zz_every_case_ran():
    """no case hides: the golden comparison ran for every v5 case named in g15 plus this module's own list, the oracle
    comparison for every case in both layouts"""
    assert _RAN_GOLDEN == set(NAMES) | set(ORACLE_ONLY)
    assert _RAN_ORACLE == {(n, b) for n in NAMES for b in (False, True)}
