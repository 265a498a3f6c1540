"""GPU parity of the YOLOX / SimOTA loss kernels (csrc/loss_yolox.hip) over hyper-parameter values and target edge cases: every
YOLOX case of tests/golden/g15_loss_edges.npz against the reference's recorded outputs, and once more against the oracle on a
seed that is not in the file (all seeds were fixed when the file was generated: no seed search here).

Bars as in test_yolox_loss_vs_oracle_640_b8: foreground masks array-equal (the reference's, which on these seeds are also the
`stable_ties` oracle's), fg_nums / tar_nums equal, loss items rtol 1e-4, balances rtol 1e-5, gradients rtol 1e-4 with atol
1e-4 * max|ref|, the caller's target tensor converted to xywh in place.

Oracle-only inputs: 16 / 17 / 128 valid boxes in one image (the matcher's rounds of 16, the 128 boxes held in LDS); 130, which
YOLOXLoss refuses with an error naming the limit; the reference's randperm fallback (loss/yolox_loss.py:270-278), where the
kernel's deterministic choice must be one the reference could have drawn and the oracle continues from the same cells; the
backward scale (see test_gpu_loss_edges.py for its bars).

Saturated logits (test_yolox_saturated_logits, use_focal_loss on): objectness and class logits of +30 / -30, where the fp32
sigmoid is exactly 1 or 1 - sigmoid is exactly 1, so that the focal factor's base is 0 and its derivative takes the branch
defined to be 0 (csrc/exact_math.h focal_factor).  Bars as above; with bf16 heads the oracle runs on the same bf16 values and
the gradients, stored in bf16, meet test_gpu_loss_edges.py's bf16 bar (rtol 6e-3, atol 1e-3 * max|ref|: half an ulp is 2^-9).  The
objectness gradient of every saturated-correct cell (foreground at +30, background at -30) is 0 as a value."""
import numpy as np
import pytest
import torch

from oracle import loss_cases as lc
from oracle.yoloxloss import YOLOXLossOracle
from yoloseries_amd.utils.synth import synth_yolox_heads

pytestmark = pytest.mark.gpu

_G = lc.load()
NAMES = [str(n) for n in _G["case_names"] if lc.spec_of(_G, str(n))["kind"] == "yolox"]
ORACLE_ONLY = ["gt16", "gt17", "gt128", "gt130_refused", "randperm_fallback", "bscale_f32", "bscale_bf16"]
_RAN_GOLDEN, _RAN_ORACLE = set(), set()


def _loss(spec, dev):
    from yoloseries_amd.loss import YOLOXLoss
    return YOLOXLoss(lc.hyp_of(spec, dev))


def _items(out):
    return np.array([out["tot_loss"].item(), out["iou_loss"], out["l1_loss"], out["cls_loss"], out["cof_loss"]], np.float64)


def _vs_oracle(dev, spec, tnp, heads, fallback_cells=None, label="", bf16=False, seen=None):
    """HIP against the stable-tie oracle on one call: masks, counts, items, balances, gradients, in-place target conversion.
    bf16: `heads` hold bf16 values and reach the kernels as bf16 tensors; seen: a dict that receives the masks and gradients"""
    lf = _loss(spec, dev)
    preds = {k: torch.from_numpy(v).to(dev).to(torch.bfloat16 if bf16 else torch.float32).requires_grad_(True) for k, v in heads.items()}
    t = torch.from_numpy(tnp.copy()).to(dev)
    out = lf(preds, t)
    masks = lf.foreground_masks()
    if callable(fallback_cells):
        fallback_cells = fallback_cells(masks)
    of = YOLOXLossOracle(lc.hyp_of(spec, "cpu"), stable_ties=True, fallback_cells=fallback_cells)
    opreds = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in heads.items()}
    ot = torch.from_numpy(tnp.copy())
    oout = of(opreds, ot)
    print(label, "hip", _items(out), out["fg_nums"], out["tar_nums"], "oracle", _items(oout), oout["fg_nums"], oout["tar_nums"])
    for s, (mk, ofg) in enumerate(zip(masks, of.last_fg)):
        np.testing.assert_array_equal(mk, ofg.numpy(), err_msg=f"foreground mask of stage {s}")
    assert out["fg_nums"] == oout["fg_nums"] and out["tar_nums"] == oout["tar_nums"]
    np.testing.assert_allclose(_items(out), _items(oout), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(lf.balances, of.balances, rtol=1e-5)
    np.testing.assert_array_equal(t.cpu().numpy(), ot.numpy())
    grads = torch.autograd.grad(out["tot_loss"], list(preds.values()))
    ograds = torch.autograd.grad(oout["tot_loss"], list(opreds.values()))
    for gr, og in zip(grads, ograds):
        r, gn = og.numpy(), gr.float().cpu().numpy()
        assert np.isfinite(gn).all()
        if bf16:
            np.testing.assert_allclose(gn, r, rtol=6e-3, atol=1e-3 * np.abs(r).max())
        else:
            np.testing.assert_allclose(gn, r, rtol=1e-4, atol=1e-4 * np.abs(r).max())
    assert np.isfinite(out["tot_loss"].item())
    if seen is not None:
        seen.update(masks=masks, grads=[g.float().cpu().numpy() for g in grads])
    return of


@pytest.mark.parametrize("name", NAMES)
def test_yolox_case_vs_reference(dev, name):
    _RAN_GOLDEN.add(name)
    spec = lc.spec_of(_G, name)
    lf = _loss(spec, dev)
    for call, seed in enumerate(spec["seeds"]):
        key = f"{name}_c{call}"
        preds = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in lc.heads_of(spec, seed).items()}
        t = torch.from_numpy(_G[f"{key}_targets"].copy()).to(dev)
        out = lf(preds, t)
        vals = _G[f"{key}_vals"]
        print(name, call, "hip", _items(out), out["fg_nums"], out["tar_nums"], "ref", vals)
        for s, mk in enumerate(lf.foreground_masks()):
            np.testing.assert_array_equal(np.packbits(mk), _G[f"{key}_fg{s}"], err_msg=f"foreground mask of stage {s}")
        assert out["fg_nums"] == vals[5] and out["tar_nums"] == vals[6]
        np.testing.assert_allclose(_items(out), vals[:5], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(lf.balances, _G[f"{key}_balances"], rtol=1e-5)
        np.testing.assert_array_equal(t.cpu().numpy(), _G[f"{key}_tars_after"])
        for s, gr in enumerate(torch.autograd.grad(out["tot_loss"], list(preds.values()))):
            gn = gr.cpu().numpy()
            assert np.isfinite(gn).all()
            if f"{key}_grad{s}" in _G:
                ref = _G[f"{key}_grad{s}"]
                assert gn.shape == ref.shape
                np.testing.assert_allclose(gn, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
            else:
                flat, ref = gn.reshape(-1), _G[f"{key}_gval{s}"]
                np.testing.assert_allclose(flat[_G[f"{key}_gidx{s}"]], ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
                np.testing.assert_allclose([flat.astype(np.float64).sum(), np.abs(flat.astype(np.float64)).sum()], _G[f"{key}_gsum{s}"], rtol=1e-4)


@pytest.mark.parametrize("name", NAMES)
def test_yolox_case_vs_oracle_fresh_seed(dev, name):
    _RAN_ORACLE.add(name)
    spec = lc.spec_of(_G, name)
    of = _vs_oracle(dev, spec, _G[f"{name}_f_targets"], lc.heads_of(spec, spec["fresh_seed"]), label=name)
    if name == "x_radius025":
        assert of.counters["ctr_is_box"] > 0


SAT_SPEC = dict(kind="yolox", img=128, B=2, hyp=dict(num_class=3, use_focal_loss=True, focal_loss_gamma=1.5))


def saturated_case():
    """-> (heads, targets): synthetic heads whose objectness and class logits are +30 / -30 in a checkerboard over (row + column +
    channel); two boxes and one padding row per image"""
    heads = lc.heads_of(SAT_SPEC, 1602)
    for h in heads.values():
        yy, xx = np.mgrid[0:h.shape[3], 0:h.shape[4]]
        for ch in range(4, h.shape[2]):
            h[:, 0, ch] = np.where((yy + xx + ch) % 2 == 0, 30.0, -30.0).astype(np.float32)
    t = np.full((2, 3, 6), -1.0, np.float32)
    t[0, 0] = [14, 20, 58, 70, 1, 0]
    t[0, 1] = [60, 36, 118, 110, 2, 0]
    t[1, 0] = [30, 12, 96, 64, 0, 1]
    t[1, 2] = [50, 66, 90, 120, 1, 1]          # row 1 of image 1 is the padding row
    return heads, t


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_yolox_saturated_logits(dev, bf16):
    heads, t = saturated_case()          # +-30 and the targets are exact in bf16; the other logits are rounded for both sides
    if bf16:
        heads = {k: torch.from_numpy(v).to(torch.bfloat16).float().numpy() for k, v in heads.items()}
    seen = {}
    _vs_oracle(dev, SAT_SPEC, t, heads, label="saturated bf16" if bf16 else "saturated f32", bf16=bf16, seen=seen)
    met = set()          # objectness logits of the foreground cells, over the stages (the 4 x 4 map has three such cells)
    for h, fg, gn in zip(heads.values(), seen["masks"], seen["grads"]):
        obj, gobj = h[:, 0, 4].reshape(-1), gn[:, 0, 4].reshape(-1)
        met |= set(obj[fg].tolist())
        assert (gobj[fg & (obj == 30)] == 0).all()          # t = 1, x = +30
        assert (gobj[~fg & (obj == -30)] == 0).all()         # t = 0, x = -30
        assert (gobj[fg & (obj == -30)] != 0).all() and (gobj[~fg & (obj == 30)] != 0).all()
    assert met == {30.0, -30.0}


def test_yolox_hyper_parameters_change_the_result():
    """the one-at-a-time cases are only worth their name if each moves the reference's result away from the default's (all of
    them share the default's targets and heads)"""
    base = _G["x_default_c0_vals"]
    same_inputs = ["x_no_l1", "x_smooth09", "x_clspw2", "x_cofpw05", "x_scales", "x_focal_g2a05", "x_iou", "x_giou", "x_topk1",
                   "x_radius025", "x_radius5"]
    for name in same_inputs:
        assert lc.spec_of(_G, name)["seeds"] == lc.spec_of(_G, "x_default")["seeds"]
        assert not np.allclose(_G[f"{name}_c0_vals"], base, rtol=1e-5), name


@pytest.mark.parametrize("n", [16, 17, 128])
def test_yolox_many_ground_truths(dev, n):
    """n valid boxes in one 640^2 image: 16 / 17 bracket the matcher's rounds of 16 ground truths, 128 is all the kernel holds"""
    _RAN_GOLDEN.add(f"gt{n}")
    spec = dict(kind="yolox", img=640, B=2, hyp={})
    t = _G[f"xo_gt{n}_targets"]
    assert int((t[0, :, 4] >= 0).sum()) == n
    of = _vs_oracle(dev, spec, t, lc.heads_of(spec, int(_G[f"xo_gt{n}_seed"][1])), label=f"gt{n}")
    assert of is not None


def test_yolox_130_ground_truths_are_refused(dev):
    """box 129 and 130 of an image must not drop out of the assignment silently: the call fails, naming the limit, before any
    launch; the same 132-row tensor with 128 valid rows in that image is accepted"""
    from yoloseries_amd._lib import YoloHipError
    _RAN_GOLDEN.add("gt130_refused")
    spec = dict(kind="yolox", img=640, B=2, hyp={})
    t = _G["xo_gt130_targets"]
    assert int((t[0, :, 4] >= 0).sum()) == 130 and t.shape[1] == 132
    heads = lc.heads_of(spec, int(_G["xo_gt130_seed"][1]))
    preds = {k: torch.from_numpy(v).to(dev) for k, v in heads.items()}
    with pytest.raises(YoloHipError, match="128"):
        _loss(spec, dev)(preds, torch.from_numpy(t.copy()).to(dev))
    t2 = t.copy()
    t2[0, 128:130] = -1
    out = _loss(spec, dev)(preds, torch.from_numpy(t2).to(dev))
    assert out["tar_nums"] == 3 * (128 + 6)


def test_yolox_randperm_fallback(dev):
    """8-12 px boxes between the cell centres of the coarser maps: the reference marks `choose_num` cells drawn at random from the
    ground truths' nearest cells.  The kernel's cells for every (stage, image) that needs the draw must be such a choice; the
    oracle then takes the same cells and everything downstream meets the usual bars, every value finite."""
    _RAN_GOLDEN.add("randperm_fallback")
    spec = dict(kind="yolox", img=128, B=2, hyp={})
    t = _G["xo_fallback_targets"]
    plan = lc.fallback_plan(t, 128)
    assert (2, 0) in plan and (2, 1) in plan          # the stride-32 map is empty for both images

    def kernel_cells(masks):
        cells = {}
        for (s, b), (near, choose) in plan.items():
            n = (128 // (8, 16, 32)[s]) ** 2
            got = masks[s].reshape(2, n)[b].nonzero()[0].tolist()
            assert len(set(near)) >= choose and len(got) == choose, ((s, b), got, near, choose)
            assert set(got) <= set(near), ((s, b), got, near)
            cells[(s, b)] = got
        return cells
    of = _vs_oracle(dev, spec, t, synth_yolox_heads(2, 128, 80, seed=int(_G["xo_fallback_seed"][0])), fallback_cells=kernel_cells,
                    label="fallback")
    assert of.counters["fallback"] == len(plan)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_yolox_backward_scale(dev, bf16):
    _RAN_GOLDEN.add("bscale_bf16" if bf16 else "bscale_f32")
    spec = lc.spec_of(_G, "x_all")
    t = _G["x_all_f_targets"]
    heads = lc.heads_of(spec, spec["fresh_seed"])

    def run(how):
        preds = {k: torch.from_numpy(v).to(dev).to(torch.bfloat16 if bf16 else torch.float32).requires_grad_(True) for k, v in heads.items()}
        tot = _loss(spec, dev)(preds, torch.from_numpy(t.copy()).to(dev))["tot_loss"]
        if how == "unit":
            return torch.autograd.grad(tot, list(preds.values()))
        if how == "mul":
            return torch.autograd.grad(tot * 3.75, list(preds.values()))
        return torch.autograd.grad(tot, list(preds.values()), grad_outputs=torch.tensor([3.75], dtype=torch.bfloat16, device=dev))
    unit = [g.float().cpu().numpy() for g in run("unit")]
    assert all(np.abs(u).max() > 0 for u in unit)
    rtol = 2.0 ** -7 if bf16 else 2e-6
    for how in ("mul", "grad_outputs"):
        for u, g in zip(unit, run(how)):
            np.testing.assert_allclose(g.float().cpu().numpy(), 3.75 * u, rtol=rtol, atol=rtol * 1e-3 * np.abs(u).max(), err_msg=how)


def test_zz_every_case_ran():
    """no case hides: the golden comparison ran for every YOLOX case named in g15 plus this module's own list, the oracle
    comparison for every case"""
    assert _RAN_GOLDEN == set(NAMES) | set(ORACLE_ONLY)
    assert _RAN_ORACLE == set(NAMES)
