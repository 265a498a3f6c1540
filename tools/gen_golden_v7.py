#!/usr/bin/env python3
"""Generate tests/golden/g22_v7loss.npz by RUNNING THE REFERENCE's YOLOV7Loss (loss/yolov7_loss.py) on the CPU in fp32.

Runs only where /root/reference exists; the reference is imported read-only with the shims of tools/gen_golden.py.  Only data
is written: per case the arguments and the head seed (yoloseries_amd.utils.synth.synth_head_outputs), the targets verbatim, the
five outputs, `balances` after the call, the gradient of tot_loss w.r.t. every head tensor, the matched rows per stage
(img, anchor, gy, gx, target row) and, beside them, the row whose anchor match produced each matched candidate (`src`) and the
dynamic_k of every (stage, image, row) (`dynk`: stage, image, row, dynamic_k, min(topk, Xp)), read from the reference's own
`dynamick` tensor inside simple_ota and asserted equal to the restatement's.

The reference returns the matched rows image by image; they are stored in candidate order (the order of the stage's candidate
list), which is the order the library keeps.  Every case: anchor_match_thr 4.0, the COCO anchors (a fourth row for four stages),
logits N(0, 1) x scale.  Cases:
  a  128^2, maps 16 / 8 / 4, B 2, M 4, nc 5, topk 10
  b  64^2, maps 8 / 4 / 2, B 3, M 3, nc 3, topk 10
  c  128^2, four stages (maps 16 / 8 / 4 / 2), otherwise as a: the x 1.4 and s = 3 / 4 path
  d  as a, logits x 3
  e  as a, topk 1, one valid box in one image
  f  as a, every row padding: N = 0, only the objectness term is non-zero
  g  as a, inputs rounded to bf16 first
  h  as a, cls_pos_weight 2.5, cof_pos_weight 1.5, focal on with gamma 2.0 / alpha 0.4, scales 2.0 / 1.0 / 1.0,
     use_iou_as_tar_cof false (stored as `h_hyp`, JSON)
  i  as a, nc 1
  j  256^2, B 2, M 1, one small box per image, logits x 0.05: some dynamic_k is strictly below min(topk, Xp)
  k  as a, two consecutive calls on one instance with different heads (seed, seed + 50); the SECOND call's values, gradients,
     rows and balances are stored: the stateful EMA
Odd images have one padding row (except e, f, j).

The seed of a case is searched until the fixture sits on no decision boundary (tools/v7loss_restated.fixture_conditions,
evaluated on the restatement's fp32 cost matrices); ASSERTED for the stored seed:
  (i)   for every target with dynamic_k < Xp the k-th and (k+1)-th smallest costs differ by >= 1e-3 relative;
  (ii)  at every multiply-taken candidate the best and the second-best target cost differ by >= 1e-3 relative;
  (iii) every sum truncated to dynamic_k lies >= 1e-3 from an integer whenever it is below the cap;
  (iv)  cases a and b have a duplicated cell whose copies are both matched, and a candidate that goes to another row than the
        one that produced it; case j has a dynamic_k below its cap;
and the restatement's matched rows equal the reference's.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_v7.py
"""
import json
import os
import sys

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g22_v7loss.npz")

A_ = dict(img=128, B=2, M=4, nc=5, nstage=3, scale=1.0, topk=10, bf16=0, boxes=None, calls=1, box=(0.15, 0.55))
CASES = {
    "a": dict(A_),
    "b": dict(A_, img=64, B=3, M=3, nc=3),
    "c": dict(A_, nstage=4),
    "d": dict(A_, scale=3.0),
    "e": dict(A_, topk=1, boxes=[1, 0]),
    "f": dict(A_, boxes=[0, 0]),
    "g": dict(A_, bf16=1),
    "h": dict(A_, hyp=dict(cls_pos_weight=2.5, cof_pos_weight=1.5, use_focal_loss=True, focal_loss_gamma=2.0, focal_loss_alpha=0.4,
                           iou_loss_scale=2.0, cof_loss_scale=1.0, cls_loss_scale=1.0, use_iou_as_tar_cof=False)),
    "i": dict(A_, nc=1),
    "j": dict(A_, img=256, M=1, scale=0.05, boxes=[1, 1], box=(0.04, 0.08)),
    "k": dict(A_, calls=2),
}


def make_targets(c, seed):
    rs = np.random.RandomState(seed)
    img, B, M = c["img"], c["B"], c["M"]
    t = -np.ones((B, M, 6), np.float32)
    for b in range(B):
        n = c["boxes"][b] if c["boxes"] is not None else (M - 1 if b % 2 else M)
        wh = rs.uniform(c["box"][0], c["box"][1], (n, 2)) * img
        ctr = rs.uniform(0.2, 0.8, (n, 2)) * img
        t[b, :n, 0:2] = np.clip(ctr - wh / 2, 0, img)
        t[b, :n, 2:4] = np.clip(ctr + wh / 2, 0, img)
        t[b, :n, 4] = rs.randint(0, c["nc"], n)
        t[b, :n, 5] = b
    return t


def make_hyp(c):
    from tools.v7loss_restated import BASE_HYP
    return dict(BASE_HYP, topk=c["topk"], num_class=c["nc"], input_img_size=[c["img"], c["img"]], device="cpu", **c.get("hyp", {}))


def ref_layout(head, nc):
    """(B, A*(5+nc), h, w) -> the reference's (B, A, h, w, 5+nc)"""
    B, _, h, w = head.shape
    return head.reshape(B, 3, 5 + nc, h, w).permute(0, 1, 3, 4, 2)


def candidate_order(ref_rows, cand):
    """the reference's matched rows of one stage (image by image, each image in candidate order) -> the same rows in the order of
    the stage's candidate list `cand` (img, anchor, gy, gx, src row), and the position of each inside it"""
    pos = []
    for b in sorted(set(ref_rows[:, 0].tolist())):
        rows = ref_rows[ref_rows[:, 0] == b]
        q = 0
        for r in rows:                                   # a subsequence of the image's candidates: first fit
            while not (cand[q, 0] == b and (cand[q, :4] == r[:4]).all()):
                q += 1
            pos.append(q)
            q += 1
    pos = np.array(pos, np.int64)
    o = np.argsort(pos, kind="stable")
    return ref_rows[o], pos[o]


def run_reference(ref_loss, c, seed, tars):
    """-> dict of what is stored, from the reference alone"""
    import torch
    from tools.v7loss_restated import anchors_for, case_heads
    anchors = anchors_for(c["nstage"])
    lf = ref_loss.YOLOV7Loss(anchors, make_hyp(c), stage_num=c["nstage"])
    rows = []
    inner = lf.simple_ota

    dynk = []
    real_clamp = torch.clamp

    def spy(batch_size, anchor_stage, ds_scale, preds, org_tar, *a):
        # simple_ota's only torch.clamp of an int tensor is `dynamick` (:316), once per image in image order: recorded from the
        # reference itself as (stage, image, row, dynamic_k, min(topk, Xp))
        seen = []

        def clamp_spy(x, *ca, **ck):
            y = real_clamp(x, *ca, **ck)
            if x.dtype == torch.int32:
                seen.append((y.clone(), int(ca[1])))
            return y
        torch.clamp = clamp_spy
        try:
            out = inner(batch_size, anchor_stage, ds_scale, preds, org_tar, *a)
        finally:
            torch.clamp = real_clamp
        assert len(seen) == batch_size
        for b, (k, kk) in enumerate(seen):
            vrows = torch.nonzero(org_tar[b, :, 4] >= 0)[:, 0]
            if kk > 0:
                dynk.extend((len(rows), b, int(vrows[t]), int(k[t]), kk) for t in range(len(vrows)))
        tbox, tcls, img, anc, gy, gx = out
        # the matched target row: the valid row of the image whose box, in stage units relative to the cell, is tbox
        fm_h, fm_w = preds.size(2), preds.size(3)
        trow = []
        for i in range(len(img)):
            t = org_tar[img[i]]
            w = (t[:, 2] - t[:, 0]) / lf.input_img_size[0] * fm_w
            h = (t[:, 3] - t[:, 1]) / lf.input_img_size[1] * fm_h
            hit = torch.nonzero((t[:, 4] >= 0) & (w == tbox[i, 2]) & (h == tbox[i, 3]) & (t[:, 4] == tcls[i]))[:, 0]
            assert len(hit) == 1, "ambiguous target row"
            trow.append(int(hit[0]))
        rows.append(torch.stack((img, anc, gy, gx, torch.tensor(trow, dtype=torch.long)), 1).numpy() if len(img) else np.zeros((0, 5), np.int64))
        return out
    lf.simple_ota = spy
    for call in range(c["calls"]):
        rows.clear()
        dynk.clear()
        heads = [h.clone().requires_grad_(True) for h in case_heads(c["B"], c["img"], c["nc"], c["nstage"], seed + 50 * call, c["scale"], c["bf16"])]
        out = lf({f"p{s}": ref_layout(h, c["nc"]) for s, h in enumerate(heads)}, tars.clone())
    grads = torch.autograd.grad(out["tot_loss"], heads)
    vals = np.array([out["tot_loss"].item(), out["iou_loss"], out["cof_loss"], out["cls_loss"], out["tar_nums"]], np.float64)
    assert np.isfinite(vals).all()
    return dict(vals=vals, balances=np.array(lf.balances, np.float64), grads=[g.numpy() for g in grads], rows=list(rows),
                dynk=np.array(dynk, np.int32).reshape(-1, 5))


def restate(c, seed, tars):
    import torch
    from tools.v7loss_restated import anchors_for, case_heads, v7loss_restated
    bal, out = None, None
    for call in range(c["calls"]):
        heads = case_heads(c["B"], c["img"], c["nc"], c["nstage"], seed + 50 * call, c["scale"], c["bf16"])
        with torch.no_grad():
            out = v7loss_restated(heads, tars, anchors_for(c["nstage"]), make_hyp(c), torch.float32, balances=bal)
        bal = out["balances"]
    return out


def main():
    if not os.path.isdir(REF):
        sys.exit("tools/gen_golden_v7.py needs /root/reference (build container only)")
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_golden import install_shims
    install_shims()
    sys.path.insert(0, REF)
    sys.path.insert(1, ROOT)
    import torch
    import loss as ref_loss
    from tools.v7loss_restated import ARG_NAMES, anchors_for, fixture_conditions, v5_candidates
    torch.set_num_threads(8)
    g = {}
    for name, c in CASES.items():
        seed0 = 2200 + 1000 * (ord(name) - ord("a"))
        for seed in range(seed0, seed0 + 1000):
            tars = torch.from_numpy(make_targets(c, seed + 1))
            out = restate(c, seed, tars)
            why, facts = fixture_conditions(out)
            if why is None and name in ("a", "b") and not (facts["dup_both"] and facts["moved"]):
                why = "no doubly matched duplicate cell / no candidate that changed rows"
            if why is None and name == "j" and not facts["dynk_below_cap"]:
                why = "no dynamic_k below its cap"
            if why is None:
                break
        else:
            sys.exit(f"case {name}: no seed in {seed0}..{seed0 + 999} meets the conditions ({why})")
        r = run_reference(ref_loss, c, seed, tars)
        hyp = make_hyp(c)
        dynk = []
        for s in range(c["nstage"]):
            fh = fw = c["img"] // (8 << s)
            cand = v5_candidates(tars, anchors_for(c["nstage"])[s] / (c["img"] / fw), fw, fh, [float(c["img"])] * 2, hyp["anchor_match_thr"]).numpy()
            rows, pos = candidate_order(r["rows"][s], cand)
            np.testing.assert_array_equal(rows, out["matches"][s], err_msg=f"case {name} stage {s}: restatement != reference")
            g[f"{name}_rows{s}"] = rows.astype(np.int32)
            g[f"{name}_src{s}"] = cand[pos, 4].astype(np.int32)
            g[f"{name}_grad{s}"] = r["grads"][s]
            for b, i in enumerate(out["info"][s]):
                if i is not None:
                    dynk += [(s, b, int(i["vrows"][t]), int(i["dynk"][t]), i["kk"]) for t in range(len(i["vrows"]))]
        assert int(r["vals"][4]) == out["tar_nums"]
        g[f"{name}_args"] = np.array([c["img"], c["B"], c["M"], c["nc"], c["nstage"], c["topk"], c["bf16"], seed, c["calls"]], np.int64)
        g[f"{name}_scale"] = np.array([c["scale"]], np.float64)
        if "hyp" in c:
            g[f"{name}_hyp"] = np.array(json.dumps(c["hyp"]))
        g[f"{name}_targets"], g[f"{name}_vals"], g[f"{name}_balances"] = tars.numpy(), r["vals"], r["balances"]
        np.testing.assert_array_equal(r["dynk"], np.array(dynk, np.int32).reshape(-1, 5), err_msg=f"case {name}: dynamic_k, restatement != reference")
        g[f"{name}_dynk"] = r["dynk"]                            # the reference's own values
        print(f"case {name}: seed {seed}, vals {r['vals']}, balances {r['balances']}, facts {facts}")
    g["arg_names"] = np.array(ARG_NAMES)
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
