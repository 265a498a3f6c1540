"""CPU: the validation metric's device path, host side.

  * `val_match_ref` — a NumPy float32 restatement of yh_val_match (csrc/metric.hip): un-letterbox + compute_tp in closed form
    (g*(p) = the same-class ground truth with the largest IoU >= 0.5, lowest row on ties; a ground truth keeps the LOWEST detection
    that chose it).  It is pinned here to the mirrored host code, mAP_v2.compute_tp, on the images of g9_map.npz and on the generated
    tables that tests/test_gpu_val_match.py gives the kernel; the GPU tests then compare the kernel with it bit for bit.
  * mAP_v2.from_matches against the fixture's results, exactly.
  * the entry point is declared and bound.

`make_case` generates the tables (seeded; shared with the GPU test) and `margins` measures the condition under which the host code,
the restatement and the kernel must agree to the bit: no same-class IoU within 1e-4 of a threshold, and no detection whose two best
same-class IoUs are closer than 1e-4.  Two IoUs that are both exactly 0 (no overlap at all: nothing to match, nothing to tie) are
not a pair in that sense; every other pair counts, matched or not.  The seeds below were searched on the CPU for that condition."""
import os
import re

import numpy as np
import pytest

from yoloseries_amd.utils.mAP import iou_np, mAP_v2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
THR = np.linspace(0.5, 0.95, 10)
NUM_CLASS = 5
MARGIN = 1e-4
F = np.float32


# ---------------------------------------------------------------------------------------------------- the restatement
def unletterbox(v, pad, scale):
    return (v.astype(F) - F(pad)) / F(scale)


def det_to_original(det, info):
    """(n, 6) letterboxed rows, info = [scale, pad_top, pad_left, org_h, org_w] -> (n, 4) float32 boxes in the original frame"""
    scale, pad_top, pad_left, org_h, org_w = (F(v) for v in info)
    hi_x, hi_y = org_w - F(1), org_h - F(1)
    x1, x2 = (np.minimum(np.maximum(unletterbox(det[:, c], pad_left, scale), F(1)), hi_x) for c in (0, 2))
    y1, y2 = (np.minimum(np.maximum(unletterbox(det[:, c], pad_top, scale), F(1)), hi_y) for c in (1, 3))
    return np.stack((x1, y1, x2, y2), axis=1)


def gt_to_original(gt, info):
    scale, pad_top, pad_left = F(info[0]), F(info[1]), F(info[2])
    return np.stack((unletterbox(gt[:, 0], pad_left, scale), unletterbox(gt[:, 1], pad_top, scale),
                     unletterbox(gt[:, 2], pad_left, scale), unletterbox(gt[:, 3], pad_top, scale)), axis=1)


def iou_rows(g, p):
    """(n_gt, 4), (n_pred, 4) -> (n_gt, n_pred) in the dtype of the boxes, the operations of iou_np one by one"""
    g = g[:, None, :]
    one = g.dtype.type
    a_g = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    a_p = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    w = np.maximum(one(0), np.minimum(g[..., 2], p[:, 2]) - np.maximum(g[..., 0], p[:, 0]))
    h = np.maximum(one(0), np.minimum(g[..., 3], p[:, 3]) - np.maximum(g[..., 1], p[:, 1]))
    inter = w * h
    return inter / np.minimum(np.maximum((a_g + a_p) - inter, one(1e-6)), one(1e7))


def match_closed_form(gt_box, gt_cls, pred_box, pred_cls, thr=THR):
    """-> (gt_idx (n_pred,) int, iou (n_pred,), tp (n_pred, len(thr)) bool); gt rows with cls < 0 are padding"""
    n_pred = len(pred_box)
    gt_idx = np.full(n_pred, -1, np.int64)
    iou = np.zeros(n_pred, pred_box.dtype)
    if len(gt_box) and n_pred:
        ious = iou_rows(gt_box, pred_box)
        ok = (ious.astype(np.float64) >= thr[0]) & (gt_cls[:, None] == pred_cls[None, :]) & (gt_cls[:, None] >= 0)
        star = np.where(ok.any(0), np.where(ok, ious, -1).argmax(0), -1)              # argmax: the lowest row on ties
        for g in np.unique(star[star >= 0]):
            p = np.nonzero(star == g)[0][0]                                          # the lowest detection keeps g
            gt_idx[p], iou[p] = g, ious[g, p]
    tp = (gt_idx >= 0)[:, None] & (iou.astype(np.float64)[:, None] >= thr[None, :])
    return gt_idx, iou, tp


def val_match_ref(det, nkeep, gt, info, out, gt_hist, thr=THR):
    """yh_val_match on NumPy tables: updates the pre-filled arrays of `out` (box conf cls iou gt_idx tp nrow) and gt_hist in place"""
    for b in range(det.shape[0]):
        nk = int(nkeep[b])
        valid = gt[b, :, 4] >= 0
        counts = nk > 0 and valid.any()
        out["nrow"][b] = nk if counts else 0
        if not counts:
            continue
        gt_hist += np.bincount(gt[b, valid, 4].astype(np.int64), minlength=len(gt_hist)).astype(gt_hist.dtype)
        d = det[b, :nk]
        box = det_to_original(d, info[b])
        gt_idx, iou, tp = match_closed_form(gt_to_original(gt[b], info[b]), gt[b, :, 4], box, d[:, 5], thr)
        out["box"][b, :nk], out["conf"][b, :nk], out["cls"][b, :nk] = box, d[:, 4], d[:, 5].astype(np.int32)
        out["iou"][b, :nk], out["gt_idx"][b, :nk] = iou, gt_idx
        out["tp"][b, :nk] = (tp.astype(np.uint16) << np.arange(len(thr), dtype=np.uint16)).sum(1).astype(np.uint16)
    return out


SENTINEL = dict(box=(F, -7.0, (4,)), conf=(F, -7.0, ()), cls=(np.int32, -77, ()), iou=(F, -7.0, ()), gt_idx=(np.int32, -77, ()),
                tp=(np.uint16, 0xABCD, ()))


def sentinel_outputs(B, max_keep):
    out = {k: np.full((B, max_keep) + tail, v, dtype=dt) for k, (dt, v, tail) in SENTINEL.items()}
    out["nrow"] = np.full(B, -77, np.int32)
    return out


def host_lists(det, nkeep, gt, info):
    """what val_yolov5.py hands mAP_v2: per image the valid ground truth (n, 5) and the detections (m, 6) in the original frame"""
    gts, preds = [], []
    for b in range(det.shape[0]):
        g = gt[b][gt[b, :, 4] >= 0]
        gts.append(np.concatenate((gt_to_original(g, info[b]), g[:, 4:5]), axis=1).astype(F))
        d = det[b, :int(nkeep[b])]
        preds.append(np.concatenate((det_to_original(d, info[b]), d[:, 4:6]), axis=1).astype(F))
    return gts, preds


# ---------------------------------------------------------------------------------------------------- generated tables
INFO = np.array([[0.83, 12, 37, 300, 420], [0.83, 20, 5, 310, 400], [0.5, 3, 50, 500, 640], [1.25, 8, 16, 200, 260]], F)
NKEEP = (300, 70, 1, 0)
# (maxbox, image with nothing but padding) -> seed for which `margins` holds on every row
CASES = {"maxbox70": (70, 2), "maxbox600": (600, 1)}
SEEDS = {"maxbox70": 8, "maxbox600": 3}
# rows of image 0 that make_case builds by hand (detections) and the ground-truth rows they refer to, by position among the valid
P_CONTEST_LO, P_CONTEST_HI, P_TWO_GT, P_OTHER_CLS, P_CLAMP_LO, P_CLAMP_HI = range(6)


def _shift(box, dx, dy):
    return box + np.array([dx, dy, dx, dy], F)


def make_case(name, seed=None, max_keep=300):
    """-> dict(det (4, max_keep, 6), nkeep, gt (4, maxbox, 6), info, special): float32 tables in the letterboxed frame.  Rows of det
    past nkeep hold random numbers, padding rows of gt hold a copy of a valid box (cls -1) and column 5 of gt is noise: none of it
    may show in the result."""
    maxbox, only_padding = CASES[name]
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    B = len(NKEEP)
    det = rng.uniform(-50, 500, (B, max_keep, 6)).astype(F)
    det[..., 5] = rng.integers(0, NUM_CLASS, (B, max_keep))
    gt = np.zeros((B, maxbox, 6), F)
    gt[..., 4] = -1
    gt[..., 5] = rng.uniform(-3, 3, (B, maxbox))
    special = {}
    for b in range(B):
        scale, pad_top, pad_left, org_h, org_w = (float(v) for v in INFO[b])
        W, H = org_w * scale, org_h * scale                        # the image's area inside the letterboxed frame
        nv = 0 if b == only_padding else max(8, maxbox // 2)
        rows = np.sort(rng.choice(maxbox, nv, replace=False))      # padding rows end up between the valid ones
        wh = rng.uniform(15, 70, (nv, 2))
        xy = rng.uniform(0, 1, (nv, 2)) * (np.array([W, H]) - wh) + np.array([pad_left, pad_top])
        boxes = np.concatenate((xy, xy + wh), axis=1).astype(F)
        cls = rng.integers(0, NUM_CLASS, nv).astype(F)
        if b == 0:
            o = np.array([pad_left, pad_top, pad_left, pad_top], F)
            boxes[0], cls[0] = o + np.array([10, 10, 70, 60], F), 0          # A: contested by two detections
            boxes[1], cls[1] = o + np.array([120, 15, 180, 75], F), 1        # C and D: two ground truths under one detection
            boxes[2], cls[2] = _shift(boxes[1], 8, 0), 1
            boxes[3], cls[3] = o + np.array([220, 20, 270, 60], F), 2        # E: a detection of another class sits on it
            special = dict(gt_a=int(rows[0]), gt_c=int(rows[1]), gt_d=int(rows[2]), gt_e=int(rows[3]))
        if nv:
            gt[b, :, :4] = boxes[rng.integers(0, nv, maxbox)]                # tempting padding
            gt[b, rows, :4], gt[b, rows, 4] = boxes, cls
        nk = NKEEP[b]
        for p in range(nk):
            if nv and (p == 0 or rng.uniform() < 0.6):                       # near a ground truth, mostly of its class
                g = rng.integers(0, nv)
                size = np.tile(boxes[g, 2:] - boxes[g, :2], 2)
                det[b, p, :4] = boxes[g] + rng.uniform(-0.12, 0.12, 4) * size
                det[b, p, 5] = cls[g] if rng.uniform() < 0.9 else rng.integers(0, NUM_CLASS)
            else:
                wh1 = rng.uniform(15, 70, 2)
                xy1 = rng.uniform(0, 1, 2) * (np.array([W, H]) - wh1) + np.array([pad_left, pad_top])
                det[b, p, :4] = np.concatenate((xy1, xy1 + wh1))
        det[b, :nk, 4] = np.sort(rng.uniform(0.05, 1, nk))[::-1]
        if b == 0:
            det[0, P_CONTEST_LO, :4], det[0, P_CONTEST_LO, 5] = _shift(boxes[0], 9, 7), 0        # IoU ~ 0.6: the lower row wins A
            det[0, P_CONTEST_HI, :4], det[0, P_CONTEST_HI, 5] = _shift(boxes[0], 1, 1), 0        # IoU ~ 0.93: ends up unmatched
            det[0, P_TWO_GT, :4], det[0, P_TWO_GT, 5] = _shift(boxes[1], 3, 0), 1
            det[0, P_OTHER_CLS, :4], det[0, P_OTHER_CLS, 5] = _shift(boxes[3], 1, 0), 3
            det[0, P_CLAMP_LO, :4] = [pad_left - 20, pad_top - 15, pad_left + 40, pad_top + 35]
            det[0, P_CLAMP_HI, :4] = [pad_left + W - 40, pad_top + H - 30, pad_left + W + 25, pad_top + H + 18]
    return dict(det=det, nkeep=np.array(NKEEP, np.int32), gt=gt, info=INFO.copy(), special=special, maxbox=maxbox,
                only_padding=only_padding)


def margins(gts, preds):
    """over the images that count -> (smallest distance of a same-class IoU to a threshold, smallest gap between a detection's two
    best same-class IoUs; pairs that are both exactly 0 left out).  gts (n, 5) / preds (m, 6) in the original frame."""
    d_thr, d_pair = np.inf, np.inf
    for g, p in zip(gts, preds):
        if not len(g) or not len(p):
            continue
        ious = iou_rows(g[:, :4], p[:, :4]).astype(np.float64)
        same = g[:, 4][:, None] == p[:, 5][None, :]
        if same.any():
            d_thr = min(d_thr, np.abs(ious[same][:, None] - THR[None, :]).min())
        top = np.sort(np.where(same, ious, -1.0), axis=0)[::-1]
        if top.shape[0] >= 2:
            pair = (top[1] >= 0) & (top[0] > 0)
            if pair.any():
                d_pair = min(d_pair, (top[0] - top[1])[pair].min())
    return d_thr, d_pair


def find_seed(name, tries=4000):
    """the search that produced SEEDS (python -c "import test_val_match_host as t; print(t.find_seed('maxbox70'))")"""
    for seed in range(tries):
        c = make_case(name, seed)
        if min(margins(*host_lists(c["det"], c["nkeep"], c["gt"], c["info"]))) < MARGIN:
            continue
        try:
            assert_required_content(c, run_ref(c)[0])
        except AssertionError:
            continue
        return seed
    raise RuntimeError(name)


def assert_margins(gts, preds):
    d_thr, d_pair = margins(gts, preds)
    assert d_thr >= MARGIN, f"a same-class IoU lies {d_thr:.2e} from a threshold"
    assert d_pair >= MARGIN, f"a detection's two best same-class IoUs differ by {d_pair:.2e}"


def assert_required_content(c, out):
    """the rows make_case builds by hand do what they are there for (on the restatement's result)"""
    s, gi, box = c["special"], out["gt_idx"][0], out["box"][0]
    gts, preds = host_lists(c["det"], c["nkeep"], c["gt"], c["info"])
    valid_rows = np.nonzero(c["gt"][0, :, 4] >= 0)[0]
    ious = iou_rows(gts[0][:, :4], preds[0][:, :4])
    pos = {k: int(np.searchsorted(valid_rows, v)) for k, v in s.items()}
    assert ious[pos["gt_a"], P_CONTEST_LO] + 0.2 < ious[pos["gt_a"], P_CONTEST_HI], "the lower row must have the lower IoU"
    assert gi[P_CONTEST_LO] == s["gt_a"] and gi[P_CONTEST_HI] == -1 and out["tp"][0, P_CONTEST_HI] == 0
    assert ious[pos["gt_c"], P_TWO_GT] >= 0.5 and ious[pos["gt_d"], P_TWO_GT] >= 0.5 and gi[P_TWO_GT] == s["gt_c"]
    assert ious[pos["gt_e"], P_OTHER_CLS] > 0.9 and gi[P_OTHER_CLS] != s["gt_e"]
    org_h, org_w = c["info"][0, 3], c["info"][0, 4]
    assert box[P_CLAMP_LO, 0] == 1 and box[P_CLAMP_LO, 1] == 1
    assert box[P_CLAMP_HI, 2] == org_w - 1 and box[P_CLAMP_HI, 3] == org_h - 1
    assert (out["gt_idx"][0, :300] >= 0).sum() > 20 and (out["gt_idx"][0, :300] < 0).sum() > 20


def run_ref(c):
    out, hist = sentinel_outputs(*c["det"].shape[:2]), np.zeros(NUM_CLASS, np.int32)
    return val_match_ref(c["det"], c["nkeep"], c["gt"], c["info"], out, hist), hist


# ---------------------------------------------------------------------------------------------------- closed form == compute_tp
def g9_lists():
    g = np.load(os.path.join(G, "g9_map.npz"), allow_pickle=False)
    n = int(g["n"])
    return g, [g[f"gt{i}"] for i in range(n)], [g[f"pred{i}"] for i in range(n)]


def test_closed_form_equals_compute_tp_on_the_fixture():
    _, gts, preds = g9_lists()
    m, seen = mAP_v2([], []), 0
    for g, p in zip(gts, preds):
        if len(g) and len(p):
            np.testing.assert_array_equal(iou_rows(g[:, :4], p[:, :4]), iou_np(g[:, :4], p[:, :4]))
            np.testing.assert_array_equal(match_closed_form(g[:, :4], g[:, 4], p[:, :4], p[:, 5])[2], m.compute_tp(g, p))
            seen += int(m.compute_tp(g, p).any())
    assert seen >= 5


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_host_code_on_the_generated_tables(name):
    c = make_case(name)
    gts, preds = host_lists(c["det"], c["nkeep"], c["gt"], c["info"])
    assert_margins(gts, preds)
    out, hist = run_ref(c)
    assert_required_content(c, out)
    m = mAP_v2([], [])
    want_hist = np.zeros(NUM_CLASS, np.int64)
    for b, (g, p) in enumerate(zip(gts, preds)):
        nk = int(c["nkeep"][b])
        if not (len(g) and len(p)):
            assert out["nrow"][b] == 0 and (out["tp"][b] == 0xABCD).all() and (out["box"][b] == -7).all()
            continue
        bits = (m.compute_tp(g, p).astype(np.uint16) << np.arange(10, dtype=np.uint16)).sum(1)
        np.testing.assert_array_equal(out["tp"][b, :nk], bits)
        np.testing.assert_array_equal(out["box"][b, :nk], p[:, :4])
        assert out["nrow"][b] == nk and (out["tp"][b, nk:] == 0xABCD).all()
        want_hist += np.bincount(g[:, 4].astype(np.int64), minlength=NUM_CLASS)
    np.testing.assert_array_equal(hist, want_hist)
    assert out["nrow"][c["only_padding"]] == 0 and out["nrow"][3] == 0


# ---------------------------------------------------------------------------------------------------- mAP_v2.from_matches
def tables_from_lists(gts, preds, num_class):
    """what MatchAccumulator.finish() returns, from compute_tp on box lists (images without ground truth or detections dropped)"""
    m = mAP_v2([], [])
    keep = [(np.asarray(g), np.asarray(p)) for g, p in zip(gts, preds) if len(g) and len(p)]
    tp = np.concatenate([m.compute_tp(g, p) for g, p in keep], axis=0)
    conf = np.concatenate([p[:, 4] for _, p in keep])
    cls = np.concatenate([p[:, 5] for _, p in keep]).astype(np.int32)
    hist = np.bincount(np.concatenate([g[:, 4] for g, _ in keep]).astype(np.int64), minlength=num_class)
    return conf, cls, tp, hist


def _assert_fixture(m, g):
    r = m.compute_ap_per_class()
    for k in ("ap", "precision", "recall", "f1", "unique_cls"):
        np.testing.assert_array_equal(r[k], g[k])
    np.testing.assert_array_equal(np.array(m.get_mean_metrics()), g["mean"])


def test_from_matches_returns_the_fixture_results():
    g, gts, preds = g9_lists()
    _assert_fixture(mAP_v2.from_matches(*tables_from_lists(gts, preds, 80)), g)
    _assert_fixture(mAP_v2(gts, preds), g)                        # the list constructor shares the code and is unchanged


def test_images_without_predictions_or_ground_truth_change_nothing():
    g, gts, preds = g9_lists()
    gts = gts + [np.array([[10, 10, 50, 50, 1]], F), np.zeros((0, 5), F)]
    preds = preds + [np.zeros((0, 6), F), np.array([[10, 10, 50, 50, 0.9, 1]], F)]
    _assert_fixture(mAP_v2.from_matches(*tables_from_lists(gts, preds, 80)), g)
    _assert_fixture(mAP_v2(gts, preds), g)


def test_from_matches_takes_the_packed_table_too():
    """(N, 10) bool is the contract; other integer types of the classes, the table and the histogram give the same"""
    g, gts, preds = g9_lists()
    conf, cls, tp, hist = tables_from_lists(gts, preds, 80)
    _assert_fixture(mAP_v2.from_matches(conf, cls.astype(np.int64), tp.astype(np.uint8), hist.astype(np.int32)), g)


# ---------------------------------------------------------------------------------------------------- the entry point
def test_val_match_is_declared_and_bound():
    import ctypes as C
    from yoloseries_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yolohip.h")).read()
    proto = re.search(r"\bint\s+yh_val_match\s*\(([^;]*)\)\s*;", hdr)
    assert proto, "include/yolohip.h does not declare yh_val_match"
    assert "yh_val_match" in _lib.EXPORTED_SYMBOLS
    res, args = _lib._SIGS["yh_val_match"]
    assert res is C.c_int32 and len(args) == len(re.sub(r"/\*.*?\*/", "", proto.group(1)).split(",")) == 20
    assert args[9] == C.POINTER(C.c_double)
