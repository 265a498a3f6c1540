"""yh_val_match (csrc/metric.hip) against its NumPy restatement (tests/test_val_match_host.py val_match_ref, which that file pins to
mAP_v2.compute_tp) on generated tables — no model here.  Bars: every output bit for bit (assert_array_equal): the kernel's
operation order is specified, so nothing is left to a tolerance.

Shapes, the smallest that reach every branch: B = 4, max_keep = 300 with nkeep = 300 (more than one pass of the 256-thread
workgroup), 70, 1 and 0; maxbox = 70 (more than one wave of ground truth) and 600 (more than one staged chunk of 512); gt_ld = 6;
padding rows between the valid ones, one image with padding only; pad_top != pad_left, org_h != org_w, scales 0.83 / 0.5 / 1.25.
The generator builds the contested ground truth (the lower detection has the lower IoU and wins), the detection over two ground
truths, the detection on a ground truth of another class and the detections that clamp at the four borders; the margin condition
(no same-class IoU within 1e-4 of a threshold, no two best IoUs of a detection within 1e-4) is asserted on the restatement first."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_val_match_host import (CASES, NUM_CLASS, THR, assert_margins, assert_required_content, host_lists, make_case, run_ref,
                                 sentinel_outputs, val_match_ref)

gpu = pytest.mark.gpu
KEYS = ("box", "conf", "cls", "iou", "gt_idx", "tp", "nrow")


def launch(dev, c, out_h, hist_d, thr=THR, n_thr=None, gt_ld=None, null=None):
    """one yh_val_match over the tables of `c` into device copies of `out_h` -> (status, outputs as NumPy)"""
    from yoloseries_amd import _lib
    t = {k: torch.from_numpy(c[k]).to(dev) for k in ("det", "nkeep", "gt", "info")}
    o = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).to(dev) for k, v in out_h.items()}
    B, K = c["det"].shape[:2]
    ptr = {k: (None if k == null else o[k].data_ptr()) for k in KEYS}
    thr_c = (C.c_double * 17)(*(list(thr) + [2.0] * (17 - len(thr))))
    rc = _lib.lib().yh_val_match(t["det"].data_ptr(), t["nkeep"].data_ptr(), t["gt"].data_ptr(), t["info"].data_ptr(), B, K,
                                 c["gt"].shape[1], c["gt"].shape[2] if gt_ld is None else gt_ld, NUM_CLASS, thr_c,
                                 len(thr) if n_thr is None else n_thr, ptr["box"], ptr["conf"], ptr["cls"], ptr["iou"], ptr["gt_idx"],
                                 ptr["tp"], ptr["nrow"], None if null == "gt_hist" else hist_d.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["tp"] = got["tp"].view(np.uint16)
    return rc, got


def assert_same(got, want):
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_restatement_bit_for_bit(dev, name):
    """every output, the sentinel in the rows the kernel must leave alone included; a second call accumulates gt_hist"""
    c = make_case(name)
    assert_margins(*host_lists(c["det"], c["nkeep"], c["gt"], c["info"]))
    want, want_hist = run_ref(c)
    assert_required_content(c, want)
    B, K = c["det"].shape[:2]
    assert want["nrow"].tolist() == [300, 0 if c["only_padding"] == 1 else 70, 0 if c["only_padding"] == 2 else 1, 0]
    hist = torch.zeros(NUM_CLASS, dtype=torch.int32, device=dev)
    rc, got = launch(dev, c, sentinel_outputs(B, K), hist)
    assert rc == 0
    assert_same(got, want)
    for k in ("box", "conf", "iou"):                                # bit-equal, NaN-proof
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
    for b in range(B):                                              # untouched rows: past nrow, and all rows of dropped images
        for k in KEYS[:-1]:
            assert (got[k][b, want["nrow"][b]:] == sentinel_outputs(1, 1)[k].reshape(-1)[0]).all(), (k, b)
    np.testing.assert_array_equal(hist.cpu().numpy(), want_hist)
    assert want_hist.sum() == sum((c["gt"][b, :, 4] >= 0).sum() for b in range(B) if want["nrow"][b] > 0) > 0
    rc, got2 = launch(dev, c, sentinel_outputs(B, K), hist)
    assert rc == 0
    assert_same(got2, want)
    np.testing.assert_array_equal(hist.cpu().numpy(), 2 * want_hist)


@gpu
def test_identical_ground_truth_rows_match_the_lowest_and_launches_agree(dev):
    """an exact IoU tie between two ground truths is outside the host code's contract; the kernel takes the lowest row, every time"""
    c = make_case("maxbox70")
    valid = np.nonzero(c["gt"][0, :, 4] >= 0)[0]
    lo, hi = int(valid[4]), int(valid[9])
    c["gt"][0, hi, :5] = c["gt"][0, lo, :5]                         # two identical rows, the copy at the higher index
    c["det"][0, 7, :4], c["det"][0, 7, 5] = c["gt"][0, lo, :4] + np.float32(1.5), c["gt"][0, lo, 4]
    B, K = c["det"].shape[:2]
    want, _ = run_ref(c)
    runs = [launch(dev, c, sentinel_outputs(B, K), torch.zeros(NUM_CLASS, dtype=torch.int32, device=dev)) for _ in range(2)]
    assert runs[0][0] == 0 and runs[1][0] == 0
    gi = runs[0][1]["gt_idx"][0]
    assert (gi == lo).sum() == 1 and (gi != hi).all(), "the copy at the higher row must stay unmatched"
    assert_same(runs[0][1], want)
    assert_same(runs[1][1], runs[0][1])


@gpu
def test_bad_arguments_return_einval_and_launch_nothing(dev):
    from yoloseries_amd import _lib
    c = make_case("maxbox70")
    B, K = c["det"].shape[:2]
    hist = torch.zeros(NUM_CLASS, dtype=torch.int32, device=dev)
    for kw, word in ((dict(n_thr=0), "n_thr"), (dict(n_thr=17), "n_thr"), (dict(gt_ld=4), "gt_ld"), (dict(null="tp"), "null"),
                     (dict(null="gt_hist"), "null")):
        rc, got = launch(dev, c, sentinel_outputs(B, K), hist, **kw)
        msg = _lib.lib().yh_last_error().decode()
        assert rc == -1 and "yh_val_match" in msg and word in msg, (kw, rc, msg)
        assert_same(got, sentinel_outputs(B, K))
        assert int(hist.sum()) == 0
    with pytest.raises(_lib.YoloHipError, match="gt_ld"):
        _lib.check(launch(dev, c, sentinel_outputs(B, K), hist, gt_ld=4)[0], "yh_val_match")


@gpu
def test_fewer_thresholds_set_fewer_bits(dev):
    """n_thr < 10: thr[0] still gates the match, bits at and past n_thr stay clear"""
    c = make_case("maxbox70")
    B, K = c["det"].shape[:2]
    want = val_match_ref(c["det"], c["nkeep"], c["gt"], c["info"], sentinel_outputs(B, K), np.zeros(NUM_CLASS, np.int32), THR[:3])
    rc, got = launch(dev, c, sentinel_outputs(B, K), torch.zeros(NUM_CLASS, dtype=torch.int32, device=dev), thr=THR[:3])
    assert rc == 0 and (want["tp"][0] < 8).all() and (want["tp"][0] == 7).any()
    assert_same(got, want)
