"""yh_val_ap (csrc/metric.hip) against its NumPy restatement (tests/test_val_ap_host.py val_ap_ref, which that file pins to
mAP_v2.compute_ap_per_class) on generated tables — no model here.  Bars: every output bit for bit, npred included: the kernel's
operation order is specified (fp64, each operation once, the AP sum left to right), so nothing is left to a tolerance.

Shapes, the smallest that reach every branch (make_case; CH = VA_CHUNK, the rows per step of the kernel's two walks): "chunks" has
80 classes and 10 thresholds with segments of 0 (ground truth, no detection), 1, 2, 63, 64, 65, CH - 3 .. CH + 1 (the backward walk
is over n + 2 elements) and 3 CH + 17 rows, the first and the last class id, a class with detections and no ground truth between
two that count, an all-TP and an all-FP segment, two segments that find all their ground truth (recall ends in 1.0), a segment whose
confidences lie inside [0.2, 0.4] (most of xs_pr takes the `left` branch, part of it `right`) and a row with conf == 1.0 (an exact
hit of xs_pr's last point); "one_class" is a single class and a single threshold over several chunks; "ties" has tied confidences
whose rows carry identical masks.  The condition of the tables (confidences of a class pairwise distinct otherwise) is asserted on
what is fed.  About 2 700 rows at most."""
import numpy as np
import pytest
import torch

from test_val_ap_host import CASES, N_THR, XS_AP, XS_PR, assert_distinct, kernel_chunk, make_case, order_ref, val_ap_ref

gpu = pytest.mark.gpu
OUT = ("ap", "precision", "recall", "npred")
SENTINEL = {"ap": -7.25, "precision": -7.25, "recall": -7.25, "npred": -77}


def launch(dev, c, order=None, null=None, xs_ap=XS_AP, xs_pr=XS_PR, **kw):
    """one yh_val_ap over the tables of `c` into sentinel-filled outputs -> (status, outputs as NumPy)"""
    from yoloseries_amd import _lib
    L = _lib.lib()
    nc, n_thr, n = kw.get("num_class", c["num_class"]), kw.get("n_thr", c["n_thr"]), kw.get("N", len(c["conf"]))
    order = order_ref(c["conf"], c["cls"]) if order is None else order
    t = dict(conf=torch.from_numpy(c["conf"]), cls=torch.from_numpy(c["cls"]), tp=torch.from_numpy(c["tp"].view(np.int16)),
             order=torch.from_numpy(order), gt_hist=torch.from_numpy(c["gt_hist"]), xs_ap=torch.from_numpy(xs_ap), xs_pr=torch.from_numpy(xs_pr))
    t = {k: v.to(dev) for k, v in t.items()}
    o = dict(ap=torch.full((c["num_class"], max(c["n_thr"], 1)), SENTINEL["ap"], dtype=torch.float64, device=dev),
             precision=torch.full((c["num_class"], len(xs_pr)), SENTINEL["precision"], dtype=torch.float64, device=dev),
             recall=torch.full((c["num_class"], len(xs_pr)), SENTINEL["recall"], dtype=torch.float64, device=dev),
             npred=torch.full((c["num_class"],), SENTINEL["npred"], dtype=torch.int32, device=dev))
    ws = torch.empty(max(int(L.yh_val_ap_ws_bytes(len(c["conf"]), c["n_thr"])), 16), dtype=torch.uint8, device=dev)
    t.update(o, ws=ws)
    p = {k: (None if k == null else v.data_ptr() + kw.get("offset", {}).get(k, 0)) for k, v in t.items()}
    rc = L.yh_val_ap(p["conf"], p["cls"], p["tp"], p["order"], n, p["gt_hist"], nc, n_thr, p["xs_ap"], kw.get("n_ap", len(xs_ap)),
                     p["xs_pr"], kw.get("n_pr", len(xs_pr)), p["ap"], p["precision"], p["recall"], p["npred"], p["ws"], _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def assert_same(got, want):
    for k in OUT:
        a, b = got[k], want[k]
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        np.testing.assert_array_equal(a, b, err_msg=k)


@gpu
def test_workspace_size():
    from yoloseries_amd import _lib
    L = _lib.lib()
    assert L.yh_val_ap_ws_bytes(1000, 10) == 40000 and L.yh_val_ap_ws_bytes(1, 1) == 4 and L.yh_val_ap_ws_bytes(0, 10) == 0


@gpu
@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_restatement_bit_for_bit(dev, name):
    """every output; the sentinels the outputs were filled with are all overwritten; a second launch gives the same"""
    c = make_case(name)
    assert_distinct(c)
    order = order_ref(c["conf"], c["cls"])
    want = val_ap_ref(c["conf"], c["cls"], c["tp"], order, c["gt_hist"], c["n_thr"])
    rc, got = launch(dev, c, order)
    assert rc == 0
    for k in OUT:
        assert not (got[k] == SENTINEL[k]).any(), k
    assert_same(got, want)
    assert want["ap"].any() and want["npred"].sum() == len(c["conf"])
    rc, again = launch(dev, c, order)
    assert rc == 0
    assert_same(again, got)


@gpu
def test_fewer_thresholds_read_fewer_bits(dev):
    """n_thr = 1 on the ten-threshold table: column 0 of the full run, the curves unchanged"""
    c = make_case("chunks")
    want = val_ap_ref(c["conf"], c["cls"], c["tp"], order_ref(c["conf"], c["cls"]), c["gt_hist"], N_THR)
    c1 = dict(c, n_thr=1)
    rc, got = launch(dev, c1)
    assert rc == 0
    assert_same(got, dict(want, ap=want["ap"][:, :1].copy()))


@gpu
def test_table_order_does_not_matter(dev):
    """the rows shuffled again, `order` rebuilt: the same results (the segments are found through order, not by position)"""
    c = make_case("chunks")
    rc, base = launch(dev, c)
    p = np.random.default_rng(5).permutation(len(c["conf"]))
    rc2, got = launch(dev, dict(c, conf=c["conf"][p].copy(), cls=c["cls"][p].copy(), tp=c["tp"][p].copy()))
    assert rc == 0 and rc2 == 0
    assert_same(got, base)


@gpu
def test_bad_arguments_return_einval_and_launch_nothing(dev):
    from yoloseries_amd import _lib
    c = make_case("ties")
    bad = [(dict(null=k), "null") for k in ("conf", "cls", "tp", "order", "gt_hist", "xs_ap", "xs_pr", "ap", "precision", "recall", "npred", "ws")]
    bad += [(dict(N=0), "N"), (dict(N=-3), "N"), (dict(num_class=0), "num_class"), (dict(n_thr=0), "n_thr"), (dict(n_thr=17), "n_thr"),
            (dict(n_ap=1), "n_ap"), (dict(n_pr=0), "n_pr"), (dict(offset={"conf": 2}), "unaligned"), (dict(offset={"tp": 1}), "unaligned"),
            (dict(offset={"ap": 4}), "unaligned"), (dict(offset={"xs_pr": 4}), "unaligned"), (dict(offset={"ws": 2}), "unaligned")]
    for kw, word in bad:
        rc, got = launch(dev, c, **kw)
        msg = _lib.lib().yh_last_error().decode()
        assert rc == -1 and "yh_val_ap" in msg and word in msg, (kw, rc, msg)
        for k in OUT:
            assert (got[k] == SENTINEL[k]).all(), (kw, k)
    with pytest.raises(_lib.YoloHipError, match="n_thr"):
        _lib.check(launch(dev, c, n_thr=17)[0], "yh_val_ap")


@gpu
def test_finish_ap_equals_restatement(dev):
    """MatchAccumulator.finish_ap: the padded per-batch tables compacted, ordered by the device's stable sort and reduced by the
    kernel give what the restatement gives on the compacted table in table order (ties included: identical masks), bit for bit"""
    from yoloseries_amd.trainer import MatchAccumulator
    for name in ("chunks", "ties"):
        c = make_case(name)
        n, K = len(c["conf"]), 300
        acc = MatchAccumulator(c["num_class"], dev)
        acc.gt_hist.copy_(torch.from_numpy(c["gt_hist"]))
        rng = np.random.default_rng(7)
        start = 0
        while start < n:                                              # batches of 3 images, a random number of rows each, padding behind
            rows = [int(r) for r in rng.integers(0, K + 1, 3)]
            conf, cls, tp = np.full((3, K), -1, np.float32), np.full((3, K), -5, np.int32), np.full((3, K), 0x7fff, np.int16)
            for b in range(3):
                r = rows[b] = min(rows[b], n - start)
                conf[b, :r], cls[b, :r], tp[b, :r] = c["conf"][start:start + r], c["cls"][start:start + r], c["tp"][start:start + r].view(np.int16)
                start += r
            acc.append(dict(conf=torch.from_numpy(conf).to(dev), cls=torch.from_numpy(cls).to(dev), tp=torch.from_numpy(tp).to(dev),
                            nrow=torch.tensor(rows, dtype=torch.int32, device=dev), gt_hist=acc.gt_hist))
        ap, precision, recall, npred, hist = acc.finish_ap()
        want = val_ap_ref(c["conf"], c["cls"], c["tp"], order_ref(c["conf"], c["cls"]), c["gt_hist"], N_THR)
        assert_same(dict(ap=ap, precision=precision, recall=recall, npred=npred), dict(want, npred=want["npred"].astype(np.int64)))
        np.testing.assert_array_equal(hist, c["gt_hist"])
        assert hist.dtype == np.int64 and npred.dtype == np.int64
    empty = MatchAccumulator(4, dev)
    ap, precision, recall, npred, hist = empty.finish_ap()
    assert ap.shape == (0, 10) and precision.shape == recall.shape == (0, 1000) and not npred.any() and not hist.any()
    assert kernel_chunk() >= 64
