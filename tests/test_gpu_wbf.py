"""yh_wbf_batched (csrc/wbf.hip) through hipk.wbf against fuse_table, the fp64 host mirror, on the same rows.

Bars: nout, members and the class column equal; boxes and scores assert_array_max_ulp(out, float32(oracle), maxulp=1) — the
kernel's fp64 running sums and the oracle's differ by about N * 2^-53 at most, and rounding to float32 can move a value by at most
one ulp.  Tables are built on the host at the smallest sizes where the kernel takes another path: one row, one wave of clusters
(63 / 64 / 65), more clusters than the workgroup has threads (257), and one cluster on either side of the kernel's LDS limit
(hipk.wbf_lds_clusters() == 1024: K = 1024 keeps every cluster's state in LDS, K = 1025 puts the last one in the workspace).
Unused rows of a table hold NaN: a kernel that reads them shows it."""
import os

import numpy as np
import pytest
import torch

from yoloseries_amd.utils import fuse_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
LDS_CLUSTERS = 1024


def table(images, cap, slots=None):
    """list of (n, 7) row arrays (or None) -> cand (B, cap, 6), weight (B, cap) float32; rows at `slots[b]` (default: the first n),
    NaN / weight 0 elsewhere"""
    B = len(images)
    cand = np.full((B, cap, 6), np.nan, np.float32)
    weight = np.zeros((B, cap), np.float32)
    for b, rows in enumerate(images):
        if rows is None or len(rows) == 0:
            continue
        rows = np.asarray(rows, np.float32).reshape(-1, 7)
        at = np.arange(len(rows)) if slots is None or slots[b] is None else np.asarray(slots[b])
        cand[b, at] = rows[:, :6]
        weight[b, at] = rows[:, 6]
    return cand, weight


def check(dev, cand, weight, thr, box_mean='reference', num_class=None):
    """hipk.wbf on the table against fuse_table of every image's rows -> (list of (out, members) per image as NumPy, oracle list)"""
    from yoloseries_amd import hipk
    out, nout, members = hipk.wbf(torch.from_numpy(cand).to(dev), torch.from_numpy(weight).to(dev), thr, box_mean, num_class=num_class)
    torch.cuda.synchronize()
    out, nout, members = out.cpu().numpy(), nout.cpu().numpy(), members.cpu().numpy()
    assert out.dtype == np.float32 and nout.dtype == np.int32 and members.dtype == np.int32
    got, want = [], []
    for b in range(cand.shape[0]):
        ref, ref_n = fuse_table(np.concatenate((cand[b], weight[b][:, None]), axis=1), thr, box_mean)
        assert nout[b] == len(ref), (b, nout[b], len(ref))
        o, m = out[b, :nout[b]], members[b, :nout[b]]
        np.testing.assert_array_equal(m, ref_n)
        np.testing.assert_array_equal(o[:, 5], ref[:, 5].astype(np.float32))
        if len(ref):
            np.testing.assert_array_max_ulp(o[:, :5], ref[:, :5].astype(np.float32), maxulp=1)
        got.append((o, m))
        want.append((ref, ref_n))
    return got, want


def row(x1, y1, x2, y2, s, c=0, w=1.0):
    return [x1, y1, x2, y2, s, c, w]


@gpu
def test_empty_single_and_small_images(dev):
    """B = 3, cap = 16: an image with no valid row, one with a single row, one with five rows in two classes"""
    five = [row(0, 0, 10, 10, 0.9, 2), row(1, 0, 11, 10, 0.6, 2), row(50, 50, 60, 60, 0.7, 2), row(0, 0, 10, 10, 0.8, 1),
            row(0, 1, 10, 11, 0.3, 1, 2.0)]
    cand, weight = table([None, [row(3, 4, 30, 40, 0.25, 1, 0.5)], five], 16)
    got, want = check(dev, cand, weight, 0.5, num_class=3)
    assert len(got[0][0]) == 0
    np.testing.assert_array_equal(got[1][0], np.asarray([[3, 4, 30, 40, 0.25, 1]], np.float32))
    np.testing.assert_array_equal(got[1][1], [1])
    np.testing.assert_array_equal(got[2][1], [2, 2, 1])                      # class 1 first, then class 2 in founding order
    np.testing.assert_array_equal(got[2][0][:, 5], [1, 2, 2])


def disjoint_pairs(K, seed):
    """K disjoint 20 x 20 boxes of one class (scores in (0.5, 1): the founders), then K rows that each overlap exactly one of them by
    IoU 0.95 (scores in (0.05, 0.5)); table order shuffled.  A halved fused box (the reference mean of two members) is 10 x 10: IoU
    <= 0.25 with any row, so every cluster ends with exactly two members."""
    rng = np.random.RandomState(seed)
    i = np.arange(K)
    x, y = 40.0 + 30.0 * (i % 64), 40.0 + 30.0 * (i // 64)
    hi = rng.uniform(0.5, 1.0, K)
    lo = rng.uniform(0.05, 0.5, K)
    a = np.stack((x, y, x + 20, y + 20, hi, np.zeros(K), np.ones(K)), axis=1)
    b = np.stack((x + 1, y, x + 20, y + 20, lo, np.zeros(K), np.full(K, 2.0)), axis=1)
    return np.concatenate((a, b))[rng.permutation(2 * K)]


@gpu
@pytest.mark.parametrize("K", [1, 63, 64, 65, 257, LDS_CLUSTERS, LDS_CLUSTERS + 1])
def test_k_clusters_of_two(dev, K):
    from yoloseries_amd import hipk
    assert hipk.wbf_lds_clusters() == LDS_CLUSTERS, "the sizes of this test straddle the kernel's LDS limit: update both"
    rows = disjoint_pairs(K, 100 + K)
    cand, weight = table([rows], 2 * K + 6)                                   # cap > the limit where K is: L is the limit itself
    got, want = check(dev, cand, weight, 0.5, num_class=1)
    np.testing.assert_array_equal(got[0][1], np.full(K, 2))


@gpu
@pytest.mark.parametrize("box_mean,thr", [("weighted", 0.5), ("reference", 0.0)])
def test_300_near_identical_boxes_are_one_cluster(dev, box_mean, thr):
    """'weighted': the fused box stays on the boxes, every row meets it at 0.5.  'reference': the box is divided by the member count,
    so from the third row on nothing overlaps it by 0.5 — one cluster there is the threshold 0, which every IoU meets."""
    rng = np.random.RandomState(7)
    n = 300
    box = np.asarray([100.0, 120.0, 300.0, 260.0]) + rng.uniform(-2, 2, (n, 4))
    rows = np.concatenate((box, rng.uniform(0.1, 1, (n, 1)), np.full((n, 1), 4.0), rng.choice([1.0, 2.0, 0.5], (n, 1))), axis=1)
    cand, weight = table([rows], 304)
    got, want = check(dev, cand, weight, thr, box_mean, num_class=5)
    np.testing.assert_array_equal(got[0][1], [n])


@gpu
def test_reference_mean_at_threshold_one_half_splits_the_same_rows(dev):
    """the 300 rows above under the reference mean at 0.5: many clusters, every one against the mirror"""
    rng = np.random.RandomState(7)
    n = 300
    box = np.asarray([100.0, 120.0, 300.0, 260.0]) + rng.uniform(-2, 2, (n, 4))
    rows = np.concatenate((box, rng.uniform(0.1, 1, (n, 1)), np.full((n, 1), 4.0), np.ones((n, 1))), axis=1)
    cand, weight = table([rows], 300)                                         # every one of cap rows valid
    got, want = check(dev, cand, weight, 0.5, num_class=5)
    assert len(got[0][1]) > 100 and got[0][1].max() == 2


@gpu
def test_a_row_joins_every_cluster_it_overlaps(dev):
    rows = [row(0, 0, 10, 10, 0.9, 1), row(6, 0, 16, 10, 0.8, 1), row(3, 0, 13, 10, 0.7, 1)]      # 0.25 apart; 7/13 with the third
    cand, weight = table([rows], 4)
    got, want = check(dev, cand, weight, 0.5, 'weighted', num_class=2)
    np.testing.assert_array_equal(got[0][1], [2, 2])


@gpu
def test_threshold_is_inclusive(dev):
    """the founder [0, 0, 2, 2] with score 0.5 has an exact fused box; [0, 0, 2, 1] meets it at IoU 2 / 4 exactly"""
    rows = [row(0, 0, 2, 2, 0.5), row(0, 0, 2, 1, 0.25)]
    cand, weight = table([rows], 4)
    got, _ = check(dev, cand, weight, 0.5, num_class=1)
    np.testing.assert_array_equal(got[0][1], [2])
    got, _ = check(dev, cand, weight, float(np.nextafter(0.5, 1)), num_class=1)
    np.testing.assert_array_equal(got[0][1], [1, 1])


def objects(rng, n_obj, num_class, weights=(1.0, 2.0, 0.5), classes=None):
    """n_obj objects seen by three passes each -> (3 * n_obj, 7), passes stacked"""
    cx, cy = rng.uniform(50, 590, n_obj), rng.uniform(50, 590, n_obj)
    w, h = rng.uniform(30, 150, n_obj), rng.uniform(30, 150, n_obj)
    cls = rng.randint(0, num_class, n_obj) if classes is None else rng.choice(classes, n_obj)
    out = []
    for wt in weights:
        j = rng.normal(0, 0.04, (4, n_obj))
        x, y, ww, hh = cx + j[0] * w, cy + j[1] * h, w * np.exp(j[2]), h * np.exp(j[3])
        out.append(np.stack((x - ww / 2, y - hh / 2, x + ww / 2, y + hh / 2, rng.uniform(0.05, 1, n_obj), cls, np.full(n_obj, wt)), axis=1))
    return np.concatenate(out)


@gpu
def test_holes_between_rows_and_a_full_table(dev):
    """valid rows interleaved with weight-0 rows (NaN in them), next to an image whose every row is valid"""
    rng = np.random.RandomState(11)
    a, b = objects(rng, 20, 3), objects(rng, 40, 3)
    cap = 120
    slots = [np.sort(rng.permutation(cap)[:len(a)]), None]
    assert len(b) == cap
    cand, weight = table([a, b], cap, slots)
    got, want = check(dev, cand, weight, 0.5, 'weighted', num_class=3)
    assert got[0][1].max() >= 2 and got[1][1].max() >= 2


@gpu
def test_classes_0_and_79_with_nothing_between(dev):
    rng = np.random.RandomState(12)
    rows = objects(rng, 30, 80, classes=[0, 79])
    cand, weight = table([rows], 96)
    for num_class in (80, None):                                               # None: taken from the table
        got, want = check(dev, cand, weight, 0.5, 'weighted', num_class=num_class)
        assert set(got[0][0][:, 5]) == {0.0, 79.0}


@gpu
@pytest.mark.parametrize("box_mean", ["reference", "weighted"])
def test_pass_weights_mix_within_clusters(dev, box_mean):
    rng = np.random.RandomState(13)
    rows = objects(rng, 60, 2, weights=(1.0, 2.0, 0.5))
    cand, weight = table([rows[rng.permutation(len(rows))]], 180)
    got, want = check(dev, cand, weight, 0.55, box_mean, num_class=2)
    assert got[0][1].max() >= 2


@gpu
def test_equal_scores_go_in_table_order(dev):
    """against the mirror only (the reference orders equal scores by an unstable sort): three overlapping rows of one score, where the
    founder decides the fused box, and far pairs of equal score, whose founding order is the output order"""
    rows = [row(0, 0, 10, 10, 0.5), row(2, 0, 12, 10, 0.5), row(1, 0, 11, 10, 0.5), row(200, 0, 210, 10, 0.5), row(100, 0, 110, 10, 0.5),
            row(100, 1, 110, 11, 0.25), row(200, 1, 210, 11, 0.25)]
    cand, weight = table([rows], 8)
    got, want = check(dev, cand, weight, 0.5, 'weighted', num_class=1)
    np.testing.assert_array_equal(got[0][0][:, 0] > 150, [False, True, False])


@gpu
def test_golden_table_equals_the_reference(dev):
    """B = 4, about 400 rows per image, 5 classes, pass weights (1, 2, 0.5): the mirror's bars, and the same bars against what the
    reference's weighted_fusion_bbox recorded"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g21_wbf.npz"))
    images = [g[f"rows_{i}"] for i in range(4)]
    cand, weight = table(images, 400)
    got, want = check(dev, cand, weight, float(g["iou_thr"]), num_class=int(g["num_class"]))
    for i, (o, m) in enumerate(got):
        fusion, sizes = g[f"fusion_{i}"], g[f"sizes_{i}"]
        np.testing.assert_array_equal(m, sizes)
        np.testing.assert_array_equal(o[:, 5], fusion[:, 5].astype(np.float32))
        np.testing.assert_array_max_ulp(o[:, :5], fusion[:, :5].astype(np.float32), maxulp=1)


@gpu
def test_argument_errors_launch_nothing_and_members_may_be_null(dev):
    from yoloseries_amd import _lib
    L = _lib.lib()
    rows = [row(0, 0, 10, 10, 0.9), row(1, 0, 11, 10, 0.6), row(50, 50, 60, 60, 0.7)]
    cand_h, weight_h = table([rows], 4)
    cand, weight = torch.from_numpy(cand_h).to(dev), torch.from_numpy(weight_h).to(dev)
    order = torch.tensor([[0, 2, 1, 3]], dtype=torch.int32, device=dev)
    nvalid = torch.tensor([3], dtype=torch.int32, device=dev)
    out = torch.full((1, 4, 6), -7.0, dtype=torch.float32, device=dev)
    nout = torch.full((1,), 123, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.yh_wbf_ws_bytes(1, 4)), dtype=torch.uint8, device=dev)
    assert int(L.yh_wbf_ws_bytes(0, 4)) == 0 and ws.numel() > 0

    def call(B=1, cap=4, nc=1, box_mean=0, thr=0.5, out_ptr=out.data_ptr(), ws_ptr=ws.data_ptr()):
        return L.yh_wbf_batched(cand.data_ptr(), weight.data_ptr(), order.data_ptr(), nvalid.data_ptr(), B, cap, nc, thr, box_mean,
                                out_ptr, nout.data_ptr(), None, ws_ptr, _lib.stream_ptr())
    for kw, word in ((dict(B=0), "positive"), (dict(cap=0), "positive"), (dict(nc=0), "positive"), (dict(box_mean=2), "box_mean"),
                     (dict(thr=float("nan")), "NaN"), (dict(out_ptr=None), "null"), (dict(ws_ptr=None), "null"),
                     (dict(ws_ptr=ws.data_ptr() + 4), "unaligned")):
        rc = call(**kw)
        msg = L.yh_last_error().decode()
        assert rc < 0 and "yh_wbf_batched" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), np.full((1, 4, 6), -7.0, np.float32))               # nothing ran
    assert int(nout.item()) == 123
    _lib.check(call(), "yh_wbf_batched")                                                                  # members == NULL
    torch.cuda.synchronize()
    ref, _ = fuse_table(np.concatenate((cand_h[0], weight_h[0][:, None]), axis=1), 0.5)
    assert int(nout.item()) == len(ref) == 2
    np.testing.assert_array_max_ulp(out.cpu().numpy()[0, :2, :5], ref[:, :5].astype(np.float32), maxulp=1)
