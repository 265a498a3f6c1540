"""CPU: the AP half of the validation metric's device path, host side.

  * `val_ap_ref` — a NumPy float64 restatement of yh_val_ap (csrc/metric.hip): per class and threshold the cumulative true positives,
    recall and precision, the precision envelope, NumPy's interp written out (`interp_ref`), the trapezoid sum over the 101-point
    grid added LEFT TO RIGHT, and the two 1000-point curves of threshold 0.  It is pinned here to the mirrored host code,
    mAP_v2.from_matches(...).compute_ap_per_class(), on the tables derived from g9_map.npz and on the generated tables that
    tests/test_gpu_val_ap.py gives the kernel: the full precision and recall curves and every ys bit for bit, ap within
    rtol = atol = 1e-12 (the pin of tests/test_oracle_golden.py::test_g9_map_v2; np.sum adds pairwise, the restatement and the kernel
    left to right, nothing else differs).  The GPU test then compares the kernel with the restatement bit for bit.
  * mAP_v2.from_curves on the restatement's output against mAP_v2.from_matches.
  * the entry points are declared and bound.

`make_case` generates the tables (seeded; shared with the GPU test).  Their condition, under which the host code (whose global
argsort is unstable), the restatement and the kernel must agree: within a class the confidences are pairwise distinct, except for
the tied rows of the "ties" case, which carry identical masks.  The confidences are a permutation of distinct float32 values, so
the host code alone satisfies it; `assert_distinct` checks it on what is fed."""
import os
import re

import numpy as np
import pytest

from yoloseries_amd.utils.mAP import mAP_v2

from test_val_match_host import g9_lists, tables_from_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XS_AP = np.linspace(0, 1, 101)
XS_PR = np.linspace(0, 1, 1000)
N_THR = 10


def kernel_chunk():
    """VA_CHUNK of csrc/metric.hip: the rows per step of the kernel's walks (the generated segment lengths straddle it)"""
    src = open(os.path.join(ROOT, "yoloseries_amd", "csrc", "metric.hip")).read()
    return int(re.search(r"^#define\s+VA_CHUNK\s+(\d+)", src, re.M).group(1))


# ---------------------------------------------------------------------------------------------------- the restatement
def order_ref(conf, cls):
    """class ascending, then conf descending, ties in table order: a stable sort of (class << 32) | (0xFFFFFFFF - bits(conf))"""
    key = (cls.astype(np.int64) << 32) | (np.int64(0xFFFFFFFF) - conf.astype(np.float32).view(np.uint32).astype(np.int64))
    return np.argsort(key, kind="stable").astype(np.int32)


def interp_ref(x, xp, fp, left=None, right=None):
    """np.interp written out: below xp[0] -> left, above xp[-1] -> right, else j = the last index with xp[j] <= x and fp[j] on an
    exact hit, ((fp[j+1] - fp[j]) / (xp[j+1] - xp[j])) * (x - xp[j]) + fp[j] otherwise"""
    x, xp, fp = np.asarray(x, np.float64), np.asarray(xp, np.float64), np.asarray(fp, np.float64)
    left = fp[0] if left is None else left
    right = fp[-1] if right is None else right
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, len(xp) - 1)
    j1 = np.minimum(j + 1, len(xp) - 1)
    with np.errstate(all="ignore"):
        mid = ((fp[j1] - fp[j]) / (xp[j1] - xp[j])) * (x - xp[j]) + fp[j]
    out = np.where((xp[j] == x) | (j == len(xp) - 1), fp[j], mid)
    return np.where(x < xp[0], left, np.where(x > xp[-1], right, out))


def val_ap_ref(conf, cls, tp, order, gt_hist, n_thr=N_THR, xs_ap=XS_AP, xs_pr=XS_PR):
    """yh_val_ap on NumPy tables (conf float32, cls int32, tp uint16 masks, order from order_ref) -> dict of ap (num_class, n_thr),
    precision / recall (num_class, n_pr), npred (num_class,) int32 and ys (num_class, n_thr, n_ap): the interpolated envelope"""
    nc = len(gt_hist)
    scls, sconf, stp = cls[order], conf[order].astype(np.float32), tp[order].astype(np.int64)
    out = dict(ap=np.zeros((nc, n_thr)), precision=np.zeros((nc, len(xs_pr))), recall=np.zeros((nc, len(xs_pr))),
               npred=np.zeros(nc, np.int32), ys=np.zeros((nc, n_thr, len(xs_ap))))
    for c in range(nc):
        s, e = np.searchsorted(scls, c), np.searchsorted(scls, c + 1)
        out["npred"][c] = e - s
        T = int(gt_hist[c])
        if e == s or T <= 0:
            continue
        xp = -sconf[s:e].astype(np.float64)
        for k in range(n_thr):
            ctp = np.cumsum((stp[s:e] >> k) & 1)
            cfp = np.arange(1, e - s + 1) - ctp
            rec = ctp / (T + 1e-16)
            pre = ctp / ((ctp + cfp) + 1e-16)
            rec1 = np.concatenate(([0.], rec, [1.]))
            env = np.maximum.accumulate(np.concatenate(([1.], pre, [0.]))[::-1])[::-1]
            ys = interp_ref(xs_ap, rec1, env)
            out["ys"][c, k] = ys
            out["ap"][c, k] = np.cumsum(((ys[1:] + ys[:-1]) / 2) * (xs_ap[1:] - xs_ap[:-1]))[-1]      # cumsum adds left to right
            if k == 0:
                out["recall"][c] = interp_ref(-xs_pr, xp, rec, left=0.)
                out["precision"][c] = interp_ref(-xs_pr, xp, pre, left=1.)
    return out


# ---------------------------------------------------------------------------------------------------- the tables
def make_case(name):
    """-> dict of conf (N,) float32, cls (N,) int32, tp (N,) uint16, gt_hist (num_class,) int32, num_class, n_thr, seg: {class:
    rows}; the rows of all classes shuffled together.  Per class: (rows, kind) with kind one of
      mixed   each row a true positive with probability 0.6, up to a random threshold (bits 0..level-1: monotone, as IoU is)
      tp, fp  every row a true positive at every threshold / at none
      full    mixed, and the ground truth is exactly the true positives at threshold 0: recall reaches 1.0
      nogt    mixed, gt_hist = 0: the class has detections and does not count
      low     mixed, the confidences inside [0.2, 0.4]
      one     mixed, the best row has conf == 1.0 (xs_pr's last point hits it exactly)"""
    ch = kernel_chunk()
    if name == "chunks":                  # 80 classes, 10 thresholds: every segment length around the wave and the chunk
        nc, n_thr, seed = 80, 10, 11
        plan = {0: (1, "tp"), 3: (0, "mixed"), 5: (2, "mixed"), 7: (63, "mixed"), 8: (64, "mixed"), 9: (65, "full"),
                11: (ch - 1, "mixed"), 12: (ch, "mixed"), 13: (ch + 1, "mixed"), 14: (40, "nogt"), 15: (3 * ch + 17, "mixed"),
                20: (ch - 3, "mixed"), 21: (ch - 2, "full"), 40: (70, "tp"), 41: (70, "fp"), 50: (50, "low"), 79: (130, "one")}
    elif name == "one_class":             # a single class, a single threshold, several chunks
        nc, n_thr, seed = 1, 1, 12
        plan = {0: (2 * ch + 5, "one")}
    elif name == "ties":                  # tied confidences whose rows carry identical masks
        nc, n_thr, seed = 5, 10, 13
        plan = {0: (90, "mixed"), 2: (ch + 9, "mixed"), 4: (7, "mixed")}
    else:
        raise KeyError(name)
    rng = np.random.default_rng(seed)
    total = sum(n for n, _ in plan.values())
    pool = np.unique(rng.uniform(0.01, 0.99, 4 * total + 64).astype(np.float32))
    pool = rng.permutation(pool[(pool < 0.2) | (pool > 0.4)])                 # the band is the "low" class's own
    low = rng.permutation(np.unique(rng.uniform(0.2, 0.4, 256).astype(np.float32)))
    conf, cls, tp, used = [], [], [], 0
    hist = np.zeros(nc, np.int32)
    for c, (n, kind) in plan.items():
        if kind == "low":
            v = low[:n].copy()
        else:
            v, used = pool[used:used + n].copy(), used + n
        level = rng.integers(1, n_thr + 1, n)
        hit = rng.random(n) < 0.6
        if kind == "tp":
            level[:], hit[:] = n_thr, True
        elif kind == "fp":
            hit[:] = False
        if kind == "one":
            v[0] = 1.0
        m = np.where(hit, (1 << level) - 1, 0).astype(np.uint16)
        if name == "ties" and n >= 7:     # rows 1, 2 take row 0's confidence and mask; rows 5, 6 row 4's
            v[1:3], m[1:3], v[5:7], m[5:7] = v[0], m[0], v[4], m[4]
        n_tp = int((m & 1).sum())
        hist[c] = 0 if kind == "nogt" else n_tp if kind == "full" else max(n_tp, 1) + int(rng.integers(0, 9))
        conf.append(v); cls.append(np.full(n, c, np.int32)); tp.append(m)                               # noqa: E702
    conf, cls, tp = np.concatenate(conf), np.concatenate(cls), np.concatenate(tp)
    p = rng.permutation(len(conf))
    return dict(conf=conf[p].astype(np.float32), cls=cls[p], tp=tp[p], gt_hist=hist, num_class=nc, n_thr=n_thr,
                seg={c: n for c, (n, _) in plan.items()}, name=name)


CASES = ("chunks", "one_class", "ties")


def assert_distinct(c):
    """the condition of the tables, on what is fed: within a class no two rows share a confidence, unless they share the mask too"""
    for k in np.unique(c["cls"]):
        m = c["cls"] == k
        conf, tp = c["conf"][m], c["tp"][m]
        u, inv = np.unique(conf, return_inverse=True)
        if c["name"] != "ties":
            assert len(u) == len(conf), k
        for g in np.nonzero(np.bincount(inv) > 1)[0]:
            assert len(np.unique(tp[inv == g])) == 1, (k, u[g])
    assert (c["conf"] > 0).all() and (c["conf"] <= 1).all()


def bits_to_bool(tp):
    return ((tp[:, None] >> np.arange(N_THR)[None, :]) & 1).astype(bool)


class HostCurves(mAP_v2):
    """mAP_v2 with its full per-class tables kept: the curves before best_i is read from them, and the ys of every compute_ap call"""

    def compute_ap(self, recall, precision, type):
        ap, rec, pre = super().compute_ap(recall, precision, type)
        self.ys.append(np.interp(np.linspace(0, 1, 101), rec, pre))                   # the call compute_ap just made
        return ap, rec, pre

    def compute_ap_per_class(self):
        self.ys = []
        return super().compute_ap_per_class()

    def _summary(self, ap, precision, recall, tot_cls):
        self.curves = dict(ap=ap, precision=precision, recall=recall, unique_cls=tot_cls)
        return mAP_v2._summary(ap, precision, recall, tot_cls)


def host_curves(conf, cls, tp_bool, hist):
    m = HostCurves.from_matches(conf, cls, tp_bool, hist)
    res = m.compute_ap_per_class()
    return m, res


def assert_ref_equals_host(conf, cls, tp, hist, n_thr):
    """the pin: val_ap_ref against compute_ap_per_class on one table (tp as uint16 masks)"""
    ref = val_ap_ref(conf, cls, tp, order_ref(conf, cls), hist, n_thr)
    m, _ = host_curves(conf, cls, bits_to_bool(tp), hist)
    tot = m.curves["unique_cls"]
    np.testing.assert_array_equal(tot, np.nonzero(hist)[0])
    np.testing.assert_array_equal(ref["precision"][tot].view(np.uint64), m.curves["precision"].view(np.uint64))
    np.testing.assert_array_equal(ref["recall"][tot].view(np.uint64), m.curves["recall"].view(np.uint64))
    np.testing.assert_allclose(ref["ap"][tot], m.curves["ap"][:, :n_thr], rtol=1e-12, atol=1e-12)
    ranked = [c for c in tot if (cls == c).any()]                     # compute_ap runs for these, threshold by threshold
    assert len(m.ys) == len(ranked) * N_THR
    for i, c in enumerate(ranked):
        for k in range(n_thr):
            np.testing.assert_array_equal(ref["ys"][c, k].view(np.uint64), m.ys[i * N_THR + k].view(np.uint64), err_msg=f"{c} {k}")
    other = np.setdiff1d(np.arange(len(hist)), ranked)
    assert not ref["ap"][other].any() and not ref["precision"][other].any() and not ref["recall"][other].any()
    np.testing.assert_array_equal(ref["npred"], np.bincount(cls, minlength=len(hist)))
    return ref, m


def g9_tables():
    _, gts, preds = g9_lists()
    conf, cls, tp, hist = tables_from_lists(gts, preds, 80)
    bits = (tp.astype(np.uint16) << np.arange(N_THR, dtype=np.uint16)).sum(1).astype(np.uint16)
    return conf.astype(np.float32), cls.astype(np.int32), bits, hist.astype(np.int32)


# ---------------------------------------------------------------------------------------------------- tests
def test_interp_ref_is_np_interp():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 4, 5, 40, 700):
        xp = np.sort(rng.random(n))
        xp[n // 2:n // 2 + 2] = xp[n // 2]                             # a duplicate abscissa
        fp = rng.random(n)
        x = np.concatenate((rng.uniform(-0.2, 1.2, 300), xp, [xp[0], xp[-1]]))
        for kw in ({}, dict(left=0.), dict(left=1., right=7.)):
            np.testing.assert_array_equal(interp_ref(x, xp, fp, **kw).view(np.uint64), np.interp(x, xp, fp, **kw).view(np.uint64))


def test_restatement_equals_host_code_on_the_fixture():
    conf, cls, tp, hist = g9_tables()
    ref, m = assert_ref_equals_host(conf, cls, tp, hist, N_THR)
    assert len(m.curves["unique_cls"]) == 5 and ref["ap"].any()


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_host_code_on_the_generated_tables(name):
    c = make_case(name)
    assert_distinct(c)
    ref, _ = assert_ref_equals_host(c["conf"], c["cls"], c["tp"], c["gt_hist"], c["n_thr"])
    for k, n in c["seg"].items():
        assert ref["npred"][k] == n
    assert ref["ap"].any()


def test_generated_tables_hold_the_required_content():
    ch = kernel_chunk()
    c = make_case("chunks")
    ref = val_ap_ref(c["conf"], c["cls"], c["tp"], order_ref(c["conf"], c["cls"]), c["gt_hist"], c["n_thr"])
    assert {0, 1, 2, 63, 64, 65, ch - 1, ch, ch + 1, 3 * ch + 17} <= set(c["seg"].values())
    assert c["num_class"] == 80 and 0 in c["seg"] and 79 in c["seg"] and c["gt_hist"][3] > 0 and c["seg"][3] == 0
    assert c["gt_hist"][14] == 0 and c["seg"][14] > 0 and c["gt_hist"][13] > 0 and c["gt_hist"][15] > 0
    assert not ref["ap"][14].any() and not ref["precision"][14].any() and ref["npred"][14] == c["seg"][14]
    assert (c["tp"][c["cls"] == 40] == 1023).all() and not c["tp"][c["cls"] == 41].any()
    assert (ref["ap"][40] > 0).all() and not ref["ap"][41].any() and not ref["recall"][41].any()
    low = c["conf"][c["cls"] == 50]
    assert 0 < low.min() and low.max() < 0.5 and (XS_PR > low.max()).sum() > 500 and (XS_PR < low.min()).sum() > 100
    assert (ref["recall"][50][XS_PR > low.max()] == 0).all() and (ref["precision"][50][XS_PR > low.max()] == 1).all()      # left
    assert len(np.unique(ref["recall"][50][XS_PR < low.min()])) == 1 and ref["recall"][50][0] > 0                          # right
    assert (c["conf"][c["cls"] == 79] == 1.0).sum() == 1
    assert ref["recall"][9].max() == 1.0 and ref["recall"][21].max() == 1.0          # all ground truth found: rec' ends 1, 1
    one = make_case("one_class")
    assert one["num_class"] == 1 and one["n_thr"] == 1 and (one["tp"] <= 1).all() and one["tp"].any()
    ties = make_case("ties")
    assert any(len(np.unique(ties["conf"][ties["cls"] == k])) < (ties["cls"] == k).sum() for k in (0, 2, 4))


@pytest.mark.parametrize("name", ("g9",) + CASES)
def test_from_curves_equals_from_matches(name):
    if name == "g9":
        conf, cls, tp, hist = g9_tables()
        n_thr = N_THR
    else:
        c = make_case(name)
        conf, cls, tp, hist, n_thr = c["conf"], c["cls"], c["tp"], c["gt_hist"], c["n_thr"]
    ref = val_ap_ref(conf, cls, tp, order_ref(conf, cls), hist, N_THR)               # ten columns, as the drivers ask for
    want_m = mAP_v2.from_matches(conf, cls, bits_to_bool(tp), hist)
    got_m = mAP_v2.from_curves(ref["ap"], ref["precision"], ref["recall"], hist)
    want, got = want_m.compute_ap_per_class(), got_m.compute_ap_per_class()
    np.testing.assert_array_equal(got["unique_cls"], want["unique_cls"])
    for k in ("f1", "precision", "recall"):                           # the same curves, so the same best_i and the same values
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_allclose(got["ap"], want["ap"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got_m.get_mean_metrics(), want_m.get_mean_metrics(), rtol=1e-12, atol=1e-12)
    assert n_thr in (1, N_THR)


def test_from_curves_without_a_row_reports_zero_curves():
    hist = np.array([0, 3, 0, 1])
    r = mAP_v2.from_curves(np.zeros((0, 10)), np.zeros((0, 1000)), np.zeros((0, 1000)), hist).compute_ap_per_class()
    np.testing.assert_array_equal(r["unique_cls"], [1, 3])
    assert r["ap"].shape == (2, 10) and not r["ap"].any() and not r["precision"].any() and not r["recall"].any()


def test_val_ap_is_declared_and_bound():
    import ctypes as C
    from yoloseries_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yolohip.h")).read()
    for name, res, count in (("yh_val_ap", r"int", 18), ("yh_val_ap_ws_bytes", r"size_t", 2)):
        proto = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (res, name), hdr)
        assert proto, f"include/yolohip.h does not declare {name}"
        assert name in _lib.EXPORTED_SYMBOLS
        ctype, args = _lib._SIGS[name]
        assert ctype is (C.c_int32 if res == "int" else C.c_size_t)
        assert len(args) == len(re.sub(r"/\*.*?\*/", "", proto.group(1)).split(",")) == count, name
