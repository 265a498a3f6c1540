"""The inputs of tests/test_gpu_postproc_edges.py exercise what they claim — proven on the CPU from the oracle alone, so a generator
(tools/postproc_cases.py) that drifts fails here and not silently on the GPU.  Nothing in this file needs a GPU."""
import importlib.util
import os
import time

import numpy as np
import pytest

from oracle import postproc as opp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    spec = importlib.util.spec_from_file_location("postproc_cases", os.path.join(ROOT, "tools", "postproc_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _cases()
_TABLES = {}
_KEEP = {}


def table(n):
    if n not in _TABLES:
        _TABLES[n] = P.nms_table(n)
    return _TABLES[n]


def uncapped_keep(name, t, class_aware, inclusive):
    """the full greedy pick list of one table (no cap, no merge filter), computed once"""
    key = (name, class_aware, inclusive)
    if key not in _KEEP:
        _KEEP[key] = opp.nms_image(t, P.IOU_THR, bool(class_aware), 1 << 30, False, inclusive=bool(inclusive))[1]
    return _KEEP[key]


def rank_of(t):
    """candidate index -> position in the kernel's sorted list"""
    order = P.sorted_positions(t)
    rank = np.full(len(t), -1, np.int64)
    rank[order] = np.arange(len(order))
    return rank


def test_generators_are_deterministic_and_shaped():
    for n in (0, 1, 65, 1025):
        a, b = P.nms_table(n), P.nms_table(n)
        assert a.shape == (n, 6) and a.dtype == np.float32
        np.testing.assert_array_equal(a, b)
    t = table(4096)
    np.testing.assert_array_equal(t[:, :4] * 4, np.round(t[:, :4] * 4))                 # quarter-pixel grid
    k = t[:, 4] * 64
    np.testing.assert_array_equal(k, np.round(k))
    assert k.min() == 0 and k.max() == 63 and 0.05 < (k == 0).mean() < 0.15
    assert set(np.unique(t[:, 5])) == {0.0, 1.0, 2.0, 3.0}
    assert (t[:, 2] >= t[:, 0]).all() and (t[:, 3] >= t[:, 1]).all()
    za = (t[:, :4] == np.array(P.ZERO_AREA, np.float32)).all(axis=1)
    assert za.sum() == P.NUM_ZERO_AREA and (t[za, 5] == 1).all() and (t[za, 4] > 0).all()
    assert tuple(P.stack_table().shape) == (1500, 6) and (P.alltie_table()[:, 4] == 0.5).all() and len(P.alltie_table()) == 200
    assert len(P.allzero_table()) == 130 and not P.allzero_table()[:, 4].any()
    assert P.one_positive_table().shape == (1, 6) and P.one_positive_table()[0, 4] == 0.5


def test_every_nms_case_runs_through_the_oracle_quickly():
    t0 = time.perf_counter()
    for n in P.NMS_SIZES:
        for ca, inc, mk, mf in P.NMS_CONFIGS:
            rows, keep = opp.nms_image(table(n), P.IOU_THR, bool(ca), mk, bool(mf), inclusive=bool(inc))
            assert len(keep) <= mk and (rows is None) == (n == 0)
    for name, make in P.DESIGNED.items():
        for ca, inc, mk, mf in P.DESIGNED_CONFIGS:
            opp.nms_image(make(), P.IOU_THR, bool(ca), mk, bool(mf), inclusive=bool(inc))
    assert time.perf_counter() - t0 < 10.0


def test_stack_has_chunks_the_kernel_must_skip():
    t = P.stack_table()
    order = P.sorted_positions(t)
    for ca, inc, _mk, _mf in P.DESIGNED_CONFIGS:
        kept = np.zeros(len(t), bool)
        kept[uncapped_keep("stack", t, ca, inc)] = True
        blocks = [kept[order[b:b + 64]].any() for b in range(0, len(order), 64)]
        assert blocks[0] and sum(not x for x in blocks) >= 10, blocks


@pytest.mark.parametrize("max_keep,min_n", [(300, 2999), (7, 63)])
def test_max_keep_is_reached_inside_a_chunk(max_keep, min_n):
    for ca, inc, mk, _mf in P.NMS_CONFIGS:
        if mk != max_keep:
            continue
        for n in (n for n in P.NMS_SIZES if n >= min_n):
            t = table(n)
            keep = uncapped_keep(n, t, ca, inc)
            assert len(keep) > max_keep, (n, ca, inc, len(keep))
            rank = rank_of(t)
            a, b = rank[keep[max_keep - 1]], rank[keep[max_keep]]
            assert a // 64 == b // 64, f"n={n} class_aware={ca} inclusive={inc}: picks {max_keep} and {max_keep + 1} at sorted positions {a}, {b}"


def test_alltie_keeps_in_index_order_across_the_first_chunk_edge():
    t = P.alltie_table()
    np.testing.assert_array_equal(P.sorted_positions(t), np.arange(len(t)))
    for ca, inc, _mk, _mf in P.DESIGNED_CONFIGS:
        keep = uncapped_keep("alltie", t, ca, inc)
        assert keep == sorted(keep) and keep[0] < 64 <= keep[-1]


def test_ties_straddle_chunk_edges_and_zero_area_rows_survive():
    for n in (n for n in P.NMS_SIZES if n >= 256):
        t = table(n)
        order = P.sorted_positions(t)
        sc = t[order, 4]
        edges = np.arange(64, len(order), 64)
        assert (sc[edges - 1] == sc[edges]).any(), n
        za = np.flatnonzero((t[:, :4] == np.array(P.ZERO_AREA, np.float32)).all(axis=1) & (t[:, 4] > 0))
        assert len(za) == P.NUM_ZERO_AREA
        assert set(za) <= set(uncapped_keep(n, t, 1, 1)), n
    t = table(256)                                           # the GPU test's degenerate case: exclusive rule, clamped union
    za = np.flatnonzero((t[:, :4] == np.array(P.ZERO_AREA, np.float32)).all(axis=1))
    assert len(za) == P.NUM_ZERO_AREA and set(za) <= set(opp.nms_image(t, P.IOU_THR, False, 300, False, inclusive=False)[1])


def test_on_threshold_pairs_are_exact_and_decide():
    """IoU(A, B) is float32(0.45) bit for bit, with and without the class offset; the inclusive rule keeps the A rows alone (the merge
    filter included: C overlaps A), the exclusive rule keeps A and B; suppression on the threshold happens inside a chunk and across"""
    t = P.on_threshold_table()
    n3 = P.NUM_TRIPLES
    A, B = np.arange(n3) * 3, np.arange(n3) * 3 + 1
    for off in (t[:, 5:6] * np.float32(4096), t[:, 5:6] * np.float32(0)):
        boxes = (t[:, :4] + off).astype(np.float32)
        iou = opp.numba_iou(boxes[A], boxes[B])
        np.testing.assert_array_equal(np.diag(iou), np.full(n3, np.float32(P.IOU_THR)))
        np.testing.assert_array_equal(np.diag(opp.gpu_iou(boxes[A], boxes[B])), np.full(n3, np.float32(P.IOU_THR)))
    (ca1, inc1, mk1, mf1), (ca2, inc2, mk2, mf2) = P.DESIGNED_CONFIGS
    assert inc1 == 1 and mf1 == 1 and inc2 == 0
    keep1 = opp.nms_image(t, P.IOU_THR, bool(ca1), mk1, bool(mf1), inclusive=True)[1]
    keep2 = opp.nms_image(t, P.IOU_THR, bool(ca2), mk2, bool(mf2), inclusive=False)[1]
    assert sorted(keep1) == list(A) and sorted(keep2) == sorted(list(A) + list(B))
    rank = rank_of(t)
    same = rank[A] // 64 == rank[B] // 64
    assert same.sum() >= 8 and (~same).sum() >= 8


def filter_reference(dec_img, mode, thr=None):
    thr = thr or P.FILTER_THR
    f = opp.candidates_yolox if mode in (1, 3) else opp.candidates_v5
    return f(dec_img, thr[0], thr[1], multi_label=mode >= 2)


def test_filter_rows_sit_on_the_thresholds_and_tie():
    """every image but the last (obj = 0: no candidate) has at least 8 candidates and fewer than N, per mode — from N = 63 on (a
    single prediction cannot); rows exactly on each threshold exist, and a tie between two classes decides cls"""
    conf, cls_thr = (np.float32(v) for v in P.FILTER_THR)
    for N in P.FILTER_N:
        for nc in P.FILTER_NC:
            d = P.decoded_rows(P.FILTER_B, N, nc, seed=N * 100 + nc)
            assert d.shape == (P.FILTER_B, N, 5 + nc) and d.dtype == np.float32
            np.testing.assert_array_equal(d[..., 4:] * 16, np.round(d[..., 4:] * 16))
            np.testing.assert_array_equal(d[..., :4] * 4, np.round(d[..., :4] * 4))
            for mode in range(4):
                counts = [len(filter_reference(d[b], mode)) for b in range(P.FILTER_B)]
                assert counts[-1] == 0
                if N >= 63:
                    assert all(8 <= c < N for c in counts[:-1]), (N, nc, mode, counts)
            live = d[:-1].reshape(-1, 5 + nc)
            prod = live[:, 5:] * live[:, 4:5]
            assert (live[:, 4] == conf).any() and (prod.max(axis=1) == cls_thr).any()
            # second pair (0.25 / 0.125): a single-label YOLOv5 candidate with obj exactly on conf_thr, a product exactly on cls_thr
            conf2, cls2 = (np.float32(v) for v in P.FILTER_THRS[1])
            assert ((live[:, 4] == conf2) & (prod.max(axis=1) > cls2)).any() and (N < 4 or (prod.max(axis=1) == cls2).any())
            if nc > 1 and N >= 3:
                srt = np.sort(live[:, 5:], axis=1)
                assert (srt[:, -1] == srt[:, -2]).mean() >= 0.05
                best = prod.max(axis=1)
                decided = (live[:, 4] >= conf) & (best > cls_thr) & ((prod == best[:, None]).sum(axis=1) >= 2)
                assert decided.any(), (N, nc)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", P.HEAD_CASES, ids=[c.id for c in P.HEAD_CASES])
def test_head_cases_yield_candidates(case, bf16):
    oracle_in, bufs = case.build(bf16)
    if case.yolox:
        dec = opp.decode_yolox(oracle_in, case.img_h)
    else:
        dec = opp.decode_v5(oracle_in, case.anchors(), case.strides())
    assert dec.shape == (case.B, case.npred, case.E) and np.isfinite(dec).all()
    for b in range(case.B):
        c = (opp.candidates_yolox if case.yolox else opp.candidates_v5)(dec[b], *P.HEAD_THR)
        assert 8 <= len(c) <= 0.9 * case.npred, (case.id, b, len(c), case.npred)
    # the kernel's buffer holds the oracle's values where a prediction lives and NaN everywhere else
    AE = case.A * case.E
    assert case.ldp >= AE
    for x, (flat, off), (h, w) in zip(case.raw(bf16), bufs, case.stages):
        assert off == case.shift and flat.dtype == (np.uint16 if bf16 else np.float32)
        f = (flat.astype(np.uint32) << 16).view(np.float32) if bf16 else flat
        body = f[off:off + case.B * h * w * case.ldp].reshape(case.B, h, w, case.ldp)
        np.testing.assert_array_equal(body[..., :AE].reshape(case.B, h, w, case.A, case.E).transpose(0, 3, 4, 1, 2), x)
        assert np.isnan(body[..., AE:]).all() and np.isnan(f[:off]).all() and np.isnan(f[off + body.size:]).all()


def test_head_cases_reach_the_paths_they_name():
    by = {c.id: c for c in P.HEAD_CASES}
    assert (by["unpadded_nc1"].ldp * 4) % 16 and (by["unpadded_nc1"].ldp * 2) % 16              # rows no multiple of 16 bytes
    assert (by["shifted_base"].ldp * 2) % 16 == 0 and by["shifted_base"].shift == 1                # aligned rows, unaligned base
    assert [h * w for h, w in by["four_stages"].stages] == [64, 65, 63, 1] and by["four_stages"].A == 2
    lr = by["long_row"]
    assert lr.A * -(-lr.stages[0][0] * lr.stages[0][1] // 64) == 1029 and lr.npred == 65709
    assert by["yolox_rect"].yolox == 1 and by["yolox_rect"].stages[0][0] != by["yolox_rect"].stages[0][1]
    assert 64 * (by["wide_row_tiny_map"].ldp * 4 + 16) > 64 * 1024
