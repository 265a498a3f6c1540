"""Test-time augmentation decoded and filtered per pass from the head tensors (yh_decode_filter_view, _tta_from_heads) against the
materialised path it replaces — test_time_augmentation (three full decodes, torch edits, concatenation) + yh_filter_decoded —
which stays the oracle.  Bars: candidate rows, their order and the counts bit-exact (assert_array_equal): the un-scale and the
un-flip are the same fp32 operations in the same order, so nothing is left to a tolerance.

The stub model returns DIFFERENT heads on each of its three calls (three seeds) and writes them into the SAME device tensors, as
the engine does with its head buffers: a pass appended at the wrong place, or heads read after the next forward, change the rows.
Seeds were chosen with oracle/postproc.py on the CPU (candidates_v5 / candidates_yolox of every call's heads: at least one
candidate per image at 0.3 / 0.3, fp32 and bf16-rounded heads); the tests assert it again on what the GPU produced."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_nms_heads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

PASSES = ((1, 0), (0.83, 2), (0.67, 3))
SEEDS = (21, 22, 23)
# (B, H, W, classes): 320x320 / 80 is the evaluators' usual head; 96x160 / 3 has heads of 12x20, 6x10 and 3x5 cells — every stage
# ends in a partial 64-pixel chunk, and H != W tells img_h from img_w
SHAPES = {"320x320": (2, 320, 320, 80), "96x160": (2, 96, 160, 3)}


def _hyp(dev, nc, h, w, thr, **kw):
    hyp = dict(device=dev, num_class=nc, input_img_size=[h, w], iou_threshold=0.2, conf_threshold=thr, cls_threshold=thr,
               max_predictions_per_img=300, iou_type="iou", mutil_label=False, agnostic=True, postprocess_bbox=True, wfb=False,
               use_tta=True, half=False, compute_metric_conf_threshold=0.001, compute_metric_iou_threshold=0.65,
               compute_metric_cls_threshold=0.001, num_anchors=1, num_stage=3)
    hyp.update(kw)
    return hyp


def heads_for(shape, yolox, seed):
    """synth_nms_heads of the square image W x W, rows cut to H: list of (B, A*(5+nc), H/s, W/s) float32"""
    B, H, W, nc = SHAPES[shape]
    hs = synth_nms_heads(B, W, nc, 1 if yolox else 3, seed=seed, clusters=10, frac=0.05)
    return [np.ascontiguousarray(h[:, :, :H // s]) for h, s in zip(hs, (8, 16, 32))]


class StubModel:
    """three calls, three sets of heads, one set of device tensors (overwritten by every call)"""

    def __init__(self, dev, shape, yolox, bf16):
        from yoloseries_amd.layout import to_cell_major
        self.sets = [[torch.from_numpy(h).to(dev) for h in heads_for(shape, yolox, sd)] for sd in SEEDS]
        if bf16:                     # the engine's layout: bf16, cell-major, consumed in place
            self.out = [to_cell_major(torch.zeros_like(h, dtype=torch.bfloat16))[0] for h in self.sets[0]]
        else:                        # the reference's layout: fp32 NCHW
            self.out = [torch.zeros_like(h) for h in self.sets[0]]
        self.calls = 0

    def __call__(self, x):
        for o, h in zip(self.out, self.sets[self.calls % 3]):
            o.copy_(h)
        self.calls += 1
        return self.out


def make_ev(dev, shape, yolox, bf16, thr=0.3, **kw):
    from yoloseries_amd.trainer import YOLOV5Evaluator, YOLOXEvaluator
    B, H, W, nc = SHAPES[shape]
    stub = StubModel(dev, shape, yolox, bf16)
    hyp = _hyp(dev, nc, H, W, thr, **kw)
    ev = YOLOXEvaluator(stub, hyp) if yolox else YOLOV5Evaluator(stub, torch.from_numpy(COCO_ANCHORS), hyp)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    return ev, stub, x


def view_pass(ev, d, ptrs, k, thr, cand, ncand, cap, two_pass, img_hw):
    from yoloseries_amd import _lib
    s, f = PASSES[k]
    xf = _lib.ViewXform(s, f, img_hw[0], img_hw[1])
    ws = torch.empty(int(_lib.lib().yh_decode_filter_ws_bytes(C.byref(d))), dtype=torch.uint8, device=cand.device) if two_pass else None
    _lib.check(_lib.lib().yh_decode_filter_view(C.byref(d), ptrs, C.byref(xf), thr, thr, cand.data_ptr(), ncand.data_ptr(), cap,
                                                ws.data_ptr() if two_pass else None, _lib.stream_ptr()), "yh_decode_filter_view")
    torch.cuda.synchronize()


def fused_table(ev, stub, x, thr, two_pass, cap=None, ncand0=None, fill=None, guard=0):
    """the three passes through yh_decode_filter_view into one table -> (cand (B, cap + guard, 6), ncand after each pass (3, B))"""
    B = x.shape[0]
    cand = ncand = None
    counts = []
    for k in range(3):
        d, canon, ptrs = ev._view_desc(stub(x), x)
        if cand is None:
            n = sum(d.num_anchor * d.H[i] * d.W[i] for i in range(d.num_stage))
            cap = cap or ((3 * n + 3) // 4) * 4
            flat = torch.full((B * cap + guard, 6), np.nan if fill is None else fill, dtype=torch.float32, device=x.device)
            cand = flat[:B * cap].view(B, cap, 6)
            ncand = torch.tensor(ncand0 or [0] * B, dtype=torch.int32, device=x.device)
        view_pass(ev, d, ptrs, k, thr, cand, ncand, cap, two_pass, x.shape[2:])
        counts.append(ncand.cpu().numpy().copy())
    return flat.cpu().numpy(), np.stack(counts), cap


_REF = {}


def ref_table(dev, shape, yolox, bf16, thr):
    """the materialised path on the same stub: _filter_decoded(test_time_augmentation(x)[0]) -> (cand, ncand), computed once"""
    key = (shape, yolox, bf16, thr)
    if key not in _REF:
        ev, stub, x = make_ev(dev, shape, yolox, bf16, thr)
        merged, _ = ev.test_time_augmentation(x)
        cand, ncand, _B, _cap = ev._filter_decoded(merged)
        _REF[key] = (cand.cpu().numpy(), ncand.cpu().numpy())
    return _REF[key]


# ---------------------------------------------------------------------------------------------------- (a) candidate tables
@gpu
@pytest.mark.parametrize("thr", [0.3, 0.001])
@pytest.mark.parametrize("two_pass", [False, True], ids=["one_block", "two_pass"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16_cell_major", "f32_nchw"])
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_candidate_table_matches_materialised_path(dev, shape, yolox, bf16, two_pass, thr):
    rc, rn = ref_table(dev, shape, yolox, bf16, thr)
    ev, stub, x = make_ev(dev, shape, yolox, bf16, thr)
    flat, counts, cap = fused_table(ev, stub, x, thr, two_pass)
    B = x.shape[0]
    got = flat.reshape(B, cap, 6)
    per_pass = np.diff(np.concatenate([np.zeros((1, B), counts.dtype), counts]), axis=0)
    assert (per_pass >= 1).all(), f"a pass without a candidate makes the comparison vacuous: {per_pass}"
    np.testing.assert_array_equal(counts[-1], rn)
    for b in range(B):
        np.testing.assert_array_equal(got[b, :rn[b]], rc[b, :rn[b]])


# ---------------------------------------------------------------------------------------------------- (b) identity
@gpu
@pytest.mark.parametrize("two_pass", [False, True], ids=["one_block", "two_pass"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16_cell_major", "f32_nchw"])
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
def test_identity_view_equals_decode_filter(dev, yolox, bf16, two_pass):
    """scale 1, no flip, ncand zeroed: yh_decode_filter's table bit for bit (x * 1.0f is x)"""
    from yoloseries_amd import _lib
    shape = "96x160"
    ev, stub, x = make_ev(dev, shape, yolox, bf16)
    B = x.shape[0]
    d, canon, ptrs = ev._view_desc(stub(x), x)
    n = sum(d.num_anchor * d.H[i] * d.W[i] for i in range(d.num_stage))
    cap = ((n + 3) // 4) * 4
    ws = torch.empty(int(_lib.lib().yh_decode_filter_ws_bytes(C.byref(d))), dtype=torch.uint8, device=dev) if two_pass else None
    c0 = torch.full((B, cap, 6), -7.0, dtype=torch.float32, device=dev)
    n0 = torch.full((B,), 123, dtype=torch.int32, device=dev)            # yh_decode_filter does not read it
    _lib.check(_lib.lib().yh_decode_filter(C.byref(d), ptrs, 0.3, 0.3, c0.data_ptr(), n0.data_ptr(), cap,
                                           ws.data_ptr() if two_pass else None, _lib.stream_ptr()), "yh_decode_filter")
    c1 = torch.full((B, cap, 6), -7.0, dtype=torch.float32, device=dev)
    n1 = torch.zeros(B, dtype=torch.int32, device=dev)
    view_pass(ev, d, ptrs, 0, 0.3, c1, n1, cap, two_pass, x.shape[2:])
    assert int(n0.min()) >= 1
    np.testing.assert_array_equal(n1.cpu().numpy(), n0.cpu().numpy())
    np.testing.assert_array_equal(c1.cpu().numpy(), c0.cpu().numpy())     # the untouched rows (-7) included


# ---------------------------------------------------------------------------------------------------- (c) append and overflow
@gpu
@pytest.mark.parametrize("two_pass", [False, True], ids=["one_block", "two_pass"])
def test_append_from_preset_base(dev, two_pass):
    """ncand = [5, 0] on entry: rows below the base keep the sentinel, the appended rows are those of a fresh call"""
    shape = "96x160"
    ev, stub, x = make_ev(dev, shape, False, True)
    fresh, fc, cap = fused_table(ev, stub, x, 0.3, two_pass, fill=-7.0)
    ev, stub, x = make_ev(dev, shape, False, True)
    got, gc, _ = fused_table(ev, stub, x, 0.3, two_pass, cap=cap + 8, ncand0=[5, 0], fill=-7.0)
    B = x.shape[0]
    fresh, got = fresh.reshape(B, cap, 6), got.reshape(B, cap + 8, 6)
    np.testing.assert_array_equal(gc, fc + np.array([5, 0]))
    for b, base in enumerate((5, 0)):
        tot = int(fc[-1, b])
        np.testing.assert_array_equal(got[b, :base], np.full((base, 6), -7.0, np.float32))
        np.testing.assert_array_equal(got[b, base:base + tot], fresh[b, :tot])
        np.testing.assert_array_equal(got[b, base + tot:], np.full((cap + 8 - base - tot, 6), -7.0, np.float32))


@gpu
@pytest.mark.parametrize("two_pass", [False, True], ids=["one_block", "two_pass"])
def test_overflow_counts_on_and_stores_nothing_past_cap(dev, two_pass):
    """cap smaller than the total: ncand reports the full count, rows below cap are right, the guard after the table is untouched.
    cap 4: later passes start past the end already; the other cap ends inside the image with the fewest candidates"""
    shape = "96x160"
    ev, stub, x = make_ev(dev, shape, False, True)
    fresh, fc, cap_full = fused_table(ev, stub, x, 0.3, two_pass)
    B = x.shape[0]
    fresh = fresh.reshape(B, cap_full, 6)
    total = fc[-1]
    guard = 64
    for cap in (4, 4 * ((int(total.min()) - 1) // 4)):
        assert cap >= 4 and (total > cap).all(), (total, cap)
        ev, stub, x = make_ev(dev, shape, False, True)
        flat, gc, _ = fused_table(ev, stub, x, 0.3, two_pass, cap=cap, fill=-7.0, guard=guard)
        np.testing.assert_array_equal(gc, fc)
        got = flat[:B * cap].reshape(B, cap, 6)
        for b in range(B):
            np.testing.assert_array_equal(got[b], fresh[b, :cap])
        np.testing.assert_array_equal(flat[B * cap:], np.full((guard, 6), -7.0, np.float32))


@gpu
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
def test_evaluator_reruns_with_a_table_that_cannot_overflow(dev, yolox, monkeypatch):
    shape = "96x160"
    ev, stub, x = make_ev(dev, shape, yolox, True)
    ref = ev.numba_nms(ev.test_time_augmentation(x)[0])
    ev, stub, x = make_ev(dev, shape, yolox, True)
    monkeypatch.setattr(ev, "_TTA_FIRST_CAP", 8)
    res = ev(x)
    assert stub.calls == 6 and max(ev.last_ncand) > 8          # three passes into 8 rows, then three into the full table
    for o, r in zip(res, ref):
        assert r is not None and len(r) > 0
        np.testing.assert_array_equal(o.numpy(), r)


# ---------------------------------------------------------------------------------------------------- (d) end to end
def _count_calls(ev, name):
    calls = []
    orig = getattr(ev, name)

    def wrapper(*a, **kw):
        calls.append(name)
        return orig(*a, **kw)
    setattr(ev, name, wrapper)
    return calls


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16_cell_major", "f32_nchw"])
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_call_with_tta_equals_oracle_composition_without_decoding(dev, shape, yolox, bf16):
    """ev(x) == numba_nms(test_time_augmentation(x)[0]) exactly, and ev(x) never materialises a decoded tensor"""
    ev, stub, x = make_ev(dev, shape, yolox, bf16)
    ref = ev.numba_nms(ev.test_time_augmentation(x)[0])
    ref_ncand = list(ev.last_ncand)
    ev, stub, x = make_ev(dev, shape, yolox, bf16)
    decoded, inferred = _count_calls(ev, "decode"), _count_calls(ev, "do_inference")
    res = ev(x)
    assert stub.calls == 3
    assert decoded == [] and inferred == [], "use_tta went through yh_decode_full"
    assert ev.last_ncand == ref_ncand
    assert any(r is not None and len(r) > 0 for r in ref)
    for o, r in zip(res, ref):
        assert (o is None) == (r is None)
        if r is not None:
            assert o.dtype == torch.float32 and o.device.type == "cpu"
            np.testing.assert_array_equal(o.numpy(), r)


@gpu
@pytest.mark.parametrize("yolox", [False, True], ids=["v5", "yolox"])
def test_multi_label_tta_stays_on_the_materialised_path(dev, yolox):
    ev, stub, x = make_ev(dev, "96x160", yolox, True, mutil_label=True)
    ref = ev.numba_nms(ev.test_time_augmentation(x)[0])
    ev, stub, x = make_ev(dev, "96x160", yolox, True, mutil_label=True)
    decoded = _count_calls(ev, "decode")
    res = ev(x)
    assert len(decoded) == 3 and stub.calls == 3
    for o, r in zip(res, ref):
        assert (o is None) == (r is None)
        if r is not None:
            np.testing.assert_array_equal(o.numpy(), r)


# ---------------------------------------------------------------------------------------------------- (e) argument errors
@gpu
def test_view_argument_errors_launch_nothing(dev):
    from yoloseries_amd import _lib
    L = _lib.lib()
    ev, stub, x = make_ev(dev, "96x160", False, True)
    d, canon, ptrs = ev._view_desc(stub(x), x)
    B, cap = x.shape[0], 64
    cand = torch.full((B, cap, 6), -7.0, dtype=torch.float32, device=dev)
    ncand = torch.full((B,), 3, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.yh_decode_filter_ws_bytes(C.byref(d))), dtype=torch.uint8, device=dev)

    def call(xf, cand_ptr=cand.data_ptr(), cap=cap, w=None):
        return L.yh_decode_filter_view(C.byref(d), ptrs, xf, 0.3, 0.3, cand_ptr, ncand.data_ptr(), cap, w, _lib.stream_ptr())
    bad = [(None, "null"), (C.byref(_lib.ViewXform(1.0, 1, 96, 160)), "flip_axis"), (C.byref(_lib.ViewXform(1.0, 4, 96, 160)), "flip_axis"),
           (C.byref(_lib.ViewXform(1.0, -1, 96, 160)), "flip_axis"), (C.byref(_lib.ViewXform(0.0, 0, 96, 160)), "scale"),
           (C.byref(_lib.ViewXform(-0.83, 2, 96, 160)), "scale"), (C.byref(_lib.ViewXform(float("nan"), 0, 96, 160)), "scale")]
    for w in (None, ws.data_ptr()):
        for xf, word in bad:
            rc = call(xf, w=w)
            msg = L.yh_last_error().decode()
            assert rc < 0 and "yh_decode_filter_view" in msg and word in msg, (rc, msg)
    ok = C.byref(_lib.ViewXform(1.0, 0, 96, 160))
    assert call(ok, cand_ptr=None) < 0 and "yh_decode_filter_view" in L.yh_last_error().decode()     # the shared checks name this entry
    assert call(ok, cap=66) < 0 and "multiple of 4" in L.yh_last_error().decode()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cand.cpu().numpy(), np.full((B, cap, 6), -7.0, np.float32))        # nothing ran
    np.testing.assert_array_equal(ncand.cpu().numpy(), np.full(B, 3, np.int32))
    with pytest.raises(_lib.YoloHipError, match="flip_axis"):
        _lib.check(call(C.byref(_lib.ViewXform(1.0, 1, 96, 160))), "yh_decode_filter_view")


# ---------------------------------------------------------------------------------------------------- (f) host side
def test_view_entry_is_declared_exported_and_bound():
    """the symbol test of test_host_logic.py picks up every entry of the header by itself; what it cannot see is the new struct:
    yh_view_xform's ctypes mirror against the members the header declares (names, order, types — all plain 4-byte scalars, so
    the header's text fixes the layout and no C compiler is needed), and the argument list bound in _lib.py against the prototype"""
    from yoloseries_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yolohip.h")).read()
    assert re.search(r"\bint\s+yh_decode_filter_view\s*\(", hdr)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "yh_decode_filter_view")
    res, args = _lib._SIGS["yh_decode_filter_view"]
    proto = re.search(r"yh_decode_filter_view\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert res is C.c_int32 and len(args) == len(re.sub(r"/\*.*?\*/", "", proto).split(",")) == 10
    assert args[2] == C.POINTER(_lib.ViewXform)
    body = re.search(r"typedef struct yh_view_xform \{(.*?)\} yh_view_xform;", hdr, re.S).group(1)
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    declared = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        if decl.strip():
            tname, names = decl.split(None, 1)
            declared += [(n.strip(), ctype[tname]) for n in names.split(",")]
    assert declared == list(_lib.ViewXform._fields_)
    assert C.sizeof(_lib.ViewXform) == 4 * len(declared) and [getattr(_lib.ViewXform, n).offset for n, _ in declared] == [0, 4, 8, 12]
