"""Post-processing kernels (csrc/postproc.hip, csrc/bbox.hip) at the sizes where they branch, through the C ABI alone
(yoloseries_amd._lib.lib()), against the oracle (oracle/postproc.py, oracle/bbox.py — pinned to the reference by the goldens).

Inputs come from tools/postproc_cases.py; tests/test_postproc_cases_host.py proves on the CPU that they reach what they claim.
  NMS      one image per launch at every size class of nms_kernel (64-chunk edges, the 1024-thread loops, the power-of-two sort
           length, LDS sort -> workspace sort at 8192 / 8193, the merge filter's 1 < n < 3000 window, max_keep inside a chunk,
           max_keep > 512, skipped chunks, ties across a chunk edge, zero-area duplicates), then a batch of unequal images, a cap
           larger than n, ncand > cap.  Bar: nkeep, keep_idx[:nkeep], out[:nkeep] bit-identical to oracle.postproc.nms_image.
  filter   yh_filter_decoded, four modes, N around the 1024-prediction loop, rows exactly on the thresholds, class ties, cap overflow.
           Bar: counts and rows bit-identical to candidates_v5 / candidates_yolox.
  decode   yh_decode_full at the contract of test_decode_golden (rtol = atol = 1e-4); yh_decode_filter one-block
           and two-pass bit-identical to each other and to candidates_* of the tensor yh_decode_full produced — on heads that reach
           the scalar staging branch of decode_scan_kernel, four stages, two anchors, 63 / 64 / 65 / 1 cells, more than 1024 chunk keys.
  boxes    yh_iou_matrix past one grid pass (bit-identical, NaN in the same places), yh_iou_pairwise at block edges (the bars of
           test_ciou_and_iou_utils).
Every buffer a kernel writes sits inside a larger sentinel-filled allocation: guards, and rows past the advertised extent, must not
change; inputs must not change either.  No tolerance is introduced here."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import bbox as obb
from oracle import postproc as opp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _cases():
    spec = importlib.util.spec_from_file_location("postproc_cases", os.path.join(ROOT, "tools", "postproc_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _cases()
SENT = -7.0
YH_EINVAL = -1
_RAN = set()
F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def _L():
    from yoloseries_amd._lib import lib
    return lib()


def _stream():
    from yoloseries_amd import _lib
    return _lib.stream_ptr()


def _ok(rc, what):
    from yoloseries_amd._lib import check
    check(rc, what)


def _bytes(t):
    return t.contiguous().view(-1).view(U8)


class Guarded:
    """a device buffer in the middle of a larger allocation filled with a sentinel; `data` (optional) is what the buffer holds"""

    def __init__(self, dev, shape, dtype, fill, data=None, guard=None):
        n = int(np.prod(shape))
        g = self.g = guard if guard is not None else (256 if dtype == U8 else 64)
        self.flat = torch.full((g + n + g,), fill, dtype=dtype, device=dev)
        self.t = self.flat[g:g + n].view(*shape)
        if data is not None:
            self.t.copy_(data)
        self.init = self.flat.clone()
        self.n = n

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        g, n = self.g, self.n
        return (torch.equal(_bytes(self.flat[:g]), _bytes(self.init[:g])) and torch.equal(_bytes(self.flat[g + n:]), _bytes(self.init[g + n:])))

    def unchanged(self):
        return torch.equal(_bytes(self.flat), _bytes(self.init))

    def np(self):
        return self.t.cpu().numpy()


# ================================================================================================================ NMS
_TABLES = {}
_NMS_REF = {}
WS_TAIL = 4096


def nms_input(name):
    if name not in _TABLES:
        _TABLES[name] = P.DESIGNED[name]() if isinstance(name, str) else P.nms_table(name)
    return _TABLES[name]


def nms_ref(name, cfg):
    """oracle rows and pick list of one table under one configuration, computed once and never modified"""
    key = (name, cfg)
    if key not in _NMS_REF:
        ca, inc, mk, mf = cfg
        rows, keep = opp.nms_image(nms_input(name), P.IOU_THR, bool(ca), mk, bool(mf), inclusive=bool(inc))
        rows = np.zeros((0, 6), np.float32) if rows is None else np.asarray(rows, np.float32).reshape(-1, 6)
        rows.setflags(write=False)
        _NMS_REF[key] = (rows, list(keep))
    return _NMS_REF[key]


def run_nms(dev, tables, cfg, cap=None, ncand=None, pad=SENT):
    """one launch of yh_nms_batched over `tables` -> (out (B, max_keep, 6), nkeep (B,), keep_idx (B, max_keep)) on the host, after
    the checks every launch owes: inputs unchanged, guards unchanged, nothing written past yh_nms_ws_bytes"""
    ca, inc, mk, mf = cfg
    B, ns = len(tables), [len(t) for t in tables]
    cap = cap or max(4, -(-max(ns) // 4) * 4)
    host = np.full((B, cap, 6), pad, np.float32)
    for b, t in enumerate(tables):
        host[b, :len(t)] = t
    cand = Guarded(dev, (B, cap, 6), F32, SENT, torch.from_numpy(host))
    nc = Guarded(dev, (B,), I32, -9, torch.tensor(ncand if ncand is not None else ns, dtype=I32))
    out = Guarded(dev, (B, mk, 6), F32, SENT)
    nkeep = Guarded(dev, (B,), I32, -3)
    keep = Guarded(dev, (B, mk), I32, -5)
    wsb = int(_L().yh_nms_ws_bytes(B, cap))
    assert wsb > 0
    ws = Guarded(dev, (wsb + WS_TAIL,), U8, 0xA5)
    _ok(_L().yh_nms_batched(cand.ptr, nc.ptr, B, cap, P.IOU_THR, ca, inc, mk, mf, out.ptr, nkeep.ptr, keep.ptr, ws.ptr, _stream()), "yh_nms_batched")
    torch.cuda.synchronize()
    assert cand.unchanged() and nc.unchanged(), "yh_nms_batched changed its inputs"
    for name, g in (("out", out), ("nkeep", nkeep), ("keep_idx", keep), ("ws", ws)):
        assert g.guards_intact(), f"yh_nms_batched wrote outside {name}"
    assert bool((ws.t[wsb:] == 0xA5).all()), "yh_nms_batched wrote past yh_nms_ws_bytes"
    return out.np(), nkeep.np(), keep.np()


def check_nms_image(res, b, ref, what):
    out, nkeep, keep = res
    rows, idx = ref
    k = int(nkeep[b])
    assert k == len(idx), f"{what}: nkeep {k}, oracle {len(idx)}"
    np.testing.assert_array_equal(keep[b, :k], np.asarray(idx, np.int32), err_msg=what)
    np.testing.assert_array_equal(out[b, :k], rows, err_msg=what)
    np.testing.assert_array_equal(out[b, k:], np.full((out.shape[1] - k, 6), SENT, np.float32), err_msg=what + ": rows past nkeep")


def _cfg_id(cfg):
    return "ca%d_inc%d_keep%d_merge%d" % cfg


@pytest.mark.parametrize("cfg", P.NMS_CONFIGS, ids=_cfg_id)
@pytest.mark.parametrize("n", P.NMS_SIZES)
def test_nms_single_image(dev, n, cfg):
    res = run_nms(dev, [nms_input(n)], cfg)
    check_nms_image(res, 0, nms_ref(n, cfg), f"n={n} {_cfg_id(cfg)}")
    _RAN.add(("nms", n, cfg))


@pytest.mark.parametrize("cfg", P.DESIGNED_CONFIGS, ids=_cfg_id)
@pytest.mark.parametrize("name", list(P.DESIGNED))
def test_nms_designed_table(dev, name, cfg):
    ref = nms_ref(name, cfg)
    if name == "allzero":
        assert ref[1] == []
    if name == "one_positive":
        assert ref[1] == [0]                              # the merge filter needs n > 1 to run at all: both configurations keep the row
    res = run_nms(dev, [nms_input(name)], cfg)
    check_nms_image(res, 0, ref, f"{name} {_cfg_id(cfg)}")
    _RAN.add(("nms", name, cfg))


def test_nms_larger_cap_with_nan_rows(dev):
    """cap = 2052 for 1025 candidates (sort length of the image 2048, of the workspace 4096), NaN in the rows past n"""
    for cfg in P.NMS_CONFIGS[:2]:
        res = run_nms(dev, [nms_input(1025)], cfg, cap=2052, pad=np.nan)
        check_nms_image(res, 0, nms_ref(1025, cfg), f"cap 2052 {_cfg_id(cfg)}")
    _RAN.add(("nms", "larger_cap"))


def test_nms_ncand_above_cap(dev):
    """ncand[b] > cap (a filter that counted past its table): the first cap rows are the candidates"""
    for cfg in P.NMS_CONFIGS[:2]:
        a = run_nms(dev, [nms_input(1024)], cfg, cap=1024, ncand=[1024])
        b = run_nms(dev, [nms_input(1024)], cfg, cap=1024, ncand=[1124])
        k = int(a[1][0])
        assert k == int(b[1][0]) > 0
        np.testing.assert_array_equal(b[0], a[0])
        np.testing.assert_array_equal(b[2][0, :k], a[2][0, :k])
        check_nms_image(b, 0, nms_ref(1024, cfg), f"ncand 1124 {_cfg_id(cfg)}")
    _RAN.add(("nms", "ncand_above_cap"))


def test_nms_batch_of_unequal_images(dev):
    """B = 4, n = [8193, 0, 65, 1024] in one launch: sort lengths 16384 (workspace), 1024, 1024, 1024 side by side"""
    ns = [8193, 0, 65, 1024]
    for cfg in P.NMS_CONFIGS[:2]:
        res = run_nms(dev, [nms_input(n) for n in ns], cfg, cap=8196)
        for b, n in enumerate(ns):
            single = run_nms(dev, [nms_input(n)], cfg)
            k = int(single[1][0])
            assert int(res[1][b]) == k
            np.testing.assert_array_equal(res[0][b], single[0][0])
            np.testing.assert_array_equal(res[2][b, :k], single[2][0, :k])
            check_nms_image(res, b, nms_ref(n, cfg), f"batch image {b} (n={n}) {_cfg_id(cfg)}")
    _RAN.add(("nms", "batch"))


def test_nms_zero_area_duplicates_survive(dev):
    """exclusive rule, union clamped at 1e-9: eight identical zero-area boxes have IoU 0 / 1e-9 = 0 with each other and all survive"""
    cfg = P.NMS_CONFIGS[1]
    t = nms_input(256)
    za = np.flatnonzero((t[:, :4] == np.array(P.ZERO_AREA, np.float32)).all(axis=1))
    ref = nms_ref(256, cfg)
    assert len(za) == P.NUM_ZERO_AREA and set(za) <= set(ref[1])
    res = run_nms(dev, [t], cfg)
    check_nms_image(res, 0, ref, "degenerate")
    assert set(za) <= set(res[2][0, :int(res[1][0])].tolist())
    _RAN.add(("nms", "degenerate"))


# ================================================================================================================ yh_filter_decoded
def filter_ref(dec_img, mode, thr=P.FILTER_THR):
    f = opp.candidates_yolox if mode in (1, 3) else opp.candidates_v5
    return np.asarray(f(dec_img, thr[0], thr[1], multi_label=mode >= 2), np.float32).reshape(-1, 6)


def run_filter(dev, dec, mode, cap, thr=P.FILTER_THR):
    B, N, E = dec.shape
    d = Guarded(dev, dec.shape, F32, float("nan"), torch.from_numpy(dec))
    cand = Guarded(dev, (B, cap, 6), F32, SENT)
    ncand = Guarded(dev, (B,), I32, -3)
    _ok(_L().yh_filter_decoded(d.ptr, B, N, E - 5, thr[0], thr[1], mode, cand.ptr, ncand.ptr, cap, _stream()), "yh_filter_decoded")
    torch.cuda.synchronize()
    assert d.unchanged(), "yh_filter_decoded changed its input"
    assert cand.guards_intact() and ncand.guards_intact(), "yh_filter_decoded wrote outside its outputs"
    return cand.np(), ncand.np()


def check_filter(got, dec, mode, cap, what, thr=P.FILTER_THR):
    cand, ncand = got
    for b in range(dec.shape[0]):
        ref = filter_ref(dec[b], mode, thr)
        assert int(ncand[b]) == len(ref), f"{what} image {b}: ncand {int(ncand[b])}, oracle {len(ref)}"
        k = min(len(ref), cap)
        np.testing.assert_array_equal(cand[b, :k], ref[:k], err_msg=f"{what} image {b}")
        np.testing.assert_array_equal(cand[b, k:], np.full((cap - k, 6), SENT, np.float32), err_msg=f"{what} image {b}: rows past the count")


@pytest.mark.parametrize("nc", P.FILTER_NC)
@pytest.mark.parametrize("N", P.FILTER_N)
def test_filter_decoded(dev, N, nc):
    dec = P.decoded_rows(P.FILTER_B, N, nc, seed=N * 100 + nc)
    for mode in range(4):
        cap = -(-(N * nc if mode >= 2 else N) // 4) * 4
        for thr in P.FILTER_THRS:
            check_filter(run_filter(dev, dec, mode, cap, thr), dec, mode, cap, f"N={N} nc={nc} mode={mode} thr={thr}", thr)
        _RAN.add(("filter", N, nc, mode))


@pytest.mark.parametrize("mode", range(4))
def test_filter_decoded_overflow(dev, mode):
    """cap = 4 below the count: ncand reports the full count, rows [:4] are the first four candidates, nothing is stored past them"""
    N, nc = 1025, 3
    dec = P.decoded_rows(P.FILTER_B, N, nc, seed=N * 100 + nc)
    assert all(len(filter_ref(dec[b], mode)) > 4 for b in range(P.FILTER_B - 1))
    check_filter(run_filter(dev, dec, mode, 4), dec, mode, 4, f"overflow mode={mode}")
    _RAN.add(("filter_overflow", mode))


# ================================================================================================================ decode
def upload_heads(dev, case, bf16):
    """-> (device tensors (kept alive), their pristine clones, DecodeDesc, pointer array)"""
    from yoloseries_amd._lib import DecodeDesc
    oracle_in, bufs = case.build(bf16)
    tens, ptrs = [], []
    for flat, off in bufs:
        t = torch.from_numpy(flat.view(np.int16)).to(dev).view(torch.bfloat16) if bf16 else torch.from_numpy(flat).to(dev)
        assert t.data_ptr() % 16 == 0
        tens.append(t)
        ptrs.append(t.data_ptr() + off * t.element_size())
    d = DecodeDesc()
    d.B, d.num_class, d.num_anchor, d.num_stage = case.B, case.nc, case.A, len(case.stages)
    for s, (h, w) in enumerate(case.stages):
        d.H[s], d.W[s], d.ldp[s], d.stride[s] = h, w, case.ldp, case.strides()[s]
        for a in range(case.A):
            d.anchors[(s * 3 + a) * 2], d.anchors[(s * 3 + a) * 2 + 1] = (float(v) for v in case.anchors()[s][a])
    d.pred_is_f32, d.yolox = int(not bf16), case.yolox
    parr = (C.c_void_p * 4)(*ptrs, *([None] * (4 - len(ptrs))))
    return oracle_in, tens, [t.clone() for t in tens], d, parr


def heads_unchanged(tens, clones):
    return all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip(tens, clones))


def oracle_decode(case, oracle_in):
    if case.yolox:
        return opp.decode_yolox(oracle_in, case.img_h)
    return opp.decode_v5(oracle_in, case.anchors(), case.strides())


def run_decode_full(dev, case, d, parr):
    out = Guarded(dev, (case.B, case.npred, case.E), F32, SENT)
    _ok(_L().yh_decode_full(C.byref(d), parr, out.ptr, _stream()), "yh_decode_full")
    torch.cuda.synchronize()
    assert out.guards_intact(), "yh_decode_full wrote outside its output"
    return out


def check_decode_full(case, dec, ref):
    assert dec.shape == ref.shape
    if case.npred > 10000:                    # long_row: the first and the last 2 000 predictions and every 97th between
        idx = np.unique(np.concatenate((np.arange(2000), np.arange(2000, case.npred - 2000, 97), np.arange(case.npred - 2000, case.npred))))
        dec, ref = dec[:, idx], ref[:, idx]
    np.testing.assert_allclose(dec, ref, rtol=1e-4, atol=1e-4)        # contract: 1e-4, as test_decode_golden


def run_decode_filter(dev, case, d, parr, thr, cap, two_pass, view=None, cand=None, ncand=None):
    """yh_decode_filter (view None) or yh_decode_filter_view into fresh guarded buffers (or the ones passed in)"""
    L = _L()
    cand = cand or Guarded(dev, (case.B, cap, 6), F32, SENT)
    ncand = ncand or Guarded(dev, (case.B,), I32, 123)
    ws = None
    if two_pass:
        wsb = int(L.yh_decode_filter_ws_bytes(C.byref(d)))
        assert wsb > 0
        ws = Guarded(dev, (wsb + WS_TAIL,), U8, 0xA5)
    wp = ws.ptr if ws is not None else None
    if view is None:
        _ok(L.yh_decode_filter(C.byref(d), parr, thr, thr, cand.ptr, ncand.ptr, cap, wp, _stream()), "yh_decode_filter")
    else:
        _ok(L.yh_decode_filter_view(C.byref(d), parr, C.byref(view), thr, thr, cand.ptr, ncand.ptr, cap, wp, _stream()), "yh_decode_filter_view")
    torch.cuda.synchronize()
    assert cand.guards_intact() and ncand.guards_intact(), "decode filter wrote outside its outputs"
    if ws is not None:
        assert ws.guards_intact() and bool((ws.t[wsb:] == 0xA5).all()), "decode filter wrote past yh_decode_filter_ws_bytes"
    return cand, ncand


def check_table(cand, ncand, refs, cap, what):
    """candidate table of every image against the reference rows: count, rows in order, sentinel in the rows never reached"""
    for b, ref in enumerate(refs):
        assert int(ncand[b]) == len(ref), f"{what} image {b}: ncand {int(ncand[b])}, reference {len(ref)}"
        k = min(len(ref), cap)
        np.testing.assert_array_equal(cand[b, :k], ref[:k], err_msg=f"{what} image {b}")
        np.testing.assert_array_equal(cand[b, k:], np.full((cap - k, 6), SENT, np.float32), err_msg=f"{what} image {b}: rows past the count")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", P.HEAD_CASES, ids=[c.id for c in P.HEAD_CASES])
def test_decode_head_case(dev, case, bf16):
    oracle_in, tens, clones, d, parr = upload_heads(dev, case, bf16)
    dec = run_decode_full(dev, case, d, parr).np()
    assert np.isfinite(dec).all(), "yh_decode_full read an element outside the prediction rows"
    check_decode_full(case, dec, oracle_decode(case, oracle_in))
    cand_of = opp.candidates_yolox if case.yolox else opp.candidates_v5
    for thr in (0.3, 0.001):
        refs = [np.asarray(cand_of(dec[b], thr, thr), np.float32).reshape(-1, 6) for b in range(case.B)]
        for cap in (-(-case.npred // 4) * 4, 8):
            got = []
            for two_pass in (False, True):
                cand, ncand = run_decode_filter(dev, case, d, parr, thr, cap, two_pass)
                got.append((cand.np(), ncand.np()))
                assert (got[-1][1] >= 1).all(), f"an image without a candidate: {got[-1][1]}"
                check_table(*got[-1], refs, cap, f"{case.id} thr={thr} cap={cap} {'two-pass' if two_pass else 'one-block'}")
            np.testing.assert_array_equal(got[1][1], got[0][1])
            np.testing.assert_array_equal(got[1][0], got[0][0])
    assert heads_unchanged(tens, clones), "a decode kernel changed the head tensors"
    _RAN.add(("decode", case.id, bf16))


@pytest.mark.parametrize("two_pass", [False, True], ids=["one_block", "two_pass"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cid", ["four_stages", "unpadded_nc1"])
def test_decode_filter_view(dev, cid, bf16, two_pass):
    """scale 1, no flip, ncand zeroed: yh_decode_filter's table.  A second pass (scale 0.83, rows flipped) appends after it; both
    against yh_filter_decoded of the decoded tensor edited the way YOLOV5Evaluator.test_time_augmentation edits it"""
    from yoloseries_amd._lib import ViewXform
    case = next(c for c in P.HEAD_CASES if c.id == cid)
    img_h, img_w, thr = 96.0, 160.0, 0.3
    oracle_in, tens, clones, d, parr = upload_heads(dev, case, bf16)
    cap = -(-2 * case.npred // 4) * 4
    c0, n0 = run_decode_filter(dev, case, d, parr, thr, cap, two_pass)
    c1 = Guarded(dev, (case.B, cap, 6), F32, SENT)
    n1 = Guarded(dev, (case.B,), I32, -3, torch.zeros(case.B, dtype=I32))
    run_decode_filter(dev, case, d, parr, thr, cap, two_pass, view=ViewXform(1.0, 0, img_h, img_w), cand=c1, ncand=n1)
    assert int(n0.t.min()) >= 1
    np.testing.assert_array_equal(n1.np(), n0.np())
    np.testing.assert_array_equal(c1.np(), c0.np())                        # the untouched rows included
    run_decode_filter(dev, case, d, parr, thr, cap, two_pass, view=ViewXform(0.83, 2, img_h, img_w), cand=c1, ncand=n1)
    assert (n1.np() > n0.np()).all()
    np.testing.assert_array_equal(c1.np()[:, :int(n0.t.min())], c0.np()[:, :int(n0.t.min())])
    # the materialised path: decode, edit (torch's device kernels, as the evaluator does), concatenate, filter
    full = run_decode_full(dev, case, d, parr).t
    ripe = full.clone()
    ripe[..., :4] /= 0.83
    ripe[..., 1] = img_h - ripe[..., 1]
    merged = torch.cat([full, ripe], dim=1).contiguous()
    rc = Guarded(dev, (case.B, cap, 6), F32, SENT)
    rn = Guarded(dev, (case.B,), I32, -3)
    _ok(_L().yh_filter_decoded(merged.data_ptr(), case.B, 2 * case.npred, case.nc, thr, thr, 0, rc.ptr, rn.ptr, cap, _stream()), "yh_filter_decoded")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(n1.np(), rn.np())
    np.testing.assert_array_equal(c1.np(), rc.np())
    assert heads_unchanged(tens, clones)
    _RAN.add(("view", cid, bf16, two_pass))


def test_decode_refusals_launch_nothing(dev):
    """YH_EINVAL, yh_last_error names the entry point, and no kernel ran: every output keeps its sentinel"""
    from yoloseries_amd._lib import ViewXform
    L = _L()
    case = next(c for c in P.HEAD_CASES if c.id == "unpadded_nc1")
    oracle_in, tens, clones, d, parr = upload_heads(dev, case, False)
    cap = 64
    cand = Guarded(dev, (case.B, cap, 6), F32, SENT)
    ncand = Guarded(dev, (case.B,), I32, 3)
    full = Guarded(dev, (case.B, case.npred, case.E), F32, SENT)
    ws = Guarded(dev, (int(L.yh_decode_filter_ws_bytes(C.byref(d))),), U8, 0xA5)
    xf = ViewXform(1.0, 0, 96.0, 160.0)

    def refused(rc, entry):
        msg = L.yh_last_error().decode()
        assert rc == YH_EINVAL and entry in msg, (rc, msg)

    ld_ok = d.ldp[1]
    d.ldp[1] = case.A * case.E - 1                           # ldp < A * (5 + nc)
    refused(L.yh_decode_full(C.byref(d), parr, full.ptr, _stream()), "yh_decode_full")
    for w in (None, ws.ptr):
        refused(L.yh_decode_filter(C.byref(d), parr, 0.3, 0.3, cand.ptr, ncand.ptr, cap, w, _stream()), "yh_decode_filter")
        refused(L.yh_decode_filter_view(C.byref(d), parr, C.byref(xf), 0.3, 0.3, cand.ptr, ncand.ptr, cap, w, _stream()), "yh_decode_filter_view")
    d.ldp[1] = ld_ok
    for w in (None, ws.ptr):                                 # cap % 4 != 0
        refused(L.yh_decode_filter(C.byref(d), parr, 0.3, 0.3, cand.ptr, ncand.ptr, 62, w, _stream()), "yh_decode_filter")
        refused(L.yh_decode_filter_view(C.byref(d), parr, C.byref(xf), 0.3, 0.3, cand.ptr, ncand.ptr, 62, w, _stream()), "yh_decode_filter_view")
    refused(L.yh_filter_decoded(full.ptr, case.B, case.npred, case.nc, 0.3, 0.3, 0, cand.ptr, ncand.ptr, 62, _stream()), "yh_filter_decoded")
    nws = Guarded(dev, (int(L.yh_nms_ws_bytes(case.B, 64)),), U8, 0xA5)
    refused(L.yh_nms_batched(cand.ptr, ncand.ptr, case.B, 62, 0.45, 1, 1, 8, 1, full.ptr, ncand.ptr, ncand.ptr, nws.ptr, _stream()), "yh_nms_batched")
    torch.cuda.synchronize()
    for g in (cand, ncand, full, ws, nws):
        assert g.unchanged(), "a refused call launched a kernel"

    # a row the 64-pixel LDS tile cannot hold: 64 * (640 * 4 + 16) bytes > 160 KB.  Refused with a workspace, served without one.
    wide = P.HeadCase("ldp640", 0, 3, 1, case.stages, B=2, ldp=640, seed=17)
    oracle_in, wt, wclones, wd, wparr = upload_heads(dev, wide, False)
    wcap = -(-wide.npred // 4) * 4
    wcand = Guarded(dev, (wide.B, wcap, 6), F32, SENT)
    wn = Guarded(dev, (wide.B,), I32, 3)
    wws = Guarded(dev, (int(L.yh_decode_filter_ws_bytes(C.byref(wd))),), U8, 0xA5)
    refused(L.yh_decode_filter(C.byref(wd), wparr, 0.3, 0.3, wcand.ptr, wn.ptr, wcap, wws.ptr, _stream()), "yh_decode_filter")
    torch.cuda.synchronize()
    assert wcand.unchanged() and wn.unchanged() and wws.unchanged()
    dec = run_decode_full(dev, wide, wd, wparr).np()
    check_decode_full(wide, dec, oracle_decode(wide, oracle_in))
    run_decode_filter(dev, wide, wd, wparr, 0.3, wcap, False, cand=wcand, ncand=wn)
    refs = [np.asarray(opp.candidates_v5(dec[b], 0.3, 0.3), np.float32).reshape(-1, 6) for b in range(wide.B)]
    assert all(len(r) >= 1 for r in refs)
    check_table(wcand.np(), wn.np(), refs, wcap, "ldp 640 one-block")
    _RAN.add(("refusals",))


# ================================================================================================================ box utilities
_IOU_SETS = {}


def iou_sets():
    """1030 and 1021 boxes: nms_table boxes, 20 zero-area boxes (ten of them shared by both sets: 0 / 0), 20 far away (both
    intersection sides negative: the unclamped product is positive)"""
    if not _IOU_SETS:
        r = np.random.RandomState(99)
        p = r.uniform(50, 600, (20, 2))
        zero = np.concatenate((p, p), axis=1)
        zero[10:, 3] += r.uniform(5, 50, 10)                # ten points, ten vertical segments
        zero = (np.round(zero * 4) / 4).astype(np.float32)
        far1 = (np.array([5000, 5000, 5040, 5030]) + 100 * np.arange(20)[:, None]).astype(np.float32)
        far2 = (np.array([-3000, 9000, -2950, 9060]) - 70 * np.arange(20)[:, None]).astype(np.float32)
        b1 = np.concatenate((P.nms_table(990, seed=4990)[:, :4], zero, far1))
        b2 = np.concatenate((P.nms_table(981, seed=4981)[:, :4], zero[::-1], far2))
        assert b1.shape == (1030, 4) and b2.shape == (1021, 4)
        _IOU_SETS["b"] = (np.ascontiguousarray(b1), np.ascontiguousarray(b2))
    return _IOU_SETS["b"]


@pytest.mark.parametrize("eps,oracle", [(1e-9, "gpu_iou"), (0.0, "numba_iou"), (-1.0, "evaluator_bbox_iou")])
def test_iou_matrix_past_one_grid_pass(dev, eps, oracle):
    b1, b2 = iou_sets()
    n1, n2 = len(b1), len(b2)
    assert n1 * n2 > 4096 * 256
    ref = getattr(obb, oracle)(b1, b2)
    assert np.isnan(ref).any() == (eps <= 0)
    if eps < 0:
        assert (ref[-20:, -20:] != 0).all()                 # far apart on both axes: the product of two negative sides is not clamped away
    d1 = Guarded(dev, b1.shape, F32, float("nan"), torch.from_numpy(b1))
    d2 = Guarded(dev, b2.shape, F32, float("nan"), torch.from_numpy(b2))
    out = Guarded(dev, (n1, n2), F32, SENT)
    _ok(_L().yh_iou_matrix(d1.ptr, n1, d2.ptr, n2, eps, out.ptr, _stream()), "yh_iou_matrix")
    torch.cuda.synchronize()
    assert d1.unchanged() and d2.unchanged() and out.guards_intact()
    got = out.np()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])
    for a, b in ((0, n2), (n1, 0)):                          # an empty side: YH_OK, nothing launched
        out2 = Guarded(dev, (4,), F32, SENT)
        assert _L().yh_iou_matrix(d1.ptr, a, d2.ptr, b, eps, out2.ptr, _stream()) == 0
        torch.cuda.synchronize()
        assert out2.unchanged()
    _RAN.add(("iou_matrix", eps))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 544])
def test_iou_pairwise_lengths(dev, n):
    """rows are independent: the first n golden values are the expected values of the first n rows (bars of test_ciou_and_iou_utils)"""
    g = np.load(os.path.join(G, "g1_boxes.npz"))
    assert len(g["b1"]) >= 544
    d1 = Guarded(dev, (n, 4), F32, float("nan"), torch.from_numpy(g["b1"][:n].copy()))
    d2 = Guarded(dev, (n, 4), F32, float("nan"), torch.from_numpy(g["b2"][:n].copy()))
    for kind, key, atol, with_grad in ((0, "giou", 1e-6, False), (1, "diou", 1e-6, False), (2, "ciou", 1e-5, False), (2, "ciou", 1e-5, True)):
        out = Guarded(dev, (n,), F32, SENT, guard=4)                       # one guard row after out / grad
        grad = Guarded(dev, (n, 4), F32, SENT, guard=4)
        _ok(_L().yh_iou_pairwise(kind, d1.ptr, d2.ptr, n, out.ptr, grad.ptr if with_grad else None, _stream()), "yh_iou_pairwise")
        torch.cuda.synchronize()
        assert out.guards_intact() and grad.guards_intact() and d1.unchanged() and d2.unchanged()
        np.testing.assert_allclose(out.np(), g[key][:n], rtol=0, atol=atol)
        if with_grad:
            np.testing.assert_allclose(grad.np(), g["ciou_grad_b1"][:n], rtol=1e-4, atol=1e-5)
        else:
            assert grad.unchanged()
    out = Guarded(dev, (4,), F32, SENT)
    grad = Guarded(dev, (4, 4), F32, SENT)
    for kind in range(3):
        assert _L().yh_iou_pairwise(kind, d1.ptr, d2.ptr, 0, out.ptr, None, _stream()) == 0          # n = 0: YH_OK
    for kind in (0, 1):
        assert _L().yh_iou_pairwise(kind, d1.ptr, d2.ptr, n, out.ptr, grad.ptr, _stream()) == YH_EINVAL
        assert "yh_iou_pairwise" in _L().yh_last_error().decode()
    torch.cuda.synchronize()
    assert out.unchanged() and grad.unchanged()
    _RAN.add(("iou_pairwise", n))


# ================================================================================================================ coverage
def test_zz_every_case_ran(dev):
    """no case hides behind a deselection, a skip or a typo: every case named in the issue ran to its end"""
    want = {("nms", n, cfg) for n in P.NMS_SIZES for cfg in P.NMS_CONFIGS}
    want |= {("nms", name, cfg) for name in P.DESIGNED for cfg in P.DESIGNED_CONFIGS}
    want |= {("nms", k) for k in ("larger_cap", "ncand_above_cap", "batch", "degenerate")}
    want |= {("filter", N, nc, mode) for N in P.FILTER_N for nc in P.FILTER_NC for mode in range(4)}
    want |= {("filter_overflow", mode) for mode in range(4)}
    want |= {("decode", c.id, bf16) for c in P.HEAD_CASES for bf16 in (False, True)}
    want |= {("view", cid, bf16, tp) for cid in ("four_stages", "unpadded_nc1") for bf16 in (False, True) for tp in (False, True)}
    want |= {("refusals",)}
    want |= {("iou_matrix", e) for e in (1e-9, 0.0, -1.0)} | {("iou_pairwise", n) for n in (1, 255, 256, 257, 544)}
    missing = sorted(map(str, want - _RAN))
    assert not missing, missing
