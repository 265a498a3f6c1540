"""csrc/postproc_v8.hip through the C ABI alone (yoloseries_amd._lib.lib()), on the heads of tools/v8post_cases.py with the seeds of
tests/golden/g20_v8post.npz.  Nothing here has a tolerance: every comparison is bit for bit.

  forms      yh_v8_decode_filter with a workspace (two passes, rows staged through LDS, four lanes per cell) and without (one workgroup
             per image, one thread per cell) give the same table; so does yh_v8_decode_full followed by yh_v8_filter_decoded, and an
             identity view that appends to an empty table.  The candidate rule restated in NumPy on the GPU's own decoded tensor gives
             that table too, single and multi label.
  heads      fp32 and bf16; rows of 19 elements with nothing behind them (76 / 38 bytes: the scalar staging path), 288-byte rows, rows
             inside a wider tensor (ldp > 4*reg + nc, NaN around them), reg 2 and 32, rectangular maps with 3.75 chunks in a stage,
             a last stage smaller than a chunk, 5 440 cells in 86 chunks.
  NMS        yh_nms_batched on the GPU's own table against oracle.postproc.nms_image on that table.
  overflow   cap below the count: counts exact, the first cap rows are the table's, nothing else written.
  append     the table starts at ncand[b]; a negative ncand[b] counts as 0.
Every buffer a kernel writes sits inside a larger sentinel-filled allocation: guards and rows past the advertised extent must not
change; inputs must not change either."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import postproc as opp
from tools import v8post_cases as vc
from tools import v8post_restated as vr

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "g20_v8post.npz")
SENT = -7.0
YH_EINVAL = -1
F32, I32, U8, BF16 = torch.float32, torch.int32, torch.uint8, torch.bfloat16
# case -> (ldp, elements in front of a row's head inside the wider row); None: ldp = 4*reg + nc rounded up to 8 (what the evaluator makes)
LAYOUT = {"a": None, "b": None, "c32": (19, 0), "c16": (19, 0), "d": None, "p": (112, 8), "q2": None, "q32": None, "r": None}
CASES = list(LAYOUT)


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

    def __init__(self, dev, shape, dtype, fill, data=None, guard=256):
        n = int(np.prod(shape))
        g = self.g = guard
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


class Heads:
    """the kernel's view of a case: per stage a guarded [B][h][w][ldp] buffer, NaN wherever the kernel has no business reading"""

    def __init__(self, dev, name, seed):
        from yoloseries_amd._lib import V8DecDesc
        c = vc.case(name)
        E = 4 * c["reg"] + c["nc"]
        ldp, lead = LAYOUT[name] or (((E + 7) // 8) * 8, 0)
        self.c, self.E, self.bufs = c, E, []
        d = self.d = V8DecDesc()
        d.B, d.num_class, d.num_stage, d.reg = c["B"], c["nc"], len(c["strides"]), c["reg"]
        d.pred_is_f32, d.img_h = int(not c["bf16"]), float(c["img"][0])
        ptrs = []
        for s, v in enumerate(vc.heads(name, seed).values()):
            B, _, h, w = v.shape
            body = np.full((B, h, w, ldp), np.nan, np.float32)       # ldp == E (cases c): the last row has nothing behind it but the guard
            body[..., lead:lead + E] = v.transpose(0, 2, 3, 1)
            body = body.reshape(-1)
            t = torch.from_numpy(body)
            gb = Guarded(dev, (body.size,), BF16 if c["bf16"] else F32, float("nan"), t.bfloat16() if c["bf16"] else t)
            self.bufs.append(gb)
            d.H[s], d.W[s], d.ldp[s] = h, w, ldp
            ptrs.append(gb.ptr + lead * (2 if c["bf16"] else 4))
        self.ptrs = (C.c_void_p * 4)(*ptrs, *([None] * (4 - len(ptrs))))
        self.N = vc.ncell(name)

    def unchanged(self):
        return all(b.unchanged() for b in self.bufs)


def run_filter(dev, H, cls_thr, cap, two_pass, xf=None, start=None):
    """yh_v8_decode_filter into guarded buffers -> (table (B, cap, 6), counts (B,)); guards, workspace tail and inputs are checked"""
    L = _L()
    B = H.d.B
    cand = Guarded(dev, (B, cap, 6), F32, SENT)
    ncand = Guarded(dev, (B,), I32, -99, None if start is None else torch.tensor(start, dtype=I32))
    ws = None
    if two_pass:
        need = int(L.yh_v8_decode_filter_ws_bytes(C.byref(H.d)))
        assert need == B * sum((H.d.H[s] * H.d.W[s] + 63) // 64 for s in range(H.d.num_stage)) * (64 * 6 * 4 + 4)
        ws = Guarded(dev, (need,), U8, 0x5A)
    _ok(L.yh_v8_decode_filter(C.byref(H.d), H.ptrs, None if xf is None else C.byref(xf), cls_thr, cand.ptr, ncand.ptr, cap,
                              ws.ptr if ws else None, _stream()), "yh_v8_decode_filter")
    torch.cuda.synchronize()
    assert cand.guards_intact() and ncand.guards_intact() and H.unchanged() and (ws is None or ws.guards_intact())
    return cand.np(), ncand.np()


def run_decoded(dev, H, cls_thr, cap, multi):
    """yh_v8_decode_full, then yh_v8_filter_decoded on its tensor -> (decoded, table, counts)"""
    L = _L()
    B, E = H.d.B, 4 + H.d.num_class
    dec = Guarded(dev, (B, H.N, E), F32, SENT)
    _ok(L.yh_v8_decode_full(C.byref(H.d), H.ptrs, dec.ptr, _stream()), "yh_v8_decode_full")
    torch.cuda.synchronize()
    assert dec.guards_intact() and H.unchanged()
    before = dec.flat.clone()
    cand = Guarded(dev, (B, cap, 6), F32, SENT)
    ncand = Guarded(dev, (B,), I32, -99)
    _ok(L.yh_v8_filter_decoded(dec.ptr, B, H.N, H.d.num_class, cls_thr, int(multi), cand.ptr, ncand.ptr, cap, _stream()), "yh_v8_filter_decoded")
    torch.cuda.synchronize()
    assert cand.guards_intact() and ncand.guards_intact() and torch.equal(_bytes(dec.flat), _bytes(before))
    return dec.np(), cand.np(), ncand.np()


def assert_table(tab, cnt, rows, what):
    """table rows [0, cnt[b]) are `rows[b]` bit for bit, everything behind them is still the sentinel"""
    for b, want in enumerate(rows):
        assert cnt[b] == len(want), f"{what}: image {b} has {cnt[b]} rows, expected {len(want)}"
        np.testing.assert_array_equal(tab[b, :len(want)].view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32), err_msg=what)
        assert (tab[b, len(want):] == SENT).all(), f"{what}: image {b} written past its count"


@pytest.fixture(scope="module")
def g():
    return np.load(G)


_RUNS = {}


def runs(dev, g, name):
    """the three routes of one case at a cap that holds every cell, computed once"""
    if name not in _RUNS:
        H = Heads(dev, name, int(g[f"{name}_seed"][0]))
        thr = float(vc.thresholds(name)[0])
        cap = ((H.N + 3) // 4) * 4
        _RUNS[name] = dict(H=H, thr=thr, cap=cap, one=run_filter(dev, H, thr, cap, False), two=run_filter(dev, H, thr, cap, True),
                           dec=run_decoded(dev, H, thr, cap, False))
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_forms_agree_bit_for_bit(dev, g, name):
    r = runs(dev, g, name)
    (t1, n1), (t2, n2), (dec, t3, n3) = r["one"], r["two"], r["dec"]
    assert n1.sum() > 0 and (n1 <= r["H"].N).all()
    rows = [t1[b, :n1[b]] for b in range(len(n1))]
    assert_table(t1, n1, rows, f"{name}: one workgroup")
    assert_table(t2, n2, rows, f"{name}: two passes against one workgroup")
    assert_table(t3, n3, rows, f"{name}: decode_full + filter_decoded against the fused form")
    want = [vr.candidates(dec[b], np.float32(r["thr"]), False) for b in range(dec.shape[0])]
    assert_table(t1, n1, want, f"{name}: the candidate rule restated on the GPU's decoded tensor")
    assert np.isfinite(dec).all()                               # no NaN around the heads was read


@pytest.mark.parametrize("name", ["a", "c16", "p"])
def test_identity_view_equals_no_view(dev, g, name):
    from yoloseries_amd._lib import ViewXform
    r = runs(dev, g, name)
    c = vc.case(name)
    xf = ViewXform(1.0, 0, float(c["img"][0]), float(c["img"][1]))
    for two in (False, True):
        t, n = run_filter(dev, r["H"], r["thr"], r["cap"], two, xf=xf, start=[0] * c["B"])
        np.testing.assert_array_equal(n, r["one"][1])
        np.testing.assert_array_equal(t.view(np.uint32), r["one"][0].view(np.uint32))


@pytest.mark.parametrize("name", ["a", "c32"])
def test_multi_label_filter(dev, g, name):
    r = runs(dev, g, name)
    H = r["H"]
    cap = ((H.N * H.d.num_class + 3) // 4) * 4
    dec, tab, cnt = run_decoded(dev, H, r["thr"], cap, True)
    want = [vr.candidates(dec[b], np.float32(r["thr"]), True) for b in range(dec.shape[0])]
    assert sum(len(w) for w in want) > r["one"][1].sum()        # some cell has two classes above the threshold
    assert_table(tab, cnt, want, f"{name}: multi label")
    small = ((min(len(w) for w in want) // 2 + 3) // 4) * 4     # overflow: counted, not stored
    _, tab, cnt = run_decoded(dev, H, r["thr"], small, True)
    for b, w in enumerate(want):
        assert cnt[b] == len(w)
        np.testing.assert_array_equal(tab[b].view(np.uint32), np.ascontiguousarray(w[:small], np.float32).view(np.uint32))


@pytest.mark.parametrize("name,cfg", [("a", (1, 1)), ("a", (0, 0)), ("d", (1, 1)), ("b", (1, 1)), ("r", (1, 1))])
def test_nms_from_the_device_table(dev, g, name, cfg):
    """yh_nms_batched consumes the table where it lies; its rows equal oracle.postproc.nms_image on the GPU's OWN table"""
    L = _L()
    r = runs(dev, g, name)
    tab, cnt = r["two"]
    B, cap, max_keep = len(cnt), r["cap"], 300
    class_aware, merge = cfg
    iou_thr = float(vc.thresholds(name)[1])
    cand = Guarded(dev, (B, cap, 6), F32, SENT, torch.from_numpy(tab))
    ncand = Guarded(dev, (B,), I32, -99, torch.from_numpy(cnt))
    out = Guarded(dev, (B, max_keep, 6), F32, SENT)
    nkeep = Guarded(dev, (B,), I32, -99)
    keep = Guarded(dev, (B, max_keep), I32, -99)
    ws = Guarded(dev, (int(L.yh_nms_ws_bytes(B, cap)),), U8, 0x5A)
    _ok(L.yh_nms_batched(cand.ptr, ncand.ptr, B, cap, iou_thr, class_aware, 1, max_keep, merge, out.ptr, nkeep.ptr, keep.ptr, ws.ptr,
                         _stream()), "yh_nms_batched")
    torch.cuda.synchronize()
    assert cand.unchanged() and ncand.unchanged() and out.guards_intact() and nkeep.guards_intact() and ws.guards_intact()
    o, nk = out.np(), nkeep.np()
    for b in range(B):
        rows, _ = opp.nms_image(tab[b, :cnt[b]], iou_thr, bool(class_aware), max_keep, bool(merge))
        assert nk[b] == len(rows)
        np.testing.assert_array_equal(o[b, :nk[b]], rows)
        assert (o[b, nk[b]:] == SENT).all()
    assert 0 < nk.sum() < cnt.sum()


@pytest.mark.parametrize("two_pass", [False, True])
def test_overflow_counts_but_does_not_store(dev, g, two_pass):
    r = runs(dev, g, "d")
    full, n = r["one"]
    assert n.min() > 64
    tab, cnt = run_filter(dev, r["H"], r["thr"], 64, two_pass)
    np.testing.assert_array_equal(cnt, n)
    np.testing.assert_array_equal(tab.view(np.uint32), full[:, :64].view(np.uint32))


@pytest.mark.parametrize("two_pass", [False, True])
def test_append_starts_at_ncand(dev, g, two_pass):
    """flipped views appended behind 5 rows (image 0) and behind a negative count (image 1: counts as 0); the rows are those of the
    plain table, un-scaled and un-flipped as the header spells it"""
    from yoloseries_amd._lib import ViewXform
    r = runs(dev, g, "a")
    full, n = r["one"]
    cap = r["cap"] + 8
    for flip, scale in ((2, 0.83), (3, 0.67), (0, 1.0)):
        tab, cnt = run_filter(dev, r["H"], r["thr"], cap, two_pass, xf=ViewXform(scale, flip, 64.0, 48.0), start=[5, -3])
        inv = np.float32(1.0) / np.float32(scale)
        for b, first in enumerate((5, 0)):
            assert cnt[b] == first + n[b]
            want = full[b, :n[b]].copy()
            want[:, :4] = want[:, :4] * inv
            if flip == 2:
                want[:, 1], want[:, 3] = np.float32(64) - want[:, 3], np.float32(64) - want[:, 1]
            if flip == 3:
                want[:, 0], want[:, 2] = np.float32(48) - want[:, 2], np.float32(48) - want[:, 0]
            np.testing.assert_array_equal(tab[b, first:cnt[b]].view(np.uint32), want.view(np.uint32))
            assert (tab[b, :first] == SENT).all() and (tab[b, cnt[b]:] == SENT).all()


def test_bad_descriptors_write_nothing(dev, g):
    from yoloseries_amd._lib import V8DecDesc, ViewXform
    L = _L()
    r = runs(dev, g, "a")
    H = r["H"]
    cand = Guarded(dev, (2, 64, 6), F32, SENT)
    ncand = Guarded(dev, (2,), I32, -99)
    ws = Guarded(dev, (int(L.yh_v8_decode_filter_ws_bytes(C.byref(H.d))),), U8, 0x5A)

    def variant(**kw):
        d = V8DecDesc.from_buffer_copy(H.d)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    bad = [variant(reg=1), variant(reg=33), variant(num_stage=0), variant(num_stage=5), variant(ldp=(2, 4 * 16 + 5 - 1)), variant(B=0),
           variant(W=(3, 0)), variant(img_h=float("inf"))]
    for d in bad:
        for w in (None, ws.ptr):
            assert L.yh_v8_decode_filter(C.byref(d), H.ptrs, None, 0.25, cand.ptr, ncand.ptr, 64, w, _stream()) == YH_EINVAL
        assert L.yh_v8_decode_full(C.byref(d), H.ptrs, cand.ptr, _stream()) == YH_EINVAL
        assert L.yh_last_error()
    for xf in (ViewXform(1.0, 1, 64, 64), ViewXform(-1.0, 0, 64, 64)):
        assert L.yh_v8_decode_filter(C.byref(H.d), H.ptrs, C.byref(xf), 0.25, cand.ptr, ncand.ptr, 64, ws.ptr, _stream()) == YH_EINVAL
    assert L.yh_v8_decode_filter(C.byref(H.d), H.ptrs, None, 0.25, cand.ptr, ncand.ptr, 66, ws.ptr, _stream()) == YH_EINVAL
    assert L.yh_v8_decode_filter(C.byref(H.d), H.ptrs, None, 0.25, cand.ptr, ncand.ptr, 64, ws.ptr + 4, _stream()) == YH_EINVAL
    assert L.yh_v8_filter_decoded(cand.ptr, 2, 0, 5, 0.25, 0, cand.ptr, ncand.ptr, 64, _stream()) == YH_EINVAL
    torch.cuda.synchronize()
    assert cand.unchanged() and ncand.unchanged() and ws.unchanged() and H.unchanged()
