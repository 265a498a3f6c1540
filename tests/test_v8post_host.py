"""YOLOv8 post-processing, host side: the fixture tests/golden/g20_v8post.npz (tools/gen_golden_v8post.py ran the reference's
YOLOV8Evaluator) sits on no decision boundary, and the NumPy restatement (tools/v8post_restated.py) in fp32 reproduces the
reference's candidate rows and final rows of every square case — classes and row counts exactly, scores within rtol / atol 2e-5
(the bar tests/test_gpu_postproc.py states for decoded sigmoid outputs), boxes within 4 * E_ref of the fp64 restatement (E_ref:
the reference's own fp32 error against it, stored per case).  Then the descriptor checks of the C entry points, which return
before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

from tools import v8post_cases as vc
from tools import v8post_restated as vr

G = os.path.join(os.path.dirname(__file__), "golden", "g20_v8post.npz")
SCORE_TOL = dict(rtol=2e-5, atol=2e-5)


def unpack(g, name, what):
    n, body = g[f"{name}_n{what}"], g[f"{name}_{what}"]
    rows, at = [], 0
    for k in n:
        rows.append(None if k < 0 else body[at:at + k])
        at += max(int(k), 0)
    return rows


def box_bar(g, name):
    return 4.0 * float(g[f"{name}_box_err_ref"][0])


def assert_rows(got, want, want64, bar, what):
    """rows (n, 6) against the reference's: count and classes exact, scores within SCORE_TOL, boxes within `bar` of the fp64 rows"""
    assert (got is None) == (want is None), what
    if want is None:
        return
    assert got.shape == want.shape, f"{what}: {got.shape} rows, reference {want.shape}"
    np.testing.assert_array_equal(got[:, 5], want[:, 5], err_msg=what)
    np.testing.assert_allclose(got[:, 4], want[:, 4], err_msg=what, **SCORE_TOL)
    if len(got):
        err = np.abs(got[:, :4].astype(np.float64) - want64[:, :4]).max()
        assert err <= bar, f"{what}: boxes {err:.3g} from the fp64 restatement, bar {bar:.3g}"


@pytest.fixture(scope="module")
def g():
    return np.load(G)


@pytest.fixture(scope="module")
def restated(g):
    """name -> (decoded, candidates, finals) of the fp32 and of the fp64 restatement, computed once"""
    out = {}
    for name in vc.CASES:
        seed = int(g[f"{name}_seed"][0])
        out[name] = (vr.run_case(name, seed, np.float32), vr.run_case(name, seed, np.float64))
    return out


@pytest.mark.parametrize("name", list(vc.CASES))
def test_fixture_sits_on_no_decision_boundary(g, restated, name):
    """the conditions the generator asserted on the reference's results, re-asserted from the fixture and the restatement alone"""
    seed = int(g[f"{name}_seed"][0])
    (dec, cands, outs), _ = restated[name]
    if name not in vc.RESTATED_ONLY:
        cands, outs = unpack(g, name, "cand"), unpack(g, name, "out")
    cls_thr, _ = vc.thresholds(name)
    ml = None if vc.make_hyp(name)["mutil_label"] else vr.cell_max_logit(name, seed, dec, cls_thr)
    assert vr.conditions(name, dec, cands, outs, ml) is None


def test_fixture_covers_what_it_claims(g):
    assert g["g_nout"][-1] == -1 and g["g_ncand"][-1] == 0 and g["g_nout"][0] > 0          # an image without candidates gives None
    b, s, y, x, c20, c25 = vc.TIE_CELL
    cell = y * (vc.case("h")["img"][1] // vc.case("h")["strides"][s]) + x
    (dec, cands, _), _ = (vr.run_case("h", int(g["h_seed"][0]), np.float32), None)
    assert dec[b, cell, 4 + c20] == 1.0 and dec[b, cell, 4 + c25] == 1.0                    # both saturate: the logits would say c25
    row = int((dec[b, :cell, 4:].max(-1) >= np.float32(0.25)).sum())
    assert g["h_cand"][row, 4] == 1.0 and g["h_cand"][row, 5] == c20                        # the reference takes the first
    assert (g["m_ncand"] == vc.ncell("m")).all()                                            # metric threshold: every cell passes
    assert len(g["t_cand"]) > 0 and (g["e_ncand"] > 0).all()
    assert os.path.getsize(G) <= 500 * 1024


@pytest.mark.parametrize("name", vc.SQUARE)
def test_restatement_reproduces_the_reference(g, restated, name):
    (dec, cands, outs), (dec64, cands64, outs64) = restated[name]
    bar = box_bar(g, name)
    ref_c, ref_o = unpack(g, name, "cand"), unpack(g, name, "out")
    for b in range(len(ref_c)):
        print(f"case {name} image {b}: {len(cands[b])} candidates (reference {len(ref_c[b])}), "
              f"{None if outs[b] is None else len(outs[b])} rows (reference {None if ref_o[b] is None else len(ref_o[b])}), bar {bar:.3g}")
        assert_rows(cands[b], ref_c[b], cands64[b], bar, f"case {name} image {b} candidates")
        if name != "h":
            assert_rows(outs[b], ref_o[b], outs64[b], bar, f"case {name} image {b} final rows")
    key = {"a": "a_decoded", "c32": "c32_decoded", "c16": "c16_decoded"}.get(name)
    if key:
        np.testing.assert_allclose(dec[..., 4:], g[key][..., 4:], **SCORE_TOL)
        assert np.abs(g[key][..., :4].astype(np.float64) - dec64[..., :4]).max() == pytest.approx(g[f"{name}_box_err_ref"][0], rel=1e-3)


# ------------------------------------------------------------------------------------------------- descriptor validation
def _desc(**kw):
    from yoloseries_amd._lib import V8DecDesc
    d = V8DecDesc()
    d.B, d.num_class, d.num_stage, d.reg, d.pred_is_f32, d.img_h = 1, 3, 2, 4, 1, 64.0
    for s in range(2):
        d.H[s], d.W[s], d.ldp[s] = 4 >> s, 4 >> s, 24
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


BAD_DESCS = [
    (dict(reg=1), "reg 1 is outside 2..32"), (dict(reg=33), "reg 33 is outside 2..32"),
    (dict(num_stage=0), "num_stage 0 is outside 1..4"), (dict(num_stage=5), "num_stage 5 is outside 1..4"),
    (dict(ldp=(1, 18)), "stage 1: ldp 18 < 4*reg + num_class = 19"), (dict(B=0), "bad dims"), (dict(num_class=0), "bad dims"),
    (dict(H=(0, 0)), "stage 0: null tensor or empty map"), (dict(img_h=0.0), "img_h must be positive and finite"),
]


@pytest.mark.parametrize("kw,msg", BAD_DESCS)
def test_bad_descriptors_are_refused_with_a_message(kw, msg):
    """YH_EINVAL comes before any launch, so the checks run without a GPU; the pointers only have to be non-null"""
    from yoloseries_amd._lib import lib
    L = lib()
    d = _desc(**kw)
    ptrs = (C.c_void_p * 4)(0x1000, 0x1000, None, None)
    for rc in (L.yh_v8_decode_full(C.byref(d), ptrs, 0x1000, None),
               L.yh_v8_decode_filter(C.byref(d), ptrs, None, 0.25, 0x1000, 0x1000, 64, None, None)):
        assert rc == -1
        assert msg in L.yh_last_error().decode()


def test_bad_arguments_are_refused_with_a_message():
    from yoloseries_amd._lib import ViewXform, lib
    L = lib()
    d = _desc()
    ptrs = (C.c_void_p * 4)(0x1000, 0x1000, None, None)
    null2 = (C.c_void_p * 4)(0x1000, None, None, None)

    def refused(rc, msg):
        assert rc == -1 and msg in L.yh_last_error().decode(), L.yh_last_error().decode()

    refused(L.yh_v8_decode_full(None, ptrs, 0x1000, None), "null desc")
    refused(L.yh_v8_decode_full(C.byref(d), null2, 0x1000, None), "stage 1: null tensor")
    refused(L.yh_v8_decode_full(C.byref(d), ptrs, None, None), "null output")
    refused(L.yh_v8_decode_filter(C.byref(d), ptrs, None, 0.25, None, 0x1000, 64, None, None), "cand/ncand null")
    refused(L.yh_v8_decode_filter(C.byref(d), ptrs, None, 0.25, 0x1000, None, 64, None, None), "cand/ncand null")
    refused(L.yh_v8_decode_filter(C.byref(d), ptrs, None, 0.25, 0x1000, 0x1000, 62, None, None), "multiple of 4")
    refused(L.yh_v8_decode_filter(C.byref(d), ptrs, None, 0.25, 0x1000, 0x1000, 64, 0x1008, None), "workspace unaligned")
    for xf, msg in ((ViewXform(1.0, 1, 64, 64), "flip_axis 1 is not 0, 2 or 3"), (ViewXform(0.0, 0, 64, 64), "scale must be positive"),
                    (ViewXform(float("inf"), 0, 64, 64), "scale must be positive"), (ViewXform(float("nan"), 2, 64, 64), "scale must be positive")):
        refused(L.yh_v8_decode_filter(C.byref(d), ptrs, C.byref(xf), 0.25, 0x1000, 0x1000, 64, None, None), msg)
    refused(L.yh_v8_filter_decoded(None, 1, 4, 3, 0.25, 0, 0x1000, 0x1000, 64, None), "null pointer")
    refused(L.yh_v8_filter_decoded(0x1000, 1, 0, 3, 0.25, 0, 0x1000, 0x1000, 64, None), "bad dims")
    refused(L.yh_v8_filter_decoded(0x1000, 1, 4, 3, 0.25, 2, 0x1000, 0x1000, 64, None), "multi_label must be 0 or 1")
    assert L.yh_v8_decode_filter_ws_bytes(None) == 0
    assert L.yh_v8_decode_filter_ws_bytes(C.byref(d)) == 2 * (64 * 6 * 4 + 4)          # one chunk per stage


def test_ctypes_descriptor_matches_the_header(tmp_path):
    """size and field offsets of V8DecDesc against the C compiler's view of include/yolohip.h"""
    import subprocess
    from yoloseries_amd._lib import V8DecDesc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f[0] for f in V8DecDesc._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "yolohip.h"', 'int main(void) {',
           '  printf("%zu\\n", sizeof(yh_v8dec_desc));']
    src += [f'  printf("%zu\\n", offsetof(yh_v8dec_desc, {n}));' for n in names]
    src += ['  return 0; }']
    (tmp_path / "p.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "p")], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(V8DecDesc)
    assert vals[1:] == [getattr(V8DecDesc, n).offset for n in names]
