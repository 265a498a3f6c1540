#!/usr/bin/env python3
"""Generate tests/golden/g20_v8post.npz by RUNNING THE REFERENCE's YOLOV8Evaluator (trainer/eval_yolov8.py) on the CPU.

Runs only where /root/reference exists; the reference is imported read-only with the shims of tools/gen_golden.py.  Only data is
written.  The cases, their inputs and the stub model are tools/v8post_cases.py; per case <n> the file holds
  <n>_seed          the head seed (the heads themselves are regenerated from it)
  <n>_ncand, <n>_cand    the reference's candidate rows per image, concatenated: the candidate rule (:175-196, restated as
                         tools/v8post_restated.candidates) applied to the reference's OWN decoded tensor
  <n>_nout, <n>_out      what the reference's __call__ returned per image, concatenated (nout -1: None)
  <n>_box_err_ref   E_ref: the largest |reference fp32 box - fp64 restatement box| over the decoded tensor (the bar of the GPU's boxes
                    is 4 * E_ref against the fp64 restatement)
  a / c32 / c16 _decoded the reference's decoded tensor (do_inference); b_decoded0 that of image 0 of case b, b_boxes the boxes of all
Case r (rectangular maps; the reference scrambles their grid) is not run through the reference: only its seed is stored, and as its
box_err_ref the error of the fp32 restatement against the fp64 one.

The seed of a case is searched until tools/v8post_restated.conditions holds on the reference's results; ASSERTED for the stored seed.
The archive is written with fixed member dates, so the same inputs give the same bytes.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_v8post.py
"""
import io
import os
import sys
import zipfile

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g20_v8post.npz")
STORE_DECODED = ("a", "c32", "c16")
MAX_SEEDS = 4000


def run_reference(ref_trainer, name, seed):
    """-> (decoded, candidate rows per image, final rows per image) of the reference for one seed"""
    import torch
    from tools import v8post_cases as vc
    from tools import v8post_restated as vr
    c, hyp = vc.case(name), vc.make_hyp(name)
    x = torch.from_numpy(vc.inputs(name))
    metric = bool(c["metric"])
    ev = ref_trainer.YOLOV8Evaluator(vc.StubYolo(name, seed), hyp, compute_metric=metric)
    dec = (ev.test_time_augmentation(x)[0] if hyp["use_tta"] else ev.do_inference(x)).numpy().copy()
    ev.yolo = vc.StubYolo(name, seed)
    outs = [None if o is None else o.numpy().copy() for o in ev(x)]
    cands = [vr.candidates(dec[b], ev.cls_threshold, bool(hyp["mutil_label"])) for b in range(dec.shape[0])]
    return dec, cands, outs


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: byte-identical for identical arrays"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def pack(rows):
    n = np.array([-1 if r is None else len(r) for r in rows], np.int32)
    body = [np.asarray(r, np.float32).reshape(-1, 6) for r in rows if r is not None]
    return n, (np.concatenate(body) if body else np.zeros((0, 6), np.float32))


def main():
    if not os.path.isdir(REF):
        sys.exit("tools/gen_golden_v8post.py needs /root/reference (build container only)")
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_golden import install_shims
    install_shims()
    sys.path.insert(0, REF)
    sys.path.insert(1, ROOT)
    import torch
    import trainer as ref_trainer
    from tools import v8post_cases as vc
    from tools import v8post_restated as vr
    torch.set_num_threads(8)
    g = {}
    for i, name in enumerate(vc.CASES):
        seed0 = 20000 + MAX_SEEDS * i
        cls_thr, _ = vc.thresholds(name)
        for seed in range(seed0, seed0 + MAX_SEEDS, 3):           # steps of 3: a TTA run uses seed, seed + 1, seed + 2
            if name in vc.RESTATED_ONLY:
                dec, cands, outs = vr.run_case(name, seed, np.float32)
            else:
                dec, cands, outs = run_reference(ref_trainer, name, seed)
            ml = None if vc.make_hyp(name)["mutil_label"] else vr.cell_max_logit(name, seed, dec, cls_thr)
            why = vr.conditions(name, dec, cands, outs, ml)
            if why is None:
                break
        else:
            sys.exit(f"case {name}: no seed in {seed0}..{seed0 + MAX_SEEDS - 1} meets the conditions")
        dec64 = vr.run_case(name, seed, np.float64)[0]
        err = float(np.abs(dec[..., :4].astype(np.float64) - dec64[..., :4]).max())
        g[f"{name}_seed"] = np.array([seed], np.int64)
        g[f"{name}_box_err_ref"] = np.array([err], np.float64)
        if name not in vc.RESTATED_ONLY:
            g[f"{name}_ncand"], g[f"{name}_cand"] = pack(cands)
            g[f"{name}_nout"], g[f"{name}_out"] = pack(outs)
            if name in STORE_DECODED:
                g[f"{name}_decoded"] = dec
            if name == "b":
                g["b_decoded0"], g["b_boxes"] = dec[0], dec[..., :4]
        print(f"case {name}: seed {seed}, candidates {[len(x) for x in cands]}, kept {[None if o is None else len(o) for o in outs]}, "
              f"E_ref {err:.3g}")
    write_npz(OUT, g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
