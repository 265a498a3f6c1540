#!/usr/bin/env python3
"""Generate tests/golden/g17_augment.npz by RUNNING THE REFERENCE's augmentation functions: utils.mosaic, utils.RandomPerspective
(its cv2 warps stubbed to record the matrix; OpenCV is absent), utils.RandomFlipLR / RandomFlipUD and utils.valid_bbox.  Runs only
where the reference tree is present (tools/gen_golden.py's REF); writes data only: per case the input images and labels, the values
`random.random()` returned in order (mosaic: 2, RandomPerspective: 9, the two flips: 1 each), the mosaic canvas and labels, M, and the
labels after the warp and after flips + valid_bbox.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_augment.py
"""
import math
import os
import random
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

OUT = os.path.join(gen_golden.OUT, "g17_augment.npz")
DST = 64                         # network input 64 x 64, mosaic canvas 128 x 128
FILL = 114
# name -> (image sizes (h, w), seed, degree, translate, scale, shear, perspective, fliplr_p, flipud_p)
CASES = {
    # 41x33: smaller than its quadrant (fill shows) and 33 * 41 * 3 bytes: the later images start at odd offsets; 150x171: cropped
    "mosaic_affine": ([(41, 33), (150, 171), (57, 63), (90, 77)], 1701, 10.0, 0.1, 0.5, 5.0, 0.0, 1.0, 0.0),
    "mosaic_persp": ([(41, 33), (150, 171), (57, 63), (90, 77)], 1702, 0.0, 0.1, 0.5, 0.0, 0.0005, 0.0, 1.0),
    "mosaic_shipped": ([(80, 96), (64, 64), (33, 45), (150, 171)], 1703, 0.0, 0.1, 0.5, 0.0, 0.0, 0.0, 0.0),
    "single": ([(70, 93)], 1704, 5.0, 0.1, 0.5, 2.0, 0.0005, 1.0, 1.0),
}


class RecordingRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.log = []

    def random(self):
        v = super().random()
        self.log.append(v)
        return v


class Cv2Stub(types.ModuleType):
    """the three cv2 functions RandomPerspective calls; the warps record M and return an image of the output size"""

    def __init__(self):
        super().__init__("cv2")
        self.warp_M = None

    @staticmethod
    def getRotationMatrix2D(angle, center, scale):
        a = angle * math.pi / 180
        alpha, beta = scale * math.cos(a), scale * math.sin(a)
        return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]],
                         [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]])

    def warpPerspective(self, img, M, dsize, borderValue=None):
        self.warp_M = np.array(M, dtype=np.float64)
        return np.zeros((dsize[1], dsize[0], 3), dtype=np.uint8)

    def warpAffine(self, img, M, dsize, borderValue=None):
        self.warp_M = np.vstack([np.array(M, dtype=np.float64), [0, 0, 1]])
        return np.zeros((dsize[1], dsize[0], 3), dtype=np.uint8)


def make_item(rs, h, w, n):
    img = rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8)
    cx, cy = rs.uniform(0.05, 0.95, n) * w, rs.uniform(0.05, 0.95, n) * h
    bw, bh = rs.uniform(3, 0.6 * w, n), rs.uniform(3, 0.6 * h, n)
    x0, y0 = np.clip(cx - bw / 2, 0, w - 2), np.clip(cy - bh / 2, 0, h - 2)
    x1, y1 = np.clip(cx + bw / 2, x0 + 1, w), np.clip(cy + bh / 2, y0 + 1, h)
    return img, np.stack([x0, y0, x1, y1], 1).astype(np.float32), rs.randint(0, 80, n).astype(np.float32)


def main():
    if not os.path.isdir(gen_golden.REF):
        sys.exit("tools/gen_golden_augment.py needs the reference tree (see tools/gen_golden.py)")
    sys.dont_write_bytecode = True
    gen_golden.install_shims()
    sys.path.insert(0, gen_golden.REF)
    import utils as ref_utils
    from utils import data_aug as ref_aug
    cv2 = Cv2Stub()
    ref_aug.cv2 = cv2
    g = {"dst": np.array(DST), "fill_value": np.array(FILL), "cases": np.array(list(CASES))}
    dropped_by_mosaic = dropped_by_candidates = 0
    for name, (sizes, seed, degree, translate, scale, shear, persp, lr_p, ud_p) in CASES.items():
        rs = np.random.RandomState(seed)
        items = [make_item(rs, h, w, 6) for h, w in sizes]
        rng = RecordingRandom(seed)
        ref_aug.random = rng
        for k, (img, box, lab) in enumerate(items):
            g[f"{name}_img{k}"], g[f"{name}_box{k}"], g[f"{name}_lab{k}"] = img, box, lab
        if len(items) == 4:
            canvas, box, lab = ref_utils.mosaic([i[0] for i in items], [i[1] for i in items], [i[2] for i in items],
                                                mosaic_shape=[2 * DST, 2 * DST], fill_value=FILL)
            g[f"{name}_canvas"], g[f"{name}_mosaic_box"], g[f"{name}_mosaic_lab"] = canvas, box, lab
            dropped_by_mosaic += sum(len(i[1]) for i in items) - len(box)
        else:
            canvas, box, lab = items[0]
        n_in = len(box)
        _, box, lab = ref_utils.RandomPerspective(canvas, box, lab, 1.0, degree, translate, scale, shear, persp, [DST, DST], FILL)
        dropped_by_candidates += n_in - len(box)
        g[f"{name}_M"], g[f"{name}_warp_box"], g[f"{name}_warp_lab"] = cv2.warp_M, box, lab
        out = np.zeros((DST, DST, 3), dtype=np.uint8)
        out, box = ref_utils.RandomFlipLR(out, box, lr_p)
        out, box = ref_utils.RandomFlipUD(out, box, ud_p)
        keep = ref_utils.valid_bbox(box)
        g[f"{name}_final_box"], g[f"{name}_final_lab"] = box[keep], lab[keep]
        g[f"{name}_draws"] = np.array(rng.log, dtype=np.float64)
        g[f"{name}_hyp"] = np.array([degree, translate, scale, shear, persp, lr_p, ud_p], dtype=np.float64)
        print(name, "boxes in", n_in, "after warp", len(g[f"{name}_warp_box"]), "final", int(keep.sum()), "draws", len(rng.log))
    assert dropped_by_mosaic > 0 and dropped_by_candidates > 0, (dropped_by_mosaic, dropped_by_candidates)
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
